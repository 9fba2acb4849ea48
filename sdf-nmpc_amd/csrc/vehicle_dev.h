// Device code shared by the vehicle kernels (vehicle.hip, vehicle_body.hip): the random normals of a (seed, stream,
// frame) and the state estimate.  Every kernel that writes an estimate inlines vehicle_estimate from here, so all of
// them write the same bits for the same frame.
#pragma once
#include <hip/hip_runtime.h>

#include "philox.h"
#include "vehicle_kernels.h"

namespace sdfn {

// Box-Muller's cosine branch on the 24-bit uniforms u = ((w >> 8) + 1) 2^-24 in (0, 1], in fp64
__device__ __forceinline__ double vnormal(unsigned w0, unsigned w1) {
#pragma clang fp contract(off)
    const double u1 = (double)((w0 >> 8) + 1u) * 0x1p-24, u2 = (double)((w1 >> 8) + 1u) * 0x1p-24;
    return sqrt(-2.0 * log(u1)) * cos(6.283185307179586 * u2);
}

// the normals n[2j], n[2j + 1] of call j
__device__ __forceinline__ void vnormal_pair(const VehicleArgs& A, unsigned j, unsigned frame, unsigned stream,
                                             double& n0, double& n1) {
    unsigned w[4];
    philox4x32_10(j, frame, stream, 1u, A.key0, A.key1, w);
    n0 = vnormal(w[0], w[1]);
    n1 = vnormal(w[2], w[3]);
}

__device__ __forceinline__ unsigned vstream(const VehicleArgs& A, long long b) {
    return A.stream_id ? (unsigned)A.stream_id[b] : (unsigned)b;
}

// xe = est(x, frame): position and velocity offset by bias + sigma n, the attitude turned about world z by
// delta = bias + sigma n (n[3..5] -> p, n[6..8] -> v, n[9] -> yaw).  Without noise and bias: a copy.  Every product
// and sum is rounded on its own (no contraction): vehicle_begin_kernel and the plant kernels must write the same
// bits for the same frame, whatever surrounds the inlined body.
__device__ __forceinline__ void vehicle_estimate(const VehicleArgs& A, long long b, unsigned frame, const double* x,
                                                 double* xe) {
#pragma clang fp contract(off)
#pragma unroll
    for (int i = 0; i < 10; ++i) xe[i] = x[i];
    if (!A.est_noise && !A.est_bias) return;
    double e[7] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0};  // p, v, yaw
    if (A.est_bias) {
#pragma unroll
        for (int i = 0; i < 7; ++i) e[i] = A.est_bias[b * 7 + i];
    }
    if (A.est_noise) {
        const unsigned st = vstream(A, b);
        double n[8], skip;  // n[3..9] and the unused n[2]
        vnormal_pair(A, 1u, frame, st, skip, n[0]);
        vnormal_pair(A, 2u, frame, st, n[1], n[2]);
        vnormal_pair(A, 3u, frame, st, n[3], n[4]);
        vnormal_pair(A, 4u, frame, st, n[5], n[6]);
#pragma unroll
        for (int i = 0; i < 3; ++i) {
            e[i] = e[i] + A.est_std_p * n[i];
            e[3 + i] = e[3 + i] + A.est_std_v * n[3 + i];
        }
        e[6] = e[6] + A.est_std_yaw * n[6];
    }
#pragma unroll
    for (int i = 0; i < 3; ++i) {
        xe[i] = x[i] + e[i];
        xe[7 + i] = x[7 + i] + e[3 + i];
    }
    double sd, cd;
    sincos(0.5 * e[6], &sd, &cd);  // [cd, 0, 0, sd] (x) q
    xe[3] = cd * x[3] - sd * x[6];
    xe[4] = cd * x[4] - sd * x[5];
    xe[5] = cd * x[5] + sd * x[4];
    xe[6] = cd * x[6] + sd * x[3];
}

}  // namespace sdfn
