// The vehicle model of a closed loop (fp64): what stands between the controller's command and the state it is told
// about -- an input delay of whole control periods, a first-order thrust lag, linear rotor drag, an
// Ornstein-Uhlenbeck gust acceleration, and a state estimate with bias and noise -- around the f_expl of plant.hip
// (plant_dev.h), one instance per lane.  Everything random is a pure function of (seed, stream, frame): Philox4x32-10
// under the counter (j, frame, stream, 1), j = 0..4, two Box-Muller normals per call in fp64; the sensor stage uses
// the last counter word 0, so a vehicle and a sensor with one seed never share words.  The gust of a call is drawn
// at its frame f, the estimate it writes at frame f + 1 (the frame whose controller step reads it), so a rollout
// cut into chunks repeats the uncut one bit for bit.
//
// A model with everything off never reaches this file: the engine dispatches it to plant_advance_kernel.
#include <hip/hip_runtime.h>

#include "plant_dev.h"
#include "vehicle_dev.h"
#include "vehicle_kernels.h"

namespace sdfn {

template <int KIND>
__global__ __launch_bounds__(64) void plant_vehicle_kernel(VehicleArgs V) {
    const PlantArgs& A = V.P;
    const long long b = (long long)blockIdx.x * 64 + threadIdx.x;
    if (b >= A.B) return;
    double x[11], u[4], ucmd[4];
#pragma unroll
    for (int i = 0; i < 10; ++i) x[i] = A.x[b * 10 + i];
#pragma unroll
    for (int i = 0; i < 4; ++i) ucmd[i] = u[i] = A.u[b * 4 + i];

    const bool log = A.x_log != nullptr;
    const double* pr = A.p + b * A.p_stride;
    if (log && A.k == 0) {  // row 0: the true state and the estimate the rollout starts from
        double* xl = A.x_log + b * (A.K + 1) * 10;
#pragma unroll
        for (int i = 0; i < 10; ++i) xl[i] = x[i];
        if (A.pts_log) log_point(pr, x, A.pts_log + b * (A.K + 1) * 3);
        if (V.xhat_log) {
            double* hl = V.xhat_log + b * (A.K + 1) * 10;
#pragma unroll
            for (int i = 0; i < 10; ++i) hl[i] = V.x_est[b * 10 + i];
        }
    }

    // ---- 1. input delay: the slot of this frame holds the command of frame f - d
    if (V.delay > 0) {
        double* slot = V.ring + (b * V.delay + (long long)(V.frame % (unsigned)V.delay)) * 4;
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            u[i] = slot[i];
            slot[i] = ucmd[i];
        }
    }

    // ---- 2. gust: one exact Ornstein-Uhlenbeck step per call, held over the period
    double w0 = 0.0, w1 = 0.0, w2 = 0.0;
    if (V.has_gust) {
        double n0, n1, n2, skip;
        const unsigned st = vstream(V, b);
        vnormal_pair(V, 0u, V.frame, st, n0, n1);
        vnormal_pair(V, 1u, V.frame, st, n2, skip);
        w0 = V.gust_phi * V.w[b * 3 + 0] + V.gust_amp * n0;
        w1 = V.gust_phi * V.w[b * 3 + 1] + V.gust_amp * n1;
        w2 = V.gust_phi * V.w[b * 3 + 2] + V.gust_amp * n2;
        V.w[b * 3 + 0] = w0;
        V.w[b * 3 + 1] = w1;
        V.w[b * 3 + 2] = w2;
    }

    // ---- 3. thrust: the command, or an 11th state that lags it
    const bool lag = V.itau_m > 0.0;
    double gcmd = u[0] * A.gamma;
    if (A.gamma_scale) gcmd = gcmd * A.gamma_scale[b];
    x[10] = lag ? V.gamma_act[b] : gcmd;

    PlantIn in{};
    in.wz = u[3] * A.wz;
    in.g = A.g;
    in.dist = A.acc_dist != nullptr;
    if (in.dist) {
        in.ad0 = A.acc_dist[b * 3 + 0];
        in.ad1 = A.acc_dist[b * 3 + 1];
        in.ad2 = A.acc_dist[b * 3 + 2];
    }
    // 'att': the commanded body rotation E = euler2rot(roll, pitch, 0), once per call; its third column is the thrust
    // direction, scaled by the stage's thrust
    double sr = 0.0, cr = 1.0, sp = 0.0, cp = 1.0;
    if constexpr (KIND == 0) {
        sincos(u[1] * A.roll, &sr, &cr);
        sincos(u[2] * A.pitch, &sp, &cp);
    } else {
        in.roll_des = u[1] * A.roll;
        in.pitch_des = u[2] * A.pitch;
        in.itau_roll = A.itau_roll;
        in.itau_pitch = A.itau_pitch;
    }
    const double d0 = cr * sp, d1 = -sr, d2 = cr * cp;
    const double dr0 = V.drag[0], dr1 = V.drag[1], dr2 = V.drag[2];

    auto f_expl = [&](const double* xs, double* f) {
        const double gam = xs[10];
        if constexpr (KIND == 0) {
            in.b0 = d0 * gam;
            in.b1 = d1 * gam;
            in.b2 = d2 * gam;
            plant_f_att(in, xs, f);
        } else {
            in.gamma = gam;
            plant_f_tau(in, xs, f);
        }
        if (in.dist) {
            f[7] = f[7] + in.ad0;
            f[8] = f[8] + in.ad1;
            f[9] = f[9] + in.ad2;
        }
        if (V.has_gust) {
            f[7] = f[7] + w0;
            f[8] = f[8] + w1;
            f[9] = f[9] + w2;
        }
        // ---- 4. rotor drag -R diag(d) R^T v with the body rotation the thrust uses
        if (V.has_drag) {
            const double vx = xs[7], vy = xs[8], vz = xs[9];
            if constexpr (KIND == 0) {  // R = Rz(yaw) E, (cos, sin)(yaw / 2) as plant_f_att forms them
                const double s03 = xs[3] * xs[3] + xs[6] * xs[6];
                double c = 1.0, s = 0.0;
                if (s03 > 0.0) {
                    const double r = prsqrt(s03);
                    c = xs[3] * r;
                    s = xs[6] * r;
                }
                const double r11 = c * c - s * s, r21 = (c * s) * 2.0, r33 = c * c + s * s;
                const double ax = r11 * vx + r21 * vy, ay = r11 * vy - r21 * vx, az = r33 * vz;  // Rz^T v
                // E = [[cp, sr sp, cr sp], [0, cr, -sr], [-sp, sr cp, cr cp]]; E^T a, scaled, E (.)
                const double b0 = (cp * ax - sp * az) * dr0;
                const double b1 = ((sr * sp) * ax + cr * ay + (sr * cp) * az) * dr1;
                const double b2 = (d0 * ax + d1 * ay + d2 * az) * dr2;
                const double e0 = cp * b0 + (sr * sp) * b1 + d0 * b2;
                const double e1 = cr * b1 + d1 * b2;
                const double e2 = (sr * cp) * b1 - sp * b0 + d2 * b2;
                f[7] = f[7] - (r11 * e0 - r21 * e1);
                f[8] = f[8] - (r21 * e0 + r11 * e1);
                f[9] = f[9] - r33 * e2;
            } else {  // R = quat2rot(q / |q|)
                const double inv = prsqrt(xs[3] * xs[3] + xs[4] * xs[4] + (xs[5] * xs[5] + xs[6] * xs[6]));
                const double q0 = xs[3] * inv, q1 = xs[4] * inv, q2 = xs[5] * inv, q3 = xs[6] * inv;
                const double r11 = q0 * q0 + q1 * q1 - q2 * q2 - q3 * q3, r12 = (q1 * q2 - q0 * q3) * 2.0,
                             r13 = (q1 * q3 + q0 * q2) * 2.0;
                const double r21 = (q1 * q2 + q0 * q3) * 2.0, r22 = q0 * q0 - q1 * q1 + q2 * q2 - q3 * q3,
                             r23 = (q2 * q3 - q0 * q1) * 2.0;
                const double r31 = (q1 * q3 - q0 * q2) * 2.0, r32 = (q2 * q3 + q0 * q1) * 2.0,
                             r33 = q0 * q0 - q1 * q1 - q2 * q2 + q3 * q3;
                const double b0 = (r11 * vx + r21 * vy + r31 * vz) * dr0;
                const double b1 = (r12 * vx + r22 * vy + r32 * vz) * dr1;
                const double b2 = (r13 * vx + r23 * vy + r33 * vz) * dr2;
                f[7] = f[7] - (r11 * b0 + r12 * b1 + r13 * b2);
                f[8] = f[8] - (r21 * b0 + r22 * b1 + r23 * b2);
                f[9] = f[9] - (r31 * b0 + r32 * b1 + r33 * b2);
            }
        }
        f[10] = lag ? (gcmd - gam) * V.itau_m : 0.0;
    };

    // ---- 5. ERK4 with plant_advance_kernel's tableau and accumulation order, on eleven states
    const double h = A.dt / (double)A.substeps;
    const double hb[4] = {h / 6, h / 3, h / 3, h / 6}, ha[4] = {0.0, h / 2, h / 2, h};
    for (int sub = 0; sub < A.substeps; ++sub) {
        double xo[11], kk[11], tmp[11];
        f_expl(x, kk);
#pragma unroll
        for (int i = 0; i < 11; ++i) xo[i] = x[i] + kk[i] * hb[0];
#pragma unroll
        for (int st = 1; st < 4; ++st) {
#pragma unroll
            for (int i = 0; i < 11; ++i) tmp[i] = x[i] + kk[i] * ha[st];
            f_expl(tmp, kk);
#pragma unroll
            for (int i = 0; i < 11; ++i) xo[i] = xo[i] + kk[i] * hb[st];
        }
#pragma unroll
        for (int i = 0; i < 11; ++i) x[i] = xo[i];
    }

#pragma unroll
    for (int i = 0; i < 10; ++i) A.x_next[b * 10 + i] = x[i];
    if (lag) V.gamma_act[b] = x[10];

    // ---- 6. the estimate the next frame's controller step reads
    double xe[10];
    vehicle_estimate(V, b, V.frame + 1u, x, xe);
#pragma unroll
    for (int i = 0; i < 10; ++i) V.x_est[b * 10 + i] = xe[i];

    if (log) {
        const long long row = b * A.K + A.k;
        double* xl = A.x_log + (b * (A.K + 1) + A.k + 1) * 10;
#pragma unroll
        for (int i = 0; i < 10; ++i) xl[i] = x[i];
#pragma unroll
        for (int i = 0; i < 4; ++i) A.u_log[row * 4 + i] = ucmd[i];
        if (A.status_log) A.status_log[row] = A.status[b];
        if (A.iters_log) A.iters_log[row] = A.iters[b];
        if (A.pts_log) log_point(pr, x, A.pts_log + (b * (A.K + 1) + A.k + 1) * 3);
        if (V.xhat_log) {
            double* hl = V.xhat_log + (b * (A.K + 1) + A.k + 1) * 10;
#pragma unroll
            for (int i = 0; i < 10; ++i) hl[i] = xe[i];
        }
        if (V.uapp_log) {
#pragma unroll
            for (int i = 0; i < 4; ++i) V.uapp_log[row * 4 + i] = u[i];
        }
    }
}

__global__ __launch_bounds__(64) void vehicle_begin_kernel(VehicleArgs V) {
    const long long b = (long long)blockIdx.x * 64 + threadIdx.x;
    if (b >= V.P.B) return;
    double x[10], xe[10];
#pragma unroll
    for (int i = 0; i < 10; ++i) x[i] = V.x_est[b * 10 + i];
    vehicle_estimate(V, b, V.frame, x, xe);
#pragma unroll
    for (int i = 0; i < 10; ++i) {
        V.P.x_next[b * 10 + i] = x[i];
        V.x_est[b * 10 + i] = xe[i];
    }
}

__global__ __launch_bounds__(64) void vehicle_reset_kernel(VehicleArgs V) {
    const long long b = (long long)blockIdx.x * 64 + threadIdx.x;
    if (b >= V.P.B) return;
    V.gamma_act[b] = V.g;
#pragma unroll
    for (int i = 0; i < 3; ++i) V.w[b * 3 + i] = 0.0;
    for (int j = 0; j < V.delay; ++j) {
        double* slot = V.ring + (b * V.delay + j) * 4;
        slot[0] = V.hover_u0;
        slot[1] = slot[2] = slot[3] = 0.0;
    }
}

hipError_t launch_vehicle(const VehicleArgs& a, hipStream_t s) {
    if (a.P.B <= 0) return hipSuccess;
    const dim3 grid((unsigned)((a.P.B + 63) / 64));
    if (a.P.kind == 1)
        hipLaunchKernelGGL(plant_vehicle_kernel<1>, grid, dim3(64), 0, s, a);
    else
        hipLaunchKernelGGL(plant_vehicle_kernel<0>, grid, dim3(64), 0, s, a);
    return hipGetLastError();
}

hipError_t launch_vehicle_begin(const VehicleArgs& a, hipStream_t s) {
    if (a.P.B <= 0) return hipSuccess;
    hipLaunchKernelGGL(vehicle_begin_kernel, dim3((unsigned)((a.P.B + 63) / 64)), dim3(64), 0, s, a);
    return hipGetLastError();
}

hipError_t launch_vehicle_reset(const VehicleArgs& a, hipStream_t s) {
    if (a.P.B <= 0) return hipSuccess;
    hipLaunchKernelGGL(vehicle_reset_kernel, dim3((unsigned)((a.P.B + 63) / 64)), dim3(64), 0, s, a);
    return hipGetLastError();
}

}  // namespace sdfn
