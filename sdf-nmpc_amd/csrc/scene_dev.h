// Device code shared by the scene kernels (scene.hip, scene_sdf.hip).
#pragma once
#include "scene_kernels.h"

namespace sdfn {

// ---- primitives with a frame that is a function of time (oriented and moving obstacles)
// c(t) = c0 + v t + amp sin(omega t + phase), R(t) = Rz(yaw_rate t) R0 (row-major), in fp64: the one place every
// dynamic kernel takes a primitive's frame from
__device__ __forceinline__ void prim_frame(const ScenePrimDyn& P, double t, double* c, double* R) {
    const double ay = P.yaw_rate * t, ah = P.omega * t + P.phase;
    const double sy = sin(ay), cy = cos(ay), sh = sin(ah);
#pragma unroll
    for (int j = 0; j < 3; ++j) {
        c[j] = P.c0[j] + P.v[j] * t + P.amp[j] * sh;
        R[j] = cy * P.R0[j] - sy * P.R0[3 + j];
        R[3 + j] = sy * P.R0[j] + cy * P.R0[3 + j];
        R[6 + j] = P.R0[6 + j];
    }
}

}  // namespace sdfn
