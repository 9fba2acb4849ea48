// The camera-frame position of a node row, shared by every kernel that evaluates a distance field there: the network
// kernels (sdf_mlp.hip, sdf_row.hip, sdf_wide.hip) and the image field (df_truth.hip: img_sdf_rows_kernel).
#pragma once
#include <hip/hip_runtime.h>

namespace sdfn {

// Co_p_B = W_R_Co^T (W_p_B - W_p_Co) in fp64, handed over as fp32 (gen_model.py:46-51).  xr: the row's state
// x[r][0..9] (the world position first), pr: its parameters p[r][0..np) (W_p_Co at 1..3, W_R_Co row-major at 4..12).
__device__ __forceinline__ float4 cam_point(const double* xr, const double* pr) {
    const double* R = pr + 4;
    const double e0 = xr[0] - pr[1], e1 = xr[1] - pr[2], e2 = xr[2] - pr[3];
    return make_float4((float)((e0 * R[0] + e1 * R[3]) + e2 * R[6]), (float)((e0 * R[1] + e1 * R[4]) + e2 * R[7]),
                       (float)((e0 * R[2] + e1 * R[5]) + e2 * R[8]), 0.0f);
}

}  // namespace sdfn
