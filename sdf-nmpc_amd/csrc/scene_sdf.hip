// The exact signed distance of an analytic scene as the preparation phase's SDF row: what sdf_mlp.hip's epilogue
// writes from the network (gen_model.py:46-61: h[2] = flag df + (1 - flag) max_df and its position gradient), written
// from the closed forms of scene.hip instead -- the yardstick controller whose distance constraint describes the
// world it flies in.  The reference has no counterpart: its SDF is always the network.
//
//   scene_sdf_rows_kernel<false>   a static scene set: the world-frame primitives of scene_distance_kernel
//   scene_sdf_rows_kernel<true>    a dynamic set: every primitive in its own frame (R(t), c(t)) at the node's time
//                                  t0 + tau[k] (t0 for every node without tau), as scene_distance_dyn_kernel
//
// fp64, one node row r = b (N+1) + k per lane.  The distance of every primitive is the formula scene_distance(_dyn)_
// kernel evaluates; its gradient g in the primitive's frame is taken on the same excesses, and the world gradient is
// R(t) g of the primitive that attains the minimum (the lowest index on a tie).  Truncated as the network's training
// target is (df_train.py:50): d >= max_df, and an empty scene, give df = max_df with a zero gradient.  No atomics, no
// cross-lane traffic: a row depends on its position, its flag, its instance's scene and its time only.  shape_sd and
// prim_sd_grad are in scene_dev.h, shared with scene_sdf_rows_grid_kernel (scene_grid.hip).
#include "scene_dev.h"

namespace sdfn {

namespace {

template <bool DYN>
__global__ __launch_bounds__(SCENE_BLOCK) void scene_sdf_rows_kernel(SceneSdfArgs A) {
    const long long r = (long long)blockIdx.x * SCENE_BLOCK + threadIdx.x;
    if (r >= A.rows) return;
    const long long b = r / A.N1;
    const int k = (int)(r - b * A.N1);
    const long long s = A.scene_of ? (long long)min(max(A.scene_of[b], 0), A.sc.S - 1) : 0;
    const int cnt = min(A.sc.count[s], SCENE_MAX_PRIMS);
    const double* xr = A.x + r * 10;
    const double px = xr[0], py = xr[1], pz = xr[2];
    double best = INFINITY, bx = 0.0, by = 0.0, bz = 0.0;
    if (DYN) {
        const ScenePrimDyn* P = A.dyn + s * SCENE_MAX_PRIMS;
        const double t = A.tau ? A.t0 + A.tau[k] : A.t0;
        for (int i = 0; i < cnt; ++i) {
            double R[9], gx, gy, gz;
            const double d = frame_sd_grad(P[i], t, px, py, pz, R, gx, gy, gz);
            if (d < best) {  // the lowest index on a tie
                best = d;
                frame_grad_world(R, gx, gy, gz, bx, by, bz);
            }
        }
    } else {
        const ScenePrimD* P = A.sc.pd + s * SCENE_MAX_PRIMS;
        for (int i = 0; i < cnt; ++i) {
            double gx, gy, gz;
            const double d = prim_sd_grad(P[i], px, py, pz, gx, gy, gz);
            if (d < best) {
                best = d;
                bx = gx; by = gy; bz = gz;
            }
        }
    }
    const bool near = best < A.max_df;  // false for an empty scene (+inf)
    const double df = near ? best : A.max_df;
    if (!near) bx = by = bz = 0.0;
    // the network epilogue's contract (sdf_mlp.hip): column 2 of h and of the ten Jacobian columns, nothing else
    const double flag = A.p[r * A.np];
    A.h[r * 3 + 2] = flag * df + (1.0 - flag) * A.max_df;
    double* J = A.Jh + r * 30 + 2;
    J[0] = flag * bx;
    J[3] = flag * by;
    J[6] = flag * bz;
#pragma unroll
    for (int j = 3; j < 10; ++j) J[j * 3] = 0.0;
}

}  // namespace

hipError_t launch_scene_sdf_rows(const SceneSdfArgs& a, hipStream_t s) {
    if (a.rows <= 0) return hipSuccess;
    const dim3 grid((unsigned)((a.rows + SCENE_BLOCK - 1) / SCENE_BLOCK));
    if (a.dyn)
        hipLaunchKernelGGL(scene_sdf_rows_kernel<true>, grid, dim3(SCENE_BLOCK), 0, s, a);
    else
        hipLaunchKernelGGL(scene_sdf_rows_kernel<false>, grid, dim3(SCENE_BLOCK), 0, s, a);
    return hipGetLastError();
}

}  // namespace sdfn
