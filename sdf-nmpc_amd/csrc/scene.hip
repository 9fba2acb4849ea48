// Analytic scenes: what a range sensor would see of a known world, rendered on the device from every
// instance's current camera pose, so that a closed-loop rollout can take a new image every control period
// without leaving the device (sdfnmpc_solver_rollout_perceive).  The reference has no counterpart: its images
// come from the simulator it is run against.
//
//   scene_render_kernel    fp32, one pixel per lane: the nearest positive hit of the pixel-centre ray over the
//                          instance's primitives (spheres, axis-aligned boxes, capped z-cylinders), written as
//                          min(range or depth, dmax) * scale -- the pixel grid and camera frame of
//                          colcheck_kernel (df_truth.hip; collision_checker.py:80-84), x forward, y left, z up
//   scene_pose_kernel      fp64, one instance per lane: state -> body pose and camera pose (controller.py:52-53
//                          with quat2rot(q / |q|) of utils/math.py:7-23)
//   scene_distance_kernel  fp64, one point per lane: the closed-form signed distance to every primitive, the
//                          minimum over the scene (negative inside)
//   scene_render_dyn_kernel, scene_distance_dyn_kernel
//                          the same two for a scene set whose primitives carry a rigid frame (R(t), c(t)): oriented
//                          boxes, tilted cylinders, moving obstacles.  Static sets never reach them.
//
// Every primitive is convex, so a ray meets it in one parameter interval [tn, tf]: the intersection of the
// slab intervals (box), of the quadratic's root interval (sphere), or of both (cylinder: side wall and caps).
// The ray hits when tf >= max(tn, 0), at t = max(tn, 0): an origin inside gives t = 0 for every ray.  No
// atomics, no cross-lane traffic: a pixel depends on its instance's pose and scene only.  The per-primitive work
// (prim_ray_hit, prim_distance) is in scene_dev.h, shared with the grid kernels of scene_grid.hip.
#include "scene_dev.h"

namespace sdfn {

namespace {

__global__ __launch_bounds__(SCENE_BLOCK) void scene_render_kernel(SceneRenderArgs A) {
    extern __shared__ float tab[];  // spherical: col [2 W] (cos, sin of the azimuth) | row [2 H] (elevation)
    __shared__ __attribute__((aligned(16))) ScenePrimF prim[SCENE_MAX_PRIMS];
    __shared__ float pose[12];      // W_p_C | W_R_C, rounded to fp32 once per block
    const int b = blockIdx.y, tid = threadIdx.x;
    const int s = A.scene_of ? min(max(A.scene_of[b], 0), A.sc.S - 1) : 0;  // clamped: never outside the scene set
    const int cnt = min(A.sc.count[s], SCENE_MAX_PRIMS);
    static_assert(SCENE_MAX_PRIMS * sizeof(ScenePrimF) / 4 <= SCENE_BLOCK, "one staging pass");
    if (tid < cnt * 8) ((int*)prim)[tid] = ((const int*)(A.sc.pf + (size_t)s * SCENE_MAX_PRIMS))[tid];
    if (tid < 3) pose[tid] = (float)A.W_p_C[(size_t)b * 3 + tid];
    else if (tid < 12) pose[tid] = (float)A.W_R_C[(size_t)b * 9 + (tid - 3)];
    const int w = A.W, h = A.H;
    if (A.is_spherical) {  // the pixel-centre angles depend on the launch only: separably, w + h entries
        for (int t = tid; t < w + h; t += SCENE_BLOCK) {
            const bool is_col = t < w;
            const int i = is_col ? t : t - w;
            const float f = 1.f - (float)(2 * i + 1) / (float)(is_col ? w : h);
            const float ang = (is_col ? A.hfov : A.vfov) * f;
            float* dst = is_col ? tab + 2 * t : tab + 2 * w + 2 * i;
            dst[0] = cosf(ang);
            dst[1] = sinf(ang);
        }
    }
    __syncthreads();
    const long long pix = (long long)blockIdx.x * SCENE_BLOCK + tid;
    if (pix >= (long long)h * w) return;
    const int v = (int)(pix / w), u = (int)(pix - (long long)v * w);

    // unit ray direction in the camera frame, then in the world frame
    float cx, cy, cz;
    if (A.is_spherical) {
        const float ca = tab[2 * u], sa = tab[2 * u + 1], ce = tab[2 * w + 2 * v], se = tab[2 * w + 2 * v + 1];
        cx = ce * ca;
        cy = ce * sa;
        cz = se;
    } else {
        const float ty = fmaf(A.ty1, (float)u, A.ty0), tz = fmaf(A.tz1, (float)v, A.tz0);
        cx = __builtin_amdgcn_rsqf(fmaf(ty, ty, fmaf(tz, tz, 1.f)));
        cy = ty * cx;
        cz = tz * cx;
    }
    const float ox = pose[0], oy = pose[1], oz = pose[2];
    const float dx = fmaf(pose[3], cx, fmaf(pose[4], cy, pose[5] * cz));
    const float dy = fmaf(pose[6], cx, fmaf(pose[7], cy, pose[8] * cz));
    const float dz = fmaf(pose[9], cx, fmaf(pose[10], cy, pose[11] * cz));
    const float ix = frcp(dx), iy = frcp(dy), iz = frcp(dz);

    float best = INFINITY;
    for (int i = 0; i < cnt; ++i) {  // wave-uniform: one scene per block
        best = prim_ray_hit(best, prim[i].kind, prim[i].a[0], prim[i].a[1], prim[i].a[2], prim[i].a[3], prim[i].a[4],
                            prim[i].a[5], ox, oy, oz, dx, dy, dz, ix, iy, iz);
    }
    float val = A.dmax;  // a miss
    if (best < INFINITY) val = fminf(A.is_depth ? best * cx : best, A.dmax);
    A.img[((size_t)b * h + v) * w + u] = val * A.scale;
}

// W_R_Bo = quat2rot(q / |q|) (utils/math.py:7-23), W_p_C = W_R_Bo B_p_C + W_p_Bo, W_R_C = W_R_Bo B_R_C
// (controller.py:52-53)
__global__ __launch_bounds__(64) void scene_pose_kernel(ScenePoseArgs A) {
    const long long b = (long long)blockIdx.x * 64 + threadIdx.x;
    if (b >= A.B) return;
    const double* x = A.x + b * 10;
    const double n = sqrt(x[3] * x[3] + x[4] * x[4] + x[5] * x[5] + x[6] * x[6]);
    const double q0 = x[3] / n, q1 = x[4] / n, q2 = x[5] / n, q3 = x[6] / n;
    double R[9];
    R[0] = q0 * q0 + q1 * q1 - q2 * q2 - q3 * q3;
    R[1] = 2 * (q1 * q2 - q0 * q3);
    R[2] = 2 * (q1 * q3 + q0 * q2);
    R[3] = 2 * (q1 * q2 + q0 * q3);
    R[4] = q0 * q0 - q1 * q1 + q2 * q2 - q3 * q3;
    R[5] = 2 * (q2 * q3 - q0 * q1);
    R[6] = 2 * (q1 * q3 - q0 * q2);
    R[7] = 2 * (q2 * q3 + q0 * q1);
    R[8] = q0 * q0 - q1 * q1 - q2 * q2 + q3 * q3;
#pragma unroll
    for (int i = 0; i < 3; ++i) {
        A.W_p_Bo[b * 3 + i] = x[i];
        A.W_p_C[b * 3 + i] = (R[i * 3] * A.B_p_C[0] + R[i * 3 + 1] * A.B_p_C[1] + R[i * 3 + 2] * A.B_p_C[2]) + x[i];
#pragma unroll
        for (int j = 0; j < 3; ++j) {
            A.W_R_Bo[b * 9 + i * 3 + j] = R[i * 3 + j];
            A.W_R_C[b * 9 + i * 3 + j] =
                R[i * 3] * A.B_R_C[j] + R[i * 3 + 1] * A.B_R_C[3 + j] + R[i * 3 + 2] * A.B_R_C[6 + j];
        }
    }
}

__global__ __launch_bounds__(SCENE_BLOCK) void scene_distance_kernel(SceneDistArgs A) {
    const long long j = (long long)blockIdx.x * SCENE_BLOCK + threadIdx.x;
    if (j >= A.n) return;
    const long long s = A.p_to_scene ? (long long)min(max(A.p_to_scene[j], 0), A.sc.S - 1) : j / A.per_scene;
    const ScenePrimD* P = A.sc.pd + s * SCENE_MAX_PRIMS;
    const int cnt = min(A.sc.count[s], SCENE_MAX_PRIMS);
    const double px = A.points[j * 3], py = A.points[j * 3 + 1], pz = A.points[j * 3 + 2];
    double best = INFINITY;
    for (int i = 0; i < cnt; ++i) best = fmin(best, prim_distance(P[i], px, py, pz));
    A.out[j] = best;
}

// ---- primitives with a frame that is a function of time (oriented and moving obstacles): prim_frame, scene_dev.h

// scene_render_kernel for a dynamic scene set: the same launch geometry, rays, hit rule and output.  Lane i < cnt
// of a block forms primitive i's frame at time t in fp64 and stores the camera in that frame, o' = R(t)^T (W_p_C -
// c(t)) and M = R(t)^T W_R_C, rounded to fp32 once (world-scale coordinates cancel in fp64, before the rounding).
// Every lane then takes its camera-frame direction into the primitive's frame, d' = M d_cam, and runs the interval
// tests of scene_render_kernel on the canonical centred shape.  A primitive without motion is R = I, v = 0 here.
__global__ __launch_bounds__(SCENE_BLOCK) void scene_render_dyn_kernel(SceneRenderDynArgs D) {
    extern __shared__ float tab[];  // spherical: col [2 W] | row [2 H], as in scene_render_kernel
    __shared__ __attribute__((aligned(16))) ScenePrimFrame fr[SCENE_MAX_PRIMS];
    static_assert(sizeof(ScenePrimFrame) == 64, "four 16-byte reads");
    const SceneRenderArgs& A = D.r;
    const int b = blockIdx.y, tid = threadIdx.x;
    const int s = A.scene_of ? min(max(A.scene_of[b], 0), A.sc.S - 1) : 0;
    const int cnt = min(A.sc.count[s], SCENE_MAX_PRIMS);
    if (tid < cnt)
        fr[tid] = prim_camera_frame(D.dyn[(size_t)s * SCENE_MAX_PRIMS + tid], D.t, A.W_p_C + (size_t)b * 3,
                                    A.W_R_C + (size_t)b * 9);
    const int w = A.W, h = A.H;
    if (A.is_spherical) {
        for (int t = tid; t < w + h; t += SCENE_BLOCK) {
            const bool is_col = t < w;
            const int i = is_col ? t : t - w;
            const float f = 1.f - (float)(2 * i + 1) / (float)(is_col ? w : h);
            const float ang = (is_col ? A.hfov : A.vfov) * f;
            float* dst = is_col ? tab + 2 * t : tab + 2 * w + 2 * i;
            dst[0] = cosf(ang);
            dst[1] = sinf(ang);
        }
    }
    __syncthreads();
    const long long pix = (long long)blockIdx.x * SCENE_BLOCK + tid;
    if (pix >= (long long)h * w) return;
    const int v = (int)(pix / w), u = (int)(pix - (long long)v * w);

    float cx, cy, cz;  // unit ray direction in the camera frame
    if (A.is_spherical) {
        const float ca = tab[2 * u], sa = tab[2 * u + 1], ce = tab[2 * w + 2 * v], se = tab[2 * w + 2 * v + 1];
        cx = ce * ca;
        cy = ce * sa;
        cz = se;
    } else {
        const float ty = fmaf(A.ty1, (float)u, A.ty0), tz = fmaf(A.tz1, (float)v, A.tz0);
        cx = __builtin_amdgcn_rsqf(fmaf(ty, ty, fmaf(tz, tz, 1.f)));
        cy = ty * cx;
        cz = tz * cx;
    }

    float best = INFINITY;
    for (int i = 0; i < cnt; ++i) {  // wave-uniform: one scene per block
        best = frame_ray_hit(best, fr[i], cx, cy, cz);
    }
    float val = A.dmax;  // a miss
    if (best < INFINITY) val = fminf(A.is_depth ? best * cx : best, A.dmax);
    A.img[((size_t)b * h + v) * w + u] = val * A.scale;
}

// scene_distance_kernel for a dynamic scene set: the point is taken into every primitive's frame at the point's own
// time, q = R(t)^T (p - c(t)), then the same closed forms on the canonical shape
__global__ __launch_bounds__(SCENE_BLOCK) void scene_distance_dyn_kernel(SceneDistDynArgs D) {
    const SceneDistArgs& A = D.d;
    const long long j = (long long)blockIdx.x * SCENE_BLOCK + threadIdx.x;
    if (j >= A.n) return;
    const long long s = A.p_to_scene ? (long long)min(max(A.p_to_scene[j], 0), A.sc.S - 1) : j / A.per_scene;
    const ScenePrimDyn* P = D.dyn + s * SCENE_MAX_PRIMS;
    const int cnt = min(A.sc.count[s], SCENE_MAX_PRIMS);
    const double t = D.times ? D.times[j] : 0.0;
    const double px = A.points[j * 3], py = A.points[j * 3 + 1], pz = A.points[j * 3 + 2];
    double best = INFINITY;
    for (int i = 0; i < cnt; ++i) best = fmin(best, frame_distance(P[i], t, px, py, pz));
    A.out[j] = best;
}

}  // namespace

hipError_t launch_scene_render_dyn(const SceneRenderDynArgs& a, hipStream_t s) {
    if (a.r.B <= 0) return hipSuccess;
    const long long tiles = ((long long)a.r.H * a.r.W + SCENE_BLOCK - 1) / SCENE_BLOCK;
    hipLaunchKernelGGL(scene_render_dyn_kernel, dim3((unsigned)tiles, (unsigned)a.r.B), dim3(SCENE_BLOCK),
                       scene_render_lds_bytes(a.r.H, a.r.W, a.r.is_spherical), s, a);
    return hipGetLastError();
}

hipError_t launch_scene_distance_dyn(const SceneDistDynArgs& a, hipStream_t s) {
    if (a.d.n <= 0) return hipSuccess;
    hipLaunchKernelGGL(scene_distance_dyn_kernel, dim3((unsigned)((a.d.n + SCENE_BLOCK - 1) / SCENE_BLOCK)),
                       dim3(SCENE_BLOCK), 0, s, a);
    return hipGetLastError();
}

hipError_t launch_scene_render(const SceneRenderArgs& a, hipStream_t s) {
    if (a.B <= 0) return hipSuccess;
    const long long tiles = ((long long)a.H * a.W + SCENE_BLOCK - 1) / SCENE_BLOCK;
    hipLaunchKernelGGL(scene_render_kernel, dim3((unsigned)tiles, (unsigned)a.B), dim3(SCENE_BLOCK),
                       scene_render_lds_bytes(a.H, a.W, a.is_spherical), s, a);
    return hipGetLastError();
}

hipError_t launch_scene_pose(const ScenePoseArgs& a, hipStream_t s) {
    if (a.B <= 0) return hipSuccess;
    hipLaunchKernelGGL(scene_pose_kernel, dim3((unsigned)((a.B + 63) / 64)), dim3(64), 0, s, a);
    return hipGetLastError();
}

hipError_t launch_scene_distance(const SceneDistArgs& a, hipStream_t s) {
    if (a.n <= 0) return hipSuccess;
    hipLaunchKernelGGL(scene_distance_kernel, dim3((unsigned)((a.n + SCENE_BLOCK - 1) / SCENE_BLOCK)), dim3(SCENE_BLOCK),
                       0, s, a);
    return hipGetLastError();
}

}  // namespace sdfn
