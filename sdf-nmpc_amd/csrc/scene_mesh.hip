// Triangle-mesh scenes: the render, the distance and the SDF rows of a mesh set (sdfnmpc_scene_create_mesh), each scene
// a static triangle mesh behind a bounding-volume hierarchy that the host built once (mesh_bvh.h).  The swept clearance
// of a mesh set is scene_swept.hip's kernel over mesh_distance.
//
//   scene_render_mesh_kernel    fp32, one pixel per lane: the pixel grid, pose rounding, range and depth values, clipping
//                               at dmax, scale and block shape of scene_render_kernel; the nearest hit over the
//                               scene's triangles by a stackless preorder walk (mesh_dev.h).  No atomics, no
//                               cross-lane traffic: a pixel depends on its instance's pose and scene only, so the
//                               image is bitwise reproducible and independent of the instance's place in the batch.
//   scene_distance_mesh_kernel  fp64, one point per lane: the distance to the nearest triangle, unsigned for an open
//                               set, signed by the pseudonormal of the nearest feature for a closed one.
//   scene_sdf_rows_mesh_kernel  fp64, one node row per lane: that distance and its gradient as the preparation phase's SDF
//                               row, in scene_sdf_rows_kernel's contract (a set created with sdf_source = 1).
//   scene_render_mesh_mixed_kernel, scene_distance_mesh_mixed_kernel, scene_sdf_rows_mesh_mixed_kernel
//                               the same three for a mesh set with movers (sdfnmpc_scene_create_mesh_mixed): up to 32
//                               movers beside the mesh, evaluated first, and the walks above started from what they give
//
// A mesh is a surface, not a solid: hits are double-sided (front and back faces) with t >= 0, and there is no "camera
// inside sees zero" convention as the primitives have -- a camera inside a closed mesh sees its inner walls.  The hit
// test is edge-consistent (mesh_dev.h), so no ray passes between two triangles that share an edge.  A scene without
// triangles renders a miss everywhere and is at distance +inf.
#include "mesh_dev.h"

namespace sdfn {

namespace {

__global__ __launch_bounds__(SCENE_BLOCK) void scene_render_mesh_kernel(MeshRenderArgs D) {
    extern __shared__ float tab[];  // spherical: col [2 W] | row [2 H], as in scene_render_kernel
    __shared__ float pose[12];      // W_p_C | W_R_C, rounded to fp32 once per block
    const SceneRenderArgs& A = D.r;
    const int b = blockIdx.y, tid = threadIdx.x;
    const int s = A.scene_of ? min(max(A.scene_of[b], 0), A.sc.S - 1) : 0;  // clamped: never outside the scene set
    if (tid < 3) pose[tid] = (float)A.W_p_C[(size_t)b * 3 + tid];
    else if (tid < 12) pose[tid] = (float)A.W_R_C[(size_t)b * 9 + (tid - 3)];
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

    const MeshHdr hd = D.mesh.hdr[s];  // wave-uniform: one scene per block
    const float best = mesh_ray_cast(D.mesh, hd, ox, oy, oz, dx, dy, dz, ix, iy, iz);
    float val = A.dmax;  // a miss
    if (best < INFINITY) val = fminf(A.is_depth ? best * cx : best, A.dmax);
    A.img[((size_t)b * h + v) * w + u] = val * A.scale;
}

__global__ __launch_bounds__(SCENE_BLOCK) void scene_distance_mesh_kernel(MeshDistArgs D) {
    const SceneDistArgs& A = D.d;
    const long long j = (long long)blockIdx.x * SCENE_BLOCK + threadIdx.x;
    if (j >= A.n) return;
    const long long s = A.p_to_scene ? (long long)min(max(A.p_to_scene[j], 0), A.sc.S - 1) : j / A.per_scene;
    const MeshHdr hd = D.mesh.hdr[s];
    A.out[j] = mesh_distance(D.mesh, hd, A.points[j * 3], A.points[j * 3 + 1], A.points[j * 3 + 2]);
}

// The rows contract of scene_sdf_rows_kernel (scene_sdf.hip) from a mesh set: truncation at max_df, the flag, column 2
// of h and of the ten Jacobian columns and nothing else.  t0 and tau are not read: a mesh set is static.
//
// An open set prunes at max_df: the search starts at the bound b0 = max_df^2 (1 + 2^-50) with no winner.  b0 as
// rounded is still > max_df^2 (two roundings of 2^-53 each against 2^-50), so a triangle with d2 > b0 has an exact
// root > max_df, its rounded root is >= max_df and the row would be truncated anyway; every triangle with d2 <= b0 is
// searched as in the full walk (mesh_search).  So the row is that of the full search followed by the truncation, bit
// for bit and for every hierarchy, and a row in free space opens no node beyond max_df.  A closed set takes the full
// walk: a point deeper than max_df inside a solid has d < max_df and keeps its value, and telling it from a point far
// outside needs the sign, which needs the nearest triangle.
__global__ __launch_bounds__(SCENE_BLOCK) void scene_sdf_rows_mesh_kernel(SceneSdfArgs A) {
#pragma clang fp contract(off)
    const long long r = (long long)blockIdx.x * SCENE_BLOCK + threadIdx.x;
    if (r >= A.rows) return;
    const long long b = r / A.N1;
    const long long s = A.scene_of ? (long long)min(max(A.scene_of[b], 0), A.sc.S - 1) : 0;
    const MeshHdr hd = A.mesh.hdr[s];
    const double* xr = A.x + r * 10;
    const double px = xr[0], py = xr[1], pz = xr[2];
    const double b0 = A.max_df * A.max_df * (1.0 + 0x1p-50);
    const MeshHit w = mesh_search(A.mesh, hd, px, py, pz, A.mesh.tn ? (double)INFINITY : b0);
    const double d = mesh_value(A.mesh, hd, w, px, py, pz);
    // not near without a winner (d2 = +inf: no triangles, none within b0, a NaN in the row) and for an infinite
    // coordinate, whose d2 is +inf or NaN and whose sign means nothing
    const bool near = w.d2 < INFINITY && d < A.max_df;
    const double df = near ? d : A.max_df;
    double gx = 0.0, gy = 0.0, gz = 0.0;
    if (near) mesh_gradient(A.mesh, hd, w, d, px, py, pz, gx, gy, gz);
    const double flag = A.p[r * A.np];
    A.h[r * 3 + 2] = flag * df + (1.0 - flag) * A.max_df;
    double* J = A.Jh + r * 30 + 2;
    J[0] = flag * gx;
    J[3] = flag * gy;
    J[6] = flag * gz;
#pragma unroll
    for (int j = 3; j < 10; ++j) J[j * 3] = 0.0;
}

// ---- mesh sets with movers (sdfnmpc_scene_create_mesh_mixed): the mesh plus mcount[s] <= SCENE_MAX_PRIMS movers
// (ScenePrimDyn records at a stride of SCENE_MAX_PRIMS, not in the hierarchy).  Every query is the minimum over both at
// the query's time.  The movers are evaluated first, by the functions the dynamic kernels call, and the walk of the
// hierarchy starts from what they give.

// scene_render_mesh_kernel's launch geometry, rays and output; lanes < mcount stage the movers' frames at time t as
// scene_render_mixed_kernel does, and the ray walk is seeded with the movers' nearest hit
__global__ __launch_bounds__(SCENE_BLOCK) void scene_render_mesh_mixed_kernel(MeshRenderMixedArgs D) {
    extern __shared__ float tab[];  // spherical: col [2 W] | row [2 H], as in scene_render_kernel
    __shared__ __attribute__((aligned(16))) ScenePrimFrame fr[SCENE_MAX_PRIMS];
    __shared__ float pose[12];      // W_p_C | W_R_C, rounded to fp32 once per block
    const SceneRenderArgs& A = D.r;
    const int b = blockIdx.y, tid = threadIdx.x;
    const int s = A.scene_of ? min(max(A.scene_of[b], 0), A.sc.S - 1) : 0;  // clamped: never outside the scene set
    const int mcnt = min(max(D.mcount[s], 0), SCENE_MAX_PRIMS);
    if (tid < mcnt)
        fr[tid] = prim_camera_frame(D.dyn[(size_t)s * SCENE_MAX_PRIMS + tid], D.t, A.W_p_C + (size_t)b * 3,
                                    A.W_R_C + (size_t)b * 9);
    if (tid < 3) pose[tid] = (float)A.W_p_C[(size_t)b * 3 + tid];
    else if (tid < 12) pose[tid] = (float)A.W_R_C[(size_t)b * 9 + (tid - 3)];
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

    float cx, cy, cz;  // unit ray direction in the camera frame: scene_render_kernel's expressions
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
    float best = INFINITY;  // a camera inside a mover sees zero; the mesh has no such rule, and the minimum keeps the zero
    for (int i = 0; i < mcnt; ++i) best = frame_ray_hit(best, fr[i], cx, cy, cz);  // wave-uniform: one scene per block

    const float ox = pose[0], oy = pose[1], oz = pose[2];
    const float dx = fmaf(pose[3], cx, fmaf(pose[4], cy, pose[5] * cz));
    const float dy = fmaf(pose[6], cx, fmaf(pose[7], cy, pose[8] * cz));
    const float dz = fmaf(pose[9], cx, fmaf(pose[10], cy, pose[11] * cz));
    const float ix = frcp(dx), iy = frcp(dy), iz = frcp(dz);
    const MeshHdr hd = D.mesh.hdr[s];  // wave-uniform: one scene per block
    best = mesh_ray_cast(D.mesh, hd, ox, oy, oz, dx, dy, dz, ix, iy, iz, best);
    float val = A.dmax;  // a miss
    if (best < INFINITY) val = fminf(A.is_depth ? best * cx : best, A.dmax);
    A.img[((size_t)b * h + v) * w + u] = val * A.scale;
}

__global__ __launch_bounds__(SCENE_BLOCK) void scene_distance_mesh_mixed_kernel(MeshDistMixedArgs D) {
    const SceneDistArgs& A = D.d;
    const long long j = (long long)blockIdx.x * SCENE_BLOCK + threadIdx.x;
    if (j >= A.n) return;
    const long long s = A.p_to_scene ? (long long)min(max(A.p_to_scene[j], 0), A.sc.S - 1) : j / A.per_scene;
    const MeshHdr hd = D.mesh.hdr[s];
    const int mcnt = min(max(D.mcount[s], 0), SCENE_MAX_PRIMS);
    A.out[j] = mesh_mixed_distance(D.mesh, hd, D.dyn + s * SCENE_MAX_PRIMS, mcnt, D.times ? D.times[j] : 0.0,
                                   A.points[j * 3], A.points[j * 3 + 1], A.points[j * 3 + 2]);
}

// scene_sdf_rows_mesh_kernel's row from the nearer of the mesh and the movers at the node's time t0 + tau[k]; on a tie
// the mesh comes before a mover, within the movers the lowest index wins.  The movers' best and its world gradient are
// kept apart from the mesh's.  An open set is searched up to min(max_df, d_m) in the squared form of the kernel above
// and of mesh_mixed_distance (not at all with d_m < 0): a triangle beyond that bound has a rounded root >= max_df, and
// is truncated, or strictly above d_m, and loses to the mover without a tie; one at or below it is treated as in the
// full search.  A closed set takes the full walk, for the sign.
__global__ __launch_bounds__(SCENE_BLOCK) void scene_sdf_rows_mesh_mixed_kernel(SceneSdfArgs A) {
#pragma clang fp contract(off)
    const long long r = (long long)blockIdx.x * SCENE_BLOCK + threadIdx.x;
    if (r >= A.rows) return;
    const long long b = r / A.N1;
    const int k = (int)(r - b * A.N1);
    const long long s = A.scene_of ? (long long)min(max(A.scene_of[b], 0), A.sc.S - 1) : 0;
    const MeshHdr hd = A.mesh.hdr[s];
    const double* xr = A.x + r * 10;
    const double px = xr[0], py = xr[1], pz = xr[2];
    const ScenePrimDyn* M = A.dyn + s * SCENE_MAX_PRIMS;
    const int mcnt = min(max(A.mcount[s], 0), SCENE_MAX_PRIMS);
    const double t = A.tau ? A.t0 + A.tau[k] : A.t0;
    double mbest = INFINITY, mx = 0.0, my = 0.0, mz = 0.0;
    for (int i = 0; i < mcnt; ++i) {
        double R[9], gx, gy, gz;
        const double d = frame_sd_grad(M[i], t, px, py, pz, R, gx, gy, gz);
        if (d < mbest) {  // the lowest index on a tie
            mbest = d;
            frame_grad_world(R, gx, gy, gz, mx, my, mz);
        }
    }
    const double bd = fmin(A.max_df, mbest);
    MeshHit w{(double)INFINITY, 0.0, 0.0, 0.0, 0, -1};
    if (A.mesh.tn) w = mesh_search(A.mesh, hd, px, py, pz, (double)INFINITY);
    else if (!(bd < 0.0)) w = mesh_search(A.mesh, hd, px, py, pz, bd * bd * (1.0 + 0x1p-50));
    const double d = mesh_value(A.mesh, hd, w, px, py, pz);
    // the mesh's row as scene_sdf_rows_mesh_kernel forms it, the movers' as scene_sdf_rows_kernel does
    const bool near = w.d2 < INFINITY && d < A.max_df;
    double df = near ? d : A.max_df;
    double gx = 0.0, gy = 0.0, gz = 0.0;
    if (near) mesh_gradient(A.mesh, hd, w, d, px, py, pz, gx, gy, gz);
    if (mbest < df) {  // strictly, and so below max_df: the mesh keeps a tie
        df = mbest;
        gx = mx; gy = my; gz = mz;
    }
    const double flag = A.p[r * A.np];
    A.h[r * 3 + 2] = flag * df + (1.0 - flag) * A.max_df;
    double* J = A.Jh + r * 30 + 2;
    J[0] = flag * gx;
    J[3] = flag * gy;
    J[6] = flag * gz;
#pragma unroll
    for (int j = 3; j < 10; ++j) J[j * 3] = 0.0;
}

}  // namespace

hipError_t launch_scene_render_mesh_mixed(const MeshRenderMixedArgs& a, hipStream_t s) {
    if (a.r.B <= 0) return hipSuccess;
    const long long tiles = ((long long)a.r.H * a.r.W + SCENE_BLOCK - 1) / SCENE_BLOCK;
    hipLaunchKernelGGL(scene_render_mesh_mixed_kernel, dim3((unsigned)tiles, (unsigned)a.r.B), dim3(SCENE_BLOCK),
                       scene_render_lds_bytes(a.r.H, a.r.W, a.r.is_spherical), s, a);
    return hipGetLastError();
}

hipError_t launch_scene_distance_mesh_mixed(const MeshDistMixedArgs& a, hipStream_t s) {
    if (a.d.n <= 0) return hipSuccess;
    hipLaunchKernelGGL(scene_distance_mesh_mixed_kernel, dim3((unsigned)((a.d.n + SCENE_BLOCK - 1) / SCENE_BLOCK)),
                       dim3(SCENE_BLOCK), 0, s, a);
    return hipGetLastError();
}

hipError_t launch_scene_sdf_rows_mesh_mixed(const SceneSdfArgs& a, hipStream_t s) {
    if (a.rows <= 0) return hipSuccess;
    hipLaunchKernelGGL(scene_sdf_rows_mesh_mixed_kernel, dim3((unsigned)((a.rows + SCENE_BLOCK - 1) / SCENE_BLOCK)),
                       dim3(SCENE_BLOCK), 0, s, a);
    return hipGetLastError();
}

hipError_t launch_scene_sdf_rows_mesh(const SceneSdfArgs& a, hipStream_t s) {
    if (a.rows <= 0) return hipSuccess;
    hipLaunchKernelGGL(scene_sdf_rows_mesh_kernel, dim3((unsigned)((a.rows + SCENE_BLOCK - 1) / SCENE_BLOCK)),
                       dim3(SCENE_BLOCK), 0, s, a);
    return hipGetLastError();
}

hipError_t launch_scene_render_mesh(const MeshRenderArgs& a, hipStream_t s) {
    if (a.r.B <= 0) return hipSuccess;
    const long long tiles = ((long long)a.r.H * a.r.W + SCENE_BLOCK - 1) / SCENE_BLOCK;
    hipLaunchKernelGGL(scene_render_mesh_kernel, dim3((unsigned)tiles, (unsigned)a.r.B), dim3(SCENE_BLOCK),
                       scene_render_lds_bytes(a.r.H, a.r.W, a.r.is_spherical), s, a);
    return hipGetLastError();
}

hipError_t launch_scene_distance_mesh(const MeshDistArgs& a, hipStream_t s) {
    if (a.d.n <= 0) return hipSuccess;
    hipLaunchKernelGGL(scene_distance_mesh_kernel, dim3((unsigned)((a.d.n + SCENE_BLOCK - 1) / SCENE_BLOCK)),
                       dim3(SCENE_BLOCK), 0, s, a);
    return hipGetLastError();
}

}  // namespace sdfn
