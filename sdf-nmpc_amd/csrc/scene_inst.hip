// Instanced mesh scenes: the render, the distance and the SDF rows of an instanced set (sdfnmpc_scene_create_instanced).
// A scene is a list of up to SCENE_MAX_INSTANCES instances, each a part of the set's pool -- a triangle mesh behind its
// own hierarchy (mesh_bvh.h), stored once -- placed by a rigid frame that is a function of time, c(t) = p + v t + amp
// sin(omega t + phase), R(t) = Rz(yaw_rate t) R(q): prim_frame's, in fp64.  The swept clearance of such a set is
// scene_swept.hip's kernel over inst_distance (inst_dev.h).
//
//   scene_render_inst_kernel    fp32, one pixel per lane, one image per blockIdx.y: scene_render_mesh_kernel's pixel
//                               grid, rays, clipping, range and depth values and scale.  The block stages every
//                               instance's camera frame (o' = R(t)^T (W_p_C - c(t)), M = R(t)^T W_R_C, formed in fp64
//                               and rounded once, as prim_camera_frame does) and part in LDS; each lane loops over the
//                               instances, takes its ray into the frame, d' = M d_cam, and walks the part from the best
//                               hit so far (mesh_ray_cast): the root's slab test is the cull of the instance.  A rigid
//                               frame keeps the ray parameter, so the hits of all instances compare as they are.
//   scene_distance_inst_kernel  fp64, one point per lane at its own time: inst_distance
//   scene_sdf_rows_inst_kernel  fp64, one node row per lane: the value and the gradient R(t) g' of the minimising
//                               instance (the lowest index on a tie), in scene_sdf_rows_mesh_kernel's row contract
//
// The top level is a linear pass: at most 256 instances per scene, read by every lane in the same order.  One scene per
// block in the render kernel, so the staged frames are LDS broadcast reads and the part's header is wave-uniform; in
// the fp64 kernels the lanes of a wave diverge only inside the walks.  No atomics and no cross-lane traffic: an image
// is a pure function of its pose, scene and time.  Hits are double-sided and edge-consistent, with no "inside sees
// zero" convention (scene_mesh.hip).  A scene without instances renders a miss everywhere and is at distance +inf.
#include "inst_dev.h"

namespace sdfn {

namespace {

__global__ __launch_bounds__(SCENE_BLOCK) void scene_render_inst_kernel(InstRenderArgs D) {
    extern __shared__ float tab[];  // spherical: col [2 W] | row [2 H], as in scene_render_kernel
    __shared__ __attribute__((aligned(16))) SceneInstFrame fr[SCENE_MAX_INSTANCES];
    const SceneRenderArgs& A = D.r;
    const int b = blockIdx.y, tid = threadIdx.x;
    const int s = A.scene_of ? min(max(A.scene_of[b], 0), A.sc.S - 1) : 0;  // clamped: never outside the scene set
    const InstRange sc = inst_range(D.inst, s);
    static_assert(SCENE_MAX_INSTANCES <= SCENE_BLOCK, "one lane stages one instance");
    if (tid < sc.cnt) {
        const ScenePrimDyn& P = sc.rec[tid];
        const ScenePrimFrame F = prim_camera_frame(P, D.t, A.W_p_C + (size_t)b * 3, A.W_R_C + (size_t)b * 9);
        SceneInstFrame G;
#pragma unroll
        for (int j = 0; j < 3; ++j) G.o[j] = F.o[j];
#pragma unroll
        for (int j = 0; j < 9; ++j) G.M[j] = F.M[j];
        G.part = inst_part(D.inst, P);
        G.pad[0] = G.pad[1] = G.pad[2] = 0;
        fr[tid] = G;
    }
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
    float best = INFINITY;
    for (int i = 0; i < sc.cnt; ++i) {  // block-uniform: one scene per block, every lane reads the same frame
        const float4* q = (const float4*)&fr[i];
        const float4 q0 = q[0], q1 = q[1], q2 = q[2];
        const float m8 = fr[i].M[8];
        const int part = __builtin_amdgcn_readfirstlane(__float_as_int(q0.w));
        // the ray in the instance's frame, scene_render_mesh_kernel's expressions with (o', M) for (W_p_C, W_R_C)
        const float ox = q0.x, oy = q0.y, oz = q0.z;
        const float dx = fmaf(q1.x, cx, fmaf(q1.y, cy, q1.z * cz));
        const float dy = fmaf(q1.w, cx, fmaf(q2.x, cy, q2.y * cz));
        const float dz = fmaf(q2.z, cx, fmaf(q2.w, cy, m8 * cz));
        const float ix = frcp(dx), iy = frcp(dy), iz = frcp(dz);
        const MeshHdr hd = D.mesh.hdr[part];
        best = mesh_ray_cast(D.mesh, hd, ox, oy, oz, dx, dy, dz, ix, iy, iz, best);
    }
    float val = A.dmax;  // a miss
    if (best < INFINITY) val = fminf(A.is_depth ? best * cx : best, A.dmax);
    A.img[((size_t)b * h + v) * w + u] = val * A.scale;
}

__global__ __launch_bounds__(SCENE_BLOCK) void scene_distance_inst_kernel(InstDistArgs D) {
    const SceneDistArgs& A = D.d;
    const long long j = (long long)blockIdx.x * SCENE_BLOCK + threadIdx.x;
    if (j >= A.n) return;
    const long long s = A.p_to_scene ? (long long)min(max(A.p_to_scene[j], 0), A.sc.S - 1) : j / A.per_scene;
    A.out[j] = inst_distance(D.mesh, D.inst, inst_range(D.inst, s), D.times ? D.times[j] : 0.0, A.points[j * 3],
                             A.points[j * 3 + 1], A.points[j * 3 + 2]);
}

// scene_sdf_rows_mesh_kernel's row from the nearest instance at the node's time t0 + tau[k].  Per instance the row's
// (d, near) is formed as that kernel forms it, and an instance replaces the best only when its d is strictly smaller:
// the lowest index keeps a tie.  An open set searches instance i up to min(max_df, best) in the squared form of
// inst_distance -- a triangle beyond that bound has a rounded root >= max_df, and is truncated, or strictly above best;
// a closed set skips an instance whose root box is strictly beyond that (inst_skip_closed) and otherwise takes the full
// walk, for the sign.  The gradient of the winner is g' of mesh_gradient in the part's frame, taken to the world by
// R(t) (frame_grad_world).
__global__ __launch_bounds__(SCENE_BLOCK) void scene_sdf_rows_inst_kernel(InstSdfArgs D) {
#pragma clang fp contract(off)
    const SceneSdfArgs& A = D.a;
    const long long r = (long long)blockIdx.x * SCENE_BLOCK + threadIdx.x;
    if (r >= A.rows) return;
    const long long b = r / A.N1;
    const int k = (int)(r - b * A.N1);
    const long long s = A.scene_of ? (long long)min(max(A.scene_of[b], 0), A.sc.S - 1) : 0;
    const InstRange sc = inst_range(D.inst, s);
    const double* xr = A.x + r * 10;
    const double px = xr[0], py = xr[1], pz = xr[2];
    const double t = A.tau ? A.t0 + A.tau[k] : A.t0;
    double df = A.max_df, gx = 0.0, gy = 0.0, gz = 0.0;  // nothing near: the truncated row
    for (int i = 0; i < sc.cnt; ++i) {
        const ScenePrimDyn& P = sc.rec[i];
        const MeshHdr hd = A.mesh.hdr[inst_part(D.inst, P)];
        double R[9], qx, qy, qz;
        frame_point(P, t, px, py, pz, R, qx, qy, qz);
        MeshHit w;
        if (A.mesh.tn) {
            if (inst_skip_closed(A.mesh, hd, qx, qy, qz, df, A.max_df)) continue;
            w = mesh_search(A.mesh, hd, qx, qy, qz, (double)INFINITY);
        } else {
            const double b2 = df * df * (1.0 + 0x1p-50);  // df <= max_df, and >= 0 for an open set
            if (inst_far(A.mesh, hd, qx, qy, qz, b2)) continue;
            w = mesh_search(A.mesh, hd, qx, qy, qz, b2);
        }
        const double d = mesh_value(A.mesh, hd, w, qx, qy, qz);
        // near as scene_sdf_rows_mesh_kernel has it, and strictly below the best: df starts at max_df
        if (!(w.d2 < INFINITY && d < df)) continue;
        double ax, ay, az;
        mesh_gradient(A.mesh, hd, w, d, qx, qy, qz, ax, ay, az);
        df = d;
        frame_grad_world(R, ax, ay, az, gx, gy, gz);
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

hipError_t launch_scene_render_inst(const InstRenderArgs& a, hipStream_t s) {
    if (a.r.B <= 0) return hipSuccess;
    const long long tiles = ((long long)a.r.H * a.r.W + SCENE_BLOCK - 1) / SCENE_BLOCK;
    hipLaunchKernelGGL(scene_render_inst_kernel, dim3((unsigned)tiles, (unsigned)a.r.B), dim3(SCENE_BLOCK),
                       scene_render_lds_bytes(a.r.H, a.r.W, a.r.is_spherical), s, a);
    return hipGetLastError();
}

hipError_t launch_scene_distance_inst(const InstDistArgs& a, hipStream_t s) {
    if (a.d.n <= 0) return hipSuccess;
    hipLaunchKernelGGL(scene_distance_inst_kernel, dim3((unsigned)((a.d.n + SCENE_BLOCK - 1) / SCENE_BLOCK)),
                       dim3(SCENE_BLOCK), 0, s, a);
    return hipGetLastError();
}

hipError_t launch_scene_sdf_rows_inst(const InstSdfArgs& a, hipStream_t s) {
    if (a.a.rows <= 0) return hipSuccess;
    hipLaunchKernelGGL(scene_sdf_rows_inst_kernel, dim3((unsigned)((a.a.rows + SCENE_BLOCK - 1) / SCENE_BLOCK)),
                       dim3(SCENE_BLOCK), 0, s, a);
    return hipGetLastError();
}

}  // namespace sdfn
