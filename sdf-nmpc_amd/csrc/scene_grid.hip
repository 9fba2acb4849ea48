// Scenes of thousands of primitives: the three scene queries through a uniform grid (SceneGridHdr, built on the host
// by sdfnmpc_scene_create_large).  Every query is a minimum over the scene's primitives, and a minimum does not depend
// on the order or on how often an element is taken: a kernel here evaluates the shared per-primitive functions of
// scene_dev.h on the primitives of the cells it visits, and stops only when no primitive it has not seen can lie below
// what it holds.  It then returns the bits of the brute-force kernel over the whole scene.
//
//   scene_render_grid_kernel    fp32, one pixel per lane: scene_render_kernel's rays, hit rule and output; a 3-D DDA
//                               from the ray's entry into the grid's box, cell after cell along the ray
//   scene_distance_grid_kernel  fp64, one point per lane: the block of cells around the point's cell, ring by ring
//   scene_sdf_rows_grid_kernel  fp64, one node row per lane: the same search bounded by max_df, with the gradient of
//                               the lowest scene index on a tie (scene_sdf_rows_kernel<false>'s contract)
//   scene_render_mixed_kernel, scene_distance_mixed_kernel, scene_sdf_rows_mixed_kernel
//                               the same three for a mixed set (sdfnmpc_scene_create_mixed): up to 32 movers beside the
//                               grid, evaluated first, and the searches above started from what they give
//
// Why the stops are conservative.  A primitive is listed in every cell its bounding box inflated by
// infl = 2^-10 cell + 2^-12 max |coordinate| overlaps, and the grid's box is padded by 2 infl.
//   Ray: the fp32 hit t of a primitive is max(tn, 0) with tn <= tf over slab and root intervals, so the point o + t d
//   lies within a few ulp of the coordinates' magnitude of every slab of the primitive's bounding box -- whatever the
//   error of t itself, which near a grazing hit is far larger.  The DDA's planes are rounded the same few ulp.  Both
//   are orders below infl, so the cell the DDA is in at parameter t lists the primitive: once the cells visited cover
//   the parameters up to T, every primitive with a hit below T has been tested, and best <= T ends the search.  The
//   comparison still leaves a relative margin of 2^-16.
//   Point: a primitive not listed in the block of cells searched lies, bounding box and inflation, beyond one of the
//   block's faces, and not beyond a face on the grid's boundary, where there is none: its distance exceeds the axis
//   gap from the point to that face by infl, which covers the fp64 rounding of the closed forms many times over.
//
// No atomics, no cross-lane traffic; every cell index is clamped or checked before it is used and every loop has a
// bound from the grid's dimensions, so a non-finite pose or point gives a wrong value, never a wild read.
#include "scene_dev.h"

namespace sdfn {

namespace {

// the cell of an fp32 coordinate in cells, clamped into [0, n): NaN gives 0
__device__ __forceinline__ int cell_f(float u, int n) { return u >= (float)(n - 1) ? n - 1 : (u > 0.f ? (int)u : 0); }

// The DDA of scene_render_grid_kernel (below) as a function of the best it starts from, for scene_render_mixed_kernel:
// best = min(best, the nearest hit of the ray o + t d (ix, iy, iz = rcp(d)) over the indexed primitives of scene s),
// cell after cell from the ray's entry into the grid's box until the cells visited cover the parameters up to
// fminf(best, tstop).  The stop only needs that no primitive it has not tested hits below the parameters covered: the
// best may come from anywhere.  scene_render_grid_kernel keeps its own copy of these lines: calling this function from
// it changed its instruction schedule, and that kernel is to stay what it was.
__device__ __forceinline__ float grid_ray_walk(float best, const SceneDev& sc, int s, float ox, float oy, float oz,
                                               float dx, float dy, float dz, float ix, float iy, float iz, float tstop) {
    const SceneGridHdr& G = sc.ghdr[s];
    const int nx = G.n[0], ny = G.n[1], nz = G.n[2];
    const float gx = (float)G.org[0], gy = (float)G.org[1], gz = (float)G.org[2], gc = (float)G.cell;  // exact
    const float gi = (float)G.inv;
    const ScenePrimF* P = sc.pf + G.prim_off;
    const int* cs = sc.cell_start + G.cell_off;
    const int* items = sc.cell_items;

    float tn = -INFINITY, tf = INFINITY;  // the ray's interval in the grid's box
    slab(gx, fmaf((float)nx, gc, gx), ox, ix, tn, tf);
    slab(gy, fmaf((float)ny, gc, gy), oy, iy, tn, tf);
    slab(gz, fmaf((float)nz, gc, gz), oz, iz, tn, tf);
    const float t0 = fmaxf(tn, 0.f);
    if (G.count > 0 && tn <= tf && tf >= 0.f && t0 <= tstop) {
        int ci = cell_f((fmaf(t0, dx, ox) - gx) * gi, nx);
        int cj = cell_f((fmaf(t0, dy, oy) - gy) * gi, ny);
        int ck = cell_f((fmaf(t0, dz, oz) - gz) * gi, nz);
        // a zero (or NaN) component never crosses a plane of its axis
        const bool mx = fabsf(dx) > 0.f, my = fabsf(dy) > 0.f, mz = fabsf(dz) > 0.f;
        const int sx = dx > 0.f ? 1 : -1, sy = dy > 0.f ? 1 : -1, sz = dz > 0.f ? 1 : -1;
        const int fx = dx > 0.f ? 1 : 0, fy = dy > 0.f ? 1 : 0, fz = dz > 0.f ? 1 : 0;  // the plane ahead of cell c: c + f
        // the parameter of the next plane of each axis, from the plane's index every time: no accumulated drift, and
        // non-decreasing along the walk
        float tx = mx ? (fmaf((float)(ci + fx), gc, gx) - ox) * ix : INFINITY;
        float ty = my ? (fmaf((float)(cj + fy), gc, gy) - oy) * iy : INFINITY;
        float tz = mz ? (fmaf((float)(ck + fz), gc, gz) - oz) * iz : INFINITY;
        const int max_steps = nx + ny + nz + 3;
        for (int it = 0; it < max_steps; ++it) {
            const int id = (ck * ny + cj) * nx + ci;  // ci, cj, ck in range: clamped at entry, checked at every step
            const int k1 = cs[id + 1];
            for (int k = cs[id]; k < k1; ++k) {
                const float4* q = (const float4*)(P + items[k]);
                const float4 q0 = q[0], q1 = q[1];
                best = prim_ray_hit(best, __float_as_int(q1.z), q0.x, q0.y, q0.z, q0.w, q1.x, q1.y, ox, oy, oz, dx, dy,
                                    dz, ix, iy, iz);
            }
            const float te = fminf(tx, fminf(ty, tz));  // the cells so far cover the parameters up to te
            if (!(te * (1.f - 0x1p-16f) < fminf(best, tstop))) break;
            if (tx <= ty && tx <= tz) {
                ci += sx;
                if ((unsigned)ci >= (unsigned)nx) break;
                tx = (fmaf((float)(ci + fx), gc, gx) - ox) * ix;
            } else if (ty <= tz) {
                cj += sy;
                if ((unsigned)cj >= (unsigned)ny) break;
                ty = (fmaf((float)(cj + fy), gc, gy) - oy) * iy;
            } else {
                ck += sz;
                if ((unsigned)ck >= (unsigned)nz) break;
                tz = (fmaf((float)(ck + fz), gc, gz) - oz) * iz;
            }
        }
    }
    return best;
}

__global__ __launch_bounds__(SCENE_BLOCK) void scene_render_grid_kernel(SceneRenderArgs A) {
    extern __shared__ float tab[];  // spherical: col [2 W] (cos, sin of the azimuth) | row [2 H] (elevation)
    __shared__ float pose[12];      // W_p_C | W_R_C, rounded to fp32 once per block
    const int b = blockIdx.y, tid = threadIdx.x;
    const int s = A.scene_of ? min(max(A.scene_of[b], 0), A.sc.S - 1) : 0;  // clamped: never outside the scene set
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

    // unit ray direction in the camera frame, then in the world frame: scene_render_kernel's expressions
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

    const SceneGridHdr& G = A.sc.ghdr[s];
    const int nx = G.n[0], ny = G.n[1], nz = G.n[2];
    const float gx = (float)G.org[0], gy = (float)G.org[1], gz = (float)G.org[2], gc = (float)G.cell;  // exact
    const float gi = (float)G.inv;
    const ScenePrimF* P = A.sc.pf + G.prim_off;
    const int* cs = A.sc.cell_start + G.cell_off;
    const int* items = A.sc.cell_items;

    // beyond tstop every hit gives the pixel of a miss: range fminf(best, dmax); depth fminf(best cx, dmax), where
    // best >= (dmax / cx) (1 + 2^-20) rounds to a product >= dmax, and with cx <= 0 nothing may be cut
    const float tstop = A.is_depth ? (cx > 0.f ? A.dmax * frcp(cx) * 1.000001f : INFINITY) : A.dmax;
    float best = INFINITY;
    float tn = -INFINITY, tf = INFINITY;  // the ray's interval in the grid's box
    slab(gx, fmaf((float)nx, gc, gx), ox, ix, tn, tf);
    slab(gy, fmaf((float)ny, gc, gy), oy, iy, tn, tf);
    slab(gz, fmaf((float)nz, gc, gz), oz, iz, tn, tf);
    const float t0 = fmaxf(tn, 0.f);
    if (G.count > 0 && tn <= tf && tf >= 0.f && t0 <= tstop) {
        int ci = cell_f((fmaf(t0, dx, ox) - gx) * gi, nx);
        int cj = cell_f((fmaf(t0, dy, oy) - gy) * gi, ny);
        int ck = cell_f((fmaf(t0, dz, oz) - gz) * gi, nz);
        // a zero (or NaN) component never crosses a plane of its axis
        const bool mx = fabsf(dx) > 0.f, my = fabsf(dy) > 0.f, mz = fabsf(dz) > 0.f;
        const int sx = dx > 0.f ? 1 : -1, sy = dy > 0.f ? 1 : -1, sz = dz > 0.f ? 1 : -1;
        const int fx = dx > 0.f ? 1 : 0, fy = dy > 0.f ? 1 : 0, fz = dz > 0.f ? 1 : 0;  // the plane ahead of cell c: c + f
        // the parameter of the next plane of each axis, from the plane's index every time: no accumulated drift, and
        // non-decreasing along the walk
        float tx = mx ? (fmaf((float)(ci + fx), gc, gx) - ox) * ix : INFINITY;
        float ty = my ? (fmaf((float)(cj + fy), gc, gy) - oy) * iy : INFINITY;
        float tz = mz ? (fmaf((float)(ck + fz), gc, gz) - oz) * iz : INFINITY;
        const int max_steps = nx + ny + nz + 3;
        for (int it = 0; it < max_steps; ++it) {
            const int id = (ck * ny + cj) * nx + ci;  // ci, cj, ck in range: clamped at entry, checked at every step
            const int k1 = cs[id + 1];
            for (int k = cs[id]; k < k1; ++k) {
                const float4* q = (const float4*)(P + items[k]);
                const float4 q0 = q[0], q1 = q[1];
                best = prim_ray_hit(best, __float_as_int(q1.z), q0.x, q0.y, q0.z, q0.w, q1.x, q1.y, ox, oy, oz, dx, dy,
                                    dz, ix, iy, iz);
            }
            const float te = fminf(tx, fminf(ty, tz));  // the cells so far cover the parameters up to te
            if (!(te * (1.f - 0x1p-16f) < fminf(best, tstop))) break;
            if (tx <= ty && tx <= tz) {
                ci += sx;
                if ((unsigned)ci >= (unsigned)nx) break;
                tx = (fmaf((float)(ci + fx), gc, gx) - ox) * ix;
            } else if (ty <= tz) {
                cj += sy;
                if ((unsigned)cj >= (unsigned)ny) break;
                ty = (fmaf((float)(cj + fy), gc, gy) - oy) * iy;
            } else {
                ck += sz;
                if ((unsigned)ck >= (unsigned)nz) break;
                tz = (fmaf((float)(ck + fz), gc, gz) - oz) * iz;
            }
        }
    }
    float val = A.dmax;  // a miss
    if (best < INFINITY) val = fminf(A.is_depth ? best * cx : best, A.dmax);
    A.img[((size_t)b * h + v) * w + u] = val * A.scale;
}

__global__ __launch_bounds__(SCENE_BLOCK) void scene_distance_grid_kernel(SceneDistArgs A) {
    const long long j = (long long)blockIdx.x * SCENE_BLOCK + threadIdx.x;
    if (j >= A.n) return;
    const long long s = A.p_to_scene ? (long long)min(max(A.p_to_scene[j], 0), A.sc.S - 1) : j / A.per_scene;
    const SceneGridHdr& G = A.sc.ghdr[s];
    const ScenePrimD* P = A.sc.pd + G.prim_off;
    const double px = A.points[j * 3], py = A.points[j * 3 + 1], pz = A.points[j * 3 + 2];
    double best = INFINITY;
    grid_ring_search(
        G, A.sc.cell_start + G.cell_off, A.sc.cell_items, px, py, pz,
        [&](int i) { best = fmin(best, prim_distance(P[i], px, py, pz)); }, [&] { return best; });
    A.out[j] = best;
}

__global__ __launch_bounds__(SCENE_BLOCK) void scene_sdf_rows_grid_kernel(SceneSdfArgs A) {
    const long long r = (long long)blockIdx.x * SCENE_BLOCK + threadIdx.x;
    if (r >= A.rows) return;
    const long long b = r / A.N1;
    const long long s = A.scene_of ? (long long)min(max(A.scene_of[b], 0), A.sc.S - 1) : 0;
    const SceneGridHdr& G = A.sc.ghdr[s];
    const ScenePrimD* P = A.sc.pd + G.prim_off;
    const double* xr = A.x + r * 10;
    const double px = xr[0], py = xr[1], pz = xr[2];
    double best = INFINITY, bx = 0.0, by = 0.0, bz = 0.0;
    int bi = 0x7fffffff;
    grid_ring_search(
        G, A.sc.cell_start + G.cell_off, A.sc.cell_items, px, py, pz,
        [&](int i) {
            double gx, gy, gz;
            const double d = prim_sd_grad(P[i], px, py, pz, gx, gy, gz);
            if (d < best || (d == best && i < bi)) {  // the lowest index of the scene on a tie, whatever the visiting order
                best = d;
                bi = i;
                bx = gx; by = gy; bz = gz;
            }
        },
        [&] { return fmin(best, A.max_df); });  // nothing at max_df or beyond changes the row
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

// ---- mixed sets: the indexed static primitives plus mcount[s] <= SCENE_MAX_PRIMS movers (ScenePrimDyn records at a
// stride of SCENE_MAX_PRIMS, not in the grid).  Every query is the minimum over both sets at the query's time.  The
// movers are evaluated first, by the functions the dynamic kernels call, and what they give bounds the search of the
// grid from its first cell on: the searches' stops hold for a best from anywhere.

// scene_render_grid_kernel's launch geometry, rays and output; lanes < mcount stage the movers' frames at time t as
// scene_render_dyn_kernel does
__global__ __launch_bounds__(SCENE_BLOCK) void scene_render_mixed_kernel(SceneRenderDynArgs D) {
    extern __shared__ float tab[];  // spherical: col [2 W] (cos, sin of the azimuth) | row [2 H] (elevation)
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
    float best = INFINITY;
    for (int i = 0; i < mcnt; ++i) best = frame_ray_hit(best, fr[i], cx, cy, cz);  // wave-uniform: one scene per block

    // the static primitives: a ray that misses the grid's box, or an empty grid, keeps the movers' best
    const float ox = pose[0], oy = pose[1], oz = pose[2];
    const float dx = fmaf(pose[3], cx, fmaf(pose[4], cy, pose[5] * cz));
    const float dy = fmaf(pose[6], cx, fmaf(pose[7], cy, pose[8] * cz));
    const float dz = fmaf(pose[9], cx, fmaf(pose[10], cy, pose[11] * cz));
    const float ix = frcp(dx), iy = frcp(dy), iz = frcp(dz);
    const float tstop = A.is_depth ? (cx > 0.f ? A.dmax * frcp(cx) * 1.000001f : INFINITY) : A.dmax;  // as above
    best = grid_ray_walk(best, A.sc, s, ox, oy, oz, dx, dy, dz, ix, iy, iz, tstop);
    float val = A.dmax;  // a miss
    if (best < INFINITY) val = fminf(A.is_depth ? best * cx : best, A.dmax);
    A.img[((size_t)b * h + v) * w + u] = val * A.scale;
}

__global__ __launch_bounds__(SCENE_BLOCK) void scene_distance_mixed_kernel(SceneDistDynArgs D) {
    const SceneDistArgs& A = D.d;
    const long long j = (long long)blockIdx.x * SCENE_BLOCK + threadIdx.x;
    if (j >= A.n) return;
    const long long s = A.p_to_scene ? (long long)min(max(A.p_to_scene[j], 0), A.sc.S - 1) : j / A.per_scene;
    const ScenePrimDyn* M = D.dyn + s * SCENE_MAX_PRIMS;
    const int mcnt = min(max(D.mcount[s], 0), SCENE_MAX_PRIMS);
    const double t = D.times ? D.times[j] : 0.0;
    const double px = A.points[j * 3], py = A.points[j * 3 + 1], pz = A.points[j * 3 + 2];
    double best = INFINITY;
    for (int i = 0; i < mcnt; ++i) best = fmin(best, frame_distance(M[i], t, px, py, pz));
    const SceneGridHdr& G = A.sc.ghdr[s];
    const ScenePrimD* P = A.sc.pd + G.prim_off;
    grid_ring_search(
        G, A.sc.cell_start + G.cell_off, A.sc.cell_items, px, py, pz,
        [&](int i) { best = fmin(best, prim_distance(P[i], px, py, pz)); }, [&] { return best; });
    A.out[j] = best;
}

// The row of the nearest primitive of either set; on a tie a static primitive comes before a mover, and within each
// set the lowest index wins.  The movers' best bounds the ring search but is kept apart from the static best: a
// static primitive the search has not seen lies beyond the bound by the grid's inflation, so a tie with the movers'
// best can only involve a static primitive that was seen.
__global__ __launch_bounds__(SCENE_BLOCK) void scene_sdf_rows_mixed_kernel(SceneSdfArgs A) {
    const long long r = (long long)blockIdx.x * SCENE_BLOCK + threadIdx.x;
    if (r >= A.rows) return;
    const long long b = r / A.N1;
    const int k = (int)(r - b * A.N1);
    const long long s = A.scene_of ? (long long)min(max(A.scene_of[b], 0), A.sc.S - 1) : 0;
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
    const SceneGridHdr& G = A.sc.ghdr[s];
    const ScenePrimD* P = A.sc.pd + G.prim_off;
    double best = INFINITY, bx = 0.0, by = 0.0, bz = 0.0;
    int bi = 0x7fffffff;
    grid_ring_search(
        G, A.sc.cell_start + G.cell_off, A.sc.cell_items, px, py, pz,
        [&](int i) {
            double gx, gy, gz;
            const double d = prim_sd_grad(P[i], px, py, pz, gx, gy, gz);
            if (d < best || (d == best && i < bi)) {  // the lowest index of the scene on a tie, whatever the visiting order
                best = d;
                bi = i;
                bx = gx; by = gy; bz = gz;
            }
        },
        [&] { return fmin(fmin(best, mbest), A.max_df); });
    if (mbest < best) {  // strictly: a static primitive keeps a tie
        best = mbest;
        bx = mx; by = my; bz = mz;
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

hipError_t launch_scene_render_mixed(const SceneRenderDynArgs& a, hipStream_t s) {
    if (a.r.B <= 0) return hipSuccess;
    const long long tiles = ((long long)a.r.H * a.r.W + SCENE_BLOCK - 1) / SCENE_BLOCK;
    hipLaunchKernelGGL(scene_render_mixed_kernel, dim3((unsigned)tiles, (unsigned)a.r.B), dim3(SCENE_BLOCK),
                       scene_render_lds_bytes(a.r.H, a.r.W, a.r.is_spherical), s, a);
    return hipGetLastError();
}

hipError_t launch_scene_distance_mixed(const SceneDistDynArgs& a, hipStream_t s) {
    if (a.d.n <= 0) return hipSuccess;
    hipLaunchKernelGGL(scene_distance_mixed_kernel, dim3((unsigned)((a.d.n + SCENE_BLOCK - 1) / SCENE_BLOCK)),
                       dim3(SCENE_BLOCK), 0, s, a);
    return hipGetLastError();
}

hipError_t launch_scene_sdf_rows_mixed(const SceneSdfArgs& a, hipStream_t s) {
    if (a.rows <= 0) return hipSuccess;
    hipLaunchKernelGGL(scene_sdf_rows_mixed_kernel, dim3((unsigned)((a.rows + SCENE_BLOCK - 1) / SCENE_BLOCK)),
                       dim3(SCENE_BLOCK), 0, s, a);
    return hipGetLastError();
}

hipError_t launch_scene_render_grid(const SceneRenderArgs& a, hipStream_t s) {
    if (a.B <= 0) return hipSuccess;
    const long long tiles = ((long long)a.H * a.W + SCENE_BLOCK - 1) / SCENE_BLOCK;
    hipLaunchKernelGGL(scene_render_grid_kernel, dim3((unsigned)tiles, (unsigned)a.B), dim3(SCENE_BLOCK),
                       scene_render_lds_bytes(a.H, a.W, a.is_spherical), s, a);
    return hipGetLastError();
}

hipError_t launch_scene_distance_grid(const SceneDistArgs& a, hipStream_t s) {
    if (a.n <= 0) return hipSuccess;
    hipLaunchKernelGGL(scene_distance_grid_kernel, dim3((unsigned)((a.n + SCENE_BLOCK - 1) / SCENE_BLOCK)),
                       dim3(SCENE_BLOCK), 0, s, a);
    return hipGetLastError();
}

hipError_t launch_scene_sdf_rows_grid(const SceneSdfArgs& a, hipStream_t s) {
    if (a.rows <= 0) return hipSuccess;
    hipLaunchKernelGGL(scene_sdf_rows_grid_kernel, dim3((unsigned)((a.rows + SCENE_BLOCK - 1) / SCENE_BLOCK)),
                       dim3(SCENE_BLOCK), 0, s, a);
    return hipGetLastError();
}

}  // namespace sdfn
