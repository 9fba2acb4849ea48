// Device code shared by the scene kernels (scene.hip, scene_sdf.hip, scene_grid.hip, scene_swept.hip): a primitive's
// frame, and the per-primitive work of the queries -- the ray's hit, the signed distance, the distance with its gradient.  The
// brute-force kernels and the grid kernels call the same functions, so that a query over a subset of the primitives
// that holds the minimiser returns the bits of the query over all of them.  The same holds for a primitive with a
// frame (frame_ray_hit, frame_distance, frame_sd_grad): the dynamic kernels and the mixed kernels of scene_grid.hip
// (a grid of static primitives plus up to 32 movers) call one function each.
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

// ---- the ray's hit (fp32)
__device__ __forceinline__ float frcp(float a) { return __builtin_amdgcn_rcpf(a); }    // 1 ulp
__device__ __forceinline__ float fsqrt(float a) { return __builtin_amdgcn_sqrtf(a); }  // 1 ulp

// the root interval of t^2 - 2 b t + c = 0 with h = sqrt(b^2 - c) given (the caller forms the discriminant
// without cancellation): the root of larger magnitude is q = b + sign(b) h, the other one c / q
__device__ __forceinline__ void root_interval(float b, float c, float h, float& tn, float& tf) {
    const float q = b + copysignf(h, b);
    const float r = c * frcp(q);  // q == 0 only with b == h == 0, c == 0: a double root at 0 (fmin / fmax drop the NaN)
    tn = fminf(q, r);
    tf = fmaxf(q, r);
}

// slab interval of one axis: (lo - o) / d and (hi - o) / d in either order; d == 0 gives -inf / +inf inside
// the slab and an empty interval outside it
__device__ __forceinline__ void slab(float lo, float hi, float o, float inv_d, float& tn, float& tf) {
    const float t1 = (lo - o) * inv_d, t2 = (hi - o) * inv_d;
    tn = fmaxf(tn, fminf(t1, t2));
    tf = fminf(tf, fmaxf(t1, t2));
}

// best = min(best, the hit of the ray o + t d with a world-frame primitive (kind, a0..a5); ix, iy, iz = rcp(d)).  Every
// primitive is convex, so the ray meets it in one parameter interval [tn, tf]; it hits when tf >= max(tn, 0), at
// t = max(tn, 0).
__device__ __forceinline__ float prim_ray_hit(float best, int kind, float a0, float a1, float a2, float a3, float a4,
                                              float a5, float ox, float oy, float oz, float dx, float dy, float dz,
                                              float ix, float iy, float iz) {
    float tn = -INFINITY, tf = INFINITY;
    if (kind == 0) {  // sphere: centre a0..a2, radius a3
        const float ex = a0 - ox, ey = a1 - oy, ez = a2 - oz;
        const float bb = fmaf(ex, dx, fmaf(ey, dy, ez * dz));
        const float wx = fmaf(-bb, dx, ex), wy = fmaf(-bb, dy, ey), wz = fmaf(-bb, dz, ez);  // foot of the centre
        const float h2 = fmaf(a3, a3, -fmaf(wx, wx, fmaf(wy, wy, wz * wz)));                 // r^2 - |w|^2
        const float cc = fmaf(ex, ex, fmaf(ey, ey, ez * ez)) - a3 * a3;
        if (h2 >= 0.f) root_interval(bb, cc, fsqrt(h2), tn, tf);
        else tf = -INFINITY;
    } else if (kind == 1) {  // box: lo a0..a2, hi a3..a5
        slab(a0, a3, ox, ix, tn, tf);
        slab(a1, a4, oy, iy, tn, tf);
        slab(a2, a5, oz, iz, tn, tf);
    } else {  // capped cylinder along z: centre a0, a1, radius a2, z in [a3, a4]
        const float ex = a0 - ox, ey = a1 - oy;
        const float aa = fmaf(dx, dx, dy * dy), e2 = fmaf(ex, ex, ey * ey);
        if (aa > 1e-12f) {  // the side wall's quadratic, divided by |d_xy|^2
            const float k = frcp(aa);
            const float bb = fmaf(ex, dx, ey * dy) * k;
            const float wx = fmaf(-bb, dx, ex), wy = fmaf(-bb, dy, ey);
            const float h2 = fmaf(a2, a2, -fmaf(wx, wx, wy * wy));
            if (h2 >= 0.f) root_interval(bb, (e2 - a2 * a2) * k, fsqrt(h2 * k), tn, tf);
            else tf = -INFINITY;
        } else if (e2 > a2 * a2) {  // along the axis, outside the wall
            tf = -INFINITY;
        }
        slab(a3, a4, oz, iz, tn, tf);  // the caps
    }
    if (tn <= tf && tf >= 0.f) best = fminf(best, fmaxf(tn, 0.f));
    return best;
}

// best = min(best, the hit of the camera-frame unit direction (cx, cy, cz) with a staged primitive frame F): the ray
// is taken into the primitive's frame, o' = F.o, d' = F.M d_cam, and meets the canonical centred shape (sphere of
// radius h0, box of half extents h0, h1, hz, capped cylinder of radius h0 and half height hz along its own z) in one
// interval, as in prim_ray_hit.  F.kind must be uniform over the wave (one scene per block).  The loop body of
// scene_render_dyn_kernel, shared with scene_render_mixed_kernel.
__device__ __forceinline__ float frame_ray_hit(float best, const ScenePrimFrame& F, float cx, float cy, float cz) {
    const float4* q = (const float4*)&F;
    const float4 q0 = q[0], q1 = q[1], q2 = q[2], q3 = q[3];
    const float ox = q0.x, oy = q0.y, oz = q0.z, h0 = q0.w, h2z = q3.z, h1 = q3.w;
    const float dx = fmaf(q1.x, cx, fmaf(q1.y, cy, q1.z * cz));  // d' = M d_cam
    const float dy = fmaf(q1.w, cx, fmaf(q2.x, cy, q2.y * cz));
    const float dz = fmaf(q2.z, cx, fmaf(q2.w, cy, q3.x * cz));
    const int kind = __builtin_amdgcn_readfirstlane(__float_as_int(q3.y));  // one scene per block: uniform
    float tn = -INFINITY, tf = INFINITY;
    if (kind == 0) {  // sphere of radius h0 about the origin
        const float ex = -ox, ey = -oy, ez = -oz;
        const float bb = fmaf(ex, dx, fmaf(ey, dy, ez * dz));
        const float wx = fmaf(-bb, dx, ex), wy = fmaf(-bb, dy, ey), wz = fmaf(-bb, dz, ez);
        const float hh = fmaf(h0, h0, -fmaf(wx, wx, fmaf(wy, wy, wz * wz)));  // r^2 - |w|^2
        const float cc = fmaf(ex, ex, fmaf(ey, ey, ez * ez)) - h0 * h0;
        if (hh >= 0.f) root_interval(bb, cc, fsqrt(hh), tn, tf);
        else tf = -INFINITY;
    } else if (kind == 1) {  // box of half extents h0, h1, h2z
        slab(-h0, h0, ox, frcp(dx), tn, tf);
        slab(-h1, h1, oy, frcp(dy), tn, tf);
        slab(-h2z, h2z, oz, frcp(dz), tn, tf);
    } else {  // capped cylinder along its own z: radius h0, half height h2z
        const float ex = -ox, ey = -oy;
        const float aa = fmaf(dx, dx, dy * dy), e2 = fmaf(ex, ex, ey * ey);
        if (aa > 1e-12f) {
            const float k = frcp(aa);
            const float bb = fmaf(ex, dx, ey * dy) * k;
            const float wx = fmaf(-bb, dx, ex), wy = fmaf(-bb, dy, ey);
            const float hh = fmaf(h0, h0, -fmaf(wx, wx, wy * wy));
            if (hh >= 0.f) root_interval(bb, (e2 - h0 * h0) * k, fsqrt(hh * k), tn, tf);
            else tf = -INFINITY;
        } else if (e2 > h0 * h0) {
            tf = -INFINITY;
        }
        slab(-h2z, h2z, oz, frcp(dz), tn, tf);  // the caps
    }
    if (tn <= tf && tf >= 0.f) best = fminf(best, fmaxf(tn, 0.f));
    return best;
}

// what lane i < count of a block stages for primitive P of a dynamic set: the camera (W_p_C, W_R_C) in the
// primitive's frame at time t, o' = R(t)^T (W_p_C - c(t)) and M = R(t)^T W_R_C, formed in fp64 and rounded to fp32
// once (world-scale coordinates cancel in fp64, before the rounding)
__device__ __forceinline__ ScenePrimFrame prim_camera_frame(const ScenePrimDyn& P, double t, const double* Wp,
                                                            const double* WR) {
    double c[3], R[9], e[3];
    prim_frame(P, t, c, R);
#pragma unroll
    for (int j = 0; j < 3; ++j) e[j] = Wp[j] - c[j];
    ScenePrimFrame F;
#pragma unroll
    for (int j = 0; j < 3; ++j) {
        F.o[j] = (float)(R[j] * e[0] + R[3 + j] * e[1] + R[6 + j] * e[2]);
#pragma unroll
        for (int k = 0; k < 3; ++k) F.M[j * 3 + k] = (float)(R[j] * WR[k] + R[3 + j] * WR[3 + k] + R[6 + j] * WR[6 + k]);
    }
    F.h0 = (float)P.h[0];
    F.h1 = (float)P.h[1];
    F.hz = (float)P.h[2];
    F.kind = P.kind;
    return F;
}

// ---- the signed distance (fp64)
// length of the positive parts plus the largest component where all are negative: the signed distance to a
// box (or, with two components, to a capped cylinder's section) from its per-axis excesses
__device__ __forceinline__ double sd_excess3(double qx, double qy, double qz) {
    const double px = fmax(qx, 0.0), py = fmax(qy, 0.0), pz = fmax(qz, 0.0);
    return sqrt(px * px + py * py + pz * pz) + fmin(fmax(qx, fmax(qy, qz)), 0.0);
}

// the closed-form signed distance from (px, py, pz) to a world-frame primitive
__device__ __forceinline__ double prim_distance(const ScenePrimD& P, double px, double py, double pz) {
    const double* a = P.a;
    if (P.kind == 0) {
        const double ex = px - a[0], ey = py - a[1], ez = pz - a[2];
        return sqrt(ex * ex + ey * ey + ez * ez) - a[3];
    }
    if (P.kind == 1)
        return sd_excess3(fabs(px - 0.5 * (a[0] + a[3])) - 0.5 * (a[3] - a[0]),
                          fabs(py - 0.5 * (a[1] + a[4])) - 0.5 * (a[4] - a[1]),
                          fabs(pz - 0.5 * (a[2] + a[5])) - 0.5 * (a[5] - a[2]));
    const double ex = px - a[0], ey = py - a[1];
    return sd_excess3(sqrt(ex * ex + ey * ey) - a[2], fabs(pz - 0.5 * (a[3] + a[4])) - 0.5 * (a[4] - a[3]), -INFINITY);
}

// ---- the signed distance with its gradient (fp64)
__device__ __forceinline__ double sgn1(double v) { return v < 0.0 ? -1.0 : 1.0; }  // sign(0) = +1

// distance and gradient of the canonical centred shape at the point q of its frame (sphere: radius h0; box: half
// extents h0, h1, hz; capped cylinder along z: radius h0, half height hz).  The distance is sd_excess3 on the per-axis
// excesses; at a kink the gradient is one of the one-sided values, finite and of norm <= 1.
__device__ __forceinline__ double shape_sd(int kind, double qx, double qy, double qz, double h0, double h1, double hz,
                                           double& gx, double& gy, double& gz) {
    if (kind == 0) {
        const double n = sqrt(qx * qx + qy * qy + qz * qz);
        const bool z = n == 0.0;
        gx = z ? 0.0 : qx / n;
        gy = z ? 0.0 : qy / n;
        gz = z ? 1.0 : qz / n;
        return n - h0;
    }
    if (kind == 1) {
        const double ax = fabs(qx) - h0, ay = fabs(qy) - h1, az = fabs(qz) - hz;
        const double px = fmax(ax, 0.0), py = fmax(ay, 0.0), pz = fmax(az, 0.0);
        const double len = sqrt(px * px + py * py + pz * pz);
        const double amax = fmax(ax, fmax(ay, az));
        if (amax > 0.0) {
            gx = sgn1(qx) * px / len;
            gy = sgn1(qy) * py / len;
            gz = sgn1(qz) * pz / len;
        } else {  // inside: the nearest face, the lowest axis on a tie
            const bool mx = ax >= ay && ax >= az, my = !mx && ay >= az;
            gx = mx ? sgn1(qx) : 0.0;
            gy = my ? sgn1(qy) : 0.0;
            gz = (!mx && !my) ? sgn1(qz) : 0.0;
        }
        return len + fmin(amax, 0.0);
    }
    const double rho = sqrt(qx * qx + qy * qy);
    const bool z = rho == 0.0;
    const double ex = z ? 1.0 : qx / rho, ey = z ? 0.0 : qy / rho;
    const double a0 = rho - h0, a1 = fabs(qz) - hz;
    const double p0 = fmax(a0, 0.0), p1 = fmax(a1, 0.0);
    const double len = sqrt(p0 * p0 + p1 * p1 + 0.0);  // sd_excess3's third component is -inf: its positive part 0
    const double amax = fmax(a0, a1);
    if (amax > 0.0) {
        gx = p0 * ex / len;
        gy = p0 * ey / len;
        gz = p1 * sgn1(qz) / len;
    } else if (a0 >= a1) {
        gx = ex; gy = ey; gz = 0.0;
    } else {
        gx = 0.0; gy = 0.0; gz = sgn1(qz);
    }
    return len + fmin(amax, 0.0);
}

// shape_sd of a world-frame primitive (its frame is the world's, translated): the distance from (px, py, pz) and
// its world gradient
__device__ __forceinline__ double prim_sd_grad(const ScenePrimD& P, double px, double py, double pz, double& gx,
                                               double& gy, double& gz) {
    const double* a = P.a;
    const int kind = P.kind;
    double qx, qy, qz, h0, h1 = 0.0, hz = 0.0;
    if (kind == 0) {
        qx = px - a[0]; qy = py - a[1]; qz = pz - a[2];
        h0 = a[3];
    } else if (kind == 1) {
        qx = px - 0.5 * (a[0] + a[3]); qy = py - 0.5 * (a[1] + a[4]); qz = pz - 0.5 * (a[2] + a[5]);
        h0 = 0.5 * (a[3] - a[0]); h1 = 0.5 * (a[4] - a[1]); hz = 0.5 * (a[5] - a[2]);
    } else {
        qx = px - a[0]; qy = py - a[1]; qz = pz - 0.5 * (a[3] + a[4]);
        h0 = a[2]; hz = 0.5 * (a[4] - a[3]);
    }
    return shape_sd(kind, qx, qy, qz, h0, h1, hz, gx, gy, gz);
}

// ---- a primitive with a frame, at a point and a time (fp64): shared by the dynamic kernels and the mixed ones
// a0 b0 + a1 b1 + a2 b2 with the fused operations written out.  Left to the compiler, which product of such a sum
// stays a multiplication depends on the code around it: the same source line gave the mixed rows kernel a last bit
// that the dynamic one did not have.  This is the form the dynamic kernels have always compiled to.
__device__ __forceinline__ double dot3_pinned(double a0, double b0, double a1, double b1, double a2, double b2) {
    return fma(a2, b2, fma(a0, b0, a1 * b1));
}

// the point in the primitive's frame at time t, q = R(t)^T (p - c(t)); R is left to the caller for the gradient
__device__ __forceinline__ void frame_point(const ScenePrimDyn& P, double t, double px, double py, double pz, double* R,
                                            double& qx, double& qy, double& qz) {
    double c[3];
    prim_frame(P, t, c, R);
    const double ex = px - c[0], ey = py - c[1], ez = pz - c[2];
    qx = dot3_pinned(R[0], ex, R[3], ey, R[6], ez);
    qy = dot3_pinned(R[1], ex, R[4], ey, R[7], ez);
    qz = dot3_pinned(R[2], ex, R[5], ey, R[8], ez);
}

// the signed distance from (px, py, pz) to the primitive at time t: scene_distance_kernel's closed forms on the
// canonical shape
__device__ __forceinline__ double frame_distance(const ScenePrimDyn& P, double t, double px, double py, double pz) {
    double R[9], qx, qy, qz;
    frame_point(P, t, px, py, pz, R, qx, qy, qz);
    const double* h = P.h;
    if (P.kind == 0) return sqrt(qx * qx + qy * qy + qz * qz) - h[0];
    if (P.kind == 1) return sd_excess3(fabs(qx) - h[0], fabs(qy) - h[1], fabs(qz) - h[2]);
    return sd_excess3(sqrt(qx * qx + qy * qy) - h[0], fabs(qz) - h[2], -INFINITY);
}

// the same distance through shape_sd with its gradient (gx, gy, gz) in the primitive's frame; the world gradient is
// R g (frame_grad_world) with the R returned here
__device__ __forceinline__ double frame_sd_grad(const ScenePrimDyn& P, double t, double px, double py, double pz,
                                                double* R, double& gx, double& gy, double& gz) {
    double qx, qy, qz;
    frame_point(P, t, px, py, pz, R, qx, qy, qz);
    return shape_sd(P.kind, qx, qy, qz, P.h[0], P.h[1], P.h[2], gx, gy, gz);
}

__device__ __forceinline__ void frame_grad_world(const double* R, double gx, double gy, double gz, double& bx,
                                                 double& by, double& bz) {
    bx = dot3_pinned(R[0], gx, R[1], gy, R[2], gz);
    by = dot3_pinned(R[3], gx, R[4], gy, R[5], gz);
    bz = dot3_pinned(R[6], gx, R[7], gy, R[8], gz);
}

// ---- the uniform grid of an indexed scene set (scene_grid.hip; the ring search also in scene_swept.hip)
// the cell of a coordinate u = (v - org) * inv in cells, clamped into [0, n): NaN gives 0
__device__ __forceinline__ int grid_cell(double u, int n) {
    return u >= (double)(n - 1) ? n - 1 : (u > 0.0 ? (int)u : 0);
}

// The ring search of a point: visit(i) for every primitive i listed in the block of cells around the point's cell
// (clamped into the grid), the block grown by one cell per side and round, until bound() <= the smallest axis gap
// from the point to a face of the block that is not on the grid's boundary.  bound() is what the caller still cares
// to find something below: its best so far, or less.
template <class Visit, class Bound>
__device__ __forceinline__ void grid_ring_search(const SceneGridHdr& G, const int* cs, const int* items, double px,
                                                 double py, double pz, Visit visit, Bound bound) {
    const double p[3] = {px, py, pz};
    int lo[3], hi[3], plo[3] = {1, 1, 1}, phi[3] = {0, 0, 0};  // the block, and the block already searched (empty)
#pragma unroll
    for (int a = 0; a < 3; ++a) lo[a] = hi[a] = grid_cell((p[a] - G.org[a]) * G.inv, G.n[a]);
    const int nx = G.n[0], ny = G.n[1];
    const int rounds = max(G.n[0], max(G.n[1], G.n[2]));  // after that many the block is the grid
    for (int r = 0; r <= rounds; ++r) {
        for (int k = lo[2]; k <= hi[2]; ++k)
            for (int j = lo[1]; j <= hi[1]; ++j) {
                const int row = (k * ny + j) * nx;
                const bool inner = k >= plo[2] && k <= phi[2] && j >= plo[1] && j <= phi[1];
                // a run of cells along x is one run of the item list; inside the old block's rows only the two ends
                if (!inner) {
                    const int k1 = cs[row + hi[0] + 1];
                    for (int q = cs[row + lo[0]]; q < k1; ++q) visit(items[q]);
                } else {
                    int k1 = cs[row + plo[0]];
                    for (int q = cs[row + lo[0]]; q < k1; ++q) visit(items[q]);
                    k1 = cs[row + hi[0] + 1];
                    for (int q = cs[row + phi[0] + 1]; q < k1; ++q) visit(items[q]);
                }
            }
        double gap = INFINITY;
        bool grown = false;
#pragma unroll
        for (int a = 0; a < 3; ++a) {
            if (lo[a] > 0) gap = fmin(gap, p[a] - (G.org[a] + (double)lo[a] * G.cell));
            if (hi[a] < G.n[a] - 1) gap = fmin(gap, (G.org[a] + (double)(hi[a] + 1) * G.cell) - p[a]);
            grown = grown || lo[a] > 0 || hi[a] < G.n[a] - 1;
        }
        if (!grown || !(bound() > gap)) break;  // the whole grid, or nothing unseen below the bound (NaN ends it too)
#pragma unroll
        for (int a = 0; a < 3; ++a) {
            plo[a] = lo[a];
            phi[a] = hi[a];
            lo[a] = max(lo[a] - 1, 0);
            hi[a] = min(hi[a] + 1, G.n[a] - 1);
        }
    }
}

}  // namespace sdfn
