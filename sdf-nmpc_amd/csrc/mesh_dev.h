// Device code of the mesh kernels (scene_mesh.hip, and scene_swept.hip's kernel over mesh_distance): the ray's hit with
// one triangle, the closest point of a triangle, and the two stackless walks of a scene's hierarchy (mesh_bvh.h: the
// layout, the boxes and why the walks end).  The distance walk is one search (mesh_search) with two epilogues: the
// value (mesh_value) that Scene.distance, the swept kernel and the SDF rows kernel share to the bit, and its gradient
// (mesh_gradient) for the rows kernel.
//
// Neither walk (nor the descent to a first leaf that precedes the distance walk) holds an array that is indexed at run
// time: a lane carries the index of its node and nothing else of the tree, so nothing lives in scratch memory.  The trip count of the node loop is bounded by the node count before
// it starts and that of a leaf's loop by the leaf's count, both read from arrays the host built: a non-finite pose or
// point ends with every read inside the set's arrays.
#pragma once
#include "scene_dev.h"

namespace sdfn {

// ---- the ray's hit (fp32)
// d . (p x q) with every fused operation written out: the two triangles of an edge call this with the same operands
// and must see the same bits whatever code surrounds the call
__device__ __forceinline__ float triple_pinned(float dx, float dy, float dz, float px, float py, float pz, float qx,
                                               float qy, float qz) {
    const float cx = fmaf(py, qz, -(pz * qy));
    const float cy = fmaf(pz, qx, -(px * qz));
    const float cz = fmaf(px, qy, -(py * qx));
    return fmaf(dx, cx, fmaf(dy, cy, dz * cz));
}

// the signed edge function of the ray with the edge p -> q (both relative to the ray's origin), evaluated with the
// endpoints in ascending vertex-index order and the sign flipped back when that is q -> p
__device__ __forceinline__ float edge_fn(bool flip, float dx, float dy, float dz, float px, float py, float pz, float qx,
                                         float qy, float qz) {
    const float e = triple_pinned(dx, dy, dz, flip ? qx : px, flip ? qy : py, flip ? qz : pz, flip ? px : qx,
                                  flip ? py : qy, flip ? pz : qz);
    return flip ? -e : e;
}

// best = min(best, the hit of the ray o + t d with the triangle T of a scene of margin m; ix, iy, iz = rcp(d)).
// Double-sided: the three edge functions all >= 0 or all <= 0, so a ray through a shared edge or vertex is accepted
// by both triangles (their edge functions are the same bits up to the sign).  t from the face plane, t >= 0, clamped
// into the slab interval [tn, tf] of the triangle's own widened box, which must not be empty nor begin beyond best:
// what makes the result independent of the hierarchy (mesh_bvh.h).
__device__ __forceinline__ float mesh_tri_hit(float best, const MeshTriF& T, float m, float ox, float oy, float oz,
                                              float dx, float dy, float dz, float ix, float iy, float iz) {
    const float ax = T.v[0], ay = T.v[1], az = T.v[2], bx = T.v[3], by = T.v[4], bz = T.v[5], cx = T.v[6], cy = T.v[7],
                cz = T.v[8];
    float tn = 0.f, tf = INFINITY;
    slab(fminf(fminf(ax, bx), cx) - m, fmaxf(fmaxf(ax, bx), cx) + m, ox, ix, tn, tf);
    slab(fminf(fminf(ay, by), cy) - m, fmaxf(fmaxf(ay, by), cy) + m, oy, iy, tn, tf);
    slab(fminf(fminf(az, bz), cz) - m, fmaxf(fmaxf(az, bz), cz) + m, oz, iz, tn, tf);
    if (!(tn <= tf && tn <= best)) return best;
    const float Ax = ax - ox, Ay = ay - oy, Az = az - oz;
    const float Bx = bx - ox, By = by - oy, Bz = bz - oz;
    const float Cx = cx - ox, Cy = cy - oy, Cz = cz - oz;
    const float e0 = edge_fn(T.flip & 1, dx, dy, dz, Ax, Ay, Az, Bx, By, Bz);
    const float e1 = edge_fn(T.flip & 2, dx, dy, dz, Bx, By, Bz, Cx, Cy, Cz);
    const float e2 = edge_fn(T.flip & 4, dx, dy, dz, Cx, Cy, Cz, Ax, Ay, Az);
    const bool inside = (e0 >= 0.f && e1 >= 0.f && e2 >= 0.f) || (e0 <= 0.f && e1 <= 0.f && e2 <= 0.f);
    const float den = fmaf(T.n[0], dx, fmaf(T.n[1], dy, T.n[2] * dz));
    const float num = fmaf(T.n[0], Ax, fmaf(T.n[1], Ay, T.n[2] * Az));
    const float t = num / den;
    if (!inside || den == 0.f || !(t >= 0.f)) return best;
    return fminf(best, fminf(fmaxf(t, tn), tf));
}

// The nearest hit of the ray over scene h: preorder, to skip when the node's slab interval (clipped to t >= 0) is empty
// or begins beyond the best hit, to the next node when it is inner, through its triangles when it is a leaf.
// best: what the walk starts from, the hit of something that is not in the hierarchy (the movers of
// scene_render_mesh_mixed_kernel); the result is fminf(best, the walk's own result from +inf).  A smaller best only
// rejects more nodes and triangles, each because its interval begins beyond best, and a triangle's hit is clamped into
// its interval, so what is rejected could not have lowered best.
__device__ __forceinline__ float mesh_ray_cast(const MeshDev& M, const MeshHdr& h, float ox, float oy, float oz, float dx,
                                               float dy, float dz, float ix, float iy, float iz, float best = INFINITY) {
    const MeshNode* N = M.nodes + h.node_off;
    const MeshTriF* T = M.tf + h.tri_off;
    const int nn = h.nnodes;
    const float m = h.margin;
    int i = 0;
    for (int it = 0; it < nn && i < nn; ++it) {
        const MeshNode nd = N[i];
        float tn = 0.f, tf = INFINITY;
        slab(nd.lo[0], nd.hi[0], ox, ix, tn, tf);
        slab(nd.lo[1], nd.hi[1], oy, iy, tn, tf);
        slab(nd.lo[2], nd.hi[2], oz, iz, tn, tf);
        if (!(tn <= tf && tn <= best)) {
            i = nd.skip;
            continue;
        }
        if (nd.count == 0) {
            ++i;
            continue;
        }
        const int e = min(nd.first + nd.count, h.ntri);
        for (int k = max(nd.first, 0); k < e; ++k) best = mesh_tri_hit(best, T[k], m, ox, oy, oz, dx, dy, dz, ix, iy, iz);
        i = nd.skip;
    }
    return best;
}

// ---- the distance (fp64)
// The closest point c of the triangle a, b, c to p by its seven Voronoi regions (0: the face; 1, 2, 3: the edges ab, bc,
// ca; 4, 5, 6: the vertices a, b, c); returns |p - c|^2
__device__ __forceinline__ double tri_closest(const double* v, double px, double py, double pz, double& qx, double& qy,
                                              double& qz, int& region) {
#pragma clang fp contract(off)  // the distance and the swept kernel must agree to the bit: no fusing left to the compiler
    const double ax = v[0], ay = v[1], az = v[2];
    const double abx = v[3] - ax, aby = v[4] - ay, abz = v[5] - az;
    const double acx = v[6] - ax, acy = v[7] - ay, acz = v[8] - az;
    const double apx = px - ax, apy = py - ay, apz = pz - az;
    const double d1 = abx * apx + aby * apy + abz * apz, d2 = acx * apx + acy * apy + acz * apz;
    const double bpx = px - v[3], bpy = py - v[4], bpz = pz - v[5];
    const double d3 = abx * bpx + aby * bpy + abz * bpz, d4 = acx * bpx + acy * bpy + acz * bpz;
    const double cpx = px - v[6], cpy = py - v[7], cpz = pz - v[8];
    const double d5 = abx * cpx + aby * cpy + abz * cpz, d6 = acx * cpx + acy * cpy + acz * cpz;
    const double vc = d1 * d4 - d3 * d2, vb = d5 * d2 - d1 * d6, va = d3 * d6 - d5 * d4;
    double s = 0.0, t = 0.0;  // c = a + s ab + t ac
    if (d1 <= 0.0 && d2 <= 0.0) {
        region = 4;
    } else if (d3 >= 0.0 && d4 <= d3) {
        region = 5;
        s = 1.0;
    } else if (vc <= 0.0 && d1 >= 0.0 && d3 <= 0.0) {
        region = 1;
        s = d1 / (d1 - d3);
    } else if (d6 >= 0.0 && d5 <= d6) {
        region = 6;
        t = 1.0;
    } else if (vb <= 0.0 && d2 >= 0.0 && d6 <= 0.0) {
        region = 3;
        t = d2 / (d2 - d6);
    } else if (va <= 0.0 && (d4 - d3) >= 0.0 && (d5 - d6) >= 0.0) {
        region = 2;
        t = (d4 - d3) / ((d4 - d3) + (d5 - d6));
        s = 1.0 - t;
    } else {
        region = 0;
        const double den = 1.0 / (va + vb + vc);
        s = vb * den;
        t = vc * den;
    }
    qx = ax + abx * s + acx * t;
    qy = ay + aby * s + acy * t;
    qz = az + abz * s + acz * t;
    const double ex = px - qx, ey = py - qy, ez = pz - qz;
    return ex * ex + ey * ey + ez * ez;
}

// the squared distance from p to a node's box, read in fp64
__device__ __forceinline__ double mesh_box_d2(const MeshNode& nd, double px, double py, double pz) {
#pragma clang fp contract(off)
    const double ex = fmax(fmax((double)nd.lo[0] - px, px - (double)nd.hi[0]), 0.0);
    const double ey = fmax(fmax((double)nd.lo[1] - py, py - (double)nd.hi[1]), 0.0);
    const double ez = fmax(fmax((double)nd.lo[2] - pz, pz - (double)nd.hi[2]), 0.0);
    return ex * ex + ey * ey + ez * ez;
}

// The winner of the search for the triangle nearest to p: its squared distance, the closest point c on it, the Voronoi
// region of the triangle c lies in (tri_closest) and the triangle's place in the scene's reordered list; pos = -1 and
// d2 = +inf when there is none.
struct MeshHit {
    double d2, cx, cy, cz;
    int region, pos;
};

// The search over scene h: the triangle of the smallest (squared distance, original index) among those with a squared
// distance <= bound, a node rejected only when its box's squared distance is strictly greater than the best, so ties
// are always visited and the result does not depend on the hierarchy.  bound = +inf is the full search.  A finite
// bound starts the walk with best = bound and no winner: a triangle or a node beyond it is never opened, one at or
// below it is treated as in the full search (best never falls below the winner's d2, so neither the winner nor a box
// above it is ever rejected), and the winner is that of the full search whenever that one's d2 <= bound -- else there
// is none.
//
// A preorder walk meets the left child first wherever the point is, and with best = inf it would open most of the
// tree before it has a bound.  So the walk is preceded by a descent to one leaf, at every inner node into the child
// whose box is nearer (the right child of i is skip of i + 1; at most nnodes steps, no stack): the triangles of that
// leaf give the first bound.  They are candidates like any other -- the result is still the smallest (d2, index) over a
// set that holds every triangle with d2 <= the final best -- and the walk meets them again without effect.
__device__ __forceinline__ MeshHit mesh_search(const MeshDev& M, const MeshHdr& h, double px, double py, double pz,
                                               double bound) {
#pragma clang fp contract(off)
    const MeshNode* N = M.nodes + h.node_off;
    const MeshTriD* T = M.td + h.tri_off;
    const int nn = h.nnodes;
    double best = bound, bx = 0.0, by = 0.0, bz = 0.0;
    int bidx = 0x7fffffff, bpos = -1, breg = 0;
    auto leaf = [&](const MeshNode& nd) {
        const int e = min(nd.first + nd.count, h.ntri);
        for (int k = max(nd.first, 0); k < e; ++k) {
            double qx, qy, qz;
            int reg;
            const double d2 = tri_closest(T[k].v, px, py, pz, qx, qy, qz, reg);
            const int orig = T[k].orig;
            if (d2 < best || (d2 == best && orig < bidx)) {
                best = d2;
                bidx = orig;
                bpos = k;
                breg = reg;
                bx = qx;
                by = qy;
                bz = qz;
            }
        }
    };
    if (nn > 0) {
        int g = 0;
        for (int it = 0; it < nn && N[g].count == 0 && g + 1 < nn; ++it) {
            const int l = g + 1, r = min(max(N[l].skip, 0), nn - 1);
            g = mesh_box_d2(N[r], px, py, pz) < mesh_box_d2(N[l], px, py, pz) ? r : l;
        }
        leaf(N[g]);
    }
    int i = 0;
    for (int it = 0; it < nn && i < nn; ++it) {
        const MeshNode nd = N[i];
        if (mesh_box_d2(nd, px, py, pz) > best) {
            i = nd.skip;
            continue;
        }
        if (nd.count == 0) {
            ++i;
            continue;
        }
        leaf(nd);
        i = nd.skip;
    }
    return MeshHit{bpos < 0 ? (double)INFINITY : best, bx, by, bz, breg, bpos};
}

// The value of the distance at p from the winner w.  An open set: sqrt(d2).  A closed set: with the sign of (p - c) . n
// for the pseudonormal n of the winner's region, a point on the surface counted as outside (+0).  No winner: +inf.
__device__ __forceinline__ double mesh_value(const MeshDev& M, const MeshHdr& h, const MeshHit& w, double px, double py,
                                             double pz) {
#pragma clang fp contract(off)
    const double d = sqrt(w.d2);
    if (!M.tn || w.pos < 0) return d;
    const double* n = M.tn[h.tri_off + w.pos].n + 3 * w.region;
    const double sgn = (px - w.cx) * n[0] + (py - w.cy) * n[1] + (pz - w.cz) * n[2];
    return sgn < 0.0 ? -d : d;
}

// The world gradient of mesh_value at p, d the value it returned.  d2 > 0: (p - c) / sqrt(d2), negated where d < 0 -- a
// unit vector away from the surface outside and towards it inside.  On the surface (d2 = 0) of a closed set: the
// pseudonormal of the winner's region, normalised (the triangle's unit face normal should it vanish); of an open set:
// the winner's unit face normal (b - a) x (c - a) / |.|, formed here from the fp64 vertices -- a one-sided value.  Always
// finite and of norm <= 1 up to rounding; zero without a winner.
__device__ __forceinline__ void mesh_gradient(const MeshDev& M, const MeshHdr& h, const MeshHit& w, double d, double px,
                                              double py, double pz, double& gx, double& gy, double& gz) {
#pragma clang fp contract(off)
    gx = gy = gz = 0.0;
    if (w.pos < 0) return;
    if (w.d2 > 0.0) {
        const double r = d < 0.0 ? -sqrt(w.d2) : sqrt(w.d2);
        gx = (px - w.cx) / r;
        gy = (py - w.cy) / r;
        gz = (pz - w.cz) / r;
        return;
    }
    double nx, ny, nz;
    if (M.tn) {
        const double* n = M.tn[h.tri_off + w.pos].n;
        nx = n[3 * w.region], ny = n[3 * w.region + 1], nz = n[3 * w.region + 2];
        if (!(nx * nx + ny * ny + nz * nz > 0.0)) nx = n[0], ny = n[1], nz = n[2];
    } else {
        const double* v = M.td[h.tri_off + w.pos].v;
        const double ux = v[3] - v[0], uy = v[4] - v[1], uz = v[5] - v[2];
        const double wx = v[6] - v[0], wy = v[7] - v[1], wz = v[8] - v[2];
        nx = uy * wz - uz * wy;
        ny = uz * wx - ux * wz;
        nz = ux * wy - uy * wx;
    }
    const double l = sqrt(nx * nx + ny * ny + nz * nz);
    if (!(l > 0.0)) return;
    gx = nx / l;
    gy = ny / l;
    gz = nz / l;
}

// The distance from p to scene h (Scene.distance, the swept kernel): the full search and its value.
__device__ __forceinline__ double mesh_distance(const MeshDev& M, const MeshHdr& h, double px, double py, double pz) {
    return mesh_value(M, h, mesh_search(M, h, px, py, pz, INFINITY), px, py, pz);
}

// The distance from p at time t to scene h of a mesh set with movers (scene_distance_mesh_mixed_kernel, the swept
// kernel): the minimum of mesh_distance and of frame_distance over the scene's mcnt movers P, the bits of
// fmin(mesh_distance, the movers' minimum).  The movers come first and give d_m.  An open set is searched only up to
// d_m: with d_m < 0 not at all (its distance is >= 0), else with the bound d_m^2 (1 + 2^-50), which as rounded is still
// > d_m^2 -- a triangle beyond it has a correctly rounded root strictly above d_m and can neither lower the minimum nor
// tie with it, and every triangle at or below it is treated as in the full search (mesh_search).  A closed set takes
// the full walk: its sign needs the nearest triangle, however far that is.
__device__ __forceinline__ double mesh_mixed_distance(const MeshDev& M, const MeshHdr& h, const ScenePrimDyn* P, int mcnt,
                                                      double t, double px, double py, double pz) {
#pragma clang fp contract(off)
    double dm = INFINITY;
    for (int i = 0; i < mcnt; ++i) dm = fmin(dm, frame_distance(P[i], t, px, py, pz));
    if (M.tn) return fmin(mesh_distance(M, h, px, py, pz), dm);
    if (dm < 0.0) return dm;
    const MeshHit w = mesh_search(M, h, px, py, pz, dm * dm * (1.0 + 0x1p-50));
    return fmin(sqrt(w.d2), dm);
}

}  // namespace sdfn
