// Device code of the instanced kernels (scene_inst.hip, and scene_swept.hip's kernel over inst_distance): the linear pass
// over a scene's instances in fp64.  An instance is a part of the set's pool -- a mesh with its own hierarchy, stored
// once in its own coordinates -- under a rigid frame c(t), R(t) (prim_frame); a query point goes into the part's frame,
// x' = R(t)^T (x - c(t)) (frame_point), and the part answers through the functions of the mesh kernels (mesh_dev.h).
//
// The answer of a scene is the minimum over its instances, the lowest instance index on a tie, and it is the same bits
// whatever is pruned: an instance or a triangle is rejected only when it is strictly farther than the best so far.
//   open set    instance i is searched with the bound best^2 (1 + 2^-50), mesh_mixed_distance's: as rounded still
//               > best^2, so a triangle beyond it has a correctly rounded root strictly above best, and every triangle at
//               or below it is treated as in the full search (mesh_search).  An instance whose root box is strictly
//               beyond that bound is not searched at all (inst_far): the search would open no node and find nothing,
//               after a descent to a first leaf that the test saves.
//   closed set  the sign needs the nearest triangle, so an instance that is visited takes the full walk.  One whose
//               root box does not contain x' is skipped when the box is farther than max(best, 0): a point outside the
//               box is outside the solid, so d_i is positive and at least the box's distance, which the margin of the
//               box (mesh_bvh.h) keeps below the distance of every triangle by far more than the rounding of either.
// With one instance at p = 0, q = identity and no motion x' is x to the bit (c = 0 and R = I exactly; dot3_pinned adds
// exact zeros), and the functions below reduce to the calls of the mesh kernels.
#pragma once
#include "mesh_dev.h"

namespace sdfn {

// scene s of an instanced set: its records and their number, clamped
struct InstRange {
    const ScenePrimDyn* rec;
    int cnt;
};
__device__ __forceinline__ InstRange inst_range(const InstDev& I, long long s) {
    return InstRange{I.rec + max(I.ioff[s], 0), min(max(I.icount[s], 0), SCENE_MAX_INSTANCES)};
}
__device__ __forceinline__ int inst_part(const InstDev& I, const ScenePrimDyn& P) {
    return min(max(P.kind, 0), I.nparts - 1);  // clamped: never outside the pool
}

// whether an open part holds nothing within the squared bound b2 of x': no triangles, or its root box strictly beyond b2
__device__ __forceinline__ bool inst_far(const MeshDev& M, const MeshHdr& h, double qx, double qy, double qz, double b2) {
    return h.nnodes <= 0 || mesh_box_d2(M.nodes[h.node_off], qx, qy, qz) > b2;
}

// whether a closed part can be left out at x' given the best value so far (cap: what the caller stops caring at, max_df
// for a row, +inf otherwise): its root box is strictly farther than max(min(best, cap), 0)
__device__ __forceinline__ bool inst_skip_closed(const MeshDev& M, const MeshHdr& h, double qx, double qy, double qz,
                                                 double best, double cap) {
#pragma clang fp contract(off)
    if (h.nnodes <= 0) return true;  // a part without triangles is at +inf
    const double b2 = mesh_box_d2(M.nodes[h.node_off], qx, qy, qz);
    const double mb = fmax(fmin(best, cap), 0.0);
    return b2 > 0.0 && b2 > mb * mb * (1.0 + 0x1p-50);
}

// The distance from p at time t to the instances of scene s (scene_distance_inst_kernel, the swept kernel): the bits
// of the minimum over i of mesh_distance of part(i) at x'_i.  No instance: +inf.
__device__ __forceinline__ double inst_distance(const MeshDev& M, const InstDev& I, const InstRange& sc, double t,
                                                double px, double py, double pz) {
#pragma clang fp contract(off)
    double best = INFINITY;
    // Two loops, so that the lanes of a wave meet at the search: each lane first runs ahead, through the cheap frame and
    // root-box tests, to *its own* next instance that needs a search, and the wave then searches one instance per lane
    // together.  A lane still visits its instances in index order with the same running best -- the bits are those of
    // the single loop -- but a wave pays the largest number of searches of any of its lanes, not the number of
    // instances that some lane has to search.  Every trip count is bounded by the scene's count.
    int i = 0;
    for (int it = 0; it < sc.cnt; ++it) {
        MeshHdr h{};
        double qx = 0.0, qy = 0.0, qz = 0.0, b2 = INFINITY;
        bool todo = false;
        for (; i < sc.cnt && !todo; ++i) {
            const ScenePrimDyn& P = sc.rec[i];
            h = M.hdr[inst_part(I, P)];
            double R[9];
            frame_point(P, t, px, py, pz, R, qx, qy, qz);
            b2 = best * best * (1.0 + 0x1p-50);
            todo = M.tn ? !inst_skip_closed(M, h, qx, qy, qz, best, INFINITY) : !inst_far(M, h, qx, qy, qz, b2);
        }
        if (!todo) break;
        if (M.tn) best = fmin(best, mesh_distance(M, h, qx, qy, qz));
        else best = fmin(best, sqrt(mesh_search(M, h, qx, qy, qz, b2).d2));
    }
    return best;
}

}  // namespace sdfn
