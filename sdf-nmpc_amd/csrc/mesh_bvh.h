// Triangle-mesh scenes, the host side (sdfnmpc_scene_create_mesh): the device layout, the check of a mesh, the
// per-triangle data and the bounding-volume hierarchy.  Header-only, plain C++ with no HIP dependency, so that a
// stand-alone host program (tools/mesh_bvh_check.cpp) can build hierarchies and walk them as the kernels do.
//
// The hierarchy.  Built top-down and deterministically over the triangles of one scene: a range of more than
// leaf_size triangles is split at the median of the triangle centroids along the longest axis of the centroid bounds
// (the lowest axis on a tie), the triangles ordered by (centroid coordinate, original index) -- a strict total order,
// so equal centroids cannot make the result depend on the sort.  Nodes are stored in depth-first preorder: the left
// child of an inner node i is i + 1, and every node carries `skip`, the index of the node that follows its subtree
// (the right child of its parent, ..., or nnodes at the end).  A traversal that rejects or finishes node i goes to
// skip, one that descends goes to i + 1: no stack.  skip > i always, so any walk ends within nnodes steps whatever
// the tests answer.  leaf_size = -1 gives one leaf that holds every triangle: the brute-force yardstick through the
// same kernels.  A scene without triangles has no nodes.
//
// Boxes and the margin.  The vertices are rounded to fp32 once; a triangle's box is the fp32 bounds of its fp32
// vertices, widened by the scene's margin m = R / 4096 (R: the largest absolute vertex coordinate of the scene) with
// one fp32 subtraction / addition per bound; a node's box is the same expression over the vertices of its range.
// fp32 rounding is monotone, so a node's box contains, bit for bit, the box of every node and triangle below it,
// and the slab interval of a ray (scene_dev.h's slab: one subtraction and one multiplication per bound, then min / max)
// of a node contains that of everything below it.  The render kernel clamps a triangle's hit into the slab interval
// of the triangle's own box and accepts it only when that interval is not empty.  So a node whose interval is empty
// or begins beyond the best hit holds no triangle that could have been accepted with a smaller value: the fp32 slab
// test can never reject a box whose triangle the fp32 hit test would accept -- by monotonicity, for every pose, and
// whatever the size of m.  What m buys is the other direction: a ray that meets a triangle in exact arithmetic
// passes through its unwidened box, and the fp32 slab errors (a few ulp of |origin| + R) stay far below R / 4096 for
// a camera within about 1000 R of the scene, so the triangle's own interval is not empty and the hit is kept.
// In the distance kernel the same boxes are read in fp64: the box of a node is at least m / sqrt(3) nearer to an
// outside point than any triangle below it, against a rounding error of about 1e-15 of the distance.
#pragma once
#include <algorithm>
#include <climits>
#include <cmath>
#include <cstdint>
#include <vector>

namespace sdfn {

// ---- the device layout (scene_mesh.hip, mesh_dev.h)
struct MeshNode {  // 48 bytes: three 16-byte reads
    float lo[3];
    int first;     // a leaf: its triangles are first .. first + count of the scene's reordered list
    float hi[3];
    int count;     // 0: an inner node (its left child is the next node)
    int skip;      // the node after this subtree, in (i, nnodes]
    int pad[3];
};
struct MeshTriF {  // 64 bytes: the render kernel's triangle
    float v[9];    // the vertices a, b, c
    float n[3];    // the unit face normal, formed in fp64 and rounded
    int flip;      // bit k: edge k (ab, bc, ca) runs from the higher vertex index to the lower one
    int pad[3];
};
struct MeshTriD {  // 80 bytes: the distance kernel's triangle
    double v[9];
    int orig;      // the triangle's index in the caller's list, for ties
    int pad;
};
struct MeshTriN {  // a closed set: the normals of the seven regions, face | edges ab, bc, ca | vertices a, b, c
    double n[21];
};
struct MeshHdr {   // one scene of the set: its nodes and triangles in the set's arrays
    int node_off, nnodes, tri_off, ntri;
    float margin;
    int pad[3];
};

constexpr int MESH_MAX_TRIS = 1 << 20;       // SDFNMPC_MESH_MAX_TRIS
constexpr int MESH_MAX_VERTS = 1 << 21;      // SDFNMPC_MESH_MAX_VERTS
constexpr long long MESH_MAX_SET_TRIS = 1 << 24;
constexpr int MESH_LEAF_DEFAULT = 4;
constexpr int MESH_LEAF_MAX = 8;

// ---- the hierarchy
struct MeshBvh {
    std::vector<MeshNode> nodes;  // preorder
    std::vector<int> order;       // reordered position -> original triangle index
};

inline float mesh_margin(const float* v, int nvert) {
    float R = 0.f;
    for (long long i = 0; i < (long long)nvert * 3; ++i) R = std::max(R, std::fabs(v[i]));
    return R / 4096.f;
}

namespace mesh_detail {

struct Builder {
    const float* v;
    const int* t;
    int leaf;
    float m;
    std::vector<double> cen;  // [ntri][3]: the sum of the three vertices (three times the centroid)
    MeshBvh& o;

    void box(int b, int e, MeshNode& n) const {
        float lo[3] = {INFINITY, INFINITY, INFINITY}, hi[3] = {-INFINITY, -INFINITY, -INFINITY};
        for (int k = b; k < e; ++k) {
            const int* tr = t + (size_t)o.order[k] * 3;
            for (int c = 0; c < 3; ++c)
                for (int a = 0; a < 3; ++a) {
                    const float x = v[(size_t)tr[c] * 3 + a];
                    lo[a] = std::min(lo[a], x);
                    hi[a] = std::max(hi[a], x);
                }
        }
        for (int a = 0; a < 3; ++a) {
            n.lo[a] = lo[a] - m;
            n.hi[a] = hi[a] + m;
        }
    }

    void rec(int b, int e) {
        const int i = (int)o.nodes.size();
        o.nodes.emplace_back();
        {
            MeshNode n{};
            box(b, e, n);
            o.nodes[i] = n;
        }
        if (e - b <= leaf) {
            std::sort(o.order.begin() + b, o.order.begin() + e);
            o.nodes[i].first = b;
            o.nodes[i].count = e - b;
            o.nodes[i].skip = i + 1;
            return;
        }
        double lo[3] = {INFINITY, INFINITY, INFINITY}, hi[3] = {-INFINITY, -INFINITY, -INFINITY};
        for (int k = b; k < e; ++k)
            for (int a = 0; a < 3; ++a) {
                const double c = cen[(size_t)o.order[k] * 3 + a];
                lo[a] = std::min(lo[a], c);
                hi[a] = std::max(hi[a], c);
            }
        int ax = 0;
        for (int a = 1; a < 3; ++a)
            if (hi[a] - lo[a] > hi[ax] - lo[ax]) ax = a;
        const int mid = b + (e - b) / 2;
        const double* cn = cen.data();
        std::nth_element(o.order.begin() + b, o.order.begin() + mid, o.order.begin() + e, [cn, ax](int p, int q) {
            const double cp = cn[(size_t)p * 3 + ax], cq = cn[(size_t)q * 3 + ax];
            return cp < cq || (cp == cq && p < q);
        });
        rec(b, mid);
        rec(mid, e);
        o.nodes[i].skip = (int)o.nodes.size();
    }
};

}  // namespace mesh_detail

// v [nvert][3] fp32 vertices, tris [ntri][3] checked indices; leaf_size 1..MESH_LEAF_MAX, or -1: one leaf
inline void mesh_bvh_build(const float* v, const int* tris, int ntri, int leaf_size, float margin, MeshBvh& out) {
    out.nodes.clear();
    out.order.resize((size_t)std::max(ntri, 0));
    for (int i = 0; i < ntri; ++i) out.order[i] = i;
    if (ntri <= 0) return;
    mesh_detail::Builder B{v, tris, leaf_size < 0 ? INT_MAX : leaf_size, margin, {}, out};
    B.cen.resize((size_t)ntri * 3);
    for (int i = 0; i < ntri; ++i)
        for (int a = 0; a < 3; ++a)
            B.cen[(size_t)i * 3 + a] = (double)v[(size_t)tris[i * 3] * 3 + a] + (double)v[(size_t)tris[i * 3 + 1] * 3 + a] +
                                       (double)v[(size_t)tris[i * 3 + 2] * 3 + a];
    out.nodes.reserve(leaf_size < 0 ? 1 : (size_t)2 * ntri / (size_t)std::max(leaf_size, 1) + 2);
    B.rec(0, ntri);
}

// ---- the check of one scene's mesh and its per-triangle data
// verts [nvert][3] fp64 as the caller gave them -> vf, the fp32 vertices.  Returns nullptr, or what is wrong.
inline const char* mesh_check(const double* verts, int nvert, const int* tris, int ntri, bool closed,
                              std::vector<float>& vf) {
    vf.resize((size_t)nvert * 3);
    for (size_t i = 0; i < (size_t)nvert * 3; ++i) {
        if (!std::isfinite(verts[i])) return "mesh: a non-finite vertex";
        vf[i] = (float)verts[i];
        if (!std::isfinite(vf[i])) return "mesh: a vertex out of fp32 range";
    }
    for (size_t i = 0; i < (size_t)ntri * 3; ++i)
        if (tris[i] < 0 || tris[i] >= nvert) return "mesh: a triangle index outside [0, nvert) of its scene";
    for (int i = 0; i < ntri; ++i) {
        const float *a = &vf[(size_t)tris[i * 3] * 3], *b = &vf[(size_t)tris[i * 3 + 1] * 3],
                    *c = &vf[(size_t)tris[i * 3 + 2] * 3];
        const double u[3] = {(double)b[0] - a[0], (double)b[1] - a[1], (double)b[2] - a[2]};
        const double w[3] = {(double)c[0] - a[0], (double)c[1] - a[1], (double)c[2] - a[2]};
        const double n[3] = {u[1] * w[2] - u[2] * w[1], u[2] * w[0] - u[0] * w[2], u[0] * w[1] - u[1] * w[0]};
        const double a2 = n[0] * n[0] + n[1] * n[1] + n[2] * n[2];
        if (!(a2 > 0.0) || !std::isfinite(a2)) return "mesh: a triangle of zero area (after rounding its vertices to fp32)";
    }
    if (closed) {  // every directed edge once, and its reverse once
        std::vector<uint64_t> e((size_t)ntri * 3);
        for (int i = 0; i < ntri; ++i)
            for (int k = 0; k < 3; ++k)
                e[(size_t)i * 3 + k] = ((uint64_t)(uint32_t)tris[i * 3 + k] << 32) | (uint32_t)tris[i * 3 + (k + 1) % 3];
        std::sort(e.begin(), e.end());
        for (size_t i = 0; i + 1 < e.size(); ++i)
            if (e[i] == e[i + 1]) return "mesh: closed = 1 needs a closed, consistently oriented manifold (an edge is "
                                         "traversed twice in the same direction)";
        for (size_t i = 0; i < e.size(); ++i) {
            const uint64_t r = (e[i] << 32) | (e[i] >> 32);
            if (!std::binary_search(e.begin(), e.end(), r))
                return "mesh: closed = 1 needs a closed, consistently oriented manifold (an edge is not shared by two "
                       "triangles in opposite directions)";
        }
    }
    return nullptr;
}

// the unit face normals [ntri][3] in fp64 from the fp32 vertices
inline void mesh_face_normals(const float* vf, const int* tris, int ntri, std::vector<double>& fn) {
    fn.resize((size_t)ntri * 3);
    for (int i = 0; i < ntri; ++i) {
        const float *a = vf + (size_t)tris[i * 3] * 3, *b = vf + (size_t)tris[i * 3 + 1] * 3, *c = vf + (size_t)tris[i * 3 + 2] * 3;
        const double u[3] = {(double)b[0] - a[0], (double)b[1] - a[1], (double)b[2] - a[2]};
        const double w[3] = {(double)c[0] - a[0], (double)c[1] - a[1], (double)c[2] - a[2]};
        const double n[3] = {u[1] * w[2] - u[2] * w[1], u[2] * w[0] - u[0] * w[2], u[0] * w[1] - u[1] * w[0]};
        const double l = std::sqrt(n[0] * n[0] + n[1] * n[1] + n[2] * n[2]);
        for (int k = 0; k < 3; ++k) fn[(size_t)i * 3 + k] = n[k] / l;
    }
}

// A closed set: per triangle (in the caller's order) the face normal, the three edge pseudonormals (the sum of the two
// adjacent unit face normals) and the three vertex pseudonormals (the angle-weighted sum of the incident unit face
// normals).  The mesh has passed mesh_check with closed = true: every edge has its one reverse.
inline void mesh_pseudonormals(const float* vf, int nvert, const int* tris, int ntri, const std::vector<double>& fn,
                               std::vector<MeshTriN>& out) {
    out.assign((size_t)ntri, MeshTriN{});
    std::vector<std::pair<uint64_t, int>> e((size_t)ntri * 3);
    for (int i = 0; i < ntri; ++i)
        for (int k = 0; k < 3; ++k)
            e[(size_t)i * 3 + k] = {((uint64_t)(uint32_t)tris[i * 3 + k] << 32) | (uint32_t)tris[i * 3 + (k + 1) % 3], i};
    std::sort(e.begin(), e.end());
    std::vector<double> vn((size_t)nvert * 3, 0.0);
    for (int i = 0; i < ntri; ++i)
        for (int k = 0; k < 3; ++k) {
            const float *p = vf + (size_t)tris[i * 3 + k] * 3, *q = vf + (size_t)tris[i * 3 + (k + 1) % 3] * 3,
                        *r = vf + (size_t)tris[i * 3 + (k + 2) % 3] * 3;
            const double u[3] = {(double)q[0] - p[0], (double)q[1] - p[1], (double)q[2] - p[2]};
            const double w[3] = {(double)r[0] - p[0], (double)r[1] - p[1], (double)r[2] - p[2]};
            const double cr[3] = {u[1] * w[2] - u[2] * w[1], u[2] * w[0] - u[0] * w[2], u[0] * w[1] - u[1] * w[0]};
            const double ang = std::atan2(std::sqrt(cr[0] * cr[0] + cr[1] * cr[1] + cr[2] * cr[2]),
                                          u[0] * w[0] + u[1] * w[1] + u[2] * w[2]);
            for (int a = 0; a < 3; ++a) vn[(size_t)tris[i * 3 + k] * 3 + a] += ang * fn[(size_t)i * 3 + a];
        }
    for (int i = 0; i < ntri; ++i) {
        MeshTriN& N = out[i];
        for (int a = 0; a < 3; ++a) N.n[a] = fn[(size_t)i * 3 + a];
        for (int k = 0; k < 3; ++k) {
            const uint64_t rev = ((uint64_t)(uint32_t)tris[i * 3 + (k + 1) % 3] << 32) | (uint32_t)tris[i * 3 + k];
            auto it = std::lower_bound(e.begin(), e.end(), std::make_pair(rev, INT_MIN));
            const int nb = (it != e.end() && it->first == rev) ? it->second : i;
            for (int a = 0; a < 3; ++a) {
                N.n[3 + k * 3 + a] = fn[(size_t)i * 3 + a] + fn[(size_t)nb * 3 + a];
                N.n[12 + k * 3 + a] = vn[(size_t)tris[i * 3 + k] * 3 + a];
            }
        }
    }
}

}  // namespace sdfn
