// Stand-alone host check of the mesh hierarchy builder (csrc/mesh_bvh.h), meant to be built with a sanitizer:
//
//   g++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all \
//       -o tools/_mesh_bvh_check tools/mesh_bvh_check.cpp && tools/_mesh_bvh_check
//
// It builds hierarchies for 0 triangles, 1 triangle, 2 identical triangles, 64 coplanar triangles with pairwise
// identical centroids and a heightfield of 10 082 triangles, at every leaf_size (1..8 and -1), with the vertices and
// indices in heap blocks of exactly their size, and checks: every triangle is in exactly one leaf, every leaf is
// within leaf_size, child boxes are inside parent boxes, each leaf's triangles are inside its box (which is their
// bounds widened by the margin), every skip index lies in (i, nnodes], and the walk from the root that rejects
// everything and the one that accepts everything both end after at most nnodes steps.  Also mesh_check's refusals and
// the pseudonormals of a closed box.  Exits non-zero on the first violation.
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../sdf-nmpc_amd/csrc/mesh_bvh.h"

using namespace sdfn;

#define CHECK(c)                                                                   \
    do {                                                                           \
        if (!(c)) {                                                                \
            std::printf("FAILED %s:%d: %s (%s)\n", __FILE__, __LINE__, #c, what);  \
            std::exit(1);                                                          \
        }                                                                          \
    } while (0)

static void check(const char* what, const std::vector<float>& verts, const std::vector<int>& tris, int leaf_size) {
    const int nv = (int)verts.size() / 3, nt = (int)tris.size() / 3;
    float* v = (float*)std::malloc(verts.empty() ? 1 : verts.size() * sizeof(float));  // exactly sized: an overrun is seen
    int* t = (int*)std::malloc(tris.empty() ? 1 : tris.size() * sizeof(int));
    if (!verts.empty()) std::memcpy(v, verts.data(), verts.size() * sizeof(float));
    if (!tris.empty()) std::memcpy(t, tris.data(), tris.size() * sizeof(int));
    const float m = mesh_margin(v, nv);
    MeshBvh b;
    mesh_bvh_build(v, t, nt, leaf_size, m, b);
    const int nn = (int)b.nodes.size();
    CHECK((int)b.order.size() == nt);
    if (nt == 0) {
        CHECK(nn == 0);
        std::free(v);
        std::free(t);
        return;
    }
    CHECK(nn >= 1 && m > 0.f);
    if (leaf_size < 0) CHECK(nn == 1);
    std::vector<int> seen((size_t)nt, 0), pos((size_t)nt, 0);
    for (int k = 0; k < nt; ++k) {
        CHECK(b.order[k] >= 0 && b.order[k] < nt);
        ++pos[b.order[k]];
    }
    for (int k = 0; k < nt; ++k) CHECK(pos[k] == 1);  // order is a permutation
    // parents by a preorder walk: the children of an inner node i are i + 1 and skip(i + 1)
    std::vector<int> parent((size_t)nn, -1);
    for (int i = 0; i < nn; ++i) {
        const MeshNode& n = b.nodes[i];
        CHECK(n.skip > i && n.skip <= nn);
        for (int a = 0; a < 3; ++a) CHECK(n.lo[a] <= n.hi[a] && std::isfinite(n.lo[a]) && std::isfinite(n.hi[a]));
        if (n.count == 0) {
            CHECK(i + 1 < nn);
            const int r = b.nodes[i + 1].skip;
            CHECK(r < nn && r < n.skip);
            parent[i + 1] = i;
            parent[r] = i;
            CHECK(b.nodes[r].skip == n.skip);
        } else {
            CHECK(n.skip == i + 1);
            CHECK(n.count >= 1 && (leaf_size < 0 || n.count <= leaf_size));
            CHECK(n.first >= 0 && n.first + n.count <= nt);
            float lo[3] = {INFINITY, INFINITY, INFINITY}, hi[3] = {-INFINITY, -INFINITY, -INFINITY};
            for (int k = n.first; k < n.first + n.count; ++k) {
                ++seen[k];
                if (k > n.first) CHECK(b.order[k] > b.order[k - 1]);  // ascending original index within a leaf
                for (int c = 0; c < 3; ++c)
                    for (int a = 0; a < 3; ++a) {
                        const float x = v[(size_t)t[b.order[k] * 3 + c] * 3 + a];
                        CHECK(x >= n.lo[a] + 0.5f * m && x <= n.hi[a] - 0.5f * m);  // inside, by the margin
                        lo[a] = std::fmin(lo[a], x);
                        hi[a] = std::fmax(hi[a], x);
                    }
            }
            for (int a = 0; a < 3; ++a) CHECK(n.lo[a] == lo[a] - m && n.hi[a] == hi[a] + m);
        }
    }
    for (int k = 0; k < nt; ++k) CHECK(seen[k] == 1);  // every triangle in exactly one leaf
    for (int i = 1; i < nn; ++i) {
        CHECK(parent[i] >= 0);
        for (int a = 0; a < 3; ++a)
            CHECK(b.nodes[i].lo[a] >= b.nodes[parent[i]].lo[a] && b.nodes[i].hi[a] <= b.nodes[parent[i]].hi[a]);
    }
    int steps = 0;
    for (int i = 0; i < nn; i = b.nodes[i].skip) CHECK(++steps <= nn);  // reject everything
    steps = 0;
    int leaves = 0;
    for (int i = 0; i < nn;) {  // accept everything
        CHECK(++steps <= nn);
        leaves += b.nodes[i].count != 0;
        i = b.nodes[i].count == 0 ? i + 1 : b.nodes[i].skip;
    }
    CHECK(steps == nn && leaves >= 1);
    // the build is deterministic
    MeshBvh c;
    mesh_bvh_build(v, t, nt, leaf_size, m, c);
    CHECK(c.order == b.order && c.nodes.size() == b.nodes.size() &&
          std::memcmp(c.nodes.data(), b.nodes.data(), b.nodes.size() * sizeof(MeshNode)) == 0);
    std::free(v);
    std::free(t);
}

int main() {
    const char* what = "setup";
    static_assert(sizeof(MeshNode) == 48 && sizeof(MeshTriF) == 64 && sizeof(MeshTriD) == 80 && sizeof(MeshTriN) == 168 &&
                      sizeof(MeshHdr) == 32, "the device layout");
    const int leaves[] = {1, 2, 3, 4, 5, 6, 7, 8, -1};
    std::vector<float> one = {0, 0, 0, 1, 0, 0, 0, 1, 0};
    // 64 coplanar triangles, identical centroids pairwise: triangle 2 k + 1 is triangle 2 k rotated about its centroid
    std::vector<float> cv;
    std::vector<int> ct;
    for (int k = 0; k < 32; ++k) {
        const float x = (float)(k % 8) * 3.f, y = (float)(k / 8) * 3.f;
        const float p[6][2] = {{x, y}, {x + 3, y}, {x, y + 3}, {x + 2, y + 2}, {x - 1, y + 2}, {x + 2, y - 1}};
        for (int i = 0; i < 6; ++i) {
            cv.push_back(p[i][0]);
            cv.push_back(p[i][1]);
            cv.push_back(0.5f);
        }
        for (int i = 0; i < 6; ++i) ct.push_back(k * 6 + i);
    }
    // a 72 x 72 heightfield: 2 * 71 * 71 = 10 082 triangles
    std::vector<float> hv;
    std::vector<int> ht;
    const int G = 72;
    for (int i = 0; i < G; ++i)
        for (int j = 0; j < G; ++j) {
            hv.push_back(-5.f + 0.15f * (float)i);
            hv.push_back(-5.f + 0.15f * (float)j);
            hv.push_back(0.4f * std::sin(0.3f * (float)i) * std::cos(0.2f * (float)j));
        }
    for (int i = 0; i + 1 < G; ++i)
        for (int j = 0; j + 1 < G; ++j) {
            const int a = i * G + j;
            const int q[6] = {a, a + G, a + G + 1, a, a + G + 1, a + 1};
            ht.insert(ht.end(), q, q + 6);
        }
    for (int leaf : leaves) {
        check("no triangles", {}, {}, leaf);
        check("one triangle", one, {0, 1, 2}, leaf);
        check("two identical triangles", one, {0, 1, 2, 0, 1, 2}, leaf);
        check("64 coplanar triangles", cv, ct, leaf);
        check("heightfield", hv, ht, leaf);
    }
    // mesh_check and the pseudonormals on a closed unit box
    const double bv[24] = {0, 0, 0, 1, 0, 0, 0, 1, 0, 1, 1, 0, 0, 0, 1, 1, 0, 1, 0, 1, 1, 1, 1, 1};
    int bt[36] = {0, 2, 3, 0, 3, 1, 4, 5, 7, 4, 7, 6, 0, 1, 5, 0, 5, 4, 2, 7, 3, 2, 6, 7, 0, 4, 6, 0, 6, 2, 1, 3, 7, 1, 7, 5};
    std::vector<float> vf;
    what = "mesh_check";
    CHECK(mesh_check(bv, 8, bt, 12, true, vf) == nullptr && vf.size() == 24);
    CHECK(mesh_check(bv, 8, bt, 11, true, vf) != nullptr && mesh_check(bv, 8, bt, 11, false, vf) == nullptr);
    CHECK(mesh_check(bv, 7, bt, 12, false, vf) != nullptr);  // an index out of range
    {
        double nanv[24];
        std::memcpy(nanv, bv, sizeof(bv));
        nanv[5] = NAN;
        CHECK(mesh_check(nanv, 8, bt, 12, false, vf) != nullptr);
        const int deg[3] = {0, 1, 1};
        CHECK(mesh_check(bv, 8, deg, 1, false, vf) != nullptr);
        int fl[36];
        std::memcpy(fl, bt, sizeof(bt));
        std::swap(fl[9], fl[11]);
        CHECK(mesh_check(bv, 8, fl, 12, true, vf) != nullptr && mesh_check(bv, 8, fl, 12, false, vf) == nullptr);
    }
    CHECK(mesh_check(bv, 8, bt, 12, true, vf) == nullptr);
    std::vector<double> fn;
    std::vector<MeshTriN> pn;
    mesh_face_normals(vf.data(), bt, 12, fn);
    mesh_pseudonormals(vf.data(), 8, bt, 12, fn, pn);
    what = "pseudonormals";
    for (int i = 0; i < 12; ++i) {
        const double c[3] = {0.5, 0.5, 0.5};
        for (int r = 0; r < 7; ++r) {  // every region normal of a convex body points away from its centre
            const int vtx = bt[i * 3 + (r == 0 ? 0 : (r - 1) % 3)];
            double dot = 0.0;
            for (int a = 0; a < 3; ++a) dot += pn[i].n[r * 3 + a] * (bv[vtx * 3 + a] - c[a]);
            CHECK(dot > 0.0);
        }
        for (int k = 0; k < 3; ++k) {  // a vertex of a box: three right angles (pi / 2 in all), so the normal is along the diagonal
            const int vtx = bt[i * 3 + k];
            for (int a = 0; a < 3; ++a)
                CHECK(std::fabs(std::fabs(pn[i].n[12 + k * 3 + a]) - std::fabs(pn[i].n[12 + k * 3])) < 1e-12 &&
                      (pn[i].n[12 + k * 3 + a] > 0) == (bv[vtx * 3 + a] > 0.5));
        }
    }
    std::printf("mesh_bvh_check: ok\n");
    return 0;
}
