// Stand-alone host check of instanced mesh sets (csrc/scene_inst.hip, csrc/inst_dev.h) through the header the library
// and the kernels share (csrc/mesh_bvh.h: the check of a part, the hierarchy, the device layout), meant to be built with
// a sanitizer:
//
//   g++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all \
//       -o tools/_mesh_inst_check tools/mesh_inst_check.cpp && tools/_mesh_inst_check
//
// It builds a pool of two parts (a closed box and an open, bumpy 9 x 9 patch) as sdfnmpc_scene_create_instanced lays it
// out -- one MeshHdr per part, the nodes and the triangles of all parts in one array each, in heap blocks of exactly
// their size -- and a scene of six instances with rotated, yawing, sliding and swinging frames, c(t) = p + v t + amp
// sin(omega t + phase), R(t) = Rz(yaw_rate t) R(q).  For 400 points at times of their own it walks the scene as the
// distance kernel of an open set does: the point taken into every instance's frame, x' = R(t)^T (x - c(t)), the part's
// hierarchy walked without a stack from the best squared distance so far, inflated by 1 + 2^-50, a node rejected only
// when its box is strictly farther.  It compares with brute force over the transformed triangles R(t) v + c(t) in world
// coordinates (1e-12), and checks that every leaf_size (1..8 and -1) and the reversed instance list give the same bits,
// that every walk ends within nnodes steps and stays inside its part's ranges, and that an identity instance gives the
// bits of the part alone.  Exits non-zero on the first violation.
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

static const char* what = "setup";

// the closest point of the triangle v (a, b, c) to p by its Voronoi regions: the squared distance
static double tri_d2(const double* v, const double* p) {
    const double *a = v, *b = v + 3, *c = v + 6;
    double ab[3], ac[3], ap[3], bp[3], cp[3];
    for (int k = 0; k < 3; ++k) {
        ab[k] = b[k] - a[k]; ac[k] = c[k] - a[k];
        ap[k] = p[k] - a[k]; bp[k] = p[k] - b[k]; cp[k] = p[k] - c[k];
    }
    auto dot = [](const double* x, const double* y) { return x[0] * y[0] + x[1] * y[1] + x[2] * y[2]; };
    const double d1 = dot(ab, ap), d2 = dot(ac, ap), d3 = dot(ab, bp), d4 = dot(ac, bp), d5 = dot(ab, cp), d6 = dot(ac, cp);
    const double vc = d1 * d4 - d3 * d2, vb = d5 * d2 - d1 * d6, va = d3 * d6 - d5 * d4;
    double s = 0.0, t = 0.0;
    if (d1 <= 0.0 && d2 <= 0.0) {
    } else if (d3 >= 0.0 && d4 <= d3) s = 1.0;
    else if (vc <= 0.0 && d1 >= 0.0 && d3 <= 0.0) s = d1 / (d1 - d3);
    else if (d6 >= 0.0 && d5 <= d6) t = 1.0;
    else if (vb <= 0.0 && d2 >= 0.0 && d6 <= 0.0) t = d2 / (d2 - d6);
    else if (va <= 0.0 && (d4 - d3) >= 0.0 && (d5 - d6) >= 0.0) {
        t = (d4 - d3) / ((d4 - d3) + (d5 - d6));
        s = 1.0 - t;
    } else {
        const double den = 1.0 / (va + vb + vc);
        s = vb * den;
        t = vc * den;
    }
    double e2 = 0.0;
    for (int k = 0; k < 3; ++k) {
        const double e = p[k] - (a[k] + ab[k] * s + ac[k] * t);
        e2 += e * e;
    }
    return e2;
}

static double box_d2(const MeshNode& nd, const double* p) {
    double e2 = 0.0;
    for (int k = 0; k < 3; ++k) {
        const double e = std::fmax(std::fmax((double)nd.lo[k] - p[k], p[k] - (double)nd.hi[k]), 0.0);
        e2 += e * e;
    }
    return e2;
}

// the pool as the library lays it out, in exactly sized heap blocks
struct Pool {
    int nparts = 0;
    MeshHdr* hdr = nullptr;
    MeshNode* nodes = nullptr;
    MeshTriD* td = nullptr;
    int nnodes = 0, ntri = 0;
    ~Pool() {
        std::free(hdr);
        std::free(nodes);
        std::free(td);
    }
};

struct Part {
    std::vector<double> verts;
    std::vector<int> tris;
    bool closed;
};

static void build_pool(const std::vector<Part>& parts, int leaf, Pool& P) {
    std::vector<MeshHdr> hdr;
    std::vector<MeshNode> nodes;
    std::vector<MeshTriD> td;
    for (const Part& p : parts) {
        const int nv = (int)p.verts.size() / 3, nt = (int)p.tris.size() / 3;
        std::vector<float> vf;
        CHECK(mesh_check(p.verts.data(), nv, p.tris.data(), nt, p.closed, vf) == nullptr);
        const float m = mesh_margin(vf.data(), nv);
        MeshBvh b;
        mesh_bvh_build(vf.data(), p.tris.data(), nt, leaf, m, b);
        hdr.push_back(MeshHdr{(int)nodes.size(), (int)b.nodes.size(), (int)td.size(), nt, m, {0, 0, 0}});
        nodes.insert(nodes.end(), b.nodes.begin(), b.nodes.end());
        for (int k = 0; k < nt; ++k) {
            MeshTriD T{};
            for (int c = 0; c < 3; ++c)
                for (int a = 0; a < 3; ++a) T.v[c * 3 + a] = (double)vf[(size_t)p.tris[b.order[k] * 3 + c] * 3 + a];
            T.orig = b.order[k];
            td.push_back(T);
        }
    }
    P.nparts = (int)hdr.size();
    P.nnodes = (int)nodes.size();
    P.ntri = (int)td.size();
    P.hdr = (MeshHdr*)std::malloc(hdr.size() * sizeof(MeshHdr));
    P.nodes = (MeshNode*)std::malloc(nodes.size() * sizeof(MeshNode));
    P.td = (MeshTriD*)std::malloc(td.size() * sizeof(MeshTriD));
    std::memcpy(P.hdr, hdr.data(), hdr.size() * sizeof(MeshHdr));
    std::memcpy(P.nodes, nodes.data(), nodes.size() * sizeof(MeshNode));
    std::memcpy(P.td, td.data(), td.size() * sizeof(MeshTriD));
}

struct Inst {
    int part;
    double p[3], q[4], yaw_rate, v[3], amp[3], omega, phase;
};

// prim_frame's frame: c(t), R(t) row-major
static void frame(const Inst& I, double t, double* c, double* R) {
    const double qn = std::sqrt(I.q[0] * I.q[0] + I.q[1] * I.q[1] + I.q[2] * I.q[2] + I.q[3] * I.q[3]);
    const double q0 = I.q[0] / qn, q1 = I.q[1] / qn, q2 = I.q[2] / qn, q3 = I.q[3] / qn;
    const double R0[9] = {q0 * q0 + q1 * q1 - q2 * q2 - q3 * q3, 2 * (q1 * q2 - q0 * q3), 2 * (q1 * q3 + q0 * q2),
                          2 * (q1 * q2 + q0 * q3), q0 * q0 - q1 * q1 + q2 * q2 - q3 * q3, 2 * (q2 * q3 - q0 * q1),
                          2 * (q1 * q3 - q0 * q2), 2 * (q2 * q3 + q0 * q1), q0 * q0 - q1 * q1 - q2 * q2 + q3 * q3};
    const double sy = std::sin(I.yaw_rate * t), cy = std::cos(I.yaw_rate * t), sh = std::sin(I.omega * t + I.phase);
    for (int j = 0; j < 3; ++j) {
        c[j] = I.p[j] + I.v[j] * t + I.amp[j] * sh;
        R[j] = cy * R0[j] - sy * R0[3 + j];
        R[3 + j] = sy * R0[j] + cy * R0[3 + j];
        R[6 + j] = R0[6 + j];
    }
}

// the walk of one part from the bound b2 (mesh_search's, without the first descent): the smallest squared distance
// <= b2, or +inf; *steps: the rounds of the node loop
static double walk_part(const Pool& P, int part, const double* q, double b2, int* steps) {
    CHECK(part >= 0 && part < P.nparts);
    const MeshHdr h = P.hdr[part];
    CHECK(h.node_off >= 0 && h.node_off + h.nnodes <= P.nnodes && h.tri_off >= 0 && h.tri_off + h.ntri <= P.ntri);
    const MeshNode* N = P.nodes + h.node_off;
    const MeshTriD* T = P.td + h.tri_off;
    double best = b2;
    bool found = false;
    int i = 0, it = 0;
    for (; it < h.nnodes && i < h.nnodes; ++it) {
        const MeshNode nd = N[i];
        CHECK(nd.skip > i && nd.skip <= h.nnodes);
        if (box_d2(nd, q) > best) {
            i = nd.skip;
            continue;
        }
        if (nd.count == 0) {
            ++i;
            continue;
        }
        CHECK(nd.first >= 0 && nd.first + nd.count <= h.ntri);
        for (int k = nd.first; k < nd.first + nd.count; ++k) {
            const double d2 = tri_d2(T[k].v, q);
            if (d2 <= best) {
                best = d2;
                found = true;
            }
        }
        i = nd.skip;
    }
    CHECK(i >= h.nnodes);  // the walk ended by leaving the tree, within nnodes rounds
    *steps += it;
    return found ? best : INFINITY;
}

// inst_distance of an open set: the linear pass over the instances, each searched from the best so far
static double scene_distance(const Pool& P, const std::vector<Inst>& sc, const double* x, double t, int* steps) {
    double best = INFINITY;
    for (const Inst& I : sc) {
        double c[3], R[9], q[3];
        frame(I, t, c, R);
        const double e[3] = {x[0] - c[0], x[1] - c[1], x[2] - c[2]};
        for (int j = 0; j < 3; ++j) q[j] = R[j] * e[0] + R[3 + j] * e[1] + R[6 + j] * e[2];
        const double d2 = walk_part(P, I.part, q, best * best * (1.0 + 0x1p-50), steps);
        best = std::fmin(best, std::sqrt(d2));
    }
    return best;
}

// brute force in world coordinates: every triangle of every instance under its frame
static double brute(const std::vector<Part>& parts, const std::vector<Inst>& sc, const double* x, double t) {
    double best = INFINITY;
    for (const Inst& I : sc) {
        double c[3], R[9];
        frame(I, t, c, R);
        const Part& p = parts[I.part];
        for (size_t k = 0; k + 2 < p.tris.size(); k += 3) {
            double w[9];
            for (int cnr = 0; cnr < 3; ++cnr) {
                double v[3];
                for (int a = 0; a < 3; ++a) v[a] = (double)(float)p.verts[(size_t)p.tris[k + cnr] * 3 + a];
                for (int a = 0; a < 3; ++a) w[cnr * 3 + a] = R[a * 3] * v[0] + R[a * 3 + 1] * v[1] + R[a * 3 + 2] * v[2] + c[a];
            }
            best = std::fmin(best, std::sqrt(tri_d2(w, x)));
        }
    }
    return best;
}

static double rnd(unsigned& s) {  // in [0, 1)
    s = s * 1664525u + 1013904223u;
    return (double)(s >> 8) / (double)(1u << 24);
}

int main() {
    static_assert(sizeof(MeshNode) == 48 && sizeof(MeshTriD) == 80 && sizeof(MeshHdr) == 32, "the device layout");
    std::vector<Part> parts(2);
    {  // a closed box, 0.8 x 0.5 x 1.2
        const double h[3] = {0.4, 0.25, 0.6};
        for (int i = 0; i < 8; ++i)
            for (int a = 0; a < 3; ++a) parts[0].verts.push_back((i >> a & 1) ? h[a] : -h[a]);
        const int t[36] = {0, 2, 3, 0, 3, 1, 4, 5, 7, 4, 7, 6, 0, 1, 5, 0, 5, 4, 2, 7, 3, 2, 6, 7, 0, 4, 6, 0, 6, 2, 1, 3, 7, 1, 7, 5};
        parts[0].tris.assign(t, t + 36);
        parts[0].closed = true;
    }
    {  // an open bumpy patch, 9 x 9 vertices, 128 triangles
        const int G = 9;
        for (int i = 0; i < G; ++i)
            for (int j = 0; j < G; ++j) {
                parts[1].verts.push_back(-1.0 + 0.25 * i);
                parts[1].verts.push_back(-1.0 + 0.25 * j);
                parts[1].verts.push_back(0.2 * std::sin(0.9 * i) * std::cos(0.7 * j));
            }
        for (int i = 0; i + 1 < G; ++i)
            for (int j = 0; j + 1 < G; ++j) {
                const int a = i * G + j;
                const int q[6] = {a, a + G, a + G + 1, a, a + G + 1, a + 1};
                parts[1].tris.insert(parts[1].tris.end(), q, q + 6);
            }
        parts[1].closed = false;
    }
    std::vector<Inst> scene = {
        {1, {0.0, 0.0, -1.5}, {1, 0, 0, 0}, 0.0, {0, 0, 0}, {0, 0, 0}, 0.0, 0.0},
        {0, {3.0, 1.0, 0.1}, {0.9, 0.1, -0.2, 0.3}, 0.4, {0.0, -0.5, 0.0}, {0, 0, 0}, 0.0, 0.0},
        {0, {1.5, -1.6, 0.0}, {0.92, 0.0, 0.0, 0.38}, 0.0, {0, 0, 0}, {0.0, 0.0, 0.25}, 2.0, 0.3},
        {1, {2.5, 0.5, 1.0}, {0.7, 0.7, 0.1, 0.0}, 1.0, {0.25, 0.5, 0.0}, {0, 0, 0}, 0.0, 0.0},
        {0, {4.5, -1.0, -0.5}, {2.0, 0.2, 0.4, 0.6}, -0.8, {0, 0, 0}, {0.5, 0.0, 0.0}, 1.5, 0.0},
        {0, {3.1, 1.1, 0.2}, {1, 0, 0, 0}, 0.0, {0, 0, 0}, {0, 0, 0}, 0.0, 0.0},  // overlaps instance 1
    };
    const int n = 400;
    std::vector<double> pts((size_t)n * 3), times((size_t)n), base((size_t)n);
    unsigned seed = 12345u;
    for (int j = 0; j < n; ++j) {
        pts[j * 3] = -1.0 + 7.0 * rnd(seed);
        pts[j * 3 + 1] = -3.0 + 6.0 * rnd(seed);
        pts[j * 3 + 2] = -2.5 + 5.0 * rnd(seed);
        times[j] = 2.0 * rnd(seed);
    }
    const int leaves[] = {-1, 1, 2, 3, 4, 5, 6, 7, 8};
    std::vector<Inst> reversed(scene.rbegin(), scene.rend());
    double worst = 0.0;
    long long steps_brute = 0, steps_tree = 0;
    for (int leaf : leaves) {
        Pool P;
        build_pool(parts, leaf, P);
        CHECK(P.nparts == 2 && P.ntri == 12 + 128);
        for (int j = 0; j < n; ++j) {
            int steps = 0;
            what = "walk";
            const double d = scene_distance(P, scene, &pts[(size_t)j * 3], times[j], &steps);
            CHECK(std::isfinite(d) && d >= 0.0);
            if (leaf == -1) {
                what = "against brute force over the transformed triangles";
                base[j] = d;
                const double w = brute(parts, scene, &pts[(size_t)j * 3], times[j]);
                worst = std::fmax(worst, std::fabs(d - w));
                CHECK(std::fabs(d - w) <= 1e-12);
                steps_brute += steps;
            } else {
                what = "the hierarchy changes no bit";
                CHECK(std::memcmp(&d, &base[j], sizeof(double)) == 0);
                if (leaf == 4) steps_tree += steps;
            }
            what = "the order of the instances changes no bit";
            int s2 = 0;
            const double r = scene_distance(P, reversed, &pts[(size_t)j * 3], times[j], &s2);
            CHECK(std::memcmp(&r, &base[j], sizeof(double)) == 0);
        }
        // an identity instance is the part alone; a NaN point ends every walk with nothing found
        what = "identity instance";
        const std::vector<Inst> ident = {{1, {0, 0, 0}, {1, 0, 0, 0}, 0.0, {0, 0, 0}, {0, 0, 0}, 0.0, 0.0}};
        for (int j = 0; j < 50; ++j) {
            int s = 0;
            const double a = scene_distance(P, ident, &pts[(size_t)j * 3], times[j], &s);
            const double b = std::sqrt(walk_part(P, 1, &pts[(size_t)j * 3], INFINITY, &s));
            CHECK(std::memcmp(&a, &b, sizeof(double)) == 0);
        }
        what = "a NaN point";
        const double nanp[3] = {NAN, 0.0, 0.0};
        int s = 0;
        CHECK(std::isinf(scene_distance(P, scene, nanp, 0.5, &s)));
        what = "no instances";
        CHECK(std::isinf(scene_distance(P, {}, &pts[0], 0.0, &s)));
    }
    std::printf("mesh_inst_check: ok (worst |walk - brute force| %.2e; node rounds per point: %.1f with leaf 4, %.1f with "
                "one leaf per part)\n", worst, (double)steps_tree / n, (double)steps_brute / n);
    return 0;
}
