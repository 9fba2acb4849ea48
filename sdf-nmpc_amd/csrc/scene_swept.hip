// Swept clearance: the minimum of the scene's signed distance over a segment of space-time, with a certificate.
//
// Segment j runs from (p0, t0) to (p1, t1): p(s) = p0 + s (p1 - p0), t(s) = t0 + s (t1 - t0), s in [0, 1], and D(s) is
// the signed distance from p(s) to the segment's scene at time t(s) -- what the distance kernels return for that point
// and time, from the device functions they call (scene_dev.h).  D is Lipschitz in s with L = |p1 - p0| + V |t1 - t0|,
// where V bounds the speed of any surface point of any mover of the scene (SceneSweptArgs::vmax, formed on the host):
// a distance field is 1-Lipschitz in space, and moves by at most the displacement of its surface in time.
//
// One lane per segment runs a deterministic Lipschitz branch and bound on dyadic intervals.  On an
// interval [a, b] of width w with end values d_a, d_b no value lies below lb = (d_a + d_b - L w) / 2.  An interval with
// lb >= best - eps is dropped; otherwise its midpoint is evaluated and its halves are searched, the left one first,
// from an explicit stack.  An interval of width 2^-SWEPT_DEPTH is not halved, and once max_evals evaluations are used
// none is: what is then on the stack is dropped as it is.  lbmin is the smallest lb of every interval dropped, for
// whatever reason, so the true minimum lies in [best - gap, best] with gap = max(0, best - lbmin), and gap <= eps when
// every interval was dropped by the test.
//
// Termination.  Every evaluation pushes two intervals and every round of the loop pops one, so 2 max_evals rounds
// empty the stack: the trip count is fixed before the loop starts.  The stack holds at most one right half per level
// and the interval in hand, SWEPT_DEPTH + 1 entries; a push is checked against SWEPT_STACK all the same.  A non-finite
// coordinate or time ends the lane before the first evaluation with NaN in dmin, s and gap and 0 in evals, and every
// comparison of the search is written so that a NaN drops the interval.  No atomics, no cross-lane traffic, no LDS.
//
// The stack is indexed at run time and lives in scratch memory: 24 entries of 24 bytes per lane, touched once per
// interval beside an evaluation that costs hundreds of fp64 operations per primitive.
#include "inst_dev.h"
#include "mesh_dev.h"
#include "scene_dev.h"

namespace sdfn {

namespace {

constexpr int SWEPT_DEPTH = 20;  // the narrowest interval is 2^-20 of the segment
constexpr int SWEPT_STACK = 24;  // >= SWEPT_DEPTH + 1

struct SweptItem {
    int level, idx;  // the interval [idx, idx + 1] 2^-level
    double da, db;   // D at its ends
};

// ---- the point evaluators: D at a point and a time for segment j of scene s, each through the functions of the
// distance kernel of its kind of set
struct EvalStatic {  // scene_distance_kernel
    const ScenePrimD* P;
    int cnt;
    __device__ EvalStatic(const SceneSweptArgs& A, long long s)
        : P(A.sc.pd + s * SCENE_MAX_PRIMS), cnt(min(A.sc.count[s], SCENE_MAX_PRIMS)) {}
    __device__ double operator()(double px, double py, double pz, double) const {
        double best = INFINITY;
        for (int i = 0; i < cnt; ++i) best = fmin(best, prim_distance(P[i], px, py, pz));
        return best;
    }
};

struct EvalDyn {  // scene_distance_dyn_kernel
    const ScenePrimDyn* P;
    int cnt;
    __device__ EvalDyn(const SceneSweptArgs& A, long long s)
        : P(A.dyn + s * SCENE_MAX_PRIMS), cnt(min(A.sc.count[s], SCENE_MAX_PRIMS)) {}
    __device__ double operator()(double px, double py, double pz, double t) const {
        double best = INFINITY;
        for (int i = 0; i < cnt; ++i) best = fmin(best, frame_distance(P[i], t, px, py, pz));
        return best;
    }
};

struct EvalGrid {  // scene_distance_grid_kernel
    const SceneGridHdr& G;
    const ScenePrimD* P;
    const int *cs, *items;
    __device__ EvalGrid(const SceneSweptArgs& A, long long s)
        : G(A.sc.ghdr[s]), P(A.sc.pd + G.prim_off), cs(A.sc.cell_start + G.cell_off), items(A.sc.cell_items) {}
    __device__ double operator()(double px, double py, double pz, double) const {
        double best = INFINITY;
        const ScenePrimD* Q = P;
        grid_ring_search(
            G, cs, items, px, py, pz, [&](int i) { best = fmin(best, prim_distance(Q[i], px, py, pz)); },
            [&] { return best; });
        return best;
    }
};

struct EvalMixed {  // scene_distance_mixed_kernel: the movers first, then the ring search bounded by what they give
    EvalGrid g;
    const ScenePrimDyn* M;
    int mcnt;
    __device__ EvalMixed(const SceneSweptArgs& A, long long s)
        : g(A, s), M(A.dyn + s * SCENE_MAX_PRIMS), mcnt(min(max(A.mcount[s], 0), SCENE_MAX_PRIMS)) {}
    __device__ double operator()(double px, double py, double pz, double t) const {
        double best = INFINITY;
        for (int i = 0; i < mcnt; ++i) best = fmin(best, frame_distance(M[i], t, px, py, pz));
        const ScenePrimD* Q = g.P;
        grid_ring_search(
            g.G, g.cs, g.items, px, py, pz, [&](int i) { best = fmin(best, prim_distance(Q[i], px, py, pz)); },
            [&] { return best; });
        return best;
    }
};

struct EvalMesh {  // scene_distance_mesh_kernel: a static set of triangles, signed when the set is closed (mesh_dev.h)
    const MeshDev& M;
    MeshHdr h;
    __device__ EvalMesh(const SceneSweptArgs& A, long long s) : M(A.mesh), h(A.mesh.hdr[s]) {}
    __device__ double operator()(double px, double py, double pz, double) const { return mesh_distance(M, h, px, py, pz); }
};

struct EvalMeshMixed {  // scene_distance_mesh_mixed_kernel: the movers first, then the mesh searched from what they give
    const MeshDev& M;
    MeshHdr h;
    const ScenePrimDyn* P;
    int mcnt;
    __device__ EvalMeshMixed(const SceneSweptArgs& A, long long s)
        : M(A.mesh), h(A.mesh.hdr[s]), P(A.dyn + s * SCENE_MAX_PRIMS), mcnt(min(max(A.mcount[s], 0), SCENE_MAX_PRIMS)) {}
    __device__ double operator()(double px, double py, double pz, double t) const {
        return mesh_mixed_distance(M, h, P, mcnt, t, px, py, pz);
    }
};

struct EvalInst {  // scene_distance_inst_kernel: the linear pass over the scene's instances at the point's time (inst_dev.h)
    const MeshDev& M;
    const InstDev& I;
    InstRange r;
    __device__ EvalInst(const InstSweptArgs& D, long long s) : M(D.a.mesh), I(D.inst), r(inst_range(D.inst, s)) {}
    __device__ double operator()(double px, double py, double pz, double t) const {
        return inst_distance(M, I, r, t, px, py, pz);
    }
};

// the kernel's argument block is SceneSweptArgs, or a structure of its own that holds one (an instanced set)
__host__ __device__ __forceinline__ const SceneSweptArgs& swept_base(const SceneSweptArgs& a) { return a; }
__host__ __device__ __forceinline__ const SceneSweptArgs& swept_base(const InstSweptArgs& a) { return a.a; }

__device__ __forceinline__ bool finite3(const double* v) { return isfinite(v[0]) && isfinite(v[1]) && isfinite(v[2]); }

// TIMED: the set is dynamic, so the times are read and the movers' speed bound enters L
template <class Eval, bool TIMED, class Args>
__global__ __launch_bounds__(SCENE_BLOCK) void scene_swept_kernel(Args AA) {
    const SceneSweptArgs& A = swept_base(AA);
    const long long j = (long long)blockIdx.x * SCENE_BLOCK + threadIdx.x;
    if (j >= A.n) return;
    const long long s = A.p_to_scene ? (long long)min(max(A.p_to_scene[j], 0), A.sc.S - 1) : j / A.per_scene;
    const double* a0 = A.p0 + j * 3;
    const double* a1 = A.p1 + j * 3;
    const double px = a0[0], py = a0[1], pz = a0[2];
    const double e[3] = {a1[0] - px, a1[1] - py, a1[2] - pz};
    double ta = 0.0, te = 0.0;
    if (TIMED && A.t0) {
        ta = A.t0[j];
        te = A.t1[j] - ta;
    }
    auto put = [&](double dmin, double sb, double gap, int evals) {
        A.dmin[j] = dmin;
        if (A.s) A.s[j] = sb;
        if (A.gap) A.gap[j] = gap;
        if (A.evals) A.evals[j] = evals;
    };
    // every point of the segment is finite when its start and its extent are
    if (!(finite3(a0) && finite3(e) && isfinite(ta) && isfinite(te))) {
        put(NAN, NAN, NAN, 0);
        return;
    }
    // rounded up by more than the norm's own rounding: L is to be a bound
    const double L = (sqrt(e[0] * e[0] + e[1] * e[1] + e[2] * e[2]) + (TIMED ? A.vmax[s] * fabs(te) : 0.0)) * (1.0 + 0x1p-50);
    const Eval D(AA, s);
    auto at = [&](double u) { return D(px + u * e[0], py + u * e[1], pz + u * e[2], ta + u * te); };

    double best = at(0.0), sbest = 0.0;
    int evals = 1;
    if (!(L > 0.0)) {  // a point: D is constant
        put(best, 0.0, 0.0, 1);
        return;
    }
    SweptItem st[SWEPT_STACK];
    {
        const double d1 = at(1.0);
        evals = 2;
        st[0] = SweptItem{0, 0, best, d1};
        if (d1 < best) {  // a tie keeps s = 0
            best = d1;
            sbest = 1.0;
        }
    }
    int sp = 1;
    double lbmin = INFINITY;
    const int max_evals = A.max_evals;
    const int rounds = 2 * max_evals;  // every evaluation pushes two intervals, every round pops one
    for (int it = 0; it < rounds && sp > 0; ++it) {
        const SweptItem q = st[--sp];
        const double w = ldexp(1.0, -q.level);
        const double lb = 0.5 * (q.da + q.db - L * w);
        const bool refine = lb < best - A.eps && q.level < SWEPT_DEPTH && evals < max_evals && sp + 2 <= SWEPT_STACK;
        if (!refine) {  // dropped: by the test, at the depth cap or out of budget (a NaN drops it too)
            lbmin = fmin(lbmin, lb);
            continue;
        }
        const double sm = ldexp((double)(2 * q.idx + 1), -(q.level + 1));
        const double dm = at(sm);
        ++evals;
        if (dm < best || (dm == best && sm < sbest)) {  // the smaller s on a tie
            best = dm;
            sbest = sm;
        }
        st[sp++] = SweptItem{q.level + 1, 2 * q.idx + 1, dm, q.db};  // the right half waits
        st[sp++] = SweptItem{q.level + 1, 2 * q.idx, q.da, dm};      // the left half is next
    }
    // an empty scene: best = lbmin = +inf, no gap
    put(best, sbest, lbmin < best ? best - lbmin : 0.0, evals);
}

template <class Eval, bool TIMED, class Args>
hipError_t launch_swept(const Args& a, hipStream_t s) {
    const long long n = swept_base(a).n;
    if (n <= 0) return hipSuccess;
    hipLaunchKernelGGL((scene_swept_kernel<Eval, TIMED, Args>), dim3((unsigned)((n + SCENE_BLOCK - 1) / SCENE_BLOCK)),
                       dim3(SCENE_BLOCK), 0, s, a);
    return hipGetLastError();
}

}  // namespace

hipError_t launch_scene_swept(const SceneSweptArgs& a, hipStream_t s) { return launch_swept<EvalStatic, false>(a, s); }
hipError_t launch_scene_swept_dyn(const SceneSweptArgs& a, hipStream_t s) { return launch_swept<EvalDyn, true>(a, s); }
hipError_t launch_scene_swept_grid(const SceneSweptArgs& a, hipStream_t s) { return launch_swept<EvalGrid, false>(a, s); }
hipError_t launch_scene_swept_mixed(const SceneSweptArgs& a, hipStream_t s) { return launch_swept<EvalMixed, true>(a, s); }
hipError_t launch_scene_swept_mesh(const SceneSweptArgs& a, hipStream_t s) { return launch_swept<EvalMesh, false>(a, s); }
hipError_t launch_scene_swept_mesh_mixed(const SceneSweptArgs& a, hipStream_t s) {
    return launch_swept<EvalMeshMixed, true>(a, s);
}
// TIMED: the times are read; the engine passes none for a set whose instances all stand still, and vmax is 0 then
hipError_t launch_scene_swept_inst(const InstSweptArgs& a, hipStream_t s) { return launch_swept<EvalInst, true>(a, s); }

}  // namespace sdfn
