// NeuralDF value + full input gradient at a handful of rows for every network other than the deployed
// one (engine.cpp is_deployed): the CasADi external's latency path (config C2: acados calls sdf_l4c /
// jac_sdf_l4c one shooting node at a time, gen_model.py:39,60) for any layer sizes, embedding, res mode,
// activation and size_latent the reference's NeuralDF accepts (neural_df.py:13-103, embeddings.py:12-111,
// activation.py).  sdf_row.hip does this for the deployed architecture with compile-time shapes; here the
// shapes are the wide schedule's (sdf_wide.hip) and the operands are its row-major [N][K] matrices
// (engine.cpp upload_wide: layer widths padded to multiples of 128, padded units with zero weights).
//
// One 512-thread workgroup per row walks the layers as GEMVs.  Every operand is row-major with K
// contiguous, so a GEMV gives each output row a group of 16 lanes (one DPP row): lane q loads the row's
// float4 chunks q, q + 16, ... (each load instruction of a group contiguous), and a DPP group sum
// reduces them; 32 rows per pass of the workgroup, eight passes x four chunks per lane unrolled so a
// 256 x 256 layer's loads are all in flight at once (at one row a layer is a chain of L2 / MALL round
// trips, as sdf_row.hip explains).  The backward pass uses the transposed copies the wide schedule keeps
// (B4, B3h, B3e, B2, B1e, Bz), so it is the same GEMV.  Each GEMV's epilogue runs on lanes 0..7 of every
// group (its eight rows of the batch at once): the activation (sin(w0 .), ReLU, Softplus with threshold
// 20) and its torch backward factor, wide_gemm_kernel's epilogues element for element.
#include <hip/hip_runtime.h>

#include <atomic>

#include "sdf_row_dev.h"

namespace sdfn {

namespace {

constexpr int WR = 8;           // waves per row workgroup
constexpr int WT = 64 * WR;     // threads
constexpr int GRP = 16;         // lanes per GEMV row
constexpr int RPP = WT / GRP;   // rows per pass
constexpr int U = 8;            // passes whose loads are in flight together
constexpr int CI = 4;           // float4 chunks per lane per batch (U x CI float4 = 128 VGPRs of loads)

__device__ __forceinline__ float dot4(float4 w, float4 x, float a) {
    a = fmaf(w.x, x.x, a);
    a = fmaf(w.y, x.y, a);
    a = fmaf(w.z, x.z, a);
    return fmaf(w.w, x.w, a);
}

// epi(j, W[j][:K1 + K2] . [x1 | x2]) for j < J, the U rows of a group's batch through the epilogue at once (on
// lanes 0..U-1 of the group); W row-major with row stride K1 + K2 (multiples of 4 floats), x1 / x2 16-byte
// aligned in LDS.  Ends with a workgroup barrier.
template <typename Epi>
__device__ __forceinline__ void gemv(const float* W_, int J, const float* x1, int K1, const float* x2, int K2,
                                     Epi&& epi) {
    const float* __restrict__ W = launder(W_);
    const int t = tix(), g = t / GRP, q = t % GRP;
    const int C1 = K1 / 4, C = (K1 + K2) / 4;
    const float4* xa = (const float4*)x1;
    const float4* xb = (const float4*)x2;
    for (int j0 = g; j0 < J; j0 += U * RPP) {
        float a[U];
#pragma unroll
        for (int u = 0; u < U; ++u) a[u] = 0.0f;
        for (int c0 = q; c0 < C; c0 += CI * GRP) {
            // U rows x CI chunks of loads issued back to back (clamped addresses, dead chunks times 0)
            float4 w[U][CI];
#pragma unroll
            for (int u = 0; u < U; ++u) {
                const int j = j0 + u * RPP, jj = j < J ? j : J - 1;  // a dead row re-reads a live one
                const float4* row = (const float4*)(W + (size_t)jj * (K1 + K2));
#pragma unroll
                for (int i = 0; i < CI; ++i) {
                    const int c = c0 + i * GRP;
                    w[u][i] = row[c < C ? c : C - 1];
                }
            }
#pragma unroll
            for (int i = 0; i < CI; ++i) {
                const int c = c0 + i * GRP;
                float4 x = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
                if (c < C) x = c < C1 ? xa[c] : xb[c - C1];
#pragma unroll
                for (int u = 0; u < U; ++u) a[u] = dot4(w[u][i], x, a[u]);
            }
        }
        // every lane of a group gets the U sums; lane q < U takes row j0 + q RPP through the epilogue
        float mine = 0.0f;
#pragma unroll
        for (int u = 0; u < U; ++u) {
            const float v = group_sum<GRP>(a[u]);
            mine = q == u ? v : mine;
        }
        const int j = j0 + q * RPP;
        if (q < U && j < J) epi(j, mine);
    }
    __syncthreads();
}

// the activation of a pre-activation t and its derivative factor (wide_gemm_kernel's forward epilogue)
__device__ __forceinline__ void act_fd(int act, float w0, float t, float& h, float& d) {
    if (act == 0) {
        sdfn_sincosf(w0 * t, &h, &d);
    } else if (act == 1) {  // torch ReLU; ReluBackward passes where the output is > 0
        h = t > 0.0f ? t : 0.0f;
        d = h > 0.0f ? 1.0f : 0.0f;
    } else {  // torch Softplus(beta 1, threshold 20) and SoftplusBackward: z / (z + 1), z = exp(t)
        const float ez = expf(t);
        h = t > 20.0f ? t : log1pf(ez);
        d = t > 20.0f ? 1.0f : ez / (ez + 1.0f);
    }
}

// LDS layout of one row's evaluation (floats, every block a multiple of 4: 16-byte aligned)
struct RowLds {
    float *e, *gm, *z, *hz, *h1, *d1, *h2, *d2, *h3, *d3, *h4, *d4, *ge3, *ge1, *red;
};
__host__ __device__ inline int r4(int n) { return (n + 3) & ~3; }
__host__ __device__ inline size_t row_lds_floats(const WideDev& a) {
    return 2 * (size_t)r4(a.NEK) + (size_t)a.LZ + (a.P1 + a.P3) + 2 * (size_t)(a.P1 + a.P2 + a.P3 + a.P4) +
           2 * (size_t)a.NEB + 8;
}
__device__ inline RowLds carve(float* q, const WideDev& a) {
    RowLds s;
    auto take = [&](int n) { float* r = q; q += r4(n); return r; };
    s.e = take(a.NEK); s.gm = take(a.NEK); s.z = take(a.LZ); s.hz = take(a.P1 + a.P3);
    s.h1 = take(a.P1); s.d1 = take(a.P1); s.h2 = take(a.P2); s.d2 = take(a.P2);
    s.h3 = take(a.P3); s.d3 = take(a.P3); s.h4 = take(a.P4); s.d4 = take(a.P4);
    s.ge3 = take(a.NEB); s.ge1 = take(a.NEB); s.red = take(8);
    return s;
}

}  // namespace

// value + gradient of row r by the whole workgroup (c.pos / c.latent / c.out may point into LDS)
__device__ __forceinline__ void row_eval_wide(const WideDev& A, const RowCall& c, const int r, float* lds) {
    const RowLds s = carve(lds, A);
    const int lane = tix() & 63, wave = tix() >> 6;
    const float w0 = A.w0;
    const int act = A.act;
    const float4 p = c.pos[r];
    // ---- embedding e = [x, sin(xb), sin(xb + pi/2)] and its derivative factors (wide_emb_kernel's arithmetic)
    for (int m = tix(); m < A.NEK; m += WT) {
        float e, g;
        embed_feature(p, m, A.nb, A.emb_tab, e, g);
        s.e[m] = e;
        s.gm[m] = g;
    }
    for (int k = tix(); k < A.LZ; k += WT) s.z[k] = k < A.LH ? c.latent[(size_t)r * A.LH + k] : 0.0f;
    if (!A.e3)
        for (int m = tix(); m < A.NEB; m += WT) s.ge3[m] = 0.0f;
    __syncthreads();
    // ---- the latent's share of layers 1 and 3: hz = [W1z ; W3z] z + [b1 | b3] (the wide schedule's hoist:
    //      its STORE epilogue, acc + bias)
    gemv(A.Hz, A.P1 + A.P3, s.z, A.LZ, nullptr, 0, [&](int j, float v) { s.hz[j] = v + A.bz[j]; });
    // ---- forward, the activation (and its derivative factor) in each GEMV's epilogue
    gemv(A.F1, A.P1, s.e, A.NEK, nullptr, 0, [&](int j, float v) { act_fd(act, w0, v + s.hz[j], s.h1[j], s.d1[j]); });
    gemv(A.F2, A.P2, s.h1, A.P1, nullptr, 0, [&](int j, float v) { act_fd(act, w0, v + A.b2[j], s.h2[j], s.d2[j]); });
    gemv(A.F3, A.P3, s.h2, A.P2, A.e3 ? s.e : nullptr, A.e3 ? A.NEK : 0,
         [&](int j, float v) { act_fd(act, w0, v + s.hz[A.P1 + j], s.h3[j], s.d3[j]); });
    gemv(A.F4, A.P4, s.h3, A.P3, nullptr, 0, [&](int j, float v) {
        float h, d;
        act_fd(act, w0, v + A.b4[j], h, d);
        s.h4[j] = h;
        s.d4[j] = act == 0 ? (A.w5[j] * d) * w0 : A.w5[j] * d;  // delta4 (wide_gemm's SIN_L4 epilogue)
    });
    if (wave == 0) {  // df = w5 . h4 + b5
        float v = 0.0f;
        for (int n = lane; n < A.P4; n += 64) v = fmaf(A.w5[n], s.h4[n], v);
        v = wave_sum(v);
        if (lane == 0) s.red[0] = v + A.b5;
    }
    // ---- backward: delta_{l-1} = (W_l^T delta_l) * act'(a_{l-1}) (* w0 for sin): torch's SinBackward then
    //      MulBackward, as wide_gemm's BWD epilogue; deltas overwrite the consumed activations
    auto bwd = [&](float* dl, const float* dv) {
        return [=](int j, float v) {
            const float dd = v * dv[j];
            dl[j] = act == 0 ? dd * w0 : dd;
        };
    };
    gemv(A.B4, A.P3, s.d4, A.P4, nullptr, 0, bwd(s.h3, s.d3));
    gemv(A.B3h, A.P2, s.h3, A.P3, nullptr, 0, bwd(s.h2, s.d2));
    if (A.e3)  // res 'latent' / 'none': layer 3 does not see the embedding (ge3 zeroed with the embedding)
        gemv(A.B3e, A.NEB, s.h3, A.P3, nullptr, 0, [&](int j, float v) { s.ge3[j] = v; });
    gemv(A.B2, A.P1, s.h2, A.P2, nullptr, 0, bwd(s.h1, s.d1));
    gemv(A.B1e, A.NEB, s.h1, A.P1, nullptr, 0, [&](int j, float v) { s.ge1[j] = v; });
    if (c.grad_latent) {  // d df / d z = [delta1 | delta3] . [W1z ; W3z]
        float* gl = c.grad_latent + (size_t)r * A.LH;
        gemv(A.Bz, A.LH, s.h1, A.P1, s.h3, A.P3, [&](int j, float v) { gl[j] = v; });
    }
    // ---- d df / d pos through the embedding (wide_final_kernel's sums, by one wave)
    if (wave == 0) {
        float s0, s1, s2;
        dpos_sum(s.ge3, s.ge1, s.gm, A.emb_tab, A.NEK, lane, s0, s1, s2);
        if (lane == 0) c.out[r] = make_float4(s.red[0], s0, s1, s2);
    }
    __syncthreads();
}

__global__ __launch_bounds__(WT) void sdf_row_wide_kernel(WideRowArgs A) {
    extern __shared__ __align__(16) float lds_w[];
    row_eval_wide(A.w, A.c, blockIdx.x, lds_w);
}

// the resident server for these networks (sdf_server_loop, sdf_row_dev.h): request and results in dynamic
// LDS after the evaluator's, at most wide_row_max_rows(LH) rows per request
__global__ __launch_bounds__(WT) void sdf_server_wide_kernel(WideRowArgs A, SdfMbox* mb, long long idle, long long life,
                                                             unsigned long long epoch) {
    extern __shared__ __align__(16) float lds_w[];
    float* s_in = lds_w + row_lds_floats(A.w);
    float* s_out = s_in + SDF_MBOX_FLOATS;
    sdf_server_loop<WT>(mb, idle, life, epoch, s_in, s_out, A.w.LH, wide_row_max_rows(A.w.LH), [&](int rows, int grad) {
        const RowCall c = staged_call(s_in, s_out, rows, grad);
        for (int r = 0; r < rows; ++r) row_eval_wide(A.w, c, r, lds_w);
    });
}

// the dynamic-LDS limit of a kernel, raised once to the largest size asked for so far (the launches on the
// host path are serialised by the context's lock; a race between contexts only repeats the call)
static std::atomic<size_t> lds_row_set{0}, lds_srv_set{0};
static hipError_t raise_lds(const void* k, size_t bytes, std::atomic<size_t>& set) {
    if (bytes <= 64 * 1024 || bytes <= set.load(std::memory_order_relaxed)) return hipSuccess;
    const hipError_t e = hipFuncSetAttribute(k, hipFuncAttributeMaxDynamicSharedMemorySize, (int)bytes);
    if (e == hipSuccess) set.store(bytes, std::memory_order_relaxed);
    return e;
}

size_t wide_row_lds_bytes(const WideDev& a) { return row_lds_floats(a) * sizeof(float); }

hipError_t launch_sdf_row_wide(const WideRowArgs& a, hipStream_t s) {
    if (a.c.rows <= 0) return hipSuccess;
    const size_t lds = wide_row_lds_bytes(a.w);
    hipError_t e = raise_lds((const void*)sdf_row_wide_kernel, lds, lds_row_set);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(sdf_row_wide_kernel, dim3((unsigned)a.c.rows), dim3(WT), lds, s, a);
    return hipGetLastError();
}

hipError_t launch_sdf_server_wide(const WideRowArgs& a, SdfMbox* mb_dev, long long idle_ticks, long long life_ticks,
                                  unsigned long long epoch, hipStream_t s) {
    const size_t lds = wide_row_lds_bytes(a.w) + 2 * SDF_MBOX_FLOATS * sizeof(float);
    hipError_t e = raise_lds((const void*)sdf_server_wide_kernel, lds, lds_srv_set);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(sdf_server_wide_kernel, dim3(1), dim3(WT), lds, s, a, mb_dev, idle_ticks, life_ticks, epoch);
    return hipGetLastError();
}

}  // namespace sdfn
