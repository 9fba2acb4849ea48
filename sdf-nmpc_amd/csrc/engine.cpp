// C ABI implementation (include/sdfnmpc.h): contexts, device-resident packed networks, launches.
//
// Host-side runtime only: all arithmetic of the hot path happens in sdf_mlp.hip / linearize.hip.
// There is no CPU fallback: without a HIP device every compute entry point fails with
// SDFNMPC_E_NODEVICE / SDFNMPC_E_HIP.
#include <algorithm>
#include <atomic>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <thread>

#include "engine.h"
#include "lin_kernels.h"
#include "qp_kernels.h"
#include "ref_kernels.h"

using namespace sdfn;

// ------------------------------------------------------------------------------------------------
// errors
static thread_local std::string g_err;
int sdfn::fail(int code, const std::string& msg) {
    g_err = msg;
    return code;
}
int sdfn::fail(int code, const char* msg) {
    g_err = msg;
    return code;
}

extern "C" int sdfnmpc_abi_version(void) { return SDFNMPC_ABI_VERSION; }
extern "C" const char* sdfnmpc_last_error(void) { return g_err.c_str(); }

// ------------------------------------------------------------------------------------------------
// context
extern "C" int sdfnmpc_ctx_create(int device, void* stream, sdfnmpc_ctx** out) {
    if (!out) return fail(SDFNMPC_E_ARG, "out is NULL");
    *out = nullptr;
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess || n <= 0)
        return fail(SDFNMPC_E_NODEVICE, "no HIP device visible: the sdfnmpc compute path has no CPU fallback");
    if (device < 0 || device >= n) return fail(SDFNMPC_E_ARG, "device index out of range");
    ScopedDevice sd(device);
    hipDeviceProp_t prop;
    HIPCHK(hipGetDeviceProperties(&prop, device));
    if (std::string(prop.gcnArchName).rfind("gfx950", 0) != 0)
        return fail(SDFNMPC_E_UNSUPPORTED, std::string("built for gfx950 only, device is ") + prop.gcnArchName);
    HIPCHK(sdf_set_lds_limits());
    auto* c = new sdfnmpc_ctx();
    c->device = device;
    c->n_cu = prop.multiProcessorCount;
    c->lds_per_cu = prop.maxSharedMemoryPerMultiProcessor;
    if (stream) {
        c->stream = (hipStream_t)stream;
    } else {
        hipError_t e = hipStreamCreateWithFlags(&c->stream, hipStreamNonBlocking);
        if (e != hipSuccess) {
            delete c;
            return fail(SDFNMPC_E_HIP, std::string("hipStreamCreate: ") + hipGetErrorString(e));
        }
        c->own_stream = true;
    }
    int lo = 0, hi = 0;
    hipError_t e = hipDeviceGetStreamPriorityRange(&lo, &hi);  // lo = least urgent
    if (e == hipSuccess) e = hipStreamCreateWithPriority(&c->aux, hipStreamNonBlocking, lo);
    // the fork / join events order kernels of this device only and the host never waits on them (it
    // synchronises on the stream), so they carry no system-scope fence: without its cache writeback the
    // step is ≈6 µs shorter
    const unsigned evf = hipEventDisableTiming | hipEventDisableSystemFence;
    if (e == hipSuccess) e = hipEventCreateWithFlags(&c->ev_fork, evf);
    if (e == hipSuccess) e = hipEventCreateWithFlags(&c->ev_join, evf);
    if (e != hipSuccess) {
        sdfnmpc_ctx_destroy(c);
        return fail(SDFNMPC_E_HIP, std::string("aux stream/events: ") + hipGetErrorString(e));
    }
    const char* sp = getenv("SDFNMPC_SERIAL_PREP");
    c->serial_prep = sp && *sp == '1';
    if (const char* qk = getenv("SDFNMPC_QP_KERNEL")) {
        if (!strcmp(qk, "serial")) c->qp_kernel = SDFNMPC_QP_SERIAL;
        else if (!strcmp(qk, "segmented")) c->qp_kernel = SDFNMPC_QP_SEGMENTED;
    }
    *out = c;
    return SDFNMPC_OK;
}

// Ask the resident SDF server to exit and wait for it, polling with a deadline (a server that stopped
// answering must not hang destroy / reconfigure while the shim's lock is held): on timeout the mailbox
// and stream are abandoned -- never freed or reused, since the server may still write to them -- and
// the host path falls back to one launch per call.  Returns false on timeout.
static void mark_abandoned(uint64_t uid);
static bool srv_stop(sdfnmpc_ctx* ctx) {
    auto& S = ctx->srv;
    if (!S.mb || S.abandoned) return !S.abandoned;
    __atomic_store_n(&S.mb->stop, 1ull, __ATOMIC_RELEASE);
    const auto t0 = std::chrono::steady_clock::now();
    for (;;) {
        const hipError_t q = hipStreamQuery(S.stream);
        if (q != hipErrorNotReady) break;
        if (std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count() > 2.0) {
            S.abandoned = true;
            S.live = false;
            S.mode = 0;
            mark_abandoned(S.net);  // its network is leaked, not freed under a running reader
            fail(SDFNMPC_E_HIP, "sdf server: did not stop within 2 s; abandoned (one launch per call from now on)");
            return false;
        }
        std::this_thread::yield();
    }
    __atomic_store_n(&S.mb->stop, 0ull, __ATOMIC_RELEASE);
    S.live = false;
    return true;
}

extern "C" void sdfnmpc_ctx_destroy(sdfnmpc_ctx* ctx) {
    if (!ctx) return;
    ScopedDevice sd(ctx->device);
    if (ctx->srv.mb && srv_stop(ctx)) {
        (void)hipStreamDestroy(ctx->srv.stream);
        (void)hipHostFree(ctx->srv.mb);
    }
    (void)hipStreamSynchronize(ctx->stream);
    for (auto& kv : ctx->stats)
        for (auto& ev : kv.second.pending) {
            (void)hipEventDestroy(ev.first);
            (void)hipEventDestroy(ev.second);
        }
    if (ctx->aux) {
        (void)hipStreamSynchronize(ctx->aux);
        (void)hipStreamDestroy(ctx->aux);
    }
    if (ctx->h_pin) (void)hipHostFree(ctx->h_pin);
    if (ctx->ev_fork) (void)hipEventDestroy(ctx->ev_fork);
    if (ctx->ev_join) (void)hipEventDestroy(ctx->ev_join);
    if (ctx->own_stream) (void)hipStreamDestroy(ctx->stream);
    delete ctx;  // device buffers are freed by their destructors, on ctx->device
}

extern "C" int sdfnmpc_ctx_device(const sdfnmpc_ctx* ctx) { return ctx ? ctx->device : -1; }

extern "C" int sdfnmpc_dev_alloc(sdfnmpc_ctx* ctx, size_t bytes, void** out) {
    if (!ctx || !out) return fail(SDFNMPC_E_ARG, "NULL argument to sdfnmpc_dev_alloc");
    ScopedDevice sd(ctx->device);
    *out = nullptr;
    HIPCHK(hipMalloc(out, bytes ? bytes : 16));
    return SDFNMPC_OK;
}

extern "C" void sdfnmpc_dev_free(sdfnmpc_ctx* ctx, void* ptr) {
    if (!ctx || !ptr) return;
    ScopedDevice sd(ctx->device);
    (void)hipStreamSynchronize(ctx->stream);
    (void)hipFree(ptr);
}

extern "C" int sdfnmpc_memcpy(sdfnmpc_ctx* ctx, void* dst, const void* src, size_t bytes, int kind) {
    if (!ctx || (bytes && (!dst || !src)) || kind < 1 || kind > 3) return fail(SDFNMPC_E_ARG, "bad sdfnmpc_memcpy arguments");
    if (!bytes) return SDFNMPC_OK;
    ScopedDevice sd(ctx->device);
    const hipMemcpyKind k = kind == 1 ? hipMemcpyHostToDevice : kind == 2 ? hipMemcpyDeviceToHost : hipMemcpyDeviceToDevice;
    HIPCHK(hipMemcpyAsync(dst, src, bytes, k, ctx->stream));
    HIPCHK(hipStreamSynchronize(ctx->stream));
    return SDFNMPC_OK;
}

// The legacy default (null) stream: PyTorch's default stream has the handle 0, which
// sdfnmpc_ctx_create / _set_stream read as "create a private stream"; this call makes the context
// launch on the null stream itself, so its kernels are ordered with the framework's default-stream work.
extern "C" int sdfnmpc_ctx_use_null_stream(sdfnmpc_ctx* ctx) {
    if (!ctx) return fail(SDFNMPC_E_ARG, "ctx is NULL");
    ScopedDevice sd(ctx->device);
    if (ctx->own_stream) {
        HIPCHK(hipStreamSynchronize(ctx->stream));
        (void)hipStreamDestroy(ctx->stream);
        ctx->own_stream = false;
    }
    ctx->stream = nullptr;
    return SDFNMPC_OK;
}

extern "C" int sdfnmpc_ctx_set_stream(sdfnmpc_ctx* ctx, void* stream) {
    if (!ctx) return fail(SDFNMPC_E_ARG, "ctx is NULL");
    ScopedDevice sd(ctx->device);
    if (ctx->own_stream) {
        HIPCHK(hipStreamSynchronize(ctx->stream));
        (void)hipStreamDestroy(ctx->stream);
        ctx->own_stream = false;
    }
    if (stream) {
        ctx->stream = (hipStream_t)stream;
    } else {
        HIPCHK(hipStreamCreateWithFlags(&ctx->stream, hipStreamNonBlocking));
        ctx->own_stream = true;
    }
    return SDFNMPC_OK;
}

extern "C" void* sdfnmpc_ctx_stream(sdfnmpc_ctx* ctx) { return ctx ? (void*)ctx->stream : nullptr; }

extern "C" int sdfnmpc_ctx_synchronize(sdfnmpc_ctx* ctx) {
    if (!ctx) return fail(SDFNMPC_E_ARG, "ctx is NULL");
    ScopedDevice sd(ctx->device);
    HIPCHK(hipStreamSynchronize(ctx->stream));
    return SDFNMPC_OK;
}

extern "C" int sdfnmpc_ctx_set_qp_kernel(sdfnmpc_ctx* ctx, int kernel) {
    if (!ctx) return fail(SDFNMPC_E_ARG, "NULL context");
    if (kernel != SDFNMPC_QP_AUTO && kernel != SDFNMPC_QP_SERIAL && kernel != SDFNMPC_QP_SEGMENTED)
        return fail(SDFNMPC_E_ARG, "qp kernel: SDFNMPC_QP_AUTO, _SERIAL or _SEGMENTED");
    ctx->qp_kernel = kernel;
    return SDFNMPC_OK;
}

static int qp_cset_check(const sdfnmpc_qp_opts* o);
static QpRows qp_rows_of(const sdfnmpc_qp_opts* o);

// AUTO: the segmented kernel for latency-sized batches of long horizons (B <= SDFNMPC_QP_SEG_AUTO_MAX_B,
// N >= SDFNMPC_QP_SEG_AUTO_MIN_N; one workgroup of four wavefronts per instance: 8-10 % lower latency than
// the serial kernel at N = 40, 24 % at N = 60, equal at N = 30, 30 % slower at N = 20 where the three
// couplings outweigh five-node segments), the serial one otherwise (one wavefront per instance: at
// B = 1024 it fills every SIMD once and is 1.6x faster than four wavefronts per instance)
// the segmented kernel covers every row set the serial one does (qp_is_seg_set: 0..3 stage rows, soft or
// hard, and up to QP_NHN terminal rows); the choice between them is the batch / horizon policy below
static int qp_kernel_for(const sdfnmpc_ctx* ctx, int N, int B, bool seg_set) {
    if (!seg_set) return (ctx && N >= 1 && B >= 0) ? SDFNMPC_QP_SERIAL : -1;
    return sdfnmpc_ctx_qp_kernel(ctx, N, B);
}
// a row set the segmented kernel serves (rti_qp_seg.hip: the stage groups of a node on three lanes, the
// nhN terminal rows on lanes 48 + j of the last wave).  T: sdfnmpc_qp_opts or QpArgs (same field names)
template <class T>
static bool qp_is_seg_set(const T& o) {
    return o.nh >= 0 && o.nh <= 3 && o.nhs >= 0 && o.nhs <= o.nh && o.nsN >= 0 && o.nsN <= 3 && o.nhN >= o.nsN &&
           o.nhN <= QP_NHN;
}

extern "C" int sdfnmpc_ctx_qp_kernel(const sdfnmpc_ctx* ctx, int N, int B) {
    if (!ctx || N < 1 || B < 0) return -1;
    if (ctx->qp_kernel == SDFNMPC_QP_SERIAL || !rti_qp_seg_supported(N)) return SDFNMPC_QP_SERIAL;
    if (ctx->qp_kernel == SDFNMPC_QP_SEGMENTED) return SDFNMPC_QP_SEGMENTED;
    // the batch bound doubles from N = 48: the serial kernel then holds two instances per CU instead of
    // four (its LDS), and the segmented one still runs two per CU (measured at N = 60: 2.10 vs 2.67 ms at
    // B = 512; at N = 40, 1.13 vs 1.08 ms at B = 512)
    const int max_b = N >= 48 ? 2 * SDFNMPC_QP_SEG_AUTO_MAX_B : SDFNMPC_QP_SEG_AUTO_MAX_B;
    return (B <= max_b && N >= SDFNMPC_QP_SEG_AUTO_MIN_N) ? SDFNMPC_QP_SEGMENTED : SDFNMPC_QP_SERIAL;
}

extern "C" int sdfnmpc_ctx_qp_kernel_for(const sdfnmpc_ctx* ctx, int N, int B, const sdfnmpc_qp_opts* o) {
    if (o && qp_cset_check(o)) return -1;
    return qp_kernel_for(ctx, N, B, o ? qp_is_seg_set(*o) : true);
}

extern "C" int sdfnmpc_qp_seg_count(int N) { return N < 1 ? 0 : rti_qp_seg_count(N); }

extern "C" long long sdfnmpc_qp_lds_bytes(int N) {
    return N < 1 ? -1 : (long long)qp_lds_bytes(N);
}

// Instances the context's device solves in one wave of QP workgroups: every CU holds as many
// instances as its LDS fits (the QP keeps each instance's iterate, duals and record window in LDS;
// rti_qp.hip: one 64-lane workgroup per instance, rti_qp_seg.hip: one workgroup of NSEG waves).

extern "C" long long sdfnmpc_qp_capacity(const sdfnmpc_ctx* ctx, int N) { return sdfnmpc_qp_capacity_for(ctx, N, nullptr); }

extern "C" long long sdfnmpc_qp_capacity_for(const sdfnmpc_ctx* ctx, int N, const sdfnmpc_qp_opts* o) {
    if (!ctx || N < 1) return -1;
    if (ctx->n_cu <= 0 || ctx->lds_per_cu == 0) return -1;
    if (o && qp_cset_check(o)) return -1;
    const QpRows rows = o ? qp_rows_of(o) : qp_rows_default();
    // a batch that fills the device: the kernel AUTO picks above SDFNMPC_QP_SEG_AUTO_MAX_B
    const bool seg = qp_kernel_for(ctx, N, 1 << 30, o ? qp_is_seg_set(*o) : true) == SDFNMPC_QP_SEGMENTED;
    const size_t per = seg ? qp_seg_lds_bytes(N) : qp_lds_bytes(N, rows);
    if (per == 0 || per > ctx->lds_per_cu) return 0;  // the horizon does not fit one CU's LDS
    // the runtime's occupancy of the kernel (LDS, registers and waves at once): the serial kernel's 375
    // registers allow one wave per SIMD, four instances per CU, whatever the LDS would admit; the segmented
    // kernel's __launch_bounds__ two or three workgroups per CU
    ScopedDevice sd(ctx->device);
    const int occ = seg ? rti_qp_seg_blocks_per_cu(N) : rti_qp_blocks_per_cu(N, rows);
    const long long by_lds = (long long)(ctx->lds_per_cu / per);
    return (long long)ctx->n_cu * std::min<long long>(by_lds, occ > 0 ? occ : 0);
}

extern "C" int sdfnmpc_ctx_set_tile_rows(sdfnmpc_ctx* ctx, int rows) {
    if (!ctx) return fail(SDFNMPC_E_ARG, "ctx is NULL");
    if (rows != 32 && rows != 64) return fail(SDFNMPC_E_ARG, "tile rows must be 32 or 64");
    ctx->tile_rows = rows;
    return SDFNMPC_OK;
}

extern "C" int sdfnmpc_ctx_enable_timing(sdfnmpc_ctx* ctx, int on) {
    if (!ctx) return fail(SDFNMPC_E_ARG, "ctx is NULL");
    ctx->timing = on != 0;
    return SDFNMPC_OK;
}

static int resolve_stats(sdfnmpc_ctx* ctx) {
    ScopedDevice sd(ctx->device);
    HIPCHK(hipStreamSynchronize(ctx->stream));
    HIPCHK(hipStreamSynchronize(ctx->aux));
    for (auto& kv : ctx->stats) {
        for (auto& ev : kv.second.pending) {
            float ms = 0.0f;
            HIPCHK(hipEventElapsedTime(&ms, ev.first, ev.second));
            kv.second.ms += ms;
            kv.second.n += 1;
            (void)hipEventDestroy(ev.first);
            (void)hipEventDestroy(ev.second);
        }
        kv.second.pending.clear();
    }
    return SDFNMPC_OK;
}

extern "C" int sdfnmpc_ctx_kernel_stats(sdfnmpc_ctx* ctx, const char* kernel, double* total_ms, long long* launches) {
    if (!ctx || !kernel) return fail(SDFNMPC_E_ARG, "ctx/kernel is NULL");
    int rc = resolve_stats(ctx);
    if (rc) return rc;
    auto it = ctx->stats.find(kernel);
    if (total_ms) *total_ms = it == ctx->stats.end() ? 0.0 : it->second.ms;
    if (launches) *launches = it == ctx->stats.end() ? 0 : it->second.n;
    return SDFNMPC_OK;
}

extern "C" int sdfnmpc_ctx_reset_stats(sdfnmpc_ctx* ctx) {
    if (!ctx) return fail(SDFNMPC_E_ARG, "ctx is NULL");
    int rc = resolve_stats(ctx);
    if (rc) return rc;
    ctx->stats.clear();
    return SDFNMPC_OK;
}

// ------------------------------------------------------------------------------------------------
// network: .sdfw parsing (sdf-nmpc_amd/weights.py:pack) and packing into the kernels' layouts
namespace {

struct HostNet {
    int nb_states = 3, L = 0, n1 = 0, n2 = 0, n3 = 0, n4 = 0, nf = 0, nd = 0;
    int res = 0;  // 0 'full' [h2 | e | z], 1 'state' [h2 | e], 2 'latent' [h2 | z], 3 plain MLP [h2] into layer 3
                  // (neural_df.py:76-78: any other `res` value)
    int act = 0;  // 0 sin(w0 .), 1 relu, 2 softplus (neural_df.py:40-47)
    float w0 = 0, max_df = 1;
    std::vector<float> dirs, freqs;                           // [3][nd], [nf]
    std::vector<float> W1, b1, W2, b2, W3, b3, W4, b4, W5, b5;  // torch order / shapes
    int E() const { return 3 + 2 * nd * nf; }
    bool e3() const { return res == 0 || res == 1; }  // layer 3 sees the embedding
    bool z3() const { return res == 0 || res == 2; }  // layer 3 sees the latent
    int c3() const { return n2 + (e3() ? E() : 0) + (z3() ? L : 0); }  // W3 row length
};

uint64_t mix64(uint64_t z) {
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ULL;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBULL;
    return z ^ (z >> 31);
}
// identical to weights.prng_uniform / oracle orc_prng_uniform
void prng_fill(uint64_t seed, uint64_t stream, std::vector<double>& out) {
    const uint64_t key = mix64(seed * 0x9E3779B97F4A7C15ULL + stream * 0xD1B54A32D192ED03ULL + 1ULL);
    for (size_t i = 0; i < out.size(); ++i)
        out[i] = (double)(mix64(key + (uint64_t)(i + 1) * 0x9E3779B97F4A7C15ULL) >> 40) * (1.0 / 16777216.0);
}

std::vector<float*> param_list(HostNet& h) {
    return {h.W1.data(), h.b1.data(), h.W2.data(), h.b2.data(), h.W3.data(),
            h.b3.data(), h.W4.data(), h.b4.data(), h.W5.data(), h.b5.data()};
}
std::vector<std::pair<int, int>> param_shapes(const HostNet& h) {
    const int E = h.E(), L = h.L;
    return {{h.n1, E + L}, {h.n1, 1}, {h.n2, h.n1}, {h.n2, 1}, {h.n3, h.c3()},
            {h.n3, 1},     {h.n4, h.n3}, {h.n4, 1}, {1, h.n4}, {1, 1}};
}
void alloc_params(HostNet& h) {
    auto sh = param_shapes(h);
    std::vector<std::vector<float>*> v = {&h.W1, &h.b1, &h.W2, &h.b2, &h.W3, &h.b3, &h.W4, &h.b4, &h.W5, &h.b5};
    for (size_t i = 0; i < v.size(); ++i) v[i]->assign((size_t)sh[i].first * sh[i].second, 0.0f);
}

// The deployed NeuralDF (layers [256,256,128,64], 'oct' x 5 frequencies, res 'full', sin) runs the fused
// sdf_mlp.hip / sdf_row.hip kernels.  Every other architecture -- config C5's [1024,1024,512,256], and the
// reference's variants: any layer sizes (zero-padded to multiples of 128: the padded units' outgoing
// weights are zero, so they change nothing), embeddings none / pos / cube / oct / dod / ico with any
// frequency count, res full / state / latent / none (a plain MLP), any size_latent, activations sin / relu /
// softplus -- runs the layer-by-layer
// GEMM schedule of sdf_wide.hip ("wide" below means exactly that: not the deployed net).
bool is_deployed(const HostNet& h) {
    return h.n1 == N1 && h.n2 == N2 && h.n3 == N3 && h.n4 == N4 && h.nd == EMB_ND && h.nf == EMB_NF && h.res == 0 &&
           h.act == 0 && h.L == L;
}
bool is_wide(const HostNet& h) { return !is_deployed(h); }
int pad128(int n) { return (n + 127) / 128 * 128; }

constexpr int L_MAX = 1024;  // size_latent bound (the wide schedule pads it to a multiple of 128)
int check_supported(const HostNet& h) {
    if (h.nb_states != 3 || h.L < 1 || h.L > L_MAX || h.E() > 256 || h.res < 0 || h.res > 3 || h.act < 0 || h.act > 2) {
        char buf[256];
        snprintf(buf, sizeof buf,
                 "network architecture (states %d, latent %d, embedding features %d, res %d, act %d) is not built "
                 "for; this build supports 3 states, latent 1..%d, at most 256 embedding features",
                 h.nb_states, h.L, h.E(), h.res, h.act, L_MAX);
        return fail(SDFNMPC_E_UNSUPPORTED, buf);
    }
    return SDFNMPC_OK;
}

int parse_sdfw(const void* blob, size_t bytes, HostNet& h) {
    // version 1: magic, version, nb_states, L, n1..n4, nb_freqs, n_dirs, res (0), w0, max_df;
    // version 2 adds the activation after res (sdf_nmpc_amd/weights.py)
    const unsigned char* p = (const unsigned char*)blob;
    if (!blob || bytes < 12 || memcmp(p, "SDFNMPCW", 8) != 0) return fail(SDFNMPC_E_FORMAT, "not an .sdfw blob");
    uint32_t ver = 0;
    memcpy(&ver, p + 8, 4);
    if (ver != 1 && ver != 2) return fail(SDFNMPC_E_FORMAT, "unsupported .sdfw version");
    const int nu = ver == 1 ? 10 : 11;
    const size_t HDR = 8 + nu * 4 + 2 * 4;
    if (bytes < HDR) return fail(SDFNMPC_E_FORMAT, "truncated .sdfw header");
    uint32_t u[11] = {};
    memcpy(u, p + 8, (size_t)nu * 4);
    float f[2];
    memcpy(f, p + 8 + nu * 4, sizeof f);
    if (ver == 1 && u[9] != 0) return fail(SDFNMPC_E_FORMAT, "version-1 .sdfw blobs are res='full'");
    h.res = (int)u[9];
    h.act = ver == 2 ? (int)u[10] : 0;
    h.nb_states = (int)u[1];
    h.L = (int)u[2];
    h.n1 = (int)u[3]; h.n2 = (int)u[4]; h.n3 = (int)u[5]; h.n4 = (int)u[6];
    h.nf = (int)u[7];
    h.nd = (int)u[8];
    h.w0 = f[0];
    h.max_df = f[1];
    if (h.nd < 0 || h.nf < 0 || h.nd > 64 || h.nf > 64 || (h.nd == 0) != (h.nf == 0) || h.L < 0 || h.n1 <= 0 ||
        h.n2 <= 0 || h.n3 <= 0 || h.n4 <= 0 || h.n1 > 65536 || h.n2 > 65536 || h.n3 > 65536 || h.n4 > 65536)
        return fail(SDFNMPC_E_FORMAT, "bad .sdfw header");
    size_t off = HDR;
    auto take = [&](std::vector<float>& v, size_t n) -> bool {
        if (off + 4 * n > bytes) return false;
        v.resize(n);
        memcpy(v.data(), p + off, 4 * n);
        off += 4 * n;
        return true;
    };
    if (!take(h.dirs, (size_t)3 * h.nd) || !take(h.freqs, (size_t)h.nf)) return fail(SDFNMPC_E_FORMAT, "truncated");
    auto sh = param_shapes(h);
    std::vector<std::vector<float>*> v = {&h.W1, &h.b1, &h.W2, &h.b2, &h.W3, &h.b3, &h.W4, &h.b4, &h.W5, &h.b5};
    for (size_t i = 0; i < v.size(); ++i)
        if (!take(*v[i], (size_t)sh[i].first * sh[i].second)) return fail(SDFNMPC_E_FORMAT, "truncated .sdfw params");
    if (off != bytes) return fail(SDFNMPC_E_FORMAT, "trailing bytes in .sdfw blob");
    return check_supported(h);
}

void siren_host(HostNet& h, uint64_t seed, float wg, float bg) {
    h.nb_states = 3; h.L = L; h.n1 = N1; h.n2 = N2; h.n3 = N3; h.n4 = N4; h.nf = EMB_NF; h.nd = EMB_ND;
    h.w0 = 20.0f;
    h.max_df = 1.0f;
    // 'oct' dirs exactly as torch builds them (embeddings.py:37-51): +-1 / fp32 sqrt(3)
    static const int sg[8][3] = {{-1, -1, -1}, {-1, -1, 1}, {-1, 1, -1}, {-1, 1, 1},
                                 {1, -1, -1},  {1, -1, 1},  {1, 1, -1},  {1, 1, 1}};
    const float nrm = sqrtf(3.0f);
    h.dirs.assign(3 * 8, 0.0f);
    for (int d = 0; d < 8; ++d)
        for (int c = 0; c < 3; ++c) h.dirs[c * 8 + d] = (float)sg[d][c] / nrm;
    h.freqs = {1.0f, 2.0f, 4.0f, 8.0f, 16.0f};
    alloc_params(h);
    auto ptr = param_list(h);
    auto sh = param_shapes(h);
    std::vector<double> u;
    for (int t = 0; t < 10; t += 2) {
        const double bound = std::sqrt(6.0 / sh[t].second) / (double)h.w0;
        u.assign((size_t)sh[t].first * sh[t].second, 0.0);
        prng_fill(seed, t, u);
        for (size_t i = 0; i < u.size(); ++i) ptr[t][i] = (float)((2.0 * u[i] - 1.0) * (bound * (double)wg));
        if (bg > 0.0f) {
            u.assign((size_t)sh[t + 1].first * sh[t + 1].second, 0.0);
            prng_fill(seed, t + 1, u);
            for (size_t i = 0; i < u.size(); ++i) ptr[t + 1][i] = (float)((2.0 * u[i] - 1.0) * (bound * (double)bg));
        }
    }
}

template <typename F>
void pack_operand(std::vector<float>& dst, int N, int K, F&& W) {
    const int CB = (N + 31) / 32, G = K / 8;
    const size_t base = dst.size();
    dst.resize(base + packed_floats(N, K), 0.0f);
    for (int cb = 0; cb < CB; ++cb)
        for (int g = 0; g < G; ++g)
            for (int ln = 0; ln < 64; ++ln)
                for (int i = 0; i < 4; ++i) {
                    const int j = cb * 32 + (ln & 31), k = (ln >> 5) * (K / 2) + 4 * g + i;
                    dst[base + (((size_t)cb * G + g) * 64 + ln) * 4 + i] = (j < N) ? W(j, k) : 0.0f;
                }
}

}  // namespace

struct sdfnmpc_net {
    int device = 0;
    HostNet host;
    void* dmem = nullptr;
    SdfArgs args{};  // weight pointers filled; per-call fields left zero
    SdfRowArgs row{};  // the single-row path's weight pointers (deployed architecture only)
    const float4* WzT = nullptr;
    const float* bias13 = nullptr;
    uint64_t fingerprint = 0;
    bool wide = false;
    WideRowArgs wrow{};    // a wide network's operands (sdf_wide.hip, sdf_row_wide.hip); per-call fields left zero
    bool wrow_ok = false;  // the row evaluator and its server fit this network (LDS, weight bytes)
    // process-unique id: caches keyed on a network (the host path's hoist) never confuse a freed
    // network with a new one allocated at the same address
    uint64_t uid = next_uid();
    static uint64_t next_uid() {
        static std::atomic<uint64_t> n{1};
        return n++;
    }
};

// [width] float4 (dir * 2^f, 0) of embedding feature m: the projected frequencies in the reference's order
// (embeddings.py:108-109: direction-major, frequency-minor; the sin half, then the same for the shifted half)
static void emb_table(const HostNet& h, std::vector<float>& blob, int width = NE) {
    const int nb = h.nd * h.nf, E = h.E();
    for (int m = 0; m < width; ++m) {
        float v[4] = {0, 0, 0, 0};
        int j = -1;
        if (m >= 3 && m < 3 + nb) j = m - 3;
        else if (m >= 3 + nb && m < E) j = m - 3 - nb;
        if (j >= 0) {
            const int d = j / h.nf, f = j % h.nf;
            for (int c = 0; c < 3; ++c) v[c] = h.dirs[c * h.nd + d] * h.freqs[f];  // freq = 2^f: exact
        }
        blob.insert(blob.end(), v, v + 4);
    }
}

static uint64_t net_fingerprint(HostNet& h) {  // FNV-1a over the parameters in torch order
    uint64_t fp = 1469598103934665603ULL;
    auto sh = param_shapes(h);
    auto pl = param_list(h);
    for (size_t t = 0; t < pl.size(); ++t) {
        const unsigned char* b = (const unsigned char*)pl[t];
        const size_t nb = (size_t)sh[t].first * sh[t].second * 4;
        for (size_t q = 0; q < nb; ++q) fp = (fp ^ b[q]) * 1099511628211ULL;
    }
    return fp;
}

// weight bytes up to which a variant network takes the row evaluator on the host path
// (SDFNMPC_WIDE_ROW_MAX_MB overrides; 0 sends every variant to the layer-by-layer schedule)
static size_t wide_row_weight_cap() {
    if (const char* e = getenv("SDFNMPC_WIDE_ROW_MAX_MB")) return (size_t)(atof(e) * 1048576.0);
    return (size_t)64 << 20;
}

static int upload_wide(sdfnmpc_ctx* ctx, HostNet&& h, sdfnmpc_net** out) {
    // layer widths zero-padded to multiples of 128 (the GEMM's column tile), the embedding to NEK (a
    // multiple of 32) as a K segment and to NEB (a multiple of 128) as the d e GEMMs' output width
    const int n1 = h.n1, n2 = h.n2, n3 = h.n3, n4 = h.n4, E = h.E(), Lh = h.L, LZ = pad128(Lh), c1 = E + Lh, c3 = h.c3();
    const int P1 = pad128(n1), P2 = pad128(n2), P3 = pad128(n3), P4 = pad128(n4);
    const int NEK = std::max(96, (E + 31) / 32 * 32), NEB = pad128(E);
    const bool e3 = h.e3(), z3 = h.z3();
    const int z3off = n2 + (e3 ? E : 0);  // first latent column of W3
    const float *W1 = h.W1.data(), *W2 = h.W2.data(), *W3 = h.W3.data(), *W4 = h.W4.data();
    std::vector<float> blob;
    std::vector<size_t> off;
    auto mat = [&](int N, int K, auto&& f) {
        off.push_back(blob.size());
        for (int j = 0; j < N; ++j)
            for (int k = 0; k < K; ++k) blob.push_back(f(j, k));
    };
    auto vec = [&](const std::vector<float>& v, int P) {
        off.push_back(blob.size());
        blob.insert(blob.end(), v.begin(), v.end());
        blob.insert(blob.end(), (size_t)(P - (int)v.size()), 0.0f);
    };
    mat(P1, NEK, [&](int j, int k) { return j < n1 && k < E ? W1[(size_t)j * c1 + k] : 0.0f; });                // F1
    mat(P2, P1, [&](int j, int k) { return j < n2 && k < n1 ? W2[(size_t)j * n1 + k] : 0.0f; });                 // F2
    mat(P3, P2 + (e3 ? NEK : 0), [&](int j, int k) {                                                             // F3
        if (j >= n3) return 0.0f;
        if (k < P2) return k < n2 ? W3[(size_t)j * c3 + k] : 0.0f;
        return k - P2 < E ? W3[(size_t)j * c3 + n2 + (k - P2)] : 0.0f;
    });
    mat(P4, P3, [&](int j, int k) { return j < n4 && k < n3 ? W4[(size_t)j * n3 + k] : 0.0f; });                 // F4
    mat(P3, P4, [&](int j, int k) { return j < n3 && k < n4 ? W4[(size_t)k * n3 + j] : 0.0f; });                 // B4
    mat(P2, P3, [&](int j, int k) { return j < n2 && k < n3 ? W3[(size_t)k * c3 + j] : 0.0f; });                 // B3h
    mat(NEB, P3, [&](int j, int k) { return e3 && j < E && k < n3 ? W3[(size_t)k * c3 + n2 + j] : 0.0f; });      // B3e
    mat(P1, P2, [&](int j, int k) { return j < n1 && k < n2 ? W2[(size_t)k * n1 + j] : 0.0f; });                 // B2
    mat(NEB, P1, [&](int j, int k) { return j < E && k < n1 ? W1[(size_t)k * c1 + j] : 0.0f; });                 // B1e
    mat(LZ, P1 + P3, [&](int j, int k) {  // Bz: d z = [delta1 | delta3] . [W1z ; W3z] (the 131-wide jac_sdf_l4c)
        if (j >= Lh) return 0.0f;
        if (k < P1) return k < n1 ? W1[(size_t)k * c1 + E + j] : 0.0f;
        return z3 && k - P1 < n3 ? W3[(size_t)(k - P1) * c3 + z3off + j] : 0.0f;
    });
    mat(P1 + P3, LZ, [&](int j, int k) {                                                                         // Hz
        if (k >= Lh) return 0.0f;
        if (j < P1) return j < n1 ? W1[(size_t)j * c1 + E + k] : 0.0f;
        return z3 && j - P1 < n3 ? W3[(size_t)(j - P1) * c3 + z3off + k] : 0.0f;
    });
    off.push_back(blob.size());  // bz = [b1 | b3], padded
    blob.insert(blob.end(), h.b1.begin(), h.b1.end());
    blob.insert(blob.end(), (size_t)(P1 - n1), 0.0f);
    blob.insert(blob.end(), h.b3.begin(), h.b3.end());
    blob.insert(blob.end(), (size_t)(P3 - n3), 0.0f);
    vec(h.b2, P2);
    vec(h.b4, P4);
    vec(h.W5, P4);
    while (blob.size() % 4) blob.push_back(0.0f);
    off.push_back(blob.size());
    emb_table(h, blob, NEK);
    for (size_t o : off)
        if (o % 4) return fail(SDFNMPC_E_FORMAT, "internal: misaligned wide operand");
    auto* net = new sdfnmpc_net();
    net->device = ctx->device;
    net->wide = true;
    ScopedDevice sd(ctx->device);
    if (hipMalloc(&net->dmem, blob.size() * sizeof(float)) != hipSuccess ||
        hipMemcpy(net->dmem, blob.data(), blob.size() * sizeof(float), hipMemcpyHostToDevice) != hipSuccess) {
        if (net->dmem) (void)hipFree(net->dmem);
        delete net;
        return fail(SDFNMPC_E_HIP, "wide net: device upload failed");
    }
    const float* d = (const float*)net->dmem;
    WideDev& w = net->wrow.w;
    int i = 0;
    w.F1 = d + off[i++]; w.F2 = d + off[i++]; w.F3 = d + off[i++]; w.F4 = d + off[i++];
    w.B4 = d + off[i++]; w.B3h = d + off[i++]; w.B3e = d + off[i++]; w.B2 = d + off[i++]; w.B1e = d + off[i++];
    w.Bz = d + off[i++];
    w.Hz = d + off[i++]; w.bz = d + off[i++]; w.b2 = d + off[i++]; w.b4 = d + off[i++]; w.w5 = d + off[i++];
    w.emb_tab = (const float4*)(d + off[i++]);
    w.P1 = P1; w.P2 = P2; w.P3 = P3; w.P4 = P4; w.NEK = NEK; w.NEB = NEB;
    w.nb = h.nd * h.nf; w.e3 = e3 ? 1 : 0; w.act = h.act; w.LH = Lh; w.LZ = LZ;
    w.b5 = h.b5[0];
    w.w0 = h.w0;
    // one workgroup per row streams every weight once per row: worth it while the weights are L2 / MALL
    // sized (a C5-sized network is faster on the layer-by-layer GEMMs)
    const size_t srv_lds = wide_row_lds_bytes(w) + 2 * SDF_MBOX_FLOATS * sizeof(float);
    net->wrow_ok = srv_lds <= 160 * 1024 && blob.size() * sizeof(float) <= wide_row_weight_cap();
    net->fingerprint = net_fingerprint(h);
    net->host = std::move(h);
    *out = net;
    return SDFNMPC_OK;
}

static int upload_net(sdfnmpc_ctx* ctx, HostNet&& h, sdfnmpc_net** out) {
    if (is_wide(h)) return upload_wide(ctx, std::move(h), out);
    const int Ein = h.E(), Lh = h.L;
    const float* W1 = h.W1.data();
    const float* W2 = h.W2.data();
    const float* W3 = h.W3.data();
    const float* W4 = h.W4.data();
    const int c1 = Ein + Lh, c3 = N2 + Ein + Lh;  // row lengths of W1, W3
    std::vector<float> blob;
    std::vector<size_t> off;
    auto mark = [&]() { off.push_back(blob.size()); };
    mark(); pack_operand(blob, N1, KE, [&](int j, int k) { return k < E ? W1[(size_t)j * c1 + k] : 0.0f; });
    mark(); pack_operand(blob, N2, N1, [&](int j, int k) { return W2[(size_t)j * N1 + k]; });
    mark(); pack_operand(blob, N3, N2, [&](int j, int k) { return W3[(size_t)j * c3 + k]; });
    mark(); pack_operand(blob, N3, KE, [&](int j, int k) { return k < E ? W3[(size_t)j * c3 + N2 + k] : 0.0f; });
    mark(); pack_operand(blob, N4, N3, [&](int j, int k) { return W4[(size_t)j * N3 + k]; });
    mark(); pack_operand(blob, N3, N4, [&](int j, int k) { return W4[(size_t)k * N3 + j]; });
    mark(); pack_operand(blob, N2, N3, [&](int j, int k) { return W3[(size_t)k * c3 + j]; });
    mark(); pack_operand(blob, NE, N3, [&](int j, int k) { return j < E ? W3[(size_t)k * c3 + N2 + j] : 0.0f; });
    mark(); pack_operand(blob, N1, N2, [&](int j, int k) { return W2[(size_t)k * N1 + j]; });
    mark(); pack_operand(blob, NE, N1, [&](int j, int k) { return j < E ? W1[(size_t)k * c1 + j] : 0.0f; });
    mark(); pack_operand(blob, L, N3, [&](int j, int k) { return W3[(size_t)k * c3 + N2 + E + j]; });
    mark(); pack_operand(blob, L, N1, [&](int j, int k) { return W1[(size_t)k * c1 + E + j]; });
    // hoist operand Wsrc(j, k) = [W1[:, E:] ; W3[:, N2+E:]](j, k): N = C13_STRIDE, K = L
    mark();
    pack_operand(blob, C13_STRIDE, L, [&](int j, int k) {
        return j < N1 ? W1[(size_t)j * c1 + E + k] : W3[(size_t)(j - N1) * c3 + N2 + E + k];
    });
    mark(); for (int j = 0; j < N1; ++j) blob.push_back(h.b1[j]); for (int j = 0; j < N3; ++j) blob.push_back(h.b3[j]);
    mark(); blob.insert(blob.end(), h.b2.begin(), h.b2.end());
    mark(); blob.insert(blob.end(), h.b4.begin(), h.b4.end());
    mark(); blob.insert(blob.end(), h.W5.begin(), h.W5.end());
    while (blob.size() % 4) blob.push_back(0.0f);
    mark();
    emb_table(h, blob);
    // torch-layout weights transposed ([K][J], J a multiple of 4) for the single-row latency path (sdf_row.hip)
    auto transposed = [&](const std::vector<float>& v, int J, int K) {
        mark();
        blob.resize(blob.size() + (size_t)J * K);
        float* t = blob.data() + off.back();
        for (int j = 0; j < J; ++j)
            for (int k = 0; k < K; ++k) t[(size_t)k * J + j] = v[(size_t)j * K + k];
    };
    transposed(h.W1, N1, c1); transposed(h.W2, N2, N1); transposed(h.W3, N3, c3); transposed(h.W4, N4, N3);
    for (size_t o : off)
        if (o % 4) return fail(SDFNMPC_E_FORMAT, "internal: misaligned packed operand");

    auto* net = new sdfnmpc_net();
    net->device = ctx->device;
    ScopedDevice sd(ctx->device);
    hipError_t e = hipMalloc(&net->dmem, blob.size() * sizeof(float));
    if (e != hipSuccess) {
        delete net;
        return fail(SDFNMPC_E_HIP, std::string("hipMalloc(net): ") + hipGetErrorString(e));
    }
    e = hipMemcpy(net->dmem, blob.data(), blob.size() * sizeof(float), hipMemcpyHostToDevice);
    if (e != hipSuccess) {
        (void)hipFree(net->dmem);
        delete net;
        return fail(SDFNMPC_E_HIP, std::string("hipMemcpy(net): ") + hipGetErrorString(e));
    }
    const float* d = (const float*)net->dmem;
    SdfArgs& a = net->args;
    int i = 0;
    a.wF1 = (const float4*)(d + off[i++]);
    a.wF2 = (const float4*)(d + off[i++]);
    a.wF3h = (const float4*)(d + off[i++]);
    a.wF3e = (const float4*)(d + off[i++]);
    a.wF4 = (const float4*)(d + off[i++]);
    a.wB4 = (const float4*)(d + off[i++]);
    a.wB3 = (const float4*)(d + off[i++]);
    a.wB3e = (const float4*)(d + off[i++]);
    a.wB2 = (const float4*)(d + off[i++]);
    a.wB1e = (const float4*)(d + off[i++]);
    a.wB3z = (const float4*)(d + off[i++]);
    a.wB1z = (const float4*)(d + off[i++]);
    net->WzT = (const float4*)(d + off[i++]);
    net->bias13 = d + off[i++];
    a.b2 = d + off[i++];
    a.b4 = d + off[i++];
    a.w5 = d + off[i++];
    a.emb_tab = (const float4*)(d + off[i++]);
    a.b5 = h.b5[0];
    a.w0 = h.w0;
    SdfRowArgs& ra = net->row;
    ra.W1T = d + off[i++];
    ra.W2T = d + off[i++];
    ra.W3T = d + off[i++];
    ra.W4T = d + off[i++];
    ra.b1 = net->bias13;
    ra.b3 = net->bias13 + N1;
    ra.b2 = a.b2;
    ra.b4 = a.b4;
    ra.w5 = a.w5;
    ra.b5 = a.b5;
    ra.w0 = a.w0;
    ra.emb_tab = a.emb_tab;
    const uint64_t fp = net_fingerprint(h);
    net->fingerprint = fp;
    net->host = std::move(h);
    *out = net;
    return SDFNMPC_OK;
}

extern "C" int sdfnmpc_net_load(sdfnmpc_ctx* ctx, const void* blob, size_t bytes, sdfnmpc_net** out) {
    if (!ctx || !out) return fail(SDFNMPC_E_ARG, "ctx/out is NULL");
    HostNet h;
    int rc = parse_sdfw(blob, bytes, h);
    if (rc) return rc;
    return upload_net(ctx, std::move(h), out);
}

extern "C" int sdfnmpc_net_load_file(sdfnmpc_ctx* ctx, const char* path, sdfnmpc_net** out) {
    if (!ctx || !path || !out) return fail(SDFNMPC_E_ARG, "NULL argument");
    FILE* f = fopen(path, "rb");
    if (!f) return fail(SDFNMPC_E_ARG, std::string("cannot open ") + path);
    std::vector<unsigned char> buf;
    unsigned char tmp[1 << 16];
    size_t n;
    while ((n = fread(tmp, 1, sizeof tmp, f)) > 0) buf.insert(buf.end(), tmp, tmp + n);
    fclose(f);
    return sdfnmpc_net_load(ctx, buf.data(), buf.size(), out);
}

extern "C" int sdfnmpc_net_siren(sdfnmpc_ctx* ctx, uint64_t seed, float wg, float bg, sdfnmpc_net** out) {
    if (!ctx || !out) return fail(SDFNMPC_E_ARG, "ctx/out is NULL");
    HostNet h;
    siren_host(h, seed, wg, bg);
    return upload_net(ctx, std::move(h), out);
}

// networks an abandoned SDF server (srv_stop timeout) may still be reading: never freed
static std::mutex g_abandoned_mu;
static std::vector<uint64_t> g_abandoned_nets;
static void mark_abandoned(uint64_t uid) {
    std::lock_guard<std::mutex> lk(g_abandoned_mu);
    g_abandoned_nets.push_back(uid);
}

extern "C" void sdfnmpc_net_free(sdfnmpc_net* net) {
    if (!net) return;
    {
        std::lock_guard<std::mutex> lk(g_abandoned_mu);
        // hipFree would also synchronise the device, i.e. wait for the very server that refused to stop
        if (std::find(g_abandoned_nets.begin(), g_abandoned_nets.end(), net->uid) != g_abandoned_nets.end()) return;
    }
    ScopedDevice sd(net->device);
    if (net->dmem) (void)hipFree(net->dmem);
    delete net;
}

extern "C" float sdfnmpc_net_max_df(const sdfnmpc_net* net) { return net ? net->host.max_df : NAN; }
extern "C" int sdfnmpc_net_size_latent(const sdfnmpc_net* net) { return net ? net->host.L : -1; }
extern "C" uint64_t sdfnmpc_net_fingerprint(const sdfnmpc_net* net) { return net ? net->fingerprint : 0; }

// ------------------------------------------------------------------------------------------------
// SDF evaluation
static int run_sdf(sdfnmpc_ctx* ctx, const sdfnmpc_net* net, long long rows, const float4* pos4, const float* c13,
                   int rows_per_inst, float4* out4, float* glat, int M, const SdfArgs* cons = nullptr) {
    if (rows > 0x7fffffffLL / 2) return fail(SDFNMPC_E_ARG, "too many rows");
    SdfArgs a = net->args;
    if (cons) {
        a.x = cons->x;
        a.p = cons->p;
        a.np = cons->np;
        a.h = cons->h;
        a.Jh = cons->Jh;
        a.max_df = cons->max_df;
    }
    a.c13 = c13;
    a.pos = pos4;
    a.out = out4;
    a.grad_latent = glat;
    a.rows = (int)rows;
    a.rows_per_inst = rows_per_inst;
    HIPCHK(timed(ctx, "sdf_mlp", [&] { return launch_sdf_mlp(a, M, glat != nullptr, ctx->stream); }));
    return SDFNMPC_OK;
}

// wide schedule (sdf_wide.hip): hoist, embedding, 4 forward + 5 backward GEMMs, final contraction.
// Latent: fp32 [n_inst][L] (zf) or fp64 at a stride (zd, the stage parameters).  Geometry: pos4, or
// x / p (then also the constraint epilogue when cons->h is set).
static int run_wide(sdfnmpc_ctx* ctx, const sdfnmpc_net* net, long long rows, const float4* pos4, const float* zf,
                    const double* zd, long long zstride, int n_inst, int rows_per_inst, float4* out4,
                    const SdfArgs* cons, float* glat = nullptr) {
    if (rows > 0x7fffffffLL / 2) return fail(SDFNMPC_E_ARG, "too many rows");
    const WideDev& w = net->wrow.w;
    const int n1 = w.P1, n2 = w.P2, n3 = w.P3, n4 = w.P4, nz = n1 + n3, R = (int)rows;
    const int NEK = w.NEK, NEB = w.NEB, LH = w.LH, LZ = w.LZ;
    const bool zpad = LH != LZ;  // size_latent not a multiple of 128: padded latent and d z staging
    const size_t per_row = 2 * (size_t)NEK + 2 * (size_t)(n1 + n2 + n3 + n4) + 2 * (size_t)NEB +
                           (zpad && glat ? (size_t)LZ : 0);
    const size_t nfl = per_row * rows + (size_t)n_inst * (LZ + nz);
    HIPCHK(ctx->wws.ensure(nfl * sizeof(float)));
    float* q = (float*)ctx->wws.p;
    auto take = [&](size_t n) { float* r = q; q += n; return r; };
    float *Eb = take((size_t)R * NEK), *Gb = take((size_t)R * NEK);
    float *H1 = take((size_t)R * n1), *D1 = take((size_t)R * n1), *H2 = take((size_t)R * n2), *D2 = take((size_t)R * n2);
    float *H3 = take((size_t)R * n3), *D3 = take((size_t)R * n3), *H4 = take((size_t)R * n4), *D4 = take((size_t)R * n4);
    float *GE3 = take((size_t)R * NEB), *GE1 = take((size_t)R * NEB);
    float* z = take((size_t)n_inst * LZ);
    float* c13 = take((size_t)n_inst * nz);
    float* gz = (zpad && glat) ? take((size_t)R * LZ) : glat;  // d df / d z before its padding is cut off
    hipStream_t st = ctx->stream;
    if (zd) {
        HIPCHK(timed(ctx, "sdf_wide_hoist", [&] { return launch_wide_latent<double>(zd, zstride, n_inst, LH, LZ, z, st); }));
        zf = z;
    } else if (zpad) {  // fp32 [n_inst][LH] -> [n_inst][LZ]
        HIPCHK(timed(ctx, "sdf_wide_hoist", [&] { return launch_wide_latent<float>(zf, LH, n_inst, LH, LZ, z, st); }));
        zf = z;
    }
    const float w0 = w.w0;
    auto gemm = [&](const float* A1, int K1, const float* A2, int K2, const float* W, int M, int N, int epi,
                    const float* bias, const float* c, const float* d, int ldd, float* o1, float* o2,
                    const char* name) -> hipError_t {
        WideGemmArgs g{};
        g.A1 = A1; g.lda1 = K1; g.K1 = K1;
        g.A2 = A2; g.lda2 = K2; g.K2 = K2;
        g.W = W; g.M = M; g.N = N;
        g.bias = bias; g.c = c; g.ldc = nz; g.rows_per_inst = rows_per_inst;
        g.d = d; g.ldd = ldd; g.w5 = w.w5;
        g.out1 = o1; g.ld1 = N; g.out2 = o2; g.ld2 = N; g.w0 = w0; g.act = w.act;
        return timed(ctx, name, [&] { return launch_wide_gemm(g, epi, st); });
    };
    HIPCHK(gemm(zf, LZ, nullptr, 0, w.Hz, n_inst, nz, WIDE_EPI_STORE, w.bz, nullptr, nullptr, 0, c13, nullptr,
                "sdf_wide_hoist"));
    WideSdfArgs ea{};
    ea.rows = R; ea.n4 = n4; ea.pos = pos4; ea.emb_tab = w.emb_tab; ea.E = Eb; ea.G = Gb;
    ea.nb = w.nb; ea.nek = NEK; ea.neb = NEB;
    if (cons) { ea.x = cons->x; ea.p = cons->p; ea.np = cons->np; ea.h = cons->h; ea.Jh = cons->Jh; ea.max_df = cons->max_df; }
    HIPCHK(timed(ctx, "sdf_wide_emb", [&] { return launch_wide_emb(ea, st); }));
    // forward: L1..L4 (layer 3 sees [h2 | e] for res full / state; its latent part is in c13)
    HIPCHK(gemm(Eb, NEK, nullptr, 0, w.F1, R, n1, WIDE_EPI_SIN, nullptr, c13, nullptr, 0, H1, D1, "sdf_wide_gemm"));
    HIPCHK(gemm(H1, n1, nullptr, 0, w.F2, R, n2, WIDE_EPI_SIN, w.b2, nullptr, nullptr, 0, H2, D2, "sdf_wide_gemm"));
    HIPCHK(gemm(H2, n2, w.e3 ? Eb : nullptr, w.e3 ? NEK : 0, w.F3, R, n3, WIDE_EPI_SIN, nullptr, c13 + n1, nullptr, 0,
                H3, D3, "sdf_wide_gemm"));
    HIPCHK(gemm(H3, n3, nullptr, 0, w.F4, R, n4, WIDE_EPI_SIN_L4, w.b4, nullptr, nullptr, 0, H4, D4, "sdf_wide_gemm"));
    // backward (deltas overwrite the consumed activations): delta3 -> H3, delta2 -> H2, delta1 -> H1
    HIPCHK(gemm(D4, n4, nullptr, 0, w.B4, R, n3, WIDE_EPI_BWD, nullptr, nullptr, D3, n3, H3, nullptr, "sdf_wide_gemm"));
    HIPCHK(gemm(H3, n3, nullptr, 0, w.B3h, R, n2, WIDE_EPI_BWD, nullptr, nullptr, D2, n2, H2, nullptr, "sdf_wide_gemm"));
    if (w.e3)
        HIPCHK(gemm(H3, n3, nullptr, 0, w.B3e, R, NEB, WIDE_EPI_STORE, nullptr, nullptr, nullptr, 0, GE3, nullptr,
                    "sdf_wide_gemm"));
    else  // res 'latent': layer 3 does not see the embedding
        HIPCHK(hipMemsetAsync(GE3, 0, (size_t)R * NEB * sizeof(float), st));
    HIPCHK(gemm(H2, n2, nullptr, 0, w.B2, R, n1, WIDE_EPI_BWD, nullptr, nullptr, D1, n1, H1, nullptr, "sdf_wide_gemm"));
    HIPCHK(gemm(H1, n1, nullptr, 0, w.B1e, R, NEB, WIDE_EPI_STORE, nullptr, nullptr, nullptr, 0, GE1, nullptr,
                "sdf_wide_gemm"));
    if (glat) {  // d df / d z = delta1 W1z + delta3 W3z: one GEMM over the two K segments [delta1 | delta3]
        HIPCHK(gemm(H1, n1, H3, n3, w.Bz, R, LZ, WIDE_EPI_STORE, nullptr, nullptr, nullptr, 0, gz, nullptr,
                    "sdf_wide_gemm"));
        if (zpad)
            HIPCHK(hipMemcpy2DAsync(glat, (size_t)LH * sizeof(float), gz, (size_t)LZ * sizeof(float),
                                    (size_t)LH * sizeof(float), (size_t)R, hipMemcpyDeviceToDevice, st));
    }
    ea.H4 = H4; ea.GE3 = GE3; ea.GE1 = GE1; ea.w5 = w.w5; ea.b5 = w.b5; ea.out = out4;
    HIPCHK(timed(ctx, "sdf_wide_final", [&] { return launch_wide_final(ea, st); }));
    return SDFNMPC_OK;
}

template <typename T>
static int run_hoist(sdfnmpc_ctx* ctx, const sdfnmpc_net* net, const T* latent, long long stride, int n_inst,
                     float* c13) {
    HoistArgs<T> h{latent, stride, net->WzT, net->bias13, c13, n_inst};
    HIPCHK(timed(ctx, "sdf_hoist", [&] { return launch_hoist<T>(h, ctx->stream); }));
    return SDFNMPC_OK;
}

extern "C" int sdfnmpc_sdf_eval(sdfnmpc_ctx* ctx, const sdfnmpc_net* net, long long rows, const float* pos4,
                                const float* latent, int rows_per_inst, float* out4, float* grad_latent) {
    if (!ctx || !net || (!pos4 && rows > 0) || (!latent && rows > 0) || (!out4 && rows > 0) || rows < 0 ||
        rows_per_inst < 1)
        return fail(SDFNMPC_E_ARG, "bad sdfnmpc_sdf_eval arguments");
    if (net->device != ctx->device) return fail(SDFNMPC_E_ARG, "net and ctx are on different devices");
    if (rows == 0) return SDFNMPC_OK;
    ScopedDevice sd(ctx->device);
    const int n_inst = (int)((rows + rows_per_inst - 1) / rows_per_inst);
    if (net->wide)
        return run_wide(ctx, net, rows, (const float4*)pos4, latent, nullptr, 0, n_inst, rows_per_inst, (float4*)out4,
                        nullptr, grad_latent);
    HIPCHK(ctx->c13.ensure((size_t)n_inst * C13_STRIDE * sizeof(float)));
    int rc = run_hoist<float>(ctx, net, latent, L, n_inst, (float*)ctx->c13.p);
    if (rc) return rc;
    return run_sdf(ctx, net, rows, (const float4*)pos4, (const float*)ctx->c13.p, rows_per_inst, (float4*)out4,
                   grad_latent, grad_latent ? 32 : ctx->tile_rows);
}

// the host-pointer path's wait for its results (polling hipStreamQuery instead measured 3 us slower per
// call; tools/launch_lat.hip: a bare launch + hipStreamSynchronize is 11 us on the box)
static hipError_t host_wait(sdfnmpc_ctx* ctx) { return hipStreamSynchronize(ctx->stream); }

static bool srv_enabled(sdfnmpc_ctx* ctx) {
    if (ctx->srv.mode < 0) {
        const char* e = getenv("SDFNMPC_SDF_SERVER");
        ctx->srv.mode = (e && *e == '0') ? 0 : 1;
        if (const char* ms = getenv("SDFNMPC_SDF_SERVER_IDLE_MS")) {
            const double v = atof(ms);
            if (v > 0.0) ctx->srv.idle_s = v * 1e-3;
        }
        if (const char* ms = getenv("SDFNMPC_SDF_SERVER_LIFE_MS")) {
            const double v = atof(ms);
            if (v > 0.0) ctx->srv.life_s = v * 1e-3;
        }
    }
    return ctx->srv.mode == 1 && !ctx->srv.abandoned;
}

// One request to the resident SDF server (sdf_row.hip): the staged fp32 request (hp [rows][4], hl
// [rows][L]) goes into the mailbox, the results come back into ho in the staged path's layout.  The
// server is (re)launched when it is not running -- first call, a different network, or after it left on
// its idle timeout or its life bound (1 ms and 0.8 ms by default: the longest a device-wide synchronisation
// elsewhere in the process waits for it); a server that exits while a request is posted writes its epoch
// to `gone`, and the caller relaunches at once (the new server serves every seq_in above the seq_out it
// finds).
constexpr int SRV_FALLBACK = 1;  // srv_call: the server was abandoned; the caller takes the per-call launch path
static int srv_call(sdfnmpc_ctx* ctx, const sdfnmpc_net* net, int rows, const float* hp, const float* hl, bool grad,
                    float* ho) {
    using clk = std::chrono::steady_clock;
    auto& S = ctx->srv;
    if (!S.mb) {
        HIPCHK(hipHostMalloc((void**)&S.mb, sizeof(SdfMbox), hipHostMallocCoherent | hipHostMallocMapped));
        memset((void*)S.mb, 0, sizeof(SdfMbox));
        HIPCHK(hipHostGetDevicePointer((void**)&S.mb_dev, S.mb, 0));
        int lo = 0, hi = 0;
        (void)hipDeviceGetStreamPriorityRange(&lo, &hi);
        HIPCHK(hipStreamCreateWithPriority(&S.stream, hipStreamNonBlocking, hi));
        int khz = 0;
        HIPCHK(hipDeviceGetAttribute(&khz, hipDeviceAttributeWallClockRate, ctx->device));
        if (khz <= 0) khz = 100000;
        S.khz = khz;
        S.idle_ticks = (long long)(S.idle_s * khz * 1e3);
        S.life_ticks = (long long)(S.life_s * khz * 1e3);
        S.seq = 0;
        S.live = false;
    }
    if (S.live && S.net != net->uid && !srv_stop(ctx)) return SRV_FALLBACK;  // abandoned: serve this call per launch
    if (S.live && __atomic_load_n(&S.mb->gone, __ATOMIC_ACQUIRE) == S.epoch) {
        // it left (idle, life or stop) after publishing its last answer: nothing of it runs any more but
        // its kernel's exit, which the stream orders before the relaunch
        S.live = false;
        __atomic_store_n(&S.mb->stop, 0ull, __ATOMIC_RELEASE);
    }
    if (S.live && (S.mb->stop || std::chrono::duration<double>(clk::now() - S.last).count() > 0.5 * S.idle_s)) {
        const hipError_t q = hipStreamQuery(S.stream);
        if (q == hipSuccess) {
            S.live = false;
            __atomic_store_n(&S.mb->stop, 0ull, __ATOMIC_RELEASE);
        } else if (q == hipErrorNotReady && S.mb->stop) {
            return fail(SDFNMPC_E_HIP, "sdf server: the previous server has not left yet");
        } else if (q != hipErrorNotReady) {
            return fail(SDFNMPC_E_HIP, std::string("sdf server: ") + hipGetErrorString(q));
        }
    }
    const int LH = net->host.L;  // the mailbox holds [rows][4] | [rows][LH] (SdfMbox)
    memcpy(S.mb->in, hp, (size_t)rows * 4 * sizeof(float));
    memcpy(S.mb->in + (size_t)rows * 4, hl, (size_t)rows * LH * sizeof(float));
    S.mb->rows = rows;
    S.mb->grad = grad ? 1 : 0;
    const unsigned long long seq = ++S.seq;
    __atomic_store_n(&S.mb->seq_in, seq, __ATOMIC_RELEASE);
    auto relaunch = [&]() {
        ++S.epoch;
        return net->wide ? launch_sdf_server_wide(net->wrow, S.mb_dev, S.idle_ticks, S.life_ticks, S.epoch, S.stream)
                         : launch_sdf_server(net->row, S.mb_dev, S.idle_ticks, S.life_ticks, S.epoch, S.stream);
    };
    if (!S.live) {
        HIPCHK(relaunch());
        S.live = true;
        S.net = net->uid;
    }
    const auto t0 = clk::now();
    for (unsigned long spin = 1;; ++spin) {
        if (__atomic_load_n(&S.mb->seq_out, __ATOMIC_ACQUIRE) == seq) break;
        if (__atomic_load_n(&S.mb->gone, __ATOMIC_ACQUIRE) == S.epoch) {
            // the server left between requests (idle / life) without seeing this one: relaunch now
            if (__atomic_load_n(&S.mb->seq_out, __ATOMIC_ACQUIRE) == seq) break;
            HIPCHK(relaunch());
            continue;
        }
        if ((spin & 1023) == 0) {
            const hipError_t q = hipStreamQuery(S.stream);
            if (q == hipSuccess) {  // the server left before it saw this request
                if (__atomic_load_n(&S.mb->seq_out, __ATOMIC_ACQUIRE) == seq) break;
                HIPCHK(relaunch());
            } else if (q != hipErrorNotReady) {
                S.live = false;
                return fail(SDFNMPC_E_HIP, std::string("sdf server: ") + hipGetErrorString(q));
            }
            if (std::chrono::duration<double>(clk::now() - t0).count() > 5.0) {
                // ask it to leave, but do not wait on a server that stopped answering; a later call
                // queries the stream and relaunches only once it has gone
                __atomic_store_n(&S.mb->stop, 1ull, __ATOMIC_RELEASE);
                return fail(SDFNMPC_E_HIP, "sdf server: no answer within 5 s");
            }
        }
    }
    const volatile float* o = S.mb->out;
    const size_t n = (size_t)rows * (grad ? 4 + LH : 4);
    for (size_t i = 0; i < n; ++i) ho[i] = o[i];
    S.last = clk::now();
    const volatile SdfMbox* vm = S.mb;
    S.acc[0] += (double)(vm->t_staged - vm->t_seen) * 1e3 / S.khz;
    S.acc[1] += (double)(vm->t_done - vm->t_staged) * 1e3 / S.khz;
    S.acc[2] += std::chrono::duration<double>(S.last - t0).count() * 1e6;
    S.acc[3] += 1.0;
    if (!net->wide)  // row_eval's phase stamps (row_eval_wide writes none)
        for (int i = 0; i < 14; ++i)
            S.ph[i] += (double)(vm->t_phase[i] - (i ? vm->t_phase[i - 1] : vm->t_staged)) * 1e3 / S.khz;
    return SDFNMPC_OK;
}

// mean microseconds per served request since the last call: [0] staging the request into LDS, [1] the
// evaluation, [2] the host's wait from posting to the answer; [3] requests; [4..17] the evaluation's
// phases (row_eval's ROW_STAMPs) (diagnostics, tools/c2_server_probe.py)
extern "C" int sdfnmpc_ctx_sdf_server_stats(sdfnmpc_ctx* ctx, double* out18) {
    if (!ctx || !out18) return fail(SDFNMPC_E_ARG, "bad sdfnmpc_ctx_sdf_server_stats arguments");
    std::lock_guard<std::mutex> lk(ctx->mu);
    const double n = ctx->srv.acc[3];
    for (int i = 0; i < 3; ++i) out18[i] = n > 0 ? ctx->srv.acc[i] / n : 0.0;
    out18[3] = n;
    for (int i = 0; i < 14; ++i) out18[4 + i] = n > 0 ? ctx->srv.ph[i] / n : 0.0;
    for (double& a : ctx->srv.acc) a = 0.0;
    for (double& a : ctx->srv.ph) a = 0.0;
    return SDFNMPC_OK;
}

extern "C" int sdfnmpc_ctx_set_sdf_server(sdfnmpc_ctx* ctx, int on) {
    if (!ctx || on < 0 || on > 1) return fail(SDFNMPC_E_ARG, "bad sdfnmpc_ctx_set_sdf_server arguments");
    std::lock_guard<std::mutex> lk(ctx->mu);
    ScopedDevice sd(ctx->device);
    if (!on && !srv_stop(ctx)) return SDFNMPC_E_HIP;
    ctx->srv.mode = on;
    return SDFNMPC_OK;
}

// one launch of the network's row evaluator on the context's stream
static hipError_t launch_row(sdfnmpc_ctx* ctx, const sdfnmpc_net* net, const RowCall& c) {
    if (net->wide) {
        WideRowArgs ra = net->wrow;
        ra.c = c;
        return timed(ctx, "sdf_row_wide", [&] { return launch_sdf_row_wide(ra, ctx->stream); });
    }
    SdfRowArgs ra = net->row;
    ra.c = c;
    return timed(ctx, "sdf_row", [&] { return launch_sdf_row(ra, ctx->stream); });
}

extern "C" int sdfnmpc_sdf_eval_host(sdfnmpc_ctx* ctx, const sdfnmpc_net* net, int rows, const double* in,
                                     double* df, double* grad) {
    if (!ctx || !net || rows < 0 || (rows > 0 && (!in || !df))) return fail(SDFNMPC_E_ARG, "bad sdf_eval_host arguments");
    if (rows == 0) return SDFNMPC_OK;
    std::lock_guard<std::mutex> lk(ctx->mu);
    ScopedDevice sd(ctx->device);
    const int L = net->host.L, D = 3 + L;  // 131 for the deployed net (and every 128-latent one)
    // pinned staging: in [rows][4] pos | [rows][L] latent, out [rows][4] (df, d/dpos) | [rows][L] d/dlatent
    // (double -> float as L4CasADi does); one copy each way, one synchronisation
    const size_t nin = (size_t)rows * (4 + L), bytes = 2 * nin * sizeof(float);
    if (bytes > ctx->h_pin_bytes) {
        if (ctx->h_pin) (void)hipHostFree(ctx->h_pin);
        ctx->h_pin = nullptr;
        ctx->h_pin_bytes = 0;
        HIPCHK(hipHostMalloc((void**)&ctx->h_pin, bytes, hipHostMallocDefault));
        ctx->h_pin_bytes = bytes;
    }
    float* hp = ctx->h_pin;
    float* hl = hp + (size_t)rows * 4;
    float* ho = ctx->h_pin + nin;
    for (int r = 0; r < rows; ++r) {
        for (int c = 0; c < 3; ++c) hp[r * 4 + c] = (float)in[(size_t)r * D + c];
        hp[r * 4 + 3] = 0.0f;
        for (int k = 0; k < L; ++k) hl[(size_t)r * L + k] = (float)in[(size_t)r * D + 3 + k];
    }
    // the row evaluators: sdf_row.hip for the deployed network, sdf_row_wide.hip for a variant that fits it
    const bool use_row = net->wide ? net->wrow_ok && rows <= wide_row_max_rows(L) : rows <= SDF_ROW_MAX;
    bool served = false;
    if (use_row && srv_enabled(ctx)) {  // the resident server: no launch, no copies, no synchronisation
        const int rc = srv_call(ctx, net, rows, hp, hl, grad != nullptr, ho);
        if (rc != SDFNMPC_OK && rc != SRV_FALLBACK) return rc;
        served = rc == SDFNMPC_OK;
    }
    if (!served) {
        HIPCHK(ctx->hin.ensure(nin * sizeof(float)));
        HIPCHK(ctx->hout.ensure(nin * sizeof(float)));
        float* dpos = (float*)ctx->hin.p;
        float* dlat = dpos + (size_t)rows * 4;
        float* dout = (float*)ctx->hout.p;
        float* dglat = grad ? dout + (size_t)rows * 4 : nullptr;
        // the batched path's latent hoist depends on the latents only: reuse it while they repeat (the same
        // image's latent at every shooting node of an RTI); the positions go up every call
        const bool same_lat = !use_row && !net->wide && ctx->h_net == net->uid &&
                              ctx->h_lat.size() == (size_t)rows * L &&
                              !memcmp(ctx->h_lat.data(), hl, (size_t)rows * L * sizeof(float));
        HIPCHK(hipMemcpyAsync(dpos, hp, (same_lat ? (size_t)rows * 4 : nin) * sizeof(float), hipMemcpyHostToDevice,
                              ctx->stream));
        int rc = SDFNMPC_OK;
        if (use_row) {  // the latency path: one launch, no hoist.  Zero-copy (the kernel reading and writing the
            // pinned block over PCIe) was measured equal in wall time: the PCIe reads add ~2 us to the kernel,
            // as much as the two staging copies cost.
            HIPCHK(launch_row(ctx, net, RowCall{(const float4*)dpos, dlat, (float4*)dout, dglat, rows}));
        } else if (net->wide) {
            rc = sdfnmpc_sdf_eval(ctx, net, rows, dpos, dlat, 1, dout, dglat);
        } else {
            if (!same_lat) {
                HIPCHK(ctx->hc13.ensure((size_t)rows * C13_STRIDE * sizeof(float)));
                rc = run_hoist<float>(ctx, net, dlat, L, rows, (float*)ctx->hc13.p);
                if (rc) return rc;
                ctx->h_lat.assign(hl, hl + (size_t)rows * L);
                ctx->h_net = net->uid;
            }
            rc = run_sdf(ctx, net, rows, (const float4*)dpos, (const float*)ctx->hc13.p, 1, (float4*)dout, dglat,
                         grad ? 32 : ctx->tile_rows);
        }
        if (rc) {
            ctx->h_net = 0;
            return rc;
        }
        HIPCHK(hipMemcpyAsync(ho, dout, (grad ? nin : (size_t)rows * 4) * sizeof(float), hipMemcpyDeviceToHost,
                              ctx->stream));
        HIPCHK(host_wait(ctx));
    }
    const float* go = ho + (size_t)rows * 4;
    for (int r = 0; r < rows; ++r) {
        df[r] = ho[(size_t)r * 4];
        if (grad) {
            for (int c = 0; c < 3; ++c) grad[(size_t)r * D + c] = ho[(size_t)r * 4 + 1 + c];
            for (int k = 0; k < L; ++k) grad[(size_t)r * D + 3 + k] = go[(size_t)r * L + k];
        }
    }
    return SDFNMPC_OK;
}

// the scene's rows kernel: a mesh set takes its own, an indexed set the grid kernel, everything else the launch it has
// always taken
static hipError_t scene_sdf_rows_enqueue(sdfnmpc_ctx* ctx, const SceneSdfArgs& a, const sdfnmpc_scene* sc) {
    if (sc->is_inst) {  // an instanced set created as an SDF source
        const InstSdfArgs ia{a, sc->inst};
        return timed(ctx, "scene_sdf_rows_inst", [&] { return launch_scene_sdf_rows_inst(ia, ctx->stream); });
    }
    if (a.mesh.hdr && a.dyn)  // a mesh set with movers, created as an SDF source
        return timed(ctx, "scene_sdf_rows_mesh_mixed", [&] { return launch_scene_sdf_rows_mesh_mixed(a, ctx->stream); });
    if (a.mesh.hdr)  // a mesh set created as an SDF source
        return timed(ctx, "scene_sdf_rows_mesh", [&] { return launch_scene_sdf_rows_mesh(a, ctx->stream); });
    if (a.sc.ghdr && a.dyn)  // a mixed set: the grid plus movers
        return timed(ctx, "scene_sdf_rows_mixed", [&] { return launch_scene_sdf_rows_mixed(a, ctx->stream); });
    if (a.sc.ghdr) return timed(ctx, "scene_sdf_rows_grid", [&] { return launch_scene_sdf_rows_grid(a, ctx->stream); });
    return timed(ctx, "scene_sdf_rows", [&] { return launch_scene_sdf_rows(a, ctx->stream); });
}

// the launch of sdfnmpc_img_sdf_rows on the context stream: the scan reads its point from a buffer, the caller's pts or a
// workspace of the context
static int img_sdf_launch(sdfnmpc_ctx* ctx, ImgSdfArgs a) {
    if (a.rows <= 0) return SDFNMPC_OK;
    if (!a.pts) {
        HIPCHK(ctx->imgpts.ensure((size_t)a.rows * 3 * sizeof(float)));
        a.pts = (float*)ctx->imgpts.p;
    }
    HIPCHK(timed(ctx, "img_sdf_rows", [&] { return launch_img_sdf_rows(a, ctx->stream); }));
    return SDFNMPC_OK;
}

// ------------------------------------------------------------------------------------------------
// batched preparation phase
// pk != NULL (sdfnmpc_rti_prepare): the QP stage records are packed in the same phase.  With ny == 11
// the pack runs after the linearisation on the aux stream, beside the SDF kernel, and only the sdf row
// of C^T waits for the join; with the sdf cost (ny == 12) H and g depend on h[2], so the whole pack
// follows the join.  With lin_args.sdf_scene no network runs: linearize, the scene's rows kernel (scene_sdf.hip) and the
// whole pack follow each other on the main stream; lin_args.sdf_image is the same sequence with the image field's rows
// kernel (df_truth.hip: img_sdf_rows_kernel) in the middle.
static int lin_impl(sdfnmpc_ctx* ctx, const sdfnmpc_net* net, const sdfnmpc_quad_model* mdl,
                    const sdfnmpc_lin_args* a, const QpArgs* pk, bool* split_out = nullptr) {
    if (!ctx || !mdl || !a) return fail(SDFNMPC_E_ARG, "NULL argument");
    if (mdl->kind != SDFNMPC_MODEL_ATT && mdl->kind != SDFNMPC_MODEL_ATT_TAU)
        return fail(SDFNMPC_E_UNSUPPORTED, "model.kind: only 0 ('att') and 1 ('att_tau') are built");
    if (mdl->kind == SDFNMPC_MODEL_ATT_TAU) {
        if (mdl->rec_feas || mdl->stability)  // gen_model.py:74: implemented only for 'att'
            return fail(SDFNMPC_E_UNSUPPORTED, "model.kind 1 ('att_tau') with rec_feas / stability");
        if (!(mdl->tau_roll > 0.0) || !(mdl->tau_pitch > 0.0))
            return fail(SDFNMPC_E_ARG, "model.kind 1 ('att_tau') needs tau_roll > 0 and tau_pitch > 0");
    }
    if (a->no_sdf && a->sdf_scene) return fail(SDFNMPC_E_ARG, "lin_args.sdf_scene together with lin_args.no_sdf");
    if (a->no_sdf && a->sdf_image) return fail(SDFNMPC_E_ARG, "lin_args.sdf_image together with lin_args.no_sdf");
    if (a->sdf_scene && a->sdf_image) return fail(SDFNMPC_E_ARG, "lin_args.sdf_image together with lin_args.sdf_scene");
    // no network is evaluated: nothing reads the SDF, or the SDF row is the scene's exact distance (sdf_scene) or the
    // field of the camera image (sdf_image)
    const bool no_sdf = a->no_sdf != 0 || a->sdf_scene || a->sdf_image;
    if (!net && !no_sdf)
        return fail(SDFNMPC_E_ARG, "NULL network (only allowed with lin_args.no_sdf, .sdf_scene or .sdf_image)");
    if (a->B < 0 || a->N < 1 || a->np < 17 + (net ? net->host.L : 0) || (a->latent_mode != 0 && a->latent_mode != 1))
        return fail(SDFNMPC_E_ARG, "bad B/N/np/latent_mode");
    const int nyN = a->nyN == 0 ? 4 : a->nyN;
    if (nyN != 4 && nyN != 5) return fail(SDFNMPC_E_ARG, "lin_args.nyN must be 4 or 5");
    if ((nyN == 5) != (mdl->stability != 0)) return fail(SDFNMPC_E_ARG, "nyN == 5 exactly with model.stability");
    if (mdl->rec_feas && (mdl->poly_deg < 0 || mdl->poly_deg > SDFNMPC_POLY_DEG_MAX))
        return fail(SDFNMPC_E_ARG, "model.poly_deg must be 0..6");
    if ((mdl->rec_feas || mdl->stability) && (!a->hE || !a->JhE))
        return fail(SDFNMPC_E_ARG, "rec_feas / stability need lin_args.hE and JhE");
    if (a->B == 0) return SDFNMPC_OK;
    if (!a->x || !a->u || !a->p || !a->dt || !a->xn || !a->AB || !a->y || !a->Jy || !a->yN || !a->JyN || !a->h ||
        !a->Jh)
        return fail(SDFNMPC_E_ARG, "NULL array in sdfnmpc_lin_args");
    if (net && net->device != ctx->device) return fail(SDFNMPC_E_ARG, "net and ctx are on different devices");
    SceneSdfArgs ssa{};
    if (a->sdf_scene)  // refused before the first launch
        if (int rc_ = scene_sdf_args(ctx, a->sdf_scene, a->B, a->N, a->np, a->x, a->p, a->h, a->Jh, ssa)) return rc_;
    ImgSdfArgs isa{};
    if (a->sdf_image)
        if (int rc_ = img_sdf_args(ctx, a->sdf_image, a->B, a->N, a->np, a->x, a->p, a->h, a->Jh, nullptr, isa))
            return rc_;
    ScopedDevice sd(ctx->device);
    const long long rows = (long long)a->B * (a->N + 1);
    float4* sdf4 = (float4*)a->sdf;
    if (!sdf4) {
        HIPCHK(ctx->sdf4.ensure((size_t)rows * 16));
        sdf4 = (float4*)ctx->sdf4.p;
    }
    const int n_inst = a->latent_mode == 0 ? a->B : (int)rows;
    if (!no_sdf && !net->wide) HIPCHK(ctx->c13.ensure((size_t)n_inst * C13_STRIDE * sizeof(float)));
    // dynamics / cost / FOV constraints (independent of the network): forked onto the low-priority
    // aux stream so they fill the CUs the SDF kernel leaves idle (its tail), joined at the end
    LinArgs la{};
    la.x = a->x; la.u = a->u; la.p = a->p; la.dt = a->dt;
    la.xn = a->xn; la.AB = a->AB; la.y = a->y; la.Jy = a->Jy; la.yN = a->yN; la.JyN = a->JyN; la.h = a->h; la.Jh = a->Jh;
    la.B = a->B; la.N = a->N; la.np = a->np;
    la.m.gamma = mdl->gamma; la.m.roll = mdl->roll; la.m.pitch = mdl->pitch; la.m.wz = mdl->wz; la.m.g = mdl->g;
    for (int i = 0; i < 3; ++i)  // B_R_C^T B_p_C + [fov_const_offset, 0, 0]
        la.m.fov_off[i] = mdl->B_R_C[0 * 3 + i] * mdl->B_p_C[0] + mdl->B_R_C[1 * 3 + i] * mdl->B_p_C[1] +
                          mdl->B_R_C[2 * 3 + i] * mdl->B_p_C[2] + (i == 0 ? mdl->fov_const_offset : 0.0);
    la.m.max_df = net ? net->host.max_df : 1.0;
    for (int i = 0; i < 9; ++i) la.m.B_R_C[i] = mdl->B_R_C[i];
    la.m.rec_feas = mdl->rec_feas ? 1 : 0;
    la.m.stability = mdl->stability ? 1 : 0;
    la.m.poly_deg = mdl->poly_deg;
    for (int i = 0; i < SDFNMPC_POLY_MAX; ++i) la.m.poly[i] = mdl->poly[i];
    la.m.kind = mdl->kind;
    if (mdl->kind == SDFNMPC_MODEL_ATT_TAU) {
        la.m.itau_roll = 1.0 / mdl->tau_roll;
        la.m.itau_pitch = 1.0 / mdl->tau_pitch;
    }
    la.hE = a->hE;
    la.JhE = a->JhE;
    la.nyN = nyN;
    QpArgs pa{};
    // serial: the linearisation (and the whole pack) after the SDF kernel on the one stream -- the diagnostic
    // SDFNMPC_SERIAL_PREP, and the few-row latency path (B = 1), where the fork / join's event waits cost
    // more than the overlap gains (round 5: 0.643 vs 0.646 ms per B = 1 step)
    const bool serial = ctx->serial_prep || (!no_sdf && !net->wide && rows <= SDF_ROW_PREP_MAX);
    const bool split = pk && pk->ny == 11 && !serial && !no_sdf;  // pack beside the SDF kernel
    if (split_out) *split_out = split;
    if (pk) {
        pa = *pk;
        pa.pack_part = split ? 1 : 0;
    }
    // the fork: ev_fork marks the main stream's state (the inputs written), the auxiliary stream waits for
    // it and runs the linearisation (+ the pack's first part) beside the SDF kernel
    auto fork_mark = [&]() -> int {
        if (serial) return SDFNMPC_OK;
        HIPCHK(hipEventRecord(ctx->ev_fork, ctx->stream));
        return SDFNMPC_OK;
    };
    auto fork_launch = [&]() -> int {
        if (serial) return SDFNMPC_OK;
        HIPCHK(hipStreamWaitEvent(ctx->aux, ctx->ev_fork, 0));
        HIPCHK(timed(ctx, "linearize", [&] { return launch_linearize(la, ctx->aux); }, ctx->aux));
        if (split) HIPCHK(timed(ctx, "rti_qp_pack", [&] { return launch_rti_qp_pack(pa, ctx->aux); }, ctx->aux));
        HIPCHK(hipEventRecord(ctx->ev_join, ctx->aux));
        return SDFNMPC_OK;
    };
    auto fork_lin = [&]() -> int {
        int rc_ = fork_mark();
        return rc_ ? rc_ : fork_launch();
    };
    // after the join: the rest of the pack on the main stream
    auto finish_pack = [&]() -> int {
        if (!pk) return SDFNMPC_OK;
        // split: the sdf row of C^T is copied by rti_qp_kernel itself (sdf_row_patch), no launch here
        if (!split) HIPCHK(timed(ctx, "rti_qp_pack", [&] { return launch_rti_qp_pack(pa, ctx->stream); }));
        return SDFNMPC_OK;
    };
    int rc;
    if (no_sdf) {  // no constraint or cost reads the network: the linearisation alone, then the pack
        HIPCHK(timed(ctx, "linearize", [&] { return launch_linearize(la, ctx->stream); }, ctx->stream));
        if (a->sdf_scene)  // the SDF row from the scene's closed forms, between the linearisation and the pack
            HIPCHK(scene_sdf_rows_enqueue(ctx, ssa, a->sdf_scene->scene));
        if (a->sdf_image)  // or from the field of the camera image
            if (int rc_ = img_sdf_launch(ctx, isa)) return rc_;
        return finish_pack();
    }
    // 2. latent hoisting (latent = p[.][17:] as fp32)
    const long long stride = a->latent_mode == 0 ? (long long)(a->N + 1) * a->np : (long long)a->np;
    SdfArgs cons{};
    cons.x = a->x;
    cons.p = a->p;
    cons.np = a->np;
    cons.h = a->h;
    cons.Jh = a->Jh;
    cons.max_df = net->host.max_df;
    if (net->wide) {  // layer-by-layer schedule, linearisation forked first so it overlaps the GEMMs
        if ((rc = fork_lin())) return rc;
        rc = run_wide(ctx, net, rows, nullptr, nullptr, a->p + 17, stride, n_inst, a->latent_mode == 0 ? a->N + 1 : 1,
                      sdf4, &cons);
        if (rc) return rc;
    } else if (rows <= SDF_ROW_PREP_MAX) {  // a few rows (B = 1): one workgroup per row, no hoist
        // the row kernel is the critical path: queued right after the fork mark, before the host spends
        // the auxiliary stream's API calls (≈15 µs at B = 1, round 5 trace), which the mark keeps it
        // independent of
        if ((rc = fork_mark())) return rc;
        SdfRowArgs ra = net->row;
        ra.x = a->x; ra.p = a->p; ra.np = a->np;
        ra.zd = a->p + 17; ra.zstride = stride; ra.rows_per_inst = a->latent_mode == 0 ? a->N + 1 : 1;
        ra.h = a->h; ra.Jh = a->Jh; ra.max_df = net->host.max_df;
        ra.c.out = sdf4;
        ra.c.rows = (int)rows;
        HIPCHK(timed(ctx, "sdf_row", [&] { return launch_sdf_row(ra, ctx->stream); }));
        if ((rc = fork_launch())) return rc;
    } else {
        // the fork before the hoist (as the wide branch): linearize reads x, u, p and dt and nothing the hoist
        // writes, and sdf_hoist's 32 workgroups leave the GPU to it until sdf_mlp starts.  The auxiliary stream
        // keeps the lowest priority: at a higher one linearize and the pack take sdf_mlp's slots and the phase
        // is slower
        if ((rc = fork_lin())) return rc;
        rc = run_hoist<double>(ctx, net, a->p + 17, stride, n_inst, (float*)ctx->c13.p);
        if (rc) return rc;
        // 3. network forward + position gradient, with the sdf row of h / J_h in its epilogue
        rc = run_sdf(ctx, net, rows, nullptr, (const float*)ctx->c13.p,
                     a->latent_mode == 0 ? a->N + 1 : 1, sdf4, nullptr, ctx->tile_rows, &cons);
        if (rc) return rc;
    }
    if (serial)
        HIPCHK(timed(ctx, "linearize", [&] { return launch_linearize(la, ctx->stream); }, ctx->stream));
    else
        HIPCHK(hipStreamWaitEvent(ctx->stream, ctx->ev_join, 0));
    return finish_pack();
}

extern "C" int sdfnmpc_linearize(sdfnmpc_ctx* ctx, const sdfnmpc_net* net, const sdfnmpc_quad_model* mdl,
                                 const sdfnmpc_lin_args* a) {
    if (ctx) ctx->prep.valid = false;  // lin outputs may change under records packed earlier
    return lin_impl(ctx, net, mdl, a, nullptr);
}

// ------------------------------------------------------------------------------------------------
// batched QP (feedback phase) and RTI step
// the constraint set of sdfnmpc_qp_opts (include/sdfnmpc.h): counts, columns and their order
static int qp_cset_check(const sdfnmpc_qp_opts* o) {
    if (o->nh < 0 || o->nh > 3) return fail(SDFNMPC_E_ARG, "qp opts: nh must be 0..3");
    for (int j = 0; j < o->nh; ++j)
        if (o->h_col[j] < 0 || o->h_col[j] > 2 || (j && o->h_col[j] == o->h_col[0]) || (j == 2 && o->h_col[2] == o->h_col[1]))
            return fail(SDFNMPC_E_ARG, "qp opts: h_col must be distinct columns 0..2");
    if (o->nhs < 0 || o->nhs > o->nh) return fail(SDFNMPC_E_ARG, "qp opts: nhs (hard stage rows) must be 0..nh");
    if (o->nhN < 0 || o->nhN > SDFNMPC_NHN_MAX || o->nsN < 0 || o->nsN > 3 || o->nsN > o->nhN || o->nhN - o->nsN > 6)
        return fail(SDFNMPC_E_ARG, "qp opts: terminal rows nhN <= 8 with nsN <= 3 soft and <= 6 hard");
    for (int j = 0; j < o->nhN; ++j) {
        if (o->hN_col[j] < -1 || o->hN_col[j] > 2 || o->hE_col[j] < -1 || o->hE_col[j] >= SDFNMPC_NHE ||
            (o->hN_col[j] < 0 && o->hE_col[j] < 0))
            return fail(SDFNMPC_E_ARG, "qp opts: terminal row j needs hN_col in -1..2 / hE_col in -1..5, not both -1");
        if (!(o->lhN[j] <= o->uhN[j])) return fail(SDFNMPC_E_ARG, "qp opts: terminal bounds lhN > uhN");
    }
    if (o->nyN != 4 && o->nyN != 5) return fail(SDFNMPC_E_ARG, "qp opts: nyN must be 4 or 5");
    return SDFNMPC_OK;
}
static QpRows qp_rows_of(const sdfnmpc_qp_opts* o) { return QpRows{o->nh, o->nhN, o->nsN, o->nhs}; }
// the network is read by a constraint row (stage h_col or terminal hN_col == 2) or the sdf cost
static bool qp_needs_sdf(const sdfnmpc_qp_opts* o) {
    bool need = o->ny == 12;
    for (int j = 0; j < o->nh; ++j) need = need || o->h_col[j] == 2;
    for (int j = 0; j < o->nhN; ++j) need = need || o->hN_col[j] == 2;
    return need;
}
// validation and kernel arguments shared by sdfnmpc_qp_solve / sdfnmpc_rti_prepare / sdfnmpc_qp_feedback
// (sizes the workspace; the caller holds the device scope)
static int qp_build(sdfnmpc_ctx* ctx, const sdfnmpc_qp_opts* o, const sdfnmpc_qp_args* a, QpArgs& q) {
    if (a->B < 0 || a->N < 1 || a->N > 200) return fail(SDFNMPC_E_ARG, "bad B/N for the QP");
    if (!a->xn || !a->AB || !a->y || !a->Jy || !a->yN || !a->JyN || !a->h || !a->Jh || !a->x || !a->u || !a->x0 ||
        !a->yref || !a->W || !a->yNref || !a->WN || !a->dt || !a->dx || !a->du)
        return fail(SDFNMPC_E_ARG, "NULL array in sdfnmpc_qp_args");
    if (o->lm <= 0.0 || o->max_iter < 1 || !(o->tol > 0.0))
        return fail(SDFNMPC_E_ARG, "qp opts: lm > 0 (strict convexity), max_iter >= 1, tol > 0 required");
    if (o->ny != 11 && o->ny != 12) return fail(SDFNMPC_E_ARG, "qp opts: ny must be 11 or 12 (sdf_cost)");
    if (int rc = qp_cset_check(o)) return rc;
    bool term_e = false;
    for (int j = 0; j < o->nhN; ++j) term_e = term_e || o->hE_col[j] >= 0;
    if (term_e && (!a->hE || !a->JhE)) return fail(SDFNMPC_E_ARG, "qp args: terminal rows read hE / JhE (NULL)");
    if (qp_lds_bytes(a->N, qp_rows_of(o)) > ctx->lds_per_cu)
        return fail(SDFNMPC_E_UNSUPPORTED, "horizon too long for the LDS-resident QP");
    HIPCHK(ctx->qpw.ensure((size_t)a->B * qp_work_doubles(a->N) * sizeof(double)));
    const bool own_st = !a->status || !a->iters || !a->res;
    if (own_st) HIPCHK(ctx->qpst.ensure((size_t)a->B * (2 * sizeof(int) + 2 * sizeof(double))));
    q = QpArgs{};
    q.B = a->B; q.N = a->N;
    q.xn = a->xn; q.AB = a->AB; q.y = a->y; q.Jy = a->Jy; q.yN = a->yN; q.JyN = a->JyN; q.h = a->h; q.Jh = a->Jh;
    q.hE = a->hE; q.JhE = a->JhE;
    q.x = a->x; q.u = a->u; q.x0 = a->x0; q.yref = a->yref; q.W = a->W; q.yNref = a->yNref; q.WN = a->WN; q.dt = a->dt;
    q.dx = a->dx; q.du = a->du; q.slack = a->slack;
    double* stbuf = (double*)ctx->qpst.p;
    q.res = a->res ? a->res : stbuf;
    q.status = a->status ? a->status : (int*)(stbuf + 2 * a->B);
    q.iters = a->iters ? a->iters : (int*)(stbuf + 2 * a->B) + a->B;
    q.work = (double*)ctx->qpw.p;
    for (int i = 0; i < 4; ++i) { q.lbu[i] = o->lbu[i]; q.ubu[i] = o->ubu[i]; }
    for (int i = 0; i < 3; ++i) { q.lh[i] = o->lh[i]; q.uh[i] = o->uh[i]; q.zl[i] = o->zl[i]; q.Zl[i] = o->Zl[i]; }
    q.lm = o->lm; q.tol = o->tol; q.max_iter = o->max_iter; q.cost_scaling = o->cost_scaling; q.ny = o->ny;
    q.lm_scaling = o->lm_scaling;
    q.warm_start = o->warm_start ? 1 : 0;
    q.nh = o->nh; q.nhN = o->nhN; q.nsN = o->nsN; q.nyN = o->nyN; q.nhs = o->nhs;
    q.seg_rows = qp_is_seg_set(*o) ? 1 : 0;
    q.sdf_row = -1;
    for (int j = 0; j < 3; ++j) {
        q.h_col[j] = j < o->nh ? o->h_col[j] : 0;
        if (j < o->nh && o->h_col[j] == 2) q.sdf_row = j;
        q.zlN[j] = o->zlN[j]; q.ZlN[j] = o->ZlN[j];
    }
    for (int j = 0; j < QP_NHN; ++j) {
        q.hN_col[j] = j < o->nhN ? o->hN_col[j] : -1;
        q.hE_col[j] = j < o->nhN ? o->hE_col[j] : -1;
        q.lhN[j] = o->lhN[j]; q.uhN[j] = o->uhN[j];
    }
    return SDFNMPC_OK;
}

// the constraint set a preparation packed its records under (stage rows' columns and kinds, terminal rows'
// columns, the terminal residual width) and the feedback must match: an FNV-1a hash of those fields
static long long cset_key(const QpArgs& q) {
    unsigned long long h = 1469598103934665603ull;
    auto mix = [&](long long v) { h = (h ^ (unsigned long long)(v + 7)) * 1099511628211ull; };
    mix(q.nh); mix(q.nhs); mix(q.nhN); mix(q.nsN); mix(q.nyN);
    for (int j = 0; j < 3; ++j) mix(q.h_col[j]);
    for (int j = 0; j < QP_NHN; ++j) { mix(q.hN_col[j]); mix(q.hE_col[j]); }
    return (long long)(h >> 1);
}

// the IPM kernel of this context and horizon: the segmented one (four wavefronts per instance,
// rti_qp_seg.hip) where it supports N, unless the context asks for the serial one (rti_qp.hip)
static hipError_t qp_launch(sdfnmpc_ctx* ctx, const QpArgs& q) {
    if (qp_kernel_for(ctx, q.N, q.B, q.seg_rows != 0) == SDFNMPC_QP_SEGMENTED) return launch_rti_qp_seg(q, ctx->stream);
    return launch_rti_qp(q, ctx->stream);
}

extern "C" int sdfnmpc_qp_solve(sdfnmpc_ctx* ctx, const sdfnmpc_qp_opts* o, const sdfnmpc_qp_args* a) {
    if (!ctx || !o || !a) return fail(SDFNMPC_E_ARG, "NULL argument");
    ctx->prep.valid = false;  // the workspace is repacked here
    if (a->B == 0) return SDFNMPC_OK;
    ScopedDevice sd(ctx->device);
    QpArgs q;
    if (int rc = qp_build(ctx, o, a, q)) return rc;
    HIPCHK(timed(ctx, "rti_qp_pack", [&] { return launch_rti_qp_pack(q, ctx->stream); }));
    HIPCHK(timed(ctx, "rti_qp", [&] { return qp_launch(ctx, q); }));
    return SDFNMPC_OK;
}

extern "C" int sdfnmpc_rti_prepare(sdfnmpc_ctx* ctx, const sdfnmpc_net* net, const sdfnmpc_quad_model* mdl,
                                   const sdfnmpc_lin_args* la, const sdfnmpc_qp_opts* o, const sdfnmpc_qp_args* qa) {
    if (!ctx || !mdl || !la || !o || !qa) return fail(SDFNMPC_E_ARG, "NULL argument");
    if (la->no_sdf && qp_needs_sdf(o)) return fail(SDFNMPC_E_ARG, "rti_prepare: lin_args.no_sdf, but the QP reads the sdf");
    if ((la->nyN == 0 ? 4 : la->nyN) != o->nyN) return fail(SDFNMPC_E_ARG, "rti_prepare: lin_args.nyN != qp opts nyN");
    ctx->prep.valid = false;
    if (la->B != qa->B || la->N != qa->N) return fail(SDFNMPC_E_ARG, "rti_prepare: lin and qp args differ in B / N");
    if (la->xn != qa->xn || la->AB != qa->AB || la->y != qa->y || la->Jy != qa->Jy || la->yN != qa->yN ||
        la->JyN != qa->JyN || la->h != qa->h || la->Jh != qa->Jh || la->x != qa->x || la->u != qa->u)
        return fail(SDFNMPC_E_ARG, "rti_prepare: the qp args must name the lin args' iterate and outputs");
    if (la->B == 0) return SDFNMPC_OK;
    ScopedDevice sd(ctx->device);
    QpArgs q;
    if (int rc = qp_build(ctx, o, qa, q)) return rc;
    bool split = false;
    if (int rc = lin_impl(ctx, net, mdl, la, &q, &split)) return rc;
    ctx->prep.valid = true;
    ctx->prep.sdf_row_patch = split;  // lin_impl's split pack: no sdf row in the records
    ctx->prep.B = qa->B;
    ctx->prep.N = qa->N;
    ctx->prep.xn = qa->xn;
    ctx->prep.work = q.work;
    ctx->prep.ny = q.ny;
    ctx->prep.lm = q.lm;
    ctx->prep.cost_scaling = q.cost_scaling;
    ctx->prep.lm_scaling = q.lm_scaling;
    ctx->prep.cset = cset_key(q);
    return SDFNMPC_OK;
}

extern "C" int sdfnmpc_qp_feedback(sdfnmpc_ctx* ctx, const sdfnmpc_qp_opts* o, const sdfnmpc_qp_args* a) {
    if (!ctx || !o || !a) return fail(SDFNMPC_E_ARG, "NULL argument");
    if (a->B == 0) return SDFNMPC_OK;
    if (!ctx->prep.valid || ctx->prep.B != a->B || ctx->prep.N != a->N || ctx->prep.xn != a->xn)
        return fail(SDFNMPC_E_ARG, "qp_feedback: no stage records from sdfnmpc_rti_prepare for these arguments");
    ScopedDevice sd(ctx->device);
    QpArgs q;
    if (int rc = qp_build(ctx, o, a, q)) return rc;
    if (q.work != ctx->prep.work) return fail(SDFNMPC_E_ARG, "qp_feedback: workspace moved since rti_prepare");
    if (q.ny != ctx->prep.ny || q.lm != ctx->prep.lm || q.cost_scaling != ctx->prep.cost_scaling ||
        q.lm_scaling != ctx->prep.lm_scaling || cset_key(q) != ctx->prep.cset)  // the stage records hold H, g, C^T
        // packed under the prepare's options
        return fail(SDFNMPC_E_ARG, "qp_feedback: ny / lm / cost scaling / the constraint set differ from sdfnmpc_rti_prepare's");
    ctx->prep.valid = false;  // one feedback per preparation, as in acados' SQP-RTI
    q.sdf_row_patch = ctx->prep.sdf_row_patch ? 1 : 0;
    HIPCHK(timed(ctx, "rti_qp", [&] { return qp_launch(ctx, q); }));
    return SDFNMPC_OK;
}

// ------------------------------------------------------------------------------------------------
// the control step as a HIP graph (include/sdfnmpc.h sdfnmpc_step_create)
struct sdfnmpc_step {
    hipGraph_t graph = nullptr;
    hipGraphExec_t exec = nullptr;
    int device = 0;
    const sdfnmpc_ctx* ctx = nullptr;  // the context whose workspaces the graph's kernels address
    unsigned long long ws_gen = 0;     // ctx_ws_gen at capture
};
// The graph's kernels hold the context's device workspaces as they were at capture.  Every reallocation
// (a later call with a larger B or N grows them: DevBuf::ensure frees the old buffer) bumps a DevBuf's
// generation, so the sum over the workspaces changes exactly when one of them moved.
static unsigned long long ctx_ws_gen(const sdfnmpc_ctx* c) {
    return c->c13.gen + c->sdf4.gen + c->lat.gen + c->out4.gen + c->glat.gen + c->qpw.gen + c->qpst.gen + c->wws.gen;
}

static int step_eager(sdfnmpc_ctx* ctx, const sdfnmpc_net* net, const sdfnmpc_quad_model* mdl, const sdfnmpc_lin_args* la,
                      const sdfnmpc_qp_opts* o, const sdfnmpc_qp_args* qa, double* u0, const int* status) {
    if (int rc = sdfnmpc_rti_prepare(ctx, net, mdl, la, o, qa)) return rc;
    if (int rc = sdfnmpc_qp_feedback(ctx, o, qa)) return rc;
    // the step applies to the iterate the QP linearised about (qp_args.x, .u: the caller's writable buffers)
    return sdfnmpc_rti_apply(ctx, qa->B, qa->N, const_cast<double*>(qa->x), const_cast<double*>(qa->u), qa->dx, qa->du, u0,
                             status);
}

extern "C" int sdfnmpc_step_create(sdfnmpc_ctx* ctx, const sdfnmpc_net* net, const sdfnmpc_quad_model* mdl,
                                   const sdfnmpc_lin_args* la, const sdfnmpc_qp_opts* o, const sdfnmpc_qp_args* qa,
                                   double* u0, const int* status, sdfnmpc_step** out) {
    if (!ctx || !mdl || !la || !o || !qa || !out) return fail(SDFNMPC_E_ARG, "NULL argument to sdfnmpc_step_create");
    *out = nullptr;
    if (qa->B < 1) return fail(SDFNMPC_E_ARG, "step_create: B must be >= 1");
    if (la->sdf_scene) return fail(SDFNMPC_E_UNSUPPORTED, "step_create: lin_args.sdf_scene (a scene as the SDF source) is not captured");
    if (la->sdf_image) return fail(SDFNMPC_E_UNSUPPORTED, "step_create: lin_args.sdf_image (an image as the SDF source) is not captured");
    // once eagerly: every workspace is allocated and every argument checked before the capture (no
    // allocation may happen inside it)
    if (int rc = step_eager(ctx, net, mdl, la, o, qa, u0, status)) return rc;
    ScopedDevice sd(ctx->device);
    HIPCHK(hipStreamSynchronize(ctx->stream));
    // capture on a private stream (the context stream may be the legacy null stream, which cannot be
    // captured); the fork / join events bring the auxiliary stream into the capture
    hipStream_t cs = nullptr;
    HIPCHK(hipStreamCreateWithFlags(&cs, hipStreamNonBlocking));
    hipStream_t saved = ctx->stream;
    const bool timing = ctx->timing;
    ctx->timing = false;
    ctx->stream = cs;
    hipGraph_t g = nullptr;
    int rc = SDFNMPC_OK;
    hipError_t e = hipStreamBeginCapture(cs, hipStreamCaptureModeRelaxed);
    if (e == hipSuccess) {
        rc = step_eager(ctx, net, mdl, la, o, qa, u0, status);
        e = hipStreamEndCapture(cs, &g);  // always ends the capture, also after a failed call
    }
    ctx->stream = saved;
    ctx->timing = timing;
    (void)hipStreamDestroy(cs);
    if (rc) {
        if (g) (void)hipGraphDestroy(g);
        return rc;
    }
    if (e != hipSuccess || !g) {
        if (g) (void)hipGraphDestroy(g);
        return fail(SDFNMPC_E_HIP, std::string("step_create: stream capture failed: ") + hipGetErrorString(e));
    }
    hipGraphExec_t x = nullptr;
    e = hipGraphInstantiate(&x, g, nullptr, nullptr, 0);
    if (e != hipSuccess) {
        (void)hipGraphDestroy(g);
        return fail(SDFNMPC_E_HIP, std::string("step_create: graph instantiation failed: ") + hipGetErrorString(e));
    }
    auto* st = new sdfnmpc_step;
    st->graph = g;
    st->exec = x;
    st->device = ctx->device;
    st->ctx = ctx;
    st->ws_gen = ctx_ws_gen(ctx);
    *out = st;
    return SDFNMPC_OK;
}

extern "C" int sdfnmpc_step_launch(sdfnmpc_ctx* ctx, sdfnmpc_step* st) {
    if (!ctx || !st) return fail(SDFNMPC_E_ARG, "NULL argument to sdfnmpc_step_launch");
    if (st->device != ctx->device || st->ctx != ctx) return fail(SDFNMPC_E_ARG, "step_launch: step captured on another context");
    if (ctx_ws_gen(ctx) != st->ws_gen)
        return fail(SDFNMPC_E_ARG, "step_launch: a context workspace was reallocated since the capture (a call with a larger "
                                   "B or N); destroy the step and create it again");
    ScopedDevice sd(ctx->device);
    HIPCHK(hipGraphLaunch(st->exec, ctx->stream));
    return SDFNMPC_OK;
}

extern "C" void sdfnmpc_step_destroy(sdfnmpc_step* st) {
    if (!st) return;
    ScopedDevice sd(st->device);
    if (st->exec) (void)hipGraphExecDestroy(st->exec);
    if (st->graph) (void)hipGraphDestroy(st->graph);
    delete st;
}

extern "C" int sdfnmpc_pack_refs(sdfnmpc_ctx* ctx, const sdfnmpc_ref_opts* o, const sdfnmpc_ref_args* a) {
    if (!ctx || !o || !a) return fail(SDFNMPC_E_ARG, "NULL argument to sdfnmpc_pack_refs");
    if (a->B < 0 || a->N < 1 || a->np < 17 || (a->ny != 11 && a->ny != 12) || !a->p)
        return fail(SDFNMPC_E_ARG, "pack_refs: bad B / N / np / ny or NULL p");
    if (o->mode < -2 || o->mode > 2) return fail(SDFNMPC_E_ARG, "pack_refs: mode must be -2..2");
    if (o->mode == -2 && (!a->W_p_Bo || !a->W_R_Bo)) return fail(SDFNMPC_E_ARG, "pack_refs: mode -2 (pose only) needs W_p_Bo and W_R_Bo");
    if (o->mode >= 0 && (!a->x0 || a->x0_stride < 7 || !a->wrow || !a->yref || !a->W || !a->yNref || !a->WN))
        return fail(SDFNMPC_E_ARG, "pack_refs: x0 (stride >= 7), wrow and the reference outputs are required");
    if (o->mode == 0 && (a->n_wp < 1 || a->n_wp > RP_MAX_WP || !a->wp_p || !a->wp_q))
        return fail(SDFNMPC_E_ARG, "pack_refs: mode 0 needs 1..32 waypoints (wp_p, wp_q)");
    if (o->mode == 1 && !a->vw) return fail(SDFNMPC_E_ARG, "pack_refs: mode 1 needs vw");
    if (o->mode != -2 && a->latent && (!a->W_p_Bo || !a->W_R_Bo || a->L < 1 || 17 + a->L > a->np))
        return fail(SDFNMPC_E_ARG, "pack_refs: latent needs W_p_Bo, W_R_Bo and 17 + L <= np");
    ScopedDevice sd(ctx->device);
    RefPackArgs r{};
    r.B = a->B; r.N = a->N; r.np_ = a->np; r.ny = a->ny; r.n_wp = a->n_wp; r.L = a->L;
    r.nyN = a->nyN == 0 ? 4 : a->nyN;
    if (r.nyN != 4 && r.nyN != 5) return fail(SDFNMPC_E_ARG, "pack_refs: nyN must be 4 or 5");
    r.mode = o->mode; r.yaw_mode = o->yaw_mode; r.st_enable = o->st_enable; r.st_mode = o->st_mode;
    r.st_dang = o->st_dang; r.align_off = o->align_off; r.dmin = o->dmin; r.vref = o->vref; r.wzref = o->wzref;
    r.T = o->T;
    for (int i = 0; i < 3; ++i) r.B_p_C[i] = o->B_p_C[i];
    for (int i = 0; i < 9; ++i) r.B_R_C[i] = o->B_R_C[i];
    r.x0 = a->x0; r.x0_stride = a->x0_stride; r.wp_p = a->wp_p; r.wp_q = a->wp_q; r.vw = a->vw; r.wrow = a->wrow;
    r.latent = a->latent; r.W_p_Bo = a->W_p_Bo; r.W_R_Bo = a->W_R_Bo; r.flag = a->flag;
    if (o->mode == -2) r.latent = r.flag = nullptr;  // pose only: the latent and flag columns stay
    r.p = a->p; r.yref = a->yref; r.W = a->W; r.yNref = a->yNref; r.WN = a->WN;
    HIPCHK(timed(ctx, "ref_pack", [&] { return launch_ref_pack(r, ctx->stream); }));
    return SDFNMPC_OK;
}

extern "C" int sdfnmpc_rti_apply(sdfnmpc_ctx* ctx, int B, int N, double* x, double* u, const double* dx,
                                 const double* du, double* u0, const int* status) {
    if (!ctx || B < 0 || N < 1 || (B > 0 && (!x || !u || !dx || !du))) return fail(SDFNMPC_E_ARG, "bad rti_apply arguments");
    ScopedDevice sd(ctx->device);
    HIPCHK(timed(ctx, "rti_apply", [&] { return launch_rti_apply(B, N, x, u, dx, du, u0, status, ctx->stream); }));
    return SDFNMPC_OK;
}

// ------------------------------------------------------------------------------------------------
// the plant of a closed loop (plant.hip).  plant_args checks the options and fills the kernel's
// argument block (nothing is launched); plant_launch launches a filled block on the context stream,
// timed as "plant".  Both are shared with sdfnmpc_solver_rollout (solver.hip), which adds the log pointers.
int sdfn::plant_args(const sdfnmpc_plant_opts* o, int B, const double* x, const double* u, double* x_next,
                     PlantArgs& out) {
    if (!o || B < 0 || (B > 0 && (!x || !u || !x_next)))
        return fail(SDFNMPC_E_ARG, "plant: NULL argument or B < 0");
    if (o->kind != SDFNMPC_MODEL_ATT && o->kind != SDFNMPC_MODEL_ATT_TAU)
        return fail(SDFNMPC_E_UNSUPPORTED, "plant opts: kind: only 0 ('att') and 1 ('att_tau') are built");
    if (o->substeps < 1 || o->substeps > PLANT_MAX_SUBSTEPS) return fail(SDFNMPC_E_ARG, "plant opts: substeps must be 1..64");
    if (!(o->dt > 0.0)) return fail(SDFNMPC_E_ARG, "plant opts: dt must be > 0");
    if (o->kind == SDFNMPC_MODEL_ATT_TAU && (!(o->tau_roll > 0.0) || !(o->tau_pitch > 0.0)))
        return fail(SDFNMPC_E_ARG, "plant opts: kind 1 ('att_tau') needs tau_roll > 0 and tau_pitch > 0");
    PlantArgs a{};
    a.B = B; a.kind = o->kind; a.substeps = o->substeps;
    a.gamma = o->gamma; a.roll = o->roll; a.pitch = o->pitch; a.wz = o->wz; a.g = o->g; a.dt = o->dt;
    if (o->kind == SDFNMPC_MODEL_ATT_TAU) {
        a.itau_roll = 1.0 / o->tau_roll;
        a.itau_pitch = 1.0 / o->tau_pitch;
    }
    a.x = x; a.u = u; a.x_next = x_next; a.acc_dist = o->acc_dist; a.gamma_scale = o->gamma_scale;
    out = a;
    return SDFNMPC_OK;
}

int sdfn::plant_launch(sdfnmpc_ctx* ctx, const PlantArgs& a) {
    ScopedDevice sd(ctx->device);
    HIPCHK(timed(ctx, "plant", [&] { return launch_plant(a, ctx->stream); }));
    return SDFNMPC_OK;
}

extern "C" int sdfnmpc_plant_step(sdfnmpc_ctx* ctx, const sdfnmpc_plant_opts* o, int B, const double* x, const double* u,
                                  double* x_next) {
    if (!ctx) return fail(SDFNMPC_E_ARG, "NULL context");
    PlantArgs a{};
    if (int rc = plant_args(o, B, x, u, x_next, a)) return rc;
    return plant_launch(ctx, a);
}

// ------------------------------------------------------------------------------------------------
// the vehicle model around the plant (vehicle.hip; struct sdfnmpc_vehicle: engine.h)

// the option half of a VehicleArgs block (the plant's block, the frame, x_est and the logs are the caller's)
static VehicleArgs vehicle_block(const sdfnmpc_vehicle* v, double dt) {
    const sdfnmpc_vehicle_opts& o = v->o;
    VehicleArgs a{};
    a.P.B = v->B;
    a.P.x_next = v->x_true;
    a.key0 = (unsigned)(o.seed & 0xffffffffull); a.key1 = (unsigned)(o.seed >> 32);
    a.delay = o.d;
    a.itau_m = o.tau_m > 0.0 ? 1.0 / o.tau_m : 0.0;
    for (int i = 0; i < 3; ++i) a.drag[i] = o.drag[i];
    a.has_drag = o.drag[0] > 0.0 || o.drag[1] > 0.0 || o.drag[2] > 0.0;
    a.has_gust = o.gust_std > 0.0;
    if (a.has_gust) {
        a.gust_phi = o.gust_tau > 0.0 ? std::exp(-dt / o.gust_tau) : 0.0;
        a.gust_amp = o.gust_std * std::sqrt(1.0 - a.gust_phi * a.gust_phi);
    }
    a.est_std_p = o.est_std_p; a.est_std_v = o.est_std_v; a.est_std_yaw = o.est_std_yaw;
    a.est_noise = o.est_std_p > 0.0 || o.est_std_v > 0.0 || o.est_std_yaw > 0.0;
    a.est_bias = o.est_bias; a.stream_id = o.stream_id;
    a.gamma_act = v->gamma_act; a.w = v->w; a.ring = v->ring;
    a.g = o.g; a.hover_u0 = o.g / o.gamma;
    return a;
}

extern "C" int sdfnmpc_vehicle_create(sdfnmpc_ctx* ctx, const sdfnmpc_vehicle_opts* o, int B, sdfnmpc_vehicle** out) {
    if (!ctx || !o || !out) return fail(SDFNMPC_E_ARG, "NULL argument to sdfnmpc_vehicle_create");
    *out = nullptr;
    if (B < 0) return fail(SDFNMPC_E_ARG, "vehicle: B < 0");
    if (o->d < 0 || o->d > VEHICLE_MAX_DELAY) return fail(SDFNMPC_E_ARG, "vehicle opts: d (the input delay) must be 0..8");
    auto ok = [](double v) { return std::isfinite(v) && v >= 0.0; };
    if (!ok(o->tau_m) || !ok(o->gust_std) || !ok(o->gust_tau) || !ok(o->est_std_p) || !ok(o->est_std_v) ||
        !ok(o->est_std_yaw) || !ok(o->drag[0]) || !ok(o->drag[1]) || !ok(o->drag[2]))
        return fail(SDFNMPC_E_ARG, "vehicle opts: tau_m, drag, gust_std, gust_tau and est_std_* must be finite and not negative");
    if (!(o->g > 0.0) || !std::isfinite(o->g) || !(o->gamma > 0.0) || !std::isfinite(o->gamma))
        return fail(SDFNMPC_E_ARG, "vehicle opts: g and gamma must be positive and finite");
    auto* v = new sdfnmpc_vehicle();
    v->ctx = ctx; v->device = ctx->device; v->B = B; v->o = *o;
    v->neutral = o->d == 0 && o->tau_m == 0.0 && o->gust_std == 0.0 && o->drag[0] == 0.0 && o->drag[1] == 0.0 &&
                 o->drag[2] == 0.0 && o->est_std_p == 0.0 && o->est_std_v == 0.0 && o->est_std_yaw == 0.0 && !o->est_bias;
    ScopedDevice sd(ctx->device);
    const size_t n = (size_t)B * (10 + 1 + 3 + 4 * (size_t)o->d + 12);
    hipError_t e = hipMalloc((void**)&v->block, n * sizeof(double) + 16);
    if (e == hipSuccess) e = hipMemsetAsync(v->block, 0, n * sizeof(double) + 16, ctx->stream);
    if (e != hipSuccess) {
        if (v->block) (void)hipFree(v->block);
        delete v;
        return fail(SDFNMPC_E_HIP, std::string("vehicle buffers: ") + hipGetErrorString(e));
    }
    v->x_true = v->block;
    v->gamma_act = v->x_true + (size_t)B * 10;
    v->w = v->gamma_act + B;
    v->ring = v->w + (size_t)B * 3;
    v->scratch = v->ring + (size_t)B * 4 * o->d;
    if (int rc = sdfnmpc_vehicle_reset(v)) {
        sdfnmpc_vehicle_destroy(v);
        return rc;
    }
    *out = v;
    return SDFNMPC_OK;
}

extern "C" void sdfnmpc_vehicle_destroy(sdfnmpc_vehicle* v) {
    if (!v) return;
    ScopedDevice sd(v->device);  // the context may be gone already: hipFree waits for the device
    if (v->block) (void)hipFree(v->block);
    if (v->body_block) (void)hipFree(v->body_block);
    delete v;
}

// the body half of a VehicleBodyArgs block around a vehicle block (the logs are the caller's)
static VehicleBodyArgs vehicle_body_block(const sdfnmpc_vehicle* v, const VehicleArgs& va) {
    const sdfnmpc_body_opts& o = v->bo;
    VehicleBodyArgs a{};
    a.V = va;
    a.m = o.mass; a.im = 1.0 / o.mass;
    for (int i = 0; i < 3; ++i) { a.J[i] = o.inertia[i]; a.iJ[i] = 1.0 / o.inertia[i]; a.k_rate[i] = o.k_rate[i]; }
    for (int i = 0; i < 12; ++i) { a.Gf[i] = o.Gf[i]; a.Gt[i] = o.Gt[i]; }
    for (int i = 0; i < 16; ++i) a.M[i] = o.mixer[i];
    a.s_min = o.wp_idle * o.wp_idle; a.s_max = o.wp_max * o.wp_max;
    a.katt = 2.0 / o.tau_att;
    a.itau_mot = o.tau_mot > 0.0 ? 1.0 / o.tau_mot : 0.0;
    for (int i = 0; i < 4; ++i)  // sqrt(mixer [m g; 0; 0; 0]), clipped as every commanded speed is
        a.hover[i] = std::sqrt(std::fmin(std::fmax(o.mixer[i * 4] * (o.mass * v->o.g), a.s_min), a.s_max));
    a.omega = v->body_block;
    a.rotor = v->body_block ? v->body_block + (size_t)v->B * 3 : nullptr;
    return a;
}

extern "C" int sdfnmpc_vehicle_reset(sdfnmpc_vehicle* v) {
    if (!v) return fail(SDFNMPC_E_ARG, "NULL vehicle");
    const VehicleArgs a = vehicle_block(v, 1.0);
    ScopedDevice sd(v->ctx->device);
    HIPCHK(timed(v->ctx, "vehicle_reset", [&] { return launch_vehicle_reset(a, v->ctx->stream); }));
    if (v->body) {
        const VehicleBodyArgs ba = vehicle_body_block(v, a);
        HIPCHK(timed(v->ctx, "vehicle_body_reset", [&] { return launch_vehicle_body_reset(ba, v->ctx->stream); }));
    }
    return SDFNMPC_OK;
}

extern "C" int sdfnmpc_vehicle_set_body(sdfnmpc_vehicle* v, const sdfnmpc_body_opts* o) {
    if (!v) return fail(SDFNMPC_E_ARG, "NULL vehicle");
    if (!o) {  // the plain vehicle again
        v->body = false;
        return SDFNMPC_OK;
    }
    auto pos = [](double a) { return std::isfinite(a) && a > 0.0; };
    if (!pos(o->mass) || !pos(o->inertia[0]) || !pos(o->inertia[1]) || !pos(o->inertia[2]) || !pos(o->wp_max) ||
        !pos(o->tau_att) || !pos(o->k_rate[0]) || !pos(o->k_rate[1]) || !pos(o->k_rate[2]))
        return fail(SDFNMPC_E_ARG, "body opts: mass, inertia, wp_max, tau_att and k_rate must be positive and finite");
    if (!pos(o->wp_idle) || !(o->wp_idle < o->wp_max)) return fail(SDFNMPC_E_ARG, "body opts: wp_idle must lie in (0, wp_max)");
    if (!std::isfinite(o->tau_mot) || o->tau_mot < 0.0) return fail(SDFNMPC_E_ARG, "body opts: tau_mot must be finite and not negative");
    for (int i = 0; i < 16; ++i)
        if (!std::isfinite(o->mixer[i]) || (i < 12 && (!std::isfinite(o->Gf[i]) || !std::isfinite(o->Gt[i]))))
            return fail(SDFNMPC_E_ARG, "body opts: Gf, Gt and mixer must be finite");
    if (v->o.tau_m > 0.0)
        return fail(SDFNMPC_E_ARG, "body: the vehicle has a thrust lag (tau_m > 0); the rotor lag tau_mot replaces it");
    ScopedDevice sd(v->ctx->device);
    if (!v->body_block && v->B > 0) {
        const hipError_t e = hipMalloc((void**)&v->body_block, (size_t)v->B * 7 * sizeof(double));
        if (e != hipSuccess) {
            v->body_block = nullptr;
            return fail(SDFNMPC_E_HIP, std::string("body buffers: ") + hipGetErrorString(e));
        }
    }
    v->bo = *o;
    v->body = true;
    const VehicleBodyArgs ba = vehicle_body_block(v, vehicle_block(v, 1.0));
    HIPCHK(timed(v->ctx, "vehicle_body_reset", [&] { return launch_vehicle_body_reset(ba, v->ctx->stream); }));
    return SDFNMPC_OK;
}

extern "C" int sdfnmpc_vehicle_body_state(sdfnmpc_vehicle* v, double** omega, double** rotor) {
    if (!v) return fail(SDFNMPC_E_ARG, "NULL vehicle");
    if (!v->body) return fail(SDFNMPC_E_ARG, "vehicle_body_state: the vehicle has no body");
    if (omega) *omega = v->body_block;
    if (rotor) *rotor = v->body_block ? v->body_block + (size_t)v->B * 3 : nullptr;
    return SDFNMPC_OK;
}

extern "C" double* sdfnmpc_vehicle_x_true(sdfnmpc_vehicle* v) { return v ? v->x_true : nullptr; }

extern "C" int sdfnmpc_vehicle_begin(sdfnmpc_ctx* ctx, sdfnmpc_vehicle* v, double* x0, int frame) {
    if (!ctx || !v) return fail(SDFNMPC_E_ARG, "NULL argument to sdfnmpc_vehicle_begin");
    if (v->ctx != ctx) return fail(SDFNMPC_E_ARG, "vehicle_begin: the vehicle lives on another context");
    if (frame < 0) return fail(SDFNMPC_E_ARG, "vehicle_begin: frame must be >= 0");
    if (v->B == 0) return SDFNMPC_OK;
    if (!x0) return fail(SDFNMPC_E_ARG, "vehicle_begin: NULL x0");
    ScopedDevice sd(ctx->device);
    if (v->neutral || (!v->o.est_bias && v->o.est_std_p == 0.0 && v->o.est_std_v == 0.0 && v->o.est_std_yaw == 0.0)) {
        HIPCHK(hipMemcpyAsync(v->x_true, x0, (size_t)v->B * 80, hipMemcpyDeviceToDevice, ctx->stream));  // est = identity
        return SDFNMPC_OK;
    }
    VehicleArgs a = vehicle_block(v, 1.0);
    a.x_est = x0;
    a.frame = (unsigned)frame;
    HIPCHK(timed(ctx, "vehicle_begin", [&] { return launch_vehicle_begin(a, ctx->stream); }));
    return SDFNMPC_OK;
}

int sdfn::vehicle_info(const sdfnmpc_vehicle* v, const sdfnmpc_ctx* ctx, int B, int* neutral, double** x_true,
                       double** scratch) {
    if (!v) return fail(SDFNMPC_E_ARG, "NULL vehicle");
    if (v->ctx != ctx) return fail(SDFNMPC_E_ARG, "vehicle: it lives on another context");
    if (v->B != B) return fail(SDFNMPC_E_ARG, "vehicle: built for " + std::to_string(v->B) + " instances, not " + std::to_string(B));
    if (neutral) *neutral = v->neutral && !v->body ? 1 : 0;
    if (x_true) *x_true = v->x_true;
    if (scratch) *scratch = v->scratch;
    return SDFNMPC_OK;
}

// frame and the log pointers are the caller's
int sdfn::vehicle_args(const sdfnmpc_vehicle* v, const PlantArgs& pa, double* x_est, VehicleArgs& out) {
    if (!v || (v->B > 0 && !x_est)) return fail(SDFNMPC_E_ARG, "vehicle: NULL argument");
    if (x_est == v->x_true) return fail(SDFNMPC_E_ARG, "vehicle: the estimate must not be written into the true state");
    if (v->body) {  // the inner loop's fastest pole against the RK4 step
        const sdfnmpc_body_opts& b = v->bo;
        double rate = std::fmax(std::fmax(b.k_rate[0], b.k_rate[1]), std::fmax(b.k_rate[2], 2.0 / b.tau_att));
        if (b.tau_mot > 0.0) rate = std::fmax(rate, 1.0 / b.tau_mot);
        if (!((pa.dt / pa.substeps) * rate <= 1.0))
            return fail(SDFNMPC_E_ARG, "body: (dt / substeps) max(1 / tau_mot, k_rate, 2 / tau_att) > 1: the inner loop needs more substeps");
    }
    VehicleArgs a = vehicle_block(v, pa.dt);
    a.P = pa;
    a.P.x = a.P.x_next = v->x_true;
    a.x_est = x_est;
    out = a;
    return SDFNMPC_OK;
}

int sdfn::vehicle_launch(sdfnmpc_ctx* ctx, const VehicleArgs& a) {
    ScopedDevice sd(ctx->device);
    HIPCHK(timed(ctx, "plant_vehicle", [&] { return launch_vehicle(a, ctx->stream); }));
    return SDFNMPC_OK;
}

// the rigid body's plant call around a filled vehicle block (vehicle_args plus frame and logs)
int sdfn::vehicle_launch_body(sdfnmpc_ctx* ctx, const sdfnmpc_vehicle* v, const VehicleArgs& a, double* omega_log,
                              double* rotor_log) {
    if (!v || !v->body) return fail(SDFNMPC_E_ARG, "vehicle: no body");
    VehicleBodyArgs ba = vehicle_body_block(v, a);
    ba.omega_log = omega_log;
    ba.rotor_log = rotor_log;
    ScopedDevice sd(ctx->device);
    HIPCHK(timed(ctx, "plant_vehicle_body", [&] { return launch_vehicle_body(ba, ctx->stream); }));
    return SDFNMPC_OK;
}

extern "C" int sdfnmpc_plant_step_vehicle(sdfnmpc_ctx* ctx, const sdfnmpc_plant_opts* o, sdfnmpc_vehicle* v, int B,
                                          const double* u, int frame, double* x_est_out) {
    if (!ctx) return fail(SDFNMPC_E_ARG, "NULL context");
    if (int rc = vehicle_info(v, ctx, B, nullptr, nullptr, nullptr)) return rc;
    if (frame < 0 || frame == 2147483647) return fail(SDFNMPC_E_ARG, "plant_step_vehicle: frame must be >= 0 and frame + 1 must not overflow");
    if (B > 0 && !x_est_out) return fail(SDFNMPC_E_ARG, "plant_step_vehicle: NULL x_est_out");
    PlantArgs pa{};
    if (int rc = plant_args(o, B, v->x_true, u, v->x_true, pa)) return rc;
    if (B == 0) return SDFNMPC_OK;
    if (v->neutral && !v->body) {  // the plant's own kernel, and the estimate a copy of the truth
        if (int rc = plant_launch(ctx, pa)) return rc;
        ScopedDevice sd(ctx->device);
        HIPCHK(hipMemcpyAsync(x_est_out, v->x_true, (size_t)B * 80, hipMemcpyDeviceToDevice, ctx->stream));
        return SDFNMPC_OK;
    }
    VehicleArgs va{};
    if (int rc = vehicle_args(v, pa, x_est_out, va)) return rc;
    va.frame = (unsigned)frame;
    if (v->body) return vehicle_launch_body(ctx, v, va, nullptr, nullptr);
    return vehicle_launch(ctx, va);
}

// ------------------------------------------------------------------------------------------------
// shooting grid: numpy.linspace(start, stop, num) = i * ((stop - start) / (num - 1)) + start, last = stop
static void np_linspace(double start, double stop, int num, double* y) {
    if (num == 1) {  // numpy: div = 0 -> y = [start]
        y[0] = start;
        return;
    }
    const double step = (stop - start) / (num - 1);
    for (int i = 0; i < num; ++i) {
        volatile double t = (double)i * step;  // two roundings as numpy, no FMA contraction
        y[i] = t + start;
    }
    if (num > 1) y[num - 1] = stop;
}

extern "C" int sdfnmpc_shooting_grid(int N, double T, int uniform, int n_short, double dt_short, double* nodes,
                                     double* dt) {
    if (N < 1 || !nodes || !dt) return fail(SDFNMPC_E_ARG, "bad grid arguments");
    if (uniform) {
        np_linspace(0.0, T, N + 1, nodes);
    } else {
        if (n_short < 1 || n_short > N) return fail(SDFNMPC_E_ARG, "nb_short_nodes out of range");
        np_linspace(0.0, dt_short * (n_short - 1), n_short, nodes);
        np_linspace(dt_short * n_short, T, N - n_short + 1, nodes + n_short);
    }
    for (int k = 0; k < N; ++k) dt[k] = nodes[k + 1] - nodes[k];
    return SDFNMPC_OK;
}

// ------------------------------------------------------------------------------------------------
// in-loop VAE encoder: .vaew blob -> device weights + activation workspace

static const int kVaeBlockIn[4] = {64, 128, 256, 512};
static const int kVaeBlockStride[4] = {2, 2, 2, 1};

extern "C" int sdfnmpc_vae_load(sdfnmpc_ctx* ctx, const void* blob, size_t bytes, sdfnmpc_vae** out) {
    if (!ctx || !blob || !out) return fail(SDFNMPC_E_ARG, "NULL argument to sdfnmpc_vae_load");
    *out = nullptr;
    struct Hdr {
        char magic[8];
        uint32_t version, nb_chan, L, H, W, n_convs, n_floats, reserved;
    } h;
    if (bytes < sizeof(Hdr)) return fail(SDFNMPC_E_FORMAT, "vaew: truncated header");
    memcpy(&h, blob, sizeof(Hdr));
    if (memcmp(h.magic, "SDFNVAEW", 8) != 0 || h.version != 1) return fail(SDFNMPC_E_FORMAT, "not a version-1 .vaew blob");
    if (h.nb_chan != 1 || h.n_convs != 13 || h.L < 1 || h.L > 4096 || h.H < 8 || h.W < 8 || h.H > 8192 || h.W > 8192)
        return fail(SDFNMPC_E_UNSUPPORTED, "vaew: only the 1-channel reference encoder (13 convolutions) is built");
    if (bytes != sizeof(Hdr) + 4ull * h.n_floats) return fail(SDFNMPC_E_FORMAT, "vaew: size mismatch");
    const float* src = (const float*)((const char*)blob + sizeof(Hdr));
    auto* v = new sdfnmpc_vae();
    v->device = ctx->device;
    v->ctx = ctx;
    v->L = (int)h.L; v->H = (int)h.H; v->W = (int)h.W;
    v->Hc = (v->H - 1) / 2 + 1; v->Wc = (v->W - 1) / 2 + 1;
    v->Hp = (v->Hc - 1) / 2 + 1; v->Wp = (v->Wc - 1) / 2 + 1;
    // expected layer list (vae.py:device_layers) and host re-layout of stem / head
    struct Spec { int cin, cout, ks, stride; };
    std::vector<Spec> specs = {{1, 64, 7, 2}};
    int hh = v->Hp, ww = v->Wp;
    for (int k = 0; k < 4; ++k) {
        const int ci = kVaeBlockIn[k], s = kVaeBlockStride[k], co = ci * s;
        specs.push_back({ci, co, 3, s});
        if (s != 1) specs.push_back({ci, co, 1, s});
        specs.push_back({co, co, 3, 1});
        hh = (hh - 1) / s + 1;
        ww = (ww - 1) / s + 1;
        v->bh[k] = hh;
        v->bw[k] = ww;
    }
    specs.push_back({2048, (int)h.L, 1, 1});
    size_t need = 0;
    for (auto& s : specs) need += (size_t)s.cout * s.ks * s.ks * s.cin + s.cout;
    if (need != h.n_floats) {
        delete v;
        return fail(SDFNMPC_E_FORMAT, "vaew: parameter count does not match the reference encoder");
    }
    // + the stem weights split exactly into three bf16 planes [3][64 n][64 k] (vae_enc.hip's split3), in
    // the kernel's K order (vae_stem_slot_tap), appended after the layers (16-byte aligned), then every
    // ResBlock convolution's weights split the same way into planes of K-tile slabs (16-byte aligned each)
    auto split3 = [](float x, unsigned short* hi, unsigned short* mid, unsigned short* lo) {
        uint32_t u, hb, mb, lb;
        memcpy(&u, &x, 4);
        hb = u & 0xffff0000u;
        float hf, r1, mf, r2;
        memcpy(&hf, &hb, 4);
        r1 = x - hf;  // exact (the leading 8 significant bits removed)
        memcpy(&u, &r1, 4);
        mb = u & 0xffff0000u;
        memcpy(&mf, &mb, 4);
        r2 = r1 - mf;
        memcpy(&u, &r2, 4);
        lb = u & 0xffff0000u;
        *hi = (unsigned short)(hb >> 16);
        *mid = (unsigned short)(mb >> 16);
        *lo = (unsigned short)(lb >> 16);
    };
    const size_t wpl_off = (need + 3) & ~(size_t)3;
    size_t cpl_end = wpl_off + 3 * VAE_STEM_PLANE / 2;  // in floats
    std::vector<size_t> cpl_off(specs.size(), 0);
    for (size_t li = 1; li + 1 < specs.size(); ++li) {
        cpl_off[li] = cpl_end;
        const size_t nw = (size_t)specs[li].cout * specs[li].ks * specs[li].ks * specs[li].cin;
        cpl_end += ((3 * nw + 1) / 2 + 3) & ~(size_t)3;
    }
    const size_t zero_off = cpl_end;  // + 16 zero floats: what a convolution tap outside the map reads
    std::vector<float> dev(cpl_end + 16, 0.0f);
    size_t off = 0;
    for (size_t li = 0; li < specs.size(); ++li) {
        const Spec& s = specs[li];
        const size_t nw = (size_t)s.cout * s.ks * s.ks * s.cin;
        if (li == 0) {  // stem [64][7][7][1] -> tap-major [49][64], and the split planes
            unsigned short* wpl = (unsigned short*)&dev[wpl_off];
            for (int c = 0; c < 64; ++c)
                for (int t = 0; t < 49; ++t) dev[off + t * 64 + c] = src[off + c * 49 + t];
            for (int c = 0; c < 64; ++c)
                for (int k = 0; k < 49; ++k)
                    split3(src[off + c * 49 + vae_stem_slot_tap(k)], &wpl[0 * VAE_STEM_PLANE + c * 64 + k],
                           &wpl[1 * VAE_STEM_PLANE + c * 64 + k], &wpl[2 * VAE_STEM_PLANE + c * 64 + k]);
        } else if (li + 1 == specs.size()) {  // head [L][2048] -> [2048][L]
            for (int o = 0; o < s.cout; ++o)
                for (int f = 0; f < 2048; ++f) dev[off + (size_t)f * s.cout + o] = src[off + (size_t)o * 2048 + f];
        } else {
            memcpy(&dev[off], src + off, nw * 4);
            unsigned short* pl = (unsigned short*)&dev[cpl_off[li]];
            // K-tile slabs in vae_conv_kernel's K order (channel block, ky, kx): weight (n, ky, kx, ci) goes
            // to K-tile t = (ci / 16) KS KS + ky KS + kx, plane element ((n / 128 KT + t) 128 + n % 128) 16
            // + ci % 16 with the two 8-element halves of rows with bit 3 set swapped -- the LDS image of the
            // kernel's B tile, so its LDS-DMA reads 1 KB contiguous per wave (one slab: 4 KB per plane)
            const int KK = s.ks * s.ks, K = KK * s.cin, KT = K / 16;
            for (int n = 0; n < s.cout; ++n)
                for (int k = 0; k < K; ++k) {
                    const int tp = k / s.cin, ci = k % s.cin, t = (ci / 16) * KK + tp, c = ci % 16;
                    const int r = n % 128, h = (c / 8) ^ ((r >> 3) & 1);
                    const size_t e = (((size_t)(n / 128) * KT + t) * 128 + r) * 16 + 8 * h + c % 8;
                    split3(src[off + (size_t)n * K + k], &pl[e], &pl[nw + e], &pl[2 * nw + e]);
                }
        }
        memcpy(&dev[off + nw], src + off + nw, (size_t)s.cout * 4);
        off += nw + s.cout;
    }
    ScopedDevice sd(ctx->device);
    if (hipMalloc(&v->dmem, dev.size() * 4) != hipSuccess ||
        hipMemcpy(v->dmem, dev.data(), dev.size() * 4, hipMemcpyHostToDevice) != hipSuccess) {
        if (v->dmem) (void)hipFree(v->dmem);
        delete v;
        return fail(SDFNMPC_E_HIP, "vaew: device upload failed");
    }
    const float* d = (const float*)v->dmem;
    v->stem_wpl = (const unsigned short*)(d + wpl_off);
    v->zero16 = d + zero_off;
    off = 0;
    for (size_t li = 0; li < specs.size(); ++li) {
        const Spec& s = specs[li];
        VaeLayer L{d + off, d + off + (size_t)s.cout * s.ks * s.ks * s.cin,
                   cpl_off[li] ? (const unsigned short*)(d + cpl_off[li]) : nullptr, s.cin, s.cout, s.ks, s.stride};
        if (li == 0) v->stem = L;
        else if (li + 1 == specs.size()) v->head = L;
        else v->conv[li - 1] = L;
        off += (size_t)s.cout * s.ks * s.ks * s.cin + s.cout;
    }
    *out = v;
    return SDFNMPC_OK;
}

extern "C" void sdfnmpc_vae_free(sdfnmpc_vae* v) {
    if (!v) return;
    ScopedDevice sd(v->device);
    if (v->dmem) (void)hipFree(v->dmem);
    delete v;
}

extern "C" int sdfnmpc_vae_size_latent(const sdfnmpc_vae* v) { return v ? v->L : -1; }

extern "C" int sdfnmpc_vae_encode(sdfnmpc_ctx* ctx, sdfnmpc_vae* v, const sdfnmpc_vae_opts* o, const void* img,
                                  float* latent, double* latent64) {
    if (!ctx || !v || !o) return fail(SDFNMPC_E_ARG, "NULL argument to sdfnmpc_vae_encode");
    if (o->B < 0 || (o->B > 0 && (!img || !latent))) return fail(SDFNMPC_E_ARG, "vae_encode: bad B or NULL image / latent");
    if (o->dtype != 0 && o->dtype != 1) return fail(SDFNMPC_E_ARG, "vae_encode: dtype must be 0 (float32) or 1 (uint16)");
    if (o->in_h < 1 || o->in_w < 1 || !(o->clip > 0.f)) return fail(SDFNMPC_E_ARG, "vae_encode: bad image size or clip");
    if (ctx->device != v->device) return fail(SDFNMPC_E_ARG, "vae_encode: encoder loaded on another device");
    const int B = o->B;
    if (B == 0) return SDFNMPC_OK;
    ScopedDevice sd(ctx->device);
    // workspace: pre [B][H][W] | X | Y (block in/out ping-pong, bf16 planes) | T (conv_a, planes) | S (shortcut,
    // fp32) | F (head features).  A planes tensor of n values per image: [3][B][n] bf16, plane stride B n.
    const size_t n_pre = (size_t)v->H * v->W;
    size_t n_x = (size_t)v->Hp * v->Wp * 64, n_t = 0;
    for (int k = 0; k < 4; ++k) {
        const size_t nb = (size_t)v->bh[k] * v->bw[k] * kVaeBlockIn[k] * kVaeBlockStride[k];
        n_x = std::max(n_x, nb);
        n_t = std::max(n_t, nb);
    }
    // in floats per image: planes take 1.5 floats a value (n_x, n_t are multiples of 64: every plane 16-byte
    // aligned once X is); the preprocessed images [B][H][W] are padded to a multiple of 64 floats, so X (and every
    // plane after it, staged by 16-byte LDS-DMA) starts 256-byte aligned for any H, W, B
    const size_t pre_pad = (n_pre * B + 63) & ~(size_t)63;
    const size_t per = n_pre + 2 * (3 * n_x / 2) + 3 * n_t / 2 + n_t + 2048;
    HIPCHK(v->ws.ensure((per * B + 64) * sizeof(float)));
    float* P = (float*)v->ws.p;
    unsigned short* X = (unsigned short*)(P + pre_pad);
    unsigned short* Y = X + 3 * n_x * B;
    unsigned short* T = Y + 3 * n_x * B;
    float* S = (float*)(T + 3 * n_t * B);
    float* F = S + n_t * B;  // [B][2048] pooled head features
    const unsigned short* zero = (const unsigned short*)v->zero16;
    hipStream_t st = ctx->stream;
    VaePreArgs pa{img, o->dtype, B, o->in_h, o->in_w, v->H, v->W, o->clip, o->yz, P};
    HIPCHK(timed(ctx, "vae_pre", [&] { return launch_vae_pre(pa, st); }));
    size_t xps = (size_t)B * v->Hp * v->Wp * 64;  // the plane stride of the tensor in X
    // a map read by a stride-2 convolution is stored in parity-phase column order (vae_col)
    auto phased = [](int k) { return k < 4 && kVaeBlockStride[k] == 2 ? 1 : 0; };
    VaeStemArgs sa{P, v->stem_wpl, v->stem.b, X, xps, B, v->H, v->W, v->Hc, v->Wc, v->Hp, v->Wp, phased(0)};
    HIPCHK(timed(ctx, "vae_stem", [&] { return launch_vae_stem(sa, ctx->n_cu, st); }));
    int h = v->Hp, w = v->Wp, li = 0;
    for (int k = 0; k < 4; ++k) {
        const int s = kVaeBlockStride[k], ho = v->bh[k], wo = v->bw[k];
        const VaeLayer& ca = v->conv[li++];
        const size_t ops = (size_t)B * ho * wo * ca.cout;  // plane stride of this block's outputs
        const int in_ph = phased(k), out_ph = phased(k + 1);
        VaeConvArgs a1{X, xps, ca.w, ca.wpl, ca.b, zero, nullptr, nullptr, 0, nullptr, T, ops,
                       B, h, w, ca.cin, ho, wo, ca.cout, 1, in_ph, 0, 0};
        HIPCHK(timed(ctx, "vae_conv", [&] { return launch_vae_conv(a1, 3, s, st); }));
        const float* resid = nullptr;
        const unsigned short* resid_pl = X;  // identity shortcut: the block input, as planes
        int res_ph = in_ph;
        if (s != 1) {
            const VaeLayer& cs = v->conv[li++];
            VaeConvArgs a2{X, xps, cs.w, cs.wpl, cs.b, zero, nullptr, nullptr, 0, S, nullptr, 0,
                           B, h, w, cs.cin, ho, wo, cs.cout, 0, in_ph, out_ph, 0};
            HIPCHK(timed(ctx, "vae_conv", [&] { return launch_vae_conv(a2, 1, s, st); }));
            resid = S;
            resid_pl = nullptr;
            res_ph = out_ph;
        }
        const VaeLayer& cb = v->conv[li++];
        VaeConvArgs a3{T, ops, cb.w, cb.wpl, cb.b, zero, resid, resid_pl, xps, nullptr, Y, ops,
                       B, ho, wo, cb.cin, ho, wo, cb.cout, 1, 0, out_ph, res_ph};
        HIPCHK(timed(ctx, "vae_conv", [&] { return launch_vae_conv(a3, 3, 1, st); }));
        std::swap(X, Y);
        xps = ops;
        h = ho;
        w = wo;
    }
    VaeHeadArgs ha{X, xps, F, v->head.w, v->head.b, latent, latent64, B, h, w, v->L};
    HIPCHK(timed(ctx, "vae_head", [&] { return launch_vae_head(ha, st); }));
    return SDFNMPC_OK;
}

// ------------------------------------------------------------------------------------------------
// VAE decoder (vae_dec.hip): .vaed blob -> device weights + activation workspace

static const int kDecH0 = 8, kDecW0 = 15, kDecC0 = 512, kDecF = 512 * 8 * 15;
static const int kDecChunk = 64;  // images decoded per pass: bounds the workspace (about 22 MB an image)

extern "C" int sdfnmpc_vae_dec_load(sdfnmpc_ctx* ctx, const void* blob, size_t bytes, sdfnmpc_vae_dec** out) {
    if (!ctx || !blob || !out) return fail(SDFNMPC_E_ARG, "NULL argument to sdfnmpc_vae_dec_load");
    *out = nullptr;
    struct Hdr {
        char magic[8];
        uint32_t version, L, batchnorm, n_floats;
    } h;
    if (bytes < sizeof(Hdr)) return fail(SDFNMPC_E_FORMAT, "vaed: truncated header");
    memcpy(&h, blob, sizeof(Hdr));
    if (memcmp(h.magic, "SDFNVAED", 8) != 0 || h.version != 1) return fail(SDFNMPC_E_FORMAT, "not a version-1 .vaed blob");
    if (h.L < 1 || h.L > (uint32_t)VAE_DEC_LMAX) return fail(SDFNMPC_E_UNSUPPORTED, "vaed: size_latent outside [1, 1024]");
    if (bytes != sizeof(Hdr) + 4ull * h.n_floats) return fail(SDFNMPC_E_FORMAT, "vaed: size mismatch");
    size_t need = (size_t)h.L * kDecF + kDecF + 25 * 32 + 1;
    for (int k = 0; k < 4; ++k) {
        const size_t ci = kDecC0 >> k, co = ci / 2;
        need += 9 * ci * co + co + ci * co + co + 9 * co * co + co;
    }
    if (need != h.n_floats) return fail(SDFNMPC_E_FORMAT, "vaed: parameter count does not match the reference decoder");
    const float* src = (const float*)((const char*)blob + sizeof(Hdr));
    auto split3 = [](float x, unsigned short* hi, unsigned short* mid, unsigned short* lo) {
        uint32_t u, hb, mb, lb;
        memcpy(&u, &x, 4);
        hb = u & 0xffff0000u;
        float hf, r1, mf, r2;
        memcpy(&hf, &hb, 4);
        r1 = x - hf;  // exact (the leading 8 significant bits removed)
        memcpy(&u, &r1, 4);
        mb = u & 0xffff0000u;
        memcpy(&mf, &mb, 4);
        r2 = r1 - mf;
        memcpy(&u, &r2, 4);
        lb = u & 0xffff0000u;
        *hi = (unsigned short)(hb >> 16);
        *mid = (unsigned short)(mb >> 16);
        *lo = (unsigned short)(lb >> 16);
    };
    auto* d = new sdfnmpc_vae_dec();
    d->device = ctx->device;
    d->ctx = ctx;
    d->L = (int)h.L;
    std::vector<float> dev;
    auto put = [&](const float* p, size_t n) {  // 16-byte aligned sections
        const size_t o = dev.size();
        dev.insert(dev.end(), p, p + n);
        dev.resize((dev.size() + 3) & ~(size_t)3, 0.0f);
        return o;
    };
    // one GEMM operand: w [KS][KS][cin][cout] (the transposed convolution's own tap indices), split into three
    // bf16 planes of K-tile rows [phase][tap cin / 16][cout][16]
    struct Tap { int ky, kx, dy, dx; };
    auto put_op = [&](VaeDecOp& op, const float* w, const float* b, int ks, int cin, int cout,
                      const std::vector<std::vector<Tap>>& phases, const int (*pyx)[2]) {
        op.cin = cin;
        op.cout = cout;
        op.nphase = (int)phases.size();
        size_t total = 0;
        for (int p = 0; p < op.nphase; ++p) {
            op.woff[p] = (unsigned)total;
            op.ntaps[p] = (int)phases[p].size();
            op.py[p] = pyx[p][0];
            op.px[p] = pyx[p][1];
            total += phases[p].size() * (size_t)cin * cout;
        }
        op.wps = total;
        op.b_off = put(b, cout);
        op.wpl_off = dev.size();
        dev.resize(dev.size() + (((3 * total + 1) / 2 + 3) & ~(size_t)3), 0.0f);
        unsigned short* pl = (unsigned short*)&dev[op.wpl_off];
        for (int p = 0; p < op.nphase; ++p)
            for (size_t t = 0; t < phases[p].size(); ++t) {
                const Tap& tp = phases[p][t];
                op.dy[p][t] = (signed char)tp.dy;
                op.dx[p][t] = (signed char)tp.dx;
                const float* wt = w + (size_t)(tp.ky * ks + tp.kx) * cin * cout;
                for (int ci = 0; ci < cin; ++ci)
                    for (int n = 0; n < cout; ++n) {
                        const size_t e = op.woff[p] + (((t * (cin / 16) + ci / 16) * (size_t)cout) + n) * 16 + ci % 16;
                        split3(wt[(size_t)ci * cout + n], &pl[e], &pl[total + e], &pl[2 * total + e]);
                    }
            }
    };
    size_t off = 0;
    const size_t head_w = put(src + off, (size_t)h.L * kDecF);
    off += (size_t)h.L * kDecF;
    const size_t head_b = put(src + off, kDecF);
    off += kDecF;
    // ConvTranspose2d(k3, s2, p1, op1): output row 2 i + 1 - 1 + ky ... o = 2 i - 1 + ky, so an even output row takes
    // ky = 1 from input row i and an odd one ky = 0 from row i + 1 and ky = 2 from row i; columns alike
    static const int pyx4[4][2] = {{0, 0}, {0, 1}, {1, 0}, {1, 1}}, pyx1[1][2] = {{0, 0}};
    std::vector<std::vector<Tap>> up_ph(4), cv_ph(1), sc_ph(1);
    for (int p = 0; p < 4; ++p) {
        const int py = pyx4[p][0], px = pyx4[p][1];
        const int ry[2][2] = {{py ? 0 : 1, py ? 1 : 0}, {2, 0}}, rx[2][2] = {{px ? 0 : 1, px ? 1 : 0}, {2, 0}};
        for (int a = 0; a < (py ? 2 : 1); ++a)
            for (int b = 0; b < (px ? 2 : 1); ++b) up_ph[p].push_back({ry[a][0], rx[b][0], ry[a][1], rx[b][1]});
    }
    // ConvTranspose2d(k3, s1, p1): o = i - 1 + ky, so tap ky reads input row o + 1 - ky
    for (int ky = 0; ky < 3; ++ky)
        for (int kx = 0; kx < 3; ++kx) cv_ph[0].push_back({ky, kx, 1 - ky, 1 - kx});
    sc_ph[0].push_back({0, 0, 0, 0});
    for (int k = 0; k < 4; ++k) {
        const int ci = kDecC0 >> k, co = ci / 2;
        put_op(d->up[k], src + off, src + off + (size_t)9 * ci * co, 3, ci, co, up_ph, pyx4);
        off += (size_t)9 * ci * co + co;
        put_op(d->sc[k], src + off, src + off + (size_t)ci * co, 1, ci, co, sc_ph, pyx1);
        off += (size_t)ci * co + co;
        put_op(d->cv[k], src + off, src + off + (size_t)9 * co * co, 3, co, co, cv_ph, pyx1);
        off += (size_t)9 * co * co + co;
    }
    const size_t tail_w = put(src + off, 25 * 32);
    off += 25 * 32;
    const size_t tail_b = put(src + off, 1);
    ScopedDevice sd(ctx->device);
    if (hipMalloc(&d->dmem, dev.size() * 4) != hipSuccess ||
        hipMemcpy(d->dmem, dev.data(), dev.size() * 4, hipMemcpyHostToDevice) != hipSuccess) {
        if (d->dmem) (void)hipFree(d->dmem);
        delete d;
        return fail(SDFNMPC_E_HIP, "vaed: device upload failed");
    }
    const float* base = (const float*)d->dmem;
    d->head_w = base + head_w;
    d->head_b = base + head_b;
    d->tail_w = base + tail_w;
    d->tail_b = base + tail_b;
    for (int k = 0; k < 4; ++k)
        for (VaeDecOp* op : {&d->up[k], &d->sc[k], &d->cv[k]}) {
            op->wpl = (const unsigned short*)(base + op->wpl_off);
            op->b = base + op->b_off;
        }
    *out = d;
    return SDFNMPC_OK;
}

extern "C" void sdfnmpc_vae_dec_free(sdfnmpc_vae_dec* d) {
    if (!d) return;
    ScopedDevice sd(d->device);
    if (d->dmem) (void)hipFree(d->dmem);
    delete d;
}

extern "C" int sdfnmpc_vae_dec_size_latent(const sdfnmpc_vae_dec* d) { return d ? d->L : -1; }

extern "C" int sdfnmpc_vae_decode(sdfnmpc_ctx* ctx, sdfnmpc_vae_dec* d, int B, const float* latent, int out_h, int out_w,
                                  float* img, float* logits) {
    if (!ctx || !d) return fail(SDFNMPC_E_ARG, "NULL argument to sdfnmpc_vae_decode");
    if (B < 0 || out_h < 1 || out_w < 1) return fail(SDFNMPC_E_ARG, "vae_decode: B < 0 or an output size < 1");
    if (B > 0 && (!latent || !img)) return fail(SDFNMPC_E_ARG, "vae_decode: NULL latent or image");
    // the activation workspace belongs to the decoder object: calls through it are ordered on one stream only
    if (d->ctx != ctx) return fail(SDFNMPC_E_ARG, "vae_decode: decoder loaded on another context");
    if (B == 0) return SDFNMPC_OK;
    ScopedDevice sd(ctx->device);
    const int Hl = kDecH0 * 16, Wl = kDecW0 * 16;            // the logits' map, 128 x 240
    const size_t n_max = (size_t)Hl * Wl * 32;               // values per image of the largest map
    const int ch = std::min(B, kDecChunk);
    // workspace: three plane tensors P0..P2 (block input, conv_a output, shortcut / block output, rotating), the
    // last block's output in fp32 for the tail, and the logits when the caller does not want them
    const size_t pl_bytes = 3 * n_max * ch * sizeof(unsigned short);
    HIPCHK(d->ws.ensure(3 * pl_bytes + (n_max + (size_t)Hl * Wl) * ch * sizeof(float)));
    unsigned short* P[3];
    for (int i = 0; i < 3; ++i) P[i] = (unsigned short*)((char*)d->ws.p + i * pl_bytes);
    float* F32 = (float*)((char*)d->ws.p + 3 * pl_bytes);
    float* LG = F32 + n_max * ch;
    hipStream_t st = ctx->stream;
    static const char* const kUp[4] = {"vae_dec_up256", "vae_dec_up128", "vae_dec_up64", "vae_dec_up32"};
    static const char* const kSc[4] = {"vae_dec_sc256", "vae_dec_sc128", "vae_dec_sc64", "vae_dec_sc32"};
    static const char* const kCv[4] = {"vae_dec_conv256", "vae_dec_conv128", "vae_dec_conv64", "vae_dec_conv32"};
    auto gemm = [&](const char* name, const VaeDecOp& op, int nb, const unsigned short* in, int hi, int wi, int hm, int wm,
                    int ho, int wo, int os, int relu, int fill3, const unsigned short* resid, unsigned short* outp,
                    float* out32) {
        VaeDecGemmArgs a{};
        a.in = in;
        a.ips = (size_t)nb * hi * wi * op.cin;
        a.wpl = op.wpl;
        a.wps = op.wps;
        a.b = op.b;
        a.resid = resid;
        a.rps = a.ops = (size_t)nb * ho * wo * op.cout;
        a.out = outp;
        a.out_f32 = out32;
        a.B = nb; a.Hi = hi; a.Wi = wi; a.Cin = op.cin; a.Hm = hm; a.Wm = wm; a.Ho = ho; a.Wo = wo; a.Cout = op.cout;
        a.os = os; a.relu = relu; a.fill3 = fill3; a.nphase = op.nphase;
        memcpy(a.ntaps, op.ntaps, sizeof a.ntaps);
        memcpy(a.py, op.py, sizeof a.py);
        memcpy(a.px, op.px, sizeof a.px);
        memcpy(a.woff, op.woff, sizeof a.woff);
        memcpy(a.dy, op.dy, sizeof a.dy);
        memcpy(a.dx, op.dx, sizeof a.dx);
        return timed(ctx, name, [&] { return launch_vae_dec_gemm(a, st); });
    };
    for (int b0 = 0; b0 < B; b0 += ch) {
        const int nb = std::min(ch, B - b0);
        unsigned short *X = P[0], *T = P[1], *O = P[2];
        VaeDecHeadArgs ha{latent + (size_t)b0 * d->L, d->head_w, d->head_b, X, (size_t)nb * kDecF, nb, d->L, kDecF, kDecC0};
        HIPCHK(timed(ctx, "vae_dec_head", [&] { return launch_vae_dec_head(ha, st); }));
        int hi = kDecH0, wi = kDecW0;
        for (int k = 0; k < 4; ++k) {
            const int ho = 2 * hi, wo = 2 * wi;
            HIPCHK(gemm(kUp[k], d->up[k], nb, X, hi, wi, hi, wi, ho, wo, 2, 1, 0, nullptr, T, nullptr));
            HIPCHK(gemm(kSc[k], d->sc[k], nb, X, hi, wi, hi, wi, ho, wo, 2, 0, 1, nullptr, O, nullptr));
            // the block's output: in place over the shortcut (a thread reads the residual it then overwrites);
            // the last block's goes out in fp32, for the tail
            HIPCHK(gemm(kCv[k], d->cv[k], nb, T, ho, wo, ho, wo, ho, wo, 1, 1, 0, O, k < 3 ? O : nullptr,
                        k < 3 ? nullptr : F32));
            std::swap(X, O);  // the next block reads O; its conv_a output and shortcut take the other two
            hi = ho;
            wi = wo;
        }
        float* lg = logits ? logits + (size_t)b0 * Hl * Wl : LG;
        VaeDecTailArgs ta{F32, d->tail_w, d->tail_b, lg, nb, Hl, Wl, 32};
        HIPCHK(timed(ctx, "vae_dec_tail", [&] { return launch_vae_dec_tail(ta, st); }));
        VaeDecResizeArgs ra{lg, img + (size_t)b0 * out_h * out_w, nb, Hl, Wl, out_h, out_w};
        HIPCHK(timed(ctx, "vae_dec_resize", [&] { return launch_vae_dec_resize(ra, st); }));
    }
    return SDFNMPC_OK;
}

// ------------------------------------------------------------------------------------------------
// ground truth from range images (df_truth.hip)
static int df_img_args(const char* who, sdfnmpc_ctx* ctx, const sdfnmpc_img_opts* o, const float* img, int n_img, int H,
                       int W, const float* points, const int* p_to_i, long long n, DfImg* im) {
    const std::string w(who);
    if (!ctx || !o) return fail(SDFNMPC_E_ARG, w + ": NULL context or options");
    if (!(o->dmax > 0.f) || !(o->hfov > 0.f) || !(o->vfov > 0.f))
        return fail(SDFNMPC_E_ARG, w + ": dmax, hfov and vfov must be positive");
    if (n_img <= 0 || H < 1 || W < 1) return fail(SDFNMPC_E_ARG, w + ": bad image count or size");
    if (n < 0 || n > 2147483647LL) return fail(SDFNMPC_E_ARG, w + ": n out of range");
    if (!p_to_i && n % n_img != 0)
        return fail(SDFNMPC_E_ARG, w + ": without p_to_i the points must divide evenly among the images");
    if (n > 0 && (!img || !points)) return fail(SDFNMPC_E_ARG, w + ": NULL image or points");
    *im = DfImg{img, n_img, H, W, o->dmax, o->hfov, o->vfov, o->is_depth != 0, o->is_spherical != 0,
                points, p_to_i, n, std::max(1LL, n / n_img)};
    return SDFNMPC_OK;
}

extern "C" int sdfnmpc_colcheck(sdfnmpc_ctx* ctx, const sdfnmpc_img_opts* o, int outside, float safe_ball,
                                const float* img, int n_img, int H, int W, const float* points, const int* p_to_i,
                                long long n, unsigned char* out) {
    ColcheckArgs a{};
    if (int rc = df_img_args("colcheck", ctx, o, img, n_img, H, W, points, p_to_i, n, &a.im)) return rc;
    if (outside < 0 || outside > 2) return fail(SDFNMPC_E_ARG, "colcheck: outside must be 0 (free), 1 (col) or 2 (extrapolate)");
    if (n == 0) return SDFNMPC_OK;
    if (!out) return fail(SDFNMPC_E_ARG, "colcheck: NULL output");
    a.outside = outside;
    a.safe_ball = safe_ball;
    a.out = out;
    ScopedDevice sd(ctx->device);
    HIPCHK(timed(ctx, "colcheck", [&] { return launch_colcheck(a, ctx->stream); }));
    return SDFNMPC_OK;
}

extern "C" int sdfnmpc_udf(sdfnmpc_ctx* ctx, const sdfnmpc_img_opts* o, float max_df, const float* img, int n_img,
                           int H, int W, const float* points, const int* p_to_i, long long n, float* udf, float* grad,
                           int* pix_idx) {
    UdfArgs a{};
    if (int rc = df_img_args("udf", ctx, o, img, n_img, H, W, points, p_to_i, n, &a.im)) return rc;
    if (H % 5 != 0 || W % 5 != 0) return fail(SDFNMPC_E_ARG, "udf: H and W must be multiples of 5 (the min-pool kernel)");
    if (udf_lds_bytes(H / 5, W / 5) > UDF_LDS_MAX) return fail(SDFNMPC_E_ARG, "udf: image too large");
    if (n == 0) return SDFNMPC_OK;
    if (!udf || !grad) return fail(SDFNMPC_E_ARG, "udf: NULL output");
    ScopedDevice sd(ctx->device);
    HIPCHK(ctx->dfpool.ensure((size_t)n_img * (H / 5) * (W / 5) * sizeof(float)));
    MinpoolArgs m{img, (float*)ctx->dfpool.p, n_img, H, W, o->dmax};
    HIPCHK(timed(ctx, "minpool5", [&] { return launch_minpool5(m, ctx->stream); }));
    a.im.img = (const float*)ctx->dfpool.p;
    a.im.H = H / 5;
    a.im.W = W / 5;
    a.max_df = max_df;
    a.udf = udf;
    a.grad = grad;
    a.pix_idx = pix_idx;
    HIPCHK(timed(ctx, "udf", [&] { return launch_udf(a, ctx->stream); }));
    return SDFNMPC_OK;
}

extern "C" int sdfnmpc_sdf_truth(sdfnmpc_ctx* ctx, const sdfnmpc_img_opts* o, float min_df, float max_df,
                                 const float* grid, const float* dist, const int* orig_idx, int G, const float* img,
                                 int n_img, int H, int W, const float* points, const int* p_to_i, long long n,
                                 float* sdf, float* grad, int* vox_idx) {
    SdfGridArgs a{};
    if (int rc = df_img_args("sdf_truth", ctx, o, img, n_img, H, W, points, p_to_i, n, &a.im)) return rc;
    if (G < 0 || (G > 0 && (!grid || !dist))) return fail(SDFNMPC_E_ARG, "sdf_truth: bad grid");
    if (!(min_df < max_df)) return fail(SDFNMPC_E_ARG, "sdf_truth: min_df must be below max_df");
    if (n == 0) return SDFNMPC_OK;
    if (!sdf || !grad) return fail(SDFNMPC_E_ARG, "sdf_truth: NULL output");
    a.min_df = min_df;
    a.max_df = max_df;
    a.grid = grid;
    a.dist = dist;
    a.orig_idx = orig_idx;
    a.G = G;
    a.sdf = sdf;
    a.grad = grad;
    a.vox_idx = vox_idx;
    ScopedDevice sd(ctx->device);
    HIPCHK(timed(ctx, "sdf_grid", [&] { return launch_sdf_grid(a, ctx->stream); }));
    return SDFNMPC_OK;
}

// the image's own field as the SDF row (df_truth.hip: img_sdf_rows_kernel): the option check and the argument block,
// split from the launch for the preparation phase (lin_args.sdf_image) and the solver.  Nothing is launched.
int sdfn::img_sdf_args(sdfnmpc_ctx* ctx, const sdfnmpc_img_sdf_opts* o, int B, int N, int np, const double* x,
                       const double* p, double* h, double* Jh, float* pts, ImgSdfArgs& out) {
    if (!ctx || !o) return fail(SDFNMPC_E_ARG, "img_sdf_rows: NULL context or options");
    if (B < 0 || N < 1 || np < 17) return fail(SDFNMPC_E_ARG, "img_sdf_rows: B >= 0, N >= 1 and np >= 17 required");
    if (!(o->img.dmax > 0.f) || !(o->img.hfov > 0.f) || !(o->img.vfov > 0.f))
        return fail(SDFNMPC_E_ARG, "img_sdf_rows: dmax, hfov and vfov must be positive");
    if (o->H < 1 || o->W < 1 || (long long)o->H * o->W > 2147483647LL)
        return fail(SDFNMPC_E_ARG, "img_sdf_rows: bad image size");
    if (!(o->max_df > 0.f) || !std::isfinite(o->max_df))
        return fail(SDFNMPC_E_ARG, "img_sdf_rows: max_df must be positive and finite");
    if (!(o->min_df < o->max_df)) return fail(SDFNMPC_E_ARG, "img_sdf_rows: min_df must be below max_df");
    if (!o->images) return fail(SDFNMPC_E_ARG, "img_sdf_rows: NULL images");
    if (o->is_signed) {
        if (!o->grid || !o->dist || o->G < 1) return fail(SDFNMPC_E_ARG, "img_sdf_rows: the signed field needs its voxel grid");
    } else {
        if (o->H % 5 != 0 || o->W % 5 != 0)
            return fail(SDFNMPC_E_ARG, "img_sdf_rows: H and W must be multiples of 5 (the min-pool kernel)");
        if (udf_lds_bytes(o->H / 5, o->W / 5) > UDF_LDS_MAX) return fail(SDFNMPC_E_ARG, "img_sdf_rows: image too large");
        if (!o->pooled) return fail(SDFNMPC_E_ARG, "img_sdf_rows: the unsigned field needs the pooled images");
    }
    if ((long long)B * (N + 1) > 2147483647LL) return fail(SDFNMPC_E_ARG, "img_sdf_rows: too many rows");
    if (B > 0 && (!x || !p || !h || !Jh)) return fail(SDFNMPC_E_ARG, "img_sdf_rows: NULL x, p, h or Jh");
    ImgSdfArgs a{};
    a.images = o->images; a.pooled = o->pooled; a.img_of = o->img_of; a.H = o->H; a.W = o->W;
    a.dmax = o->img.dmax; a.hfov = o->img.hfov; a.vfov = o->img.vfov;
    a.is_depth = o->img.is_depth != 0; a.is_spherical = o->img.is_spherical != 0;
    a.is_signed = o->is_signed != 0; a.min_df = o->min_df; a.max_df = o->max_df;
    a.grid = o->grid; a.dist = o->dist; a.orig_idx = o->orig_idx; a.G = o->G;
    a.rows = (long long)B * (N + 1); a.N1 = N + 1; a.np = np;
    a.x = x; a.p = p; a.h = h; a.Jh = Jh; a.pts = pts;
    out = a;
    return SDFNMPC_OK;
}

extern "C" int sdfnmpc_img_sdf_rows(sdfnmpc_ctx* ctx, const sdfnmpc_img_sdf_opts* o, int B, int N, int np,
                                    const double* x, const double* p, double* h, double* Jh, float* pts) {
    ImgSdfArgs a{};
    if (int rc = img_sdf_args(ctx, o, B, N, np, x, p, h, Jh, pts, a)) return rc;
    if (B == 0) return SDFNMPC_OK;
    ScopedDevice sd(ctx->device);
    return img_sdf_launch(ctx, a);
}

// the min-pool of an image source's images into its pooled buffer: what sdfnmpc_udf does in front of its scan
extern "C" int sdfnmpc_img_sdf_pool(sdfnmpc_ctx* ctx, const sdfnmpc_img_sdf_opts* o, int n_img) {
    if (!ctx || !o) return fail(SDFNMPC_E_ARG, "img_sdf_pool: NULL context or options");
    if (n_img < 0 || o->H < 1 || o->W < 1 || o->H % 5 != 0 || o->W % 5 != 0)
        return fail(SDFNMPC_E_ARG, "img_sdf_pool: n_img >= 0 and H, W positive multiples of 5 required");
    if (!(o->img.dmax > 0.f)) return fail(SDFNMPC_E_ARG, "img_sdf_pool: dmax must be positive");
    if ((long long)n_img * o->H * o->W > 2147483647LL) return fail(SDFNMPC_E_ARG, "img_sdf_pool: too many pixels");
    if (n_img == 0) return SDFNMPC_OK;
    if (!o->images || !o->pooled) return fail(SDFNMPC_E_ARG, "img_sdf_pool: NULL images or pooled buffer");
    ScopedDevice sd(ctx->device);
    MinpoolArgs m{o->images, const_cast<float*>(o->pooled), n_img, o->H, o->W, o->img.dmax};
    HIPCHK(timed(ctx, "minpool5", [&] { return launch_minpool5(m, ctx->stream); }));
    return SDFNMPC_OK;
}

// ------------------------------------------------------------------------------------------------
// analytic scenes (scene.hip)

// kind, values and ranges of one primitive, as sdfnmpc_scene_create checks them; na = the number of values read
static int scene_prim_check(const sdfnmpc_prim* p, int* na) {
    const double* a = p->a;
    bool ok = false;
    if (p->kind == SDFNMPC_PRIM_SPHERE) { *na = 4; ok = a[3] > 0.0; }
    else if (p->kind == SDFNMPC_PRIM_BOX) { *na = 6; ok = a[0] < a[3] && a[1] < a[4] && a[2] < a[5]; }
    else if (p->kind == SDFNMPC_PRIM_CYLINDER) { *na = 5; ok = a[2] > 0.0 && a[3] < a[4]; }
    else return fail(SDFNMPC_E_ARG, "scene: unknown primitive kind (0 sphere, 1 box, 2 cylinder)");
    for (int k = 0; k < *na; ++k) ok = ok && std::isfinite(a[k]);
    if (!ok) return fail(SDFNMPC_E_ARG, "scene: a primitive needs finite values, a radius > 0 and lo < hi");
    return SDFNMPC_OK;
}

// the motion records of `total` primitives, as sdfnmpc_scene_create_moving checks them; *dynamic: whether some record
// has a rotation other than the identity or a non-zero yaw_rate, v or amp
static int scene_motion_check(const sdfnmpc_prim_motion* motion, long long total, bool* dynamic) {
    *dynamic = false;
    for (long long i = 0; motion && i < total; ++i) {
        const sdfnmpc_prim_motion& m = motion[i];
        bool fin = std::isfinite(m.yaw_rate) && std::isfinite(m.omega) && std::isfinite(m.phase);
        for (int k = 0; k < 4; ++k) fin = fin && std::isfinite(m.q[k]);
        for (int k = 0; k < 3; ++k) fin = fin && std::isfinite(m.v[k]) && std::isfinite(m.amp[k]);
        if (!fin) return fail(SDFNMPC_E_ARG, "scene: a motion record needs finite values");
        if (m.q[0] == 0.0 && m.q[1] == 0.0 && m.q[2] == 0.0 && m.q[3] == 0.0)
            return fail(SDFNMPC_E_ARG, "scene: a motion record needs a non-zero quaternion");
        *dynamic = *dynamic || m.q[1] != 0.0 || m.q[2] != 0.0 || m.q[3] != 0.0 || m.yaw_rate != 0.0;
        for (int k = 0; k < 3; ++k) *dynamic = *dynamic || m.v[k] != 0.0 || m.amp[k] != 0.0;
    }
    return SDFNMPC_OK;
}

// the device record of a checked primitive with its motion (mo == NULL: none): the canonical centred shape and its
// frame at t = 0, R(q / |q|) of utils/math.py:7-23 in fp64
static void scene_dyn_fill(ScenePrimDyn& y, const sdfnmpc_prim* p, const sdfnmpc_prim_motion* mo) {
    static const sdfnmpc_prim_motion identity = {{1.0, 0.0, 0.0, 0.0}, 0.0, {0.0, 0.0, 0.0}, {0.0, 0.0, 0.0}, 0.0, 0.0};
    const sdfnmpc_prim_motion& m = mo ? *mo : identity;
    const double* a = p->a;
    y.kind = p->kind;
    if (p->kind == SDFNMPC_PRIM_SPHERE) {
        for (int k = 0; k < 3; ++k) { y.c0[k] = a[k]; y.h[k] = a[3]; }
    } else if (p->kind == SDFNMPC_PRIM_BOX) {
        for (int k = 0; k < 3; ++k) { y.c0[k] = 0.5 * (a[k] + a[3 + k]); y.h[k] = 0.5 * (a[3 + k] - a[k]); }
    } else {
        y.c0[0] = a[0]; y.c0[1] = a[1]; y.c0[2] = 0.5 * (a[3] + a[4]);
        y.h[0] = y.h[1] = a[2]; y.h[2] = 0.5 * (a[4] - a[3]);
    }
    const double qs = std::max(std::max(std::fabs(m.q[0]), std::fabs(m.q[1])),
                               std::max(std::fabs(m.q[2]), std::fabs(m.q[3])));  // no overflow in the norm
    double q[4];
    for (int k = 0; k < 4; ++k) q[k] = m.q[k] / qs;
    const double qn = std::sqrt(q[0] * q[0] + q[1] * q[1] + q[2] * q[2] + q[3] * q[3]);
    const double q0 = q[0] / qn, q1 = q[1] / qn, q2 = q[2] / qn, q3 = q[3] / qn;
    y.R0[0] = q0 * q0 + q1 * q1 - q2 * q2 - q3 * q3;
    y.R0[1] = 2 * (q1 * q2 - q0 * q3);
    y.R0[2] = 2 * (q1 * q3 + q0 * q2);
    y.R0[3] = 2 * (q1 * q2 + q0 * q3);
    y.R0[4] = q0 * q0 - q1 * q1 + q2 * q2 - q3 * q3;
    y.R0[5] = 2 * (q2 * q3 - q0 * q1);
    y.R0[6] = 2 * (q1 * q3 - q0 * q2);
    y.R0[7] = 2 * (q2 * q3 + q0 * q1);
    y.R0[8] = q0 * q0 - q1 * q1 - q2 * q2 + q3 * q3;
    for (int k = 0; k < 3; ++k) { y.v[k] = m.v[k]; y.amp[k] = m.amp[k]; }
    y.yaw_rate = m.yaw_rate; y.omega = m.omega; y.phase = m.phase;
}

// A bound on the speed of any surface point of a filled record, |v| + |omega| |amp| + |yaw_rate| rho in Euclidean norms:
// the centre's speed plus the yaw's at the farthest point of the shape from its centre (rho: 0 for a sphere, the half
// diagonal of a box, sqrt(r^2 + hz^2) for a cylinder).  The scene's distance at a fixed point changes no faster
// (scene_swept.hip).
static double scene_dyn_speed(const ScenePrimDyn& y) {
    const double rho = y.kind == SDFNMPC_PRIM_SPHERE ? 0.0
                       : y.kind == SDFNMPC_PRIM_BOX  ? std::hypot(y.h[0], y.h[1], y.h[2])
                                                     : std::hypot(y.h[0], y.h[2]);
    return std::hypot(y.v[0], y.v[1], y.v[2]) + std::fabs(y.omega) * std::hypot(y.amp[0], y.amp[1], y.amp[2]) +
           std::fabs(y.yaw_rate) * rho;
}

// vmax [S] of the filled records hm [S][32], count[s] of them in use, inflated by 1 + 1e-12 over its own rounding
static void scene_speed_bounds(const ScenePrimDyn* hm, int S, const int* count, double* vmax) {
    for (int s = 0; s < S; ++s) {
        double v = 0.0;
        for (int i = 0; i < count[s]; ++i) v = std::max(v, scene_dyn_speed(hm[(size_t)s * SCENE_MAX_PRIMS + i]));
        vmax[s] = v * (1.0 + 1e-12);
    }
}

extern "C" int sdfnmpc_scene_create(sdfnmpc_ctx* ctx, int S, const int* count, const sdfnmpc_prim* prims,
                                    sdfnmpc_scene** out) {
    return sdfnmpc_scene_create_moving(ctx, S, count, prims, nullptr, out);
}

extern "C" int sdfnmpc_scene_create_moving(sdfnmpc_ctx* ctx, int S, const int* count, const sdfnmpc_prim* prims,
                                           const sdfnmpc_prim_motion* motion, sdfnmpc_scene** out) {
    if (!ctx || !count || !out) return fail(SDFNMPC_E_ARG, "NULL argument to sdfnmpc_scene_create");
    *out = nullptr;
    if (S < 1 || S > (1 << 20)) return fail(SDFNMPC_E_ARG, "scene: S must be 1..2^20");
    long long total = 0;
    for (int s = 0; s < S; ++s) {
        if (count[s] < 0 || count[s] > SCENE_MAX_PRIMS)
            return fail(SDFNMPC_E_ARG, "scene: at most 32 primitives per scene (and no negative count)");
        total += count[s];
    }
    if (total > 0 && !prims) return fail(SDFNMPC_E_ARG, "scene: NULL primitives");
    // the device image: counts padded to 16 bytes, then the fp64 and the fp32 primitives at a fixed stride of 32
    const size_t cnt_bytes = ((size_t)S * sizeof(int) + 15) & ~(size_t)15;
    const size_t n = (size_t)S * SCENE_MAX_PRIMS;
    // a set is dynamic when some primitive has a rotation other than the identity or a non-zero yaw_rate, v or amp
    bool dynamic = false;
    if (int rc = scene_motion_check(motion, total, &dynamic)) return rc;
    const size_t static_bytes = cnt_bytes + n * (sizeof(ScenePrimD) + sizeof(ScenePrimF));
    const size_t dyn_bytes = dynamic ? n * sizeof(ScenePrimDyn) : 0;  // then vmax [S]
    std::vector<char> host(static_bytes + dyn_bytes + (dynamic ? (size_t)S * sizeof(double) : 0), 0);
    ScenePrimDyn* hm = dynamic ? (ScenePrimDyn*)(host.data() + static_bytes) : nullptr;
    static_assert((sizeof(ScenePrimD) + sizeof(ScenePrimF)) * SCENE_MAX_PRIMS % 16 == 0, "fp64 alignment of the motion block");
    int* hc = (int*)host.data();
    ScenePrimD* hd = (ScenePrimD*)(host.data() + cnt_bytes);
    ScenePrimF* hf = (ScenePrimF*)(host.data() + cnt_bytes + n * sizeof(ScenePrimD));
    const sdfnmpc_prim* p = prims;
    for (int s = 0; s < S; ++s) {
        hc[s] = count[s];
        for (int i = 0; i < count[s]; ++i, ++p) {
            const double* a = p->a;
            int na = 0;
            if (int rc = scene_prim_check(p, &na)) return rc;
            ScenePrimD& d = hd[(size_t)s * SCENE_MAX_PRIMS + i];
            ScenePrimF& f = hf[(size_t)s * SCENE_MAX_PRIMS + i];
            d.kind = f.kind = p->kind;
            for (int k = 0; k < na; ++k) {
                d.a[k] = a[k];
                f.a[k] = (float)a[k];
            }
            if (hm) scene_dyn_fill(hm[(size_t)s * SCENE_MAX_PRIMS + i], p, motion + (p - prims));
        }
    }
    static_assert(sizeof(ScenePrimDyn) % 8 == 0, "fp64 alignment of the speed bounds");
    std::vector<double> vmax((size_t)S, 0.0);
    if (hm) {
        scene_speed_bounds(hm, S, count, vmax.data());
        std::memcpy(host.data() + static_bytes + dyn_bytes, vmax.data(), (size_t)S * sizeof(double));
    }
    ScopedDevice sd(ctx->device);
    auto* sc = new sdfnmpc_scene();
    sc->device = ctx->device; sc->ctx = ctx; sc->S = S;
    hipError_t e = hipMalloc(&sc->dmem, host.size());
    if (e == hipSuccess) e = hipMemcpy(sc->dmem, host.data(), host.size(), hipMemcpyHostToDevice);
    if (e != hipSuccess) {
        if (sc->dmem) (void)hipFree(sc->dmem);
        delete sc;
        return fail(SDFNMPC_E_HIP, std::string("scene upload: ") + hipGetErrorString(e));
    }
    char* d = (char*)sc->dmem;
    sc->dev = SceneDev{S, (const int*)d, (const ScenePrimF*)(d + cnt_bytes + n * sizeof(ScenePrimD)),
                       (const ScenePrimD*)(d + cnt_bytes)};
    sc->vmax = std::move(vmax);
    if (dynamic) {
        sc->dyn = (const ScenePrimDyn*)(d + static_bytes);
        sc->dvmax = (const double*)(d + static_bytes + dyn_bytes);
    }
    *out = sc;
    return SDFNMPC_OK;
}

static void scene_prim_bbox(const sdfnmpc_prim& p, double* lo, double* hi) {
    const double* a = p.a;
    if (p.kind == SDFNMPC_PRIM_SPHERE) {
        for (int k = 0; k < 3; ++k) { lo[k] = a[k] - a[3]; hi[k] = a[k] + a[3]; }
    } else if (p.kind == SDFNMPC_PRIM_BOX) {
        for (int k = 0; k < 3; ++k) { lo[k] = a[k]; hi[k] = a[3 + k]; }
    } else {
        for (int k = 0; k < 2; ++k) { lo[k] = a[k] - a[2]; hi[k] = a[k] + a[2]; }
        lo[2] = a[3]; hi[2] = a[4];
    }
}

// Static scenes of up to SDFNMPC_SCENE_LARGE_MAX_PRIMS primitives with a uniform grid each, built here on the host
// (the layout: SceneGridHdr, scene_kernels.h; why the inflation and the padding: scene_grid.hip)
// mcount == NULL: the indexed set of sdfnmpc_scene_create_large.  Otherwise mcount [S] in 0..32, mprims and mmotion
// (or NULL) already checked by the caller: the movers of a mixed set (sdfnmpc_scene_create_mixed), appended to the
// device image as mcount [S] | ScenePrimDyn [S][32]; the grid covers the static primitives only
static int scene_create_indexed(sdfnmpc_ctx* ctx, int S, const int* count, const sdfnmpc_prim* prims, double cell,
                                const int* mcount, const sdfnmpc_prim* mprims, const sdfnmpc_prim_motion* mmotion,
                                sdfnmpc_scene** out) {
    if (!ctx || !count || !out) return fail(SDFNMPC_E_ARG, "NULL argument to sdfnmpc_scene_create_large");
    *out = nullptr;
    if (S < 1 || S > (1 << 20)) return fail(SDFNMPC_E_ARG, "scene: S must be 1..2^20");
    if (!std::isfinite(cell)) return fail(SDFNMPC_E_ARG, "scene: the grid's cell size must be finite (<= 0: the default)");
    long long total = 0;
    for (int s = 0; s < S; ++s) {
        if (count[s] < 0 || count[s] > SCENE_LARGE_MAX_PRIMS)
            return fail(SDFNMPC_E_ARG, "scene: at most 65536 primitives per indexed scene (and no negative count)");
        total += count[s];
    }
    if (total > 0 && !prims) return fail(SDFNMPC_E_ARG, "scene: NULL primitives");
    if (total > 2147483647LL / 64) return fail(SDFNMPC_E_ARG, "scene: more than 2^25 primitives in an indexed set");
    for (long long i = 0; i < total; ++i) {
        int na;
        if (int rc = scene_prim_check(prims + i, &na)) return rc;
    }
    std::vector<SceneGridHdr> hdr((size_t)S);
    std::vector<int> cell_start, cell_items;
    const char* too_big = "scene: the grid is too large (at most 1024 cells per axis, 2^22 cells per scene, 2^26 cells "
                          "and cell-list entries per set): choose a larger cell";
    const sdfnmpc_prim* p = prims;
    for (int s = 0; s < S; p += count[s], ++s) {
        SceneGridHdr& G = hdr[(size_t)s];
        const int n = count[s];
        G = SceneGridHdr{};
        G.count = n;
        G.prim_off = (int)(p - prims);
        G.cell_off = (int)cell_start.size();
        if (n == 0) {  // an empty grid: one cell without entries
            G.cell = G.inv = 1.0;
            G.n[0] = G.n[1] = G.n[2] = 1;
            cell_start.push_back((int)cell_items.size());
            cell_start.push_back((int)cell_items.size());
            continue;
        }
        double lo[3] = {INFINITY, INFINITY, INFINITY}, hi[3] = {-INFINITY, -INFINITY, -INFINITY};
        for (int i = 0; i < n; ++i) {
            double bl[3], bh[3];
            scene_prim_bbox(p[i], bl, bh);
            for (int k = 0; k < 3; ++k) { lo[k] = std::min(lo[k], bl[k]); hi[k] = std::max(hi[k], bh[k]); }
        }
        double R = 0.0, ext_max = 0.0, vol = 1.0;
        for (int k = 0; k < 3; ++k) {
            R = std::max(R, std::max(std::fabs(lo[k]), std::fabs(hi[k])));
            ext_max = std::max(ext_max, hi[k] - lo[k]);
            vol *= hi[k] - lo[k];
        }
        // the default: cubes of the volume of the primitives' bounding box over 4 n, about 4 cells per primitive, and
        // not smaller than 1 / 250 of the padded box's longest edge (at most 256 cells per axis)
        double c = cell > 0.0 ? cell : std::max(std::cbrt(vol / (4.0 * n)), (ext_max + R * 0x1p-10) / 250.0);
        c = (double)(float)c;
        if (!(c > 0.0) || !std::isfinite(c) || !std::isfinite(R) || !std::isfinite(ext_max))
            return fail(SDFNMPC_E_ARG, "scene: the grid's cell size or the scene's extent is out of fp32 range");
        const double infl = c * 0x1p-10 + R * 0x1p-12;
        long long cells = 1;
        for (int k = 0; k < 3; ++k) {
            float o = (float)(lo[k] - 2.0 * infl);
            if ((double)o > lo[k] - 2.0 * infl) o = std::nextafterf(o, -INFINITY);
            G.org[k] = (double)o;
            const double top = hi[k] + 2.0 * infl;
            const double m = std::ceil((top - G.org[k]) / c);
            if (!(m <= (double)SCENE_GRID_MAX_AXIS)) return fail(SDFNMPC_E_ARG, too_big);
            G.n[k] = std::max(1, (int)m);
            while (G.org[k] + G.n[k] * c < top) ++G.n[k];
            if (G.n[k] > SCENE_GRID_MAX_AXIS) return fail(SDFNMPC_E_ARG, too_big);
            cells *= G.n[k];
        }
        G.cell = c;
        G.inv = 1.0 / c;
        if (cells > SCENE_GRID_MAX_CELLS || (long long)cell_start.size() + cells + 1 > SCENE_GRID_MAX_ITEMS)
            return fail(SDFNMPC_E_ARG, too_big);
        // the cells of every primitive's inflated box, counted, then filled in ascending primitive order
        std::vector<int> box((size_t)n * 6);
        std::vector<long long> cnt((size_t)cells + 1, 0);
        long long listed = 0;
        for (int i = 0; i < n; ++i) {
            double bl[3], bh[3];
            scene_prim_bbox(p[i], bl, bh);
            int* q = &box[(size_t)i * 6];
            for (int k = 0; k < 3; ++k) {
                q[k] = std::min(std::max((int)std::floor((bl[k] - infl - G.org[k]) / c), 0), G.n[k] - 1);
                q[3 + k] = std::min(std::max((int)std::floor((bh[k] + infl - G.org[k]) / c), 0), G.n[k] - 1);
            }
            listed += (long long)(q[3] - q[0] + 1) * (q[4] - q[1] + 1) * (q[5] - q[2] + 1);
            if ((long long)cell_items.size() + listed > SCENE_GRID_MAX_ITEMS) return fail(SDFNMPC_E_ARG, too_big);
            for (int z = q[2]; z <= q[5]; ++z)
                for (int y = q[1]; y <= q[4]; ++y)
                    for (int x = q[0]; x <= q[3]; ++x) ++cnt[(size_t)((long long)(z * G.n[1] + y) * G.n[0] + x) + 1];
        }
        const size_t base = cell_items.size(), cs0 = cell_start.size();
        cell_items.resize(base + (size_t)listed);
        cell_start.resize(cs0 + (size_t)cells + 1);
        for (long long id = 0; id < cells; ++id) cnt[(size_t)id + 1] += cnt[(size_t)id];
        for (long long id = 0; id <= cells; ++id) cell_start[cs0 + (size_t)id] = (int)(base + cnt[(size_t)id]);
        for (int i = 0; i < n; ++i) {
            const int* q = &box[(size_t)i * 6];
            for (int z = q[2]; z <= q[5]; ++z)
                for (int y = q[1]; y <= q[4]; ++y)
                    for (int x = q[0]; x <= q[3]; ++x)
                        cell_items[base + (size_t)cnt[(size_t)((long long)(z * G.n[1] + y) * G.n[0] + x)]++] = i;
        }
    }
    // the device image
    auto up16 = [](size_t v) { return (v + 15) & ~(size_t)15; };
    const size_t o_hdr = up16((size_t)S * sizeof(int));
    const size_t o_pd = up16(o_hdr + (size_t)S * sizeof(SceneGridHdr));
    const size_t o_pf = up16(o_pd + (size_t)total * sizeof(ScenePrimD));
    const size_t o_cs = up16(o_pf + (size_t)total * sizeof(ScenePrimF));
    const size_t o_ci = up16(o_cs + cell_start.size() * sizeof(int));
    const size_t o_mc = up16(o_ci + cell_items.size() * sizeof(int)) + 16;  // the indexed set's image ends here
    const size_t o_dyn = up16(o_mc + (size_t)S * sizeof(int));
    const size_t o_vmax = o_dyn + (size_t)S * SCENE_MAX_PRIMS * sizeof(ScenePrimDyn);  // a mixed set's speed bounds [S]
    std::vector<char> host(mcount ? o_vmax + (size_t)S * sizeof(double) : o_mc, 0);
    std::vector<double> vmax((size_t)S, 0.0);
    if (mcount) {
        std::memcpy(host.data() + o_mc, mcount, (size_t)S * sizeof(int));
        ScenePrimDyn* hm = (ScenePrimDyn*)(host.data() + o_dyn);
        const sdfnmpc_prim* q = mprims;
        for (int s = 0; s < S; ++s)
            for (int i = 0; i < mcount[s]; ++i, ++q)
                scene_dyn_fill(hm[(size_t)s * SCENE_MAX_PRIMS + i], q, mmotion ? mmotion + (q - mprims) : nullptr);
        scene_speed_bounds(hm, S, mcount, vmax.data());
        std::memcpy(host.data() + o_vmax, vmax.data(), (size_t)S * sizeof(double));
    }
    std::memcpy(host.data(), count, (size_t)S * sizeof(int));
    std::memcpy(host.data() + o_hdr, hdr.data(), (size_t)S * sizeof(SceneGridHdr));
    ScenePrimD* hd = (ScenePrimD*)(host.data() + o_pd);
    ScenePrimF* hf = (ScenePrimF*)(host.data() + o_pf);
    for (long long i = 0; i < total; ++i) {
        int na = 0;
        (void)scene_prim_check(prims + i, &na);
        hd[i].kind = hf[i].kind = prims[i].kind;
        for (int k = 0; k < na; ++k) {
            hd[i].a[k] = prims[i].a[k];
            hf[i].a[k] = (float)prims[i].a[k];
        }
    }
    std::memcpy(host.data() + o_cs, cell_start.data(), cell_start.size() * sizeof(int));
    if (!cell_items.empty()) std::memcpy(host.data() + o_ci, cell_items.data(), cell_items.size() * sizeof(int));
    ScopedDevice sd(ctx->device);
    auto* sc = new sdfnmpc_scene();
    sc->device = ctx->device; sc->ctx = ctx; sc->S = S;
    hipError_t e = hipMalloc(&sc->dmem, host.size());
    if (e == hipSuccess) e = hipMemcpy(sc->dmem, host.data(), host.size(), hipMemcpyHostToDevice);
    if (e != hipSuccess) {
        if (sc->dmem) (void)hipFree(sc->dmem);
        delete sc;
        return fail(SDFNMPC_E_HIP, std::string("scene upload: ") + hipGetErrorString(e));
    }
    char* d = (char*)sc->dmem;
    sc->dev = SceneDev{S, (const int*)d, (const ScenePrimF*)(d + o_pf), (const ScenePrimD*)(d + o_pd),
                       (const SceneGridHdr*)(d + o_hdr), (const int*)(d + o_cs), (const int*)(d + o_ci)};
    sc->vmax = std::move(vmax);
    if (mcount) {
        sc->mcount = (const int*)(d + o_mc);
        sc->dyn = (const ScenePrimDyn*)(d + o_dyn);
        sc->dvmax = (const double*)(d + o_vmax);
    }
    *out = sc;
    return SDFNMPC_OK;
}

extern "C" int sdfnmpc_scene_create_large(sdfnmpc_ctx* ctx, int S, const int* count, const sdfnmpc_prim* prims,
                                          double cell, sdfnmpc_scene** out) {
    return scene_create_indexed(ctx, S, count, prims, cell, nullptr, nullptr, nullptr, out);
}

// An indexed static set plus up to 32 movers per scene (scene_grid.hip's *_mixed kernels).  The movers are checked
// here as sdfnmpc_scene_create_moving checks its primitives, the static set by the builder of
// sdfnmpc_scene_create_large; without a mover in any scene the handle is that function's
extern "C" int sdfnmpc_scene_create_mixed(sdfnmpc_ctx* ctx, int S, const int* count, const sdfnmpc_prim* prims,
                                          double cell, const int* mcount, const sdfnmpc_prim* mprims,
                                          const sdfnmpc_prim_motion* mmotion, sdfnmpc_scene** out) {
    if (!ctx || !count || !mcount || !out) return fail(SDFNMPC_E_ARG, "NULL argument to sdfnmpc_scene_create_mixed");
    *out = nullptr;
    if (S < 1 || S > (1 << 20)) return fail(SDFNMPC_E_ARG, "scene: S must be 1..2^20");
    long long mtotal = 0;
    for (int s = 0; s < S; ++s) {
        if (mcount[s] < 0 || mcount[s] > SCENE_MAX_PRIMS)
            return fail(SDFNMPC_E_ARG, "scene: at most 32 movers per scene (and no negative count)");
        mtotal += mcount[s];
    }
    if (mtotal > 0 && !mprims) return fail(SDFNMPC_E_ARG, "scene: NULL movers");
    bool dynamic = false;
    if (int rc = scene_motion_check(mmotion, mtotal, &dynamic)) return rc;
    for (long long i = 0; i < mtotal; ++i) {
        int na;
        if (int rc = scene_prim_check(mprims + i, &na)) return rc;
    }
    // a mover without motion still takes the mover path: the set is mixed as soon as it holds one
    const bool mixed = mtotal > 0;
    return scene_create_indexed(ctx, S, count, prims, cell, mixed ? mcount : nullptr, mprims, mmotion, out);
}

// Mesh sets (scene_mesh.hip): S static triangle meshes, each checked, rounded to fp32 and put behind a hierarchy here on
// the host (mesh_bvh.h: the layout, the split rule, the boxes and their margin)
// mcount == NULL: the mesh set of sdfnmpc_scene_create_mesh.  Otherwise mcount [S] in 0..32, mprims and mmotion (or
// NULL) already checked by the caller: the movers of sdfnmpc_scene_create_mesh_mixed, appended to the device image as
// mcount [S] | ScenePrimDyn [S][32] | vmax [S], as scene_create_indexed appends them to a grid's
//
// inst != NULL: the set of sdfnmpc_scene_create_instanced.  The S "scenes" built here are then the parts of its pool,
// and the handle's scenes are the inst->S lists of instances, already checked by the caller and appended to the image as
// icount [S] | ioff [S] | ScenePrimDyn [sum of icount] | vmax [S]
struct InstHost {
    int S;
    const int* icount;                // [S]
    const sdfnmpc_mesh_instance* in;  // [sum of icount]
};
static int scene_create_mesh_set(sdfnmpc_ctx* ctx, int S, const int* nvert, const double* verts, const int* ntri,
                                 const int* tris, const sdfnmpc_mesh_opts* opts, const int* mcount,
                                 const sdfnmpc_prim* mprims, const sdfnmpc_prim_motion* mmotion, sdfnmpc_scene** out,
                                 const InstHost* inst = nullptr) {
    if (!ctx || !nvert || !ntri || !out) return fail(SDFNMPC_E_ARG, "NULL argument to sdfnmpc_scene_create_mesh");
    *out = nullptr;
    if (S < 1 || S > (1 << 20)) return fail(SDFNMPC_E_ARG, "mesh: S must be 1..2^20");
    const sdfnmpc_mesh_opts o = opts ? *opts : sdfnmpc_mesh_opts{0, 0, 0};
    if (!(o.leaf_size == -1 || (o.leaf_size >= 0 && o.leaf_size <= MESH_LEAF_MAX)))
        return fail(SDFNMPC_E_ARG, "mesh: leaf_size must be 1..8, 0 (the default) or -1 (no hierarchy)");
    if (o.closed != 0 && o.closed != 1) return fail(SDFNMPC_E_ARG, "mesh: closed must be 0 or 1");
    if (o.sdf_source != 0 && o.sdf_source != 1) return fail(SDFNMPC_E_ARG, "mesh: sdf_source must be 0 or 1");
    const int leaf = o.leaf_size == 0 ? MESH_LEAF_DEFAULT : o.leaf_size;
    long long tv = 0, tt = 0;
    for (int s = 0; s < S; ++s) {
        if (nvert[s] < 0 || nvert[s] > MESH_MAX_VERTS)
            return fail(SDFNMPC_E_ARG, "mesh: at most 2^21 vertices per scene (and no negative count)");
        if (ntri[s] < 0 || ntri[s] > MESH_MAX_TRIS)
            return fail(SDFNMPC_E_ARG, "mesh: at most 2^20 triangles per scene (and no negative count)");
        tv += nvert[s];
        tt += ntri[s];
    }
    if (tt > MESH_MAX_SET_TRIS) return fail(SDFNMPC_E_ARG, "mesh: more than 2^24 triangles in the set");
    if ((tv > 0 && !verts) || (tt > 0 && !tris)) return fail(SDFNMPC_E_ARG, "mesh: NULL vertices or triangles");
    // per scene: the check, the fp32 vertices, the hierarchy and the triangles in its order
    std::vector<MeshHdr> hdr((size_t)S);
    std::vector<MeshNode> nodes;
    std::vector<MeshTriF> tf((size_t)tt);
    std::vector<MeshTriD> td((size_t)tt);
    std::vector<MeshTriN> tn(o.closed ? (size_t)tt : 0);
    std::vector<double> rho((size_t)S, 0.0);  // the largest |vertex| of each mesh, of its fp32 vertices
    {
        const double* v = verts;
        const int* t = tris;
        long long toff = 0;
        std::vector<float> vf;
        std::vector<double> fn;
        std::vector<MeshTriN> pn;
        MeshBvh bvh;
        for (int s = 0; s < S; v += (size_t)nvert[s] * 3, t += (size_t)ntri[s] * 3, ++s) {
            if (const char* why = mesh_check(v, nvert[s], t, ntri[s], o.closed != 0, vf)) return fail(SDFNMPC_E_ARG, why);
            const float m = mesh_margin(vf.data(), nvert[s]);
            for (int i = 0; i < nvert[s]; ++i)
                rho[s] = std::max(rho[s], std::hypot((double)vf[(size_t)i * 3], (double)vf[(size_t)i * 3 + 1],
                                                     (double)vf[(size_t)i * 3 + 2]));
            mesh_bvh_build(vf.data(), t, ntri[s], leaf, m, bvh);
            mesh_face_normals(vf.data(), t, ntri[s], fn);
            if (o.closed) mesh_pseudonormals(vf.data(), nvert[s], t, ntri[s], fn, pn);
            hdr[s] = MeshHdr{(int)nodes.size(), (int)bvh.nodes.size(), (int)toff, ntri[s], m, {0, 0, 0}};
            nodes.insert(nodes.end(), bvh.nodes.begin(), bvh.nodes.end());
            for (int k = 0; k < ntri[s]; ++k) {
                const int g = bvh.order[k];
                MeshTriF& F = tf[(size_t)toff + k];
                MeshTriD& Dd = td[(size_t)toff + k];
                F = MeshTriF{};
                Dd = MeshTriD{};
                for (int c = 0; c < 3; ++c)
                    for (int a = 0; a < 3; ++a) {
                        F.v[c * 3 + a] = vf[(size_t)t[g * 3 + c] * 3 + a];
                        Dd.v[c * 3 + a] = (double)F.v[c * 3 + a];
                    }
                for (int a = 0; a < 3; ++a) F.n[a] = (float)fn[(size_t)g * 3 + a];
                for (int c = 0; c < 3; ++c)
                    if (t[g * 3 + c] > t[g * 3 + (c + 1) % 3]) F.flip |= 1 << c;
                Dd.orig = g;
                if (o.closed) tn[(size_t)toff + k] = pn[(size_t)g];
            }
            toff += ntri[s];
        }
    }
    auto up16 = [](size_t v) { return (v + 15) & ~(size_t)15; };
    const size_t o_nodes = up16((size_t)S * sizeof(MeshHdr));
    const size_t o_tf = up16(o_nodes + nodes.size() * sizeof(MeshNode));
    const size_t o_td = up16(o_tf + tf.size() * sizeof(MeshTriF));
    const size_t o_tn = up16(o_td + td.size() * sizeof(MeshTriD));
    const size_t o_mc = up16(o_tn + tn.size() * sizeof(MeshTriN)) + 16;  // the mesh set's image ends here
    const size_t o_dyn = up16(o_mc + (size_t)S * sizeof(int));
    const size_t o_vmax = o_dyn + (size_t)S * SCENE_MAX_PRIMS * sizeof(ScenePrimDyn);  // the movers' speed bounds [S]
    static_assert(SCENE_MAX_PRIMS * sizeof(ScenePrimDyn) % 16 == 0, "fp64 alignment of the speed bounds");
    size_t bytes = mcount ? o_vmax + (size_t)S * sizeof(double) : o_mc;
    const int HS = inst ? inst->S : S;  // the scenes of the handle
    std::vector<double> vmax((size_t)HS, 0.0);
    std::vector<ScenePrimDyn> hm;
    // an instanced set: the records (the frame of a primitive at c0 = p, the part in `kind`) and the speed bounds
    std::vector<int> ioff;
    bool inst_moves = false;
    size_t o_ic = 0, o_io = 0, o_rec = 0, o_iv = 0;
    if (inst) {
        ioff.assign((size_t)HS, 0);
        long long total = 0;
        for (int s = 0; s < HS; ++s) {
            ioff[s] = (int)total;
            total += inst->icount[s];
        }
        hm.assign((size_t)total, ScenePrimDyn{});
        for (int s = 0; s < HS; ++s)
            for (int i = 0; i < inst->icount[s]; ++i) {
                const sdfnmpc_mesh_instance& q = inst->in[(size_t)ioff[s] + i];
                ScenePrimDyn& y = hm[(size_t)ioff[s] + i];
                const sdfnmpc_prim centre = {SDFNMPC_PRIM_SPHERE, {q.p[0], q.p[1], q.p[2], 1.0, 0.0, 0.0}};
                scene_dyn_fill(y, &centre, &q.motion);
                y.kind = q.part;
                y.h[0] = rho[(size_t)q.part];
                y.h[1] = y.h[2] = 0.0;
                const sdfnmpc_prim_motion& m = q.motion;
                inst_moves = inst_moves || m.yaw_rate != 0.0;
                for (int k = 0; k < 3; ++k) inst_moves = inst_moves || m.v[k] != 0.0 || m.amp[k] != 0.0;
                // scene_dyn_speed's bound with rho the largest |vertex| of the part, inflated like scene_speed_bounds
                vmax[s] = std::max(vmax[s], std::hypot(y.v[0], y.v[1], y.v[2]) +
                                                std::fabs(y.omega) * std::hypot(y.amp[0], y.amp[1], y.amp[2]) +
                                                std::fabs(y.yaw_rate) * y.h[0]);
            }
        for (int s = 0; s < HS; ++s) vmax[s] *= 1.0 + 1e-12;
        o_ic = o_mc;
        o_io = up16(o_ic + (size_t)HS * sizeof(int));
        o_rec = up16(o_io + (size_t)HS * sizeof(int));
        o_iv = up16(o_rec + hm.size() * sizeof(ScenePrimDyn));
        bytes = o_iv + (size_t)HS * sizeof(double);
    }
    if (mcount) {
        hm.assign((size_t)S * SCENE_MAX_PRIMS, ScenePrimDyn{});
        const sdfnmpc_prim* q = mprims;
        for (int s = 0; s < S; ++s)
            for (int i = 0; i < mcount[s]; ++i, ++q)
                scene_dyn_fill(hm[(size_t)s * SCENE_MAX_PRIMS + i], q, mmotion ? mmotion + (q - mprims) : nullptr);
        scene_speed_bounds(hm.data(), S, mcount, vmax.data());
    }
    ScopedDevice sd(ctx->device);
    auto* sc = new sdfnmpc_scene();
    sc->device = ctx->device; sc->ctx = ctx; sc->S = HS;
    hipError_t e = hipMalloc(&sc->dmem, bytes);
    char* d = (char*)sc->dmem;
    auto put = [&](size_t off, const void* src, size_t n) {
        if (e == hipSuccess && n) e = hipMemcpy(d + off, src, n, hipMemcpyHostToDevice);
    };
    put(0, hdr.data(), (size_t)S * sizeof(MeshHdr));
    put(o_nodes, nodes.data(), nodes.size() * sizeof(MeshNode));
    put(o_tf, tf.data(), tf.size() * sizeof(MeshTriF));
    put(o_td, td.data(), td.size() * sizeof(MeshTriD));
    put(o_tn, tn.data(), tn.size() * sizeof(MeshTriN));
    if (mcount) {
        put(o_mc, mcount, (size_t)S * sizeof(int));
        put(o_dyn, hm.data(), hm.size() * sizeof(ScenePrimDyn));
        put(o_vmax, vmax.data(), (size_t)S * sizeof(double));
    }
    if (inst) {
        put(o_ic, inst->icount, (size_t)HS * sizeof(int));
        put(o_io, ioff.data(), (size_t)HS * sizeof(int));
        put(o_rec, hm.data(), hm.size() * sizeof(ScenePrimDyn));
        put(o_iv, vmax.data(), (size_t)HS * sizeof(double));
    }
    if (e != hipSuccess) {
        if (sc->dmem) (void)hipFree(sc->dmem);
        delete sc;
        return fail(SDFNMPC_E_HIP, std::string("mesh upload: ") + hipGetErrorString(e));
    }
    sc->dev = SceneDev{};
    sc->dev.S = HS;
    sc->is_mesh = !inst;
    sc->sdf_source = o.sdf_source != 0;
    sc->mesh = MeshDev{(const MeshHdr*)d, (const MeshNode*)(d + o_nodes), (const MeshTriF*)(d + o_tf),
                       (const MeshTriD*)(d + o_td), o.closed ? (const MeshTriN*)(d + o_tn) : nullptr};
    sc->vmax = std::move(vmax);
    if (mcount) {
        sc->mcount = (const int*)(d + o_mc);
        sc->dyn = (const ScenePrimDyn*)(d + o_dyn);
        sc->dvmax = (const double*)(d + o_vmax);
    }
    if (inst) {
        sc->is_inst = true;
        sc->inst_moves = inst_moves;
        sc->inst = InstDev{S, (const int*)(d + o_ic), (const int*)(d + o_io), (const ScenePrimDyn*)(d + o_rec)};
        sc->dvmax = (const double*)(d + o_iv);
    }
    *out = sc;
    return SDFNMPC_OK;
}

extern "C" int sdfnmpc_scene_create_mesh(sdfnmpc_ctx* ctx, int S, const int* nvert, const double* verts, const int* ntri,
                                         const int* tris, const sdfnmpc_mesh_opts* opts, sdfnmpc_scene** out) {
    return scene_create_mesh_set(ctx, S, nvert, verts, ntri, tris, opts, nullptr, nullptr, nullptr, out);
}

// A mesh set plus up to 32 movers per scene (scene_mesh.hip's *_mesh_mixed kernels).  The movers are checked here as
// sdfnmpc_scene_create_mixed checks its own, the mesh by the builder of sdfnmpc_scene_create_mesh; without a mover in
// any scene the handle is that function's
extern "C" int sdfnmpc_scene_create_mesh_mixed(sdfnmpc_ctx* ctx, int S, const int* nvert, const double* verts,
                                               const int* ntri, const int* tris, const sdfnmpc_mesh_opts* opts,
                                               const int* mcount, const sdfnmpc_prim* mprims,
                                               const sdfnmpc_prim_motion* mmotion, sdfnmpc_scene** out) {
    if (!ctx || !nvert || !ntri || !mcount || !out)
        return fail(SDFNMPC_E_ARG, "NULL argument to sdfnmpc_scene_create_mesh_mixed");
    *out = nullptr;
    if (S < 1 || S > (1 << 20)) return fail(SDFNMPC_E_ARG, "mesh: S must be 1..2^20");
    long long mtotal = 0;
    for (int s = 0; s < S; ++s) {
        if (mcount[s] < 0 || mcount[s] > SCENE_MAX_PRIMS)
            return fail(SDFNMPC_E_ARG, "scene: at most 32 movers per scene (and no negative count)");
        mtotal += mcount[s];
    }
    if (mtotal > 0 && !mprims) return fail(SDFNMPC_E_ARG, "scene: NULL movers");
    bool dynamic = false;
    if (int rc = scene_motion_check(mmotion, mtotal, &dynamic)) return rc;
    for (long long i = 0; i < mtotal; ++i) {
        int na;
        if (int rc = scene_prim_check(mprims + i, &na)) return rc;
    }
    // a mover without motion still takes the mover path: the set has movers as soon as it holds one
    return scene_create_mesh_set(ctx, S, nvert, verts, ntri, tris, opts, mtotal > 0 ? mcount : nullptr, mprims, mmotion, out);
}

// An instanced set (scene_inst.hip): nparts meshes, built as the scenes of a mesh set are, and S lists of instances
// that place them.  The instances are checked here, the parts by the builder of sdfnmpc_scene_create_mesh
extern "C" int sdfnmpc_scene_create_instanced(sdfnmpc_ctx* ctx, int nparts, const int* nvert, const double* verts,
                                              const int* ntri, const int* tris, const sdfnmpc_mesh_opts* opts, int S,
                                              const int* icount, const sdfnmpc_mesh_instance* instances,
                                              sdfnmpc_scene** out) {
    if (!ctx || !nvert || !ntri || !icount || !out)
        return fail(SDFNMPC_E_ARG, "NULL argument to sdfnmpc_scene_create_instanced");
    *out = nullptr;
    if (nparts < 1 || nparts > (1 << 20)) return fail(SDFNMPC_E_ARG, "instanced: nparts must be 1..2^20");
    if (S < 1 || S > (1 << 20)) return fail(SDFNMPC_E_ARG, "instanced: S must be 1..2^20");
    long long total = 0;
    for (int s = 0; s < S; ++s) {
        if (icount[s] < 0 || icount[s] > SCENE_MAX_INSTANCES)
            return fail(SDFNMPC_E_ARG, "instanced: at most 256 instances per scene (and no negative count)");
        total += icount[s];
    }
    if (total > 0 && !instances) return fail(SDFNMPC_E_ARG, "instanced: NULL instances");
    for (long long i = 0; i < total; ++i) {
        const sdfnmpc_mesh_instance& q = instances[i];
        if (q.part < 0 || q.part >= nparts) return fail(SDFNMPC_E_ARG, "instanced: a part index outside [0, nparts)");
        if (!(std::isfinite(q.p[0]) && std::isfinite(q.p[1]) && std::isfinite(q.p[2])))
            return fail(SDFNMPC_E_ARG, "instanced: an instance needs a finite position");
        bool dynamic = false;
        if (int rc = scene_motion_check(&q.motion, 1, &dynamic)) return rc;
    }
    const InstHost ih{S, icount, instances};
    return scene_create_mesh_set(ctx, nparts, nvert, verts, ntri, tris, opts, nullptr, nullptr, nullptr, out, &ih);
}

extern "C" int sdfnmpc_scene_is_instanced(const sdfnmpc_scene* sc) { return sc && sc->is_inst; }

extern "C" int sdfnmpc_scene_is_mesh(const sdfnmpc_scene* sc) { return sc && sc->is_mesh; }

// a mesh set or an instanced set is a source only when it was created as one
extern "C" int sdfnmpc_scene_is_sdf_source(const sdfnmpc_scene* sc) {
    return sc && (!(sc->is_mesh || sc->is_inst) || sc->sdf_source);
}

extern "C" int sdfnmpc_scene_is_indexed(const sdfnmpc_scene* sc) { return sc && sc->dev.ghdr; }

extern "C" void sdfnmpc_scene_free(sdfnmpc_scene* sc) {
    if (!sc) return;
    ScopedDevice sd(sc->device);
    if (sc->dmem) (void)hipFree(sc->dmem);
    delete sc;
}

extern "C" int sdfnmpc_scene_is_dynamic(const sdfnmpc_scene* sc) { return sc && (sc->dyn || sc->inst_moves); }

// the option checks of the two launches a rollout repeats, split from the launches as the plant's are
int sdfn::scene_render_args(sdfnmpc_ctx* ctx, const sdfnmpc_scene* sc, const int* scene_of, const sdfnmpc_img_opts* o,
                            int H, int W, float scale, int B, const double* W_p_C, const double* W_R_C, float* img,
                            SceneRenderArgs& out) {
    if (!ctx || !sc || !o) return fail(SDFNMPC_E_ARG, "scene_render: NULL context, scene or options");
    if (sc->device != ctx->device) return fail(SDFNMPC_E_ARG, "scene_render: the scene lives on another device");
    if (B < 0 || B > 65535) return fail(SDFNMPC_E_ARG, "scene_render: B must be 0..65535");
    if (H < 1 || W < 1 || (long long)H * W > 2147483647LL) return fail(SDFNMPC_E_ARG, "scene_render: bad image size");
    auto pos = [](float v) { return v > 0.f && std::isfinite(v); };
    if (!pos(o->dmax) || !pos(o->hfov) || !pos(o->vfov) || !pos(scale))
        return fail(SDFNMPC_E_ARG, "scene_render: dmax, hfov, vfov and scale must be positive and finite");
    const double half_pi = 1.5707963267948966;
    if (!o->is_spherical && ((double)o->hfov >= half_pi || (double)o->vfov >= half_pi))
        return fail(SDFNMPC_E_ARG, "scene_render: a pinhole image needs hfov and vfov below pi / 2");
    if (scene_render_lds_bytes(H, W, o->is_spherical != 0) > SCENE_LDS_MAX)
        return fail(SDFNMPC_E_ARG, "scene_render: spherical image too large (H + W <= 6144)");
    // an instanced set stages its 256 frames (16 KB) beside the spherical tables
    if (sc->is_inst && scene_render_lds_bytes(H, W, o->is_spherical != 0) + SCENE_MAX_INSTANCES * sizeof(SceneInstFrame) >
                           SCENE_LDS_MAX)
        return fail(SDFNMPC_E_ARG, "scene_render: spherical image too large for an instanced set (H + W <= 4096)");
    if (B > 0 && (!W_p_C || !W_R_C || !img)) return fail(SDFNMPC_E_ARG, "scene_render: NULL pose or image");
    SceneRenderArgs a{};
    a.sc = sc->dev; a.scene_of = scene_of; a.B = B; a.H = H; a.W = W; a.W_p_C = W_p_C; a.W_R_C = W_R_C;
    a.dmax = o->dmax; a.scale = scale; a.hfov = o->hfov; a.vfov = o->vfov;
    a.is_depth = o->is_depth != 0; a.is_spherical = o->is_spherical != 0;
    if (!a.is_spherical) {  // tangent coordinates of the pixel centres: t (1 - (2 i + 1) / n) = t (1 - 1 / n) - (2 t / n) i
        const double th = std::tan((double)o->hfov), tv = std::tan((double)o->vfov);
        a.ty0 = (float)(th * (1.0 - 1.0 / W)); a.ty1 = (float)(-2.0 * th / W);
        a.tz0 = (float)(tv * (1.0 - 1.0 / H)); a.tz1 = (float)(-2.0 * tv / H);
    }
    a.img = img;
    out = a;
    return SDFNMPC_OK;
}

static int scene_render_static(sdfnmpc_ctx* ctx, const SceneRenderArgs& a) {
    ScopedDevice sd(ctx->device);
    if (a.sc.ghdr) {  // an indexed set
        HIPCHK(timed(ctx, "scene_render_grid", [&] { return launch_scene_render_grid(a, ctx->stream); }));
        return SDFNMPC_OK;
    }
    HIPCHK(timed(ctx, "scene_render", [&] { return launch_scene_render(a, ctx->stream); }));
    return SDFNMPC_OK;
}

// the scene at time t: a static set takes the launch above whatever t is, a dynamic one its own kernel
int sdfn::scene_render_launch(sdfnmpc_ctx* ctx, const sdfnmpc_scene& sc, const SceneRenderArgs& a, double t) {
    if (sc.is_inst) {  // an instanced set, its frames at time t
        const InstRenderArgs ia{a, sc.mesh, sc.inst, t};
        ScopedDevice sd(ctx->device);
        HIPCHK(timed(ctx, "scene_render_inst", [&] { return launch_scene_render_inst(ia, ctx->stream); }));
        return SDFNMPC_OK;
    }
    if (sc.is_mesh && sc.dyn) {  // a mesh set with movers, at time t
        const MeshRenderMixedArgs ma{a, sc.mesh, sc.dyn, sc.mcount, t};
        ScopedDevice sd(ctx->device);
        HIPCHK(timed(ctx, "scene_render_mesh_mixed", [&] { return launch_scene_render_mesh_mixed(ma, ctx->stream); }));
        return SDFNMPC_OK;
    }
    if (sc.is_mesh) {  // a mesh set is static: the time does not matter
        const MeshRenderArgs ma{a, sc.mesh};
        ScopedDevice sd(ctx->device);
        HIPCHK(timed(ctx, "scene_render_mesh", [&] { return launch_scene_render_mesh(ma, ctx->stream); }));
        return SDFNMPC_OK;
    }
    if (!sc.dyn) return scene_render_static(ctx, a);
    const SceneRenderDynArgs da{a, sc.dyn, t, sc.mcount};
    ScopedDevice sd(ctx->device);
    if (a.sc.ghdr) {  // a mixed set: the grid plus movers
        HIPCHK(timed(ctx, "scene_render_mixed", [&] { return launch_scene_render_mixed(da, ctx->stream); }));
        return SDFNMPC_OK;
    }
    HIPCHK(timed(ctx, "scene_render_dyn", [&] { return launch_scene_render_dyn(da, ctx->stream); }));
    return SDFNMPC_OK;
}

int sdfn::scene_pose_args(const double* B_p_C, const double* B_R_C, int B, const double* x, double* W_p_Bo,
                          double* W_R_Bo, double* W_p_C, double* W_R_C, ScenePoseArgs& out) {
    if (!B_p_C || !B_R_C) return fail(SDFNMPC_E_ARG, "scene_pose: NULL extrinsics");
    if (B < 0) return fail(SDFNMPC_E_ARG, "scene_pose: B < 0");
    if (B > 0 && (!x || !W_p_Bo || !W_R_Bo || !W_p_C || !W_R_C)) return fail(SDFNMPC_E_ARG, "scene_pose: NULL state or output");
    ScenePoseArgs a{};
    a.B = B; a.x = x;
    for (int i = 0; i < 3; ++i) a.B_p_C[i] = B_p_C[i];
    for (int i = 0; i < 9; ++i) a.B_R_C[i] = B_R_C[i];
    a.W_p_Bo = W_p_Bo; a.W_R_Bo = W_R_Bo; a.W_p_C = W_p_C; a.W_R_C = W_R_C;
    out = a;
    return SDFNMPC_OK;
}

int sdfn::scene_pose_launch(sdfnmpc_ctx* ctx, const ScenePoseArgs& a) {
    ScopedDevice sd(ctx->device);
    HIPCHK(timed(ctx, "scene_pose", [&] { return launch_scene_pose(a, ctx->stream); }));
    return SDFNMPC_OK;
}

extern "C" int sdfnmpc_scene_render(sdfnmpc_ctx* ctx, const sdfnmpc_scene* sc, const int* scene_of,
                                    const sdfnmpc_img_opts* o, int H, int W, float scale, int B, const double* W_p_C,
                                    const double* W_R_C, float* img) {
    SceneRenderArgs a{};
    if (int rc = scene_render_args(ctx, sc, scene_of, o, H, W, scale, B, W_p_C, W_R_C, img, a)) return rc;
    return B == 0 ? SDFNMPC_OK : scene_render_launch(ctx, *sc, a, 0.0);  // a dynamic set at t = 0
}

extern "C" int sdfnmpc_scene_render_at(sdfnmpc_ctx* ctx, const sdfnmpc_scene* sc, const int* scene_of,
                                       const sdfnmpc_img_opts* o, int H, int W, float scale, int B, const double* W_p_C,
                                       const double* W_R_C, double t, float* img) {
    SceneRenderArgs a{};
    if (int rc = scene_render_args(ctx, sc, scene_of, o, H, W, scale, B, W_p_C, W_R_C, img, a)) return rc;
    if (!std::isfinite(t)) return fail(SDFNMPC_E_ARG, "scene_render: the time must be finite");
    return B == 0 ? SDFNMPC_OK : scene_render_launch(ctx, *sc, a, t);
}

extern "C" int sdfnmpc_scene_pose(sdfnmpc_ctx* ctx, const double* B_p_C, const double* B_R_C, int B, const double* x,
                                  double* W_p_Bo, double* W_R_Bo, double* W_p_C, double* W_R_C) {
    if (!ctx) return fail(SDFNMPC_E_ARG, "NULL context");
    ScenePoseArgs a{};
    if (int rc = scene_pose_args(B_p_C, B_R_C, B, x, W_p_Bo, W_R_Bo, W_p_C, W_R_C, a)) return rc;
    return B == 0 ? SDFNMPC_OK : scene_pose_launch(ctx, a);
}

extern "C" int sdfnmpc_scene_distance(sdfnmpc_ctx* ctx, const sdfnmpc_scene* sc, const double* points,
                                      const int* p_to_scene, long long n, double* out) {
    return sdfnmpc_scene_distance_at(ctx, sc, points, p_to_scene, nullptr, n, out);
}

extern "C" int sdfnmpc_scene_distance_at(sdfnmpc_ctx* ctx, const sdfnmpc_scene* sc, const double* points,
                                         const int* p_to_scene, const double* times, long long n, double* out) {
    if (!ctx || !sc) return fail(SDFNMPC_E_ARG, "scene_distance: NULL context or scene");
    if (sc->device != ctx->device) return fail(SDFNMPC_E_ARG, "scene_distance: the scene lives on another device");
    if (n < 0 || n > 2147483647LL) return fail(SDFNMPC_E_ARG, "scene_distance: n out of range");
    if (!p_to_scene && n % sc->S != 0)
        return fail(SDFNMPC_E_ARG, "scene_distance: without p_to_scene the points must divide evenly among the scenes");
    if (n == 0) return SDFNMPC_OK;
    if (!points || !out) return fail(SDFNMPC_E_ARG, "scene_distance: NULL points or output");
    SceneDistArgs a{sc->dev, points, p_to_scene, n, std::max(1LL, n / sc->S), out};
    ScopedDevice sd(ctx->device);
    if (sc->is_inst) {  // an instanced set, at the points' times
        const InstDistArgs ia{a, sc->mesh, sc->inst, times};
        HIPCHK(timed(ctx, "scene_dist_inst", [&] { return launch_scene_distance_inst(ia, ctx->stream); }));
        return SDFNMPC_OK;
    }
    if (sc->is_mesh && sc->dyn) {  // a mesh set with movers, at the points' times
        const MeshDistMixedArgs ma{a, sc->mesh, sc->dyn, sc->mcount, times};
        HIPCHK(timed(ctx, "scene_dist_mesh_mixed", [&] { return launch_scene_distance_mesh_mixed(ma, ctx->stream); }));
        return SDFNMPC_OK;
    }
    if (sc->is_mesh) {  // a mesh set is static: the times do not matter
        const MeshDistArgs ma{a, sc->mesh};
        HIPCHK(timed(ctx, "scene_dist_mesh", [&] { return launch_scene_distance_mesh(ma, ctx->stream); }));
        return SDFNMPC_OK;
    }
    if (a.sc.ghdr && sc->dyn) {  // a mixed set: the grid plus movers at the points' times
        const SceneDistDynArgs da{a, sc->dyn, times, sc->mcount};
        HIPCHK(timed(ctx, "scene_dist_mixed", [&] { return launch_scene_distance_mixed(da, ctx->stream); }));
        return SDFNMPC_OK;
    }
    if (a.sc.ghdr) {  // an indexed set is static: the times do not matter
        HIPCHK(timed(ctx, "scene_dist_grid", [&] { return launch_scene_distance_grid(a, ctx->stream); }));
        return SDFNMPC_OK;
    }
    if (sc->dyn) {
        const SceneDistDynArgs da{a, sc->dyn, times, nullptr};
        HIPCHK(timed(ctx, "scene_dist_dyn", [&] { return launch_scene_distance_dyn(da, ctx->stream); }));
        return SDFNMPC_OK;
    }
    HIPCHK(timed(ctx, "scene_dist", [&] { return launch_scene_distance(a, ctx->stream); }));
    return SDFNMPC_OK;
}

// the minimum of sdfnmpc_scene_distance_at over segments of space-time (scene_swept.hip), dispatched on the handle as
// that function is; a set that is not dynamic does not read the times
extern "C" int sdfnmpc_scene_swept_distance(sdfnmpc_ctx* ctx, const sdfnmpc_scene* sc, const double* p0, const double* p1,
                                            const int* p_to_scene, const double* t0, const double* t1, long long n,
                                            double eps, int max_evals, double* dmin, double* s, double* gap, int* evals) {
    if (!ctx || !sc) return fail(SDFNMPC_E_ARG, "scene_swept_distance: NULL context or scene");
    if (sc->ctx != ctx) return fail(SDFNMPC_E_ARG, "scene_swept_distance: the scene lives on another context");
    if (!p0 || !p1 || !dmin) return fail(SDFNMPC_E_ARG, "scene_swept_distance: NULL p0, p1 or dmin");
    if (n < 0 || n > 2147483647LL) return fail(SDFNMPC_E_ARG, "scene_swept_distance: n out of range");
    if (!p_to_scene && n % sc->S != 0)
        return fail(SDFNMPC_E_ARG,
                    "scene_swept_distance: without p_to_scene the segments must divide evenly among the scenes");
    if ((t0 == nullptr) != (t1 == nullptr))
        return fail(SDFNMPC_E_ARG, "scene_swept_distance: t0 and t1 go together (both NULL: t = 0)");
    if (!std::isfinite(eps) || eps < 1e-6) return fail(SDFNMPC_E_ARG, "scene_swept_distance: eps must be finite and >= 1e-6");
    if (max_evals < 2 || max_evals > 65536) return fail(SDFNMPC_E_ARG, "scene_swept_distance: max_evals must be 2..65536");
    if (n == 0) return SDFNMPC_OK;
    SceneSweptArgs a{};
    a.sc = sc->dev; a.dyn = sc->dyn; a.mcount = sc->mcount; a.vmax = sc->dvmax;
    a.p0 = p0; a.p1 = p1; a.p_to_scene = p_to_scene;
    a.t0 = sc->dyn ? t0 : nullptr; a.t1 = sc->dyn ? t1 : nullptr;
    a.n = n; a.per_scene = std::max(1LL, n / sc->S);
    a.eps = eps; a.max_evals = max_evals;
    a.dmin = dmin; a.s = s; a.gap = gap; a.evals = evals;
    ScopedDevice sd(ctx->device);
    if (sc->is_inst) {  // the times only when some instance moves: a set that is not dynamic does not read them
        a.mesh = sc->mesh;
        a.t0 = sc->inst_moves ? t0 : nullptr; a.t1 = sc->inst_moves ? t1 : nullptr;
        const InstSweptArgs ia{a, sc->inst};
        HIPCHK(timed(ctx, "scene_swept_inst", [&] { return launch_scene_swept_inst(ia, ctx->stream); }));
        return SDFNMPC_OK;
    }
    if (sc->is_mesh && sc->dyn) {
        a.mesh = sc->mesh;
        HIPCHK(timed(ctx, "scene_swept_mesh_mixed", [&] { return launch_scene_swept_mesh_mixed(a, ctx->stream); }));
        return SDFNMPC_OK;
    }
    if (sc->is_mesh) {
        a.mesh = sc->mesh;
        HIPCHK(timed(ctx, "scene_swept_mesh", [&] { return launch_scene_swept_mesh(a, ctx->stream); }));
        return SDFNMPC_OK;
    }
    if (a.sc.ghdr && sc->dyn) {
        HIPCHK(timed(ctx, "scene_swept_mixed", [&] { return launch_scene_swept_mixed(a, ctx->stream); }));
        return SDFNMPC_OK;
    }
    if (a.sc.ghdr) {
        HIPCHK(timed(ctx, "scene_swept_grid", [&] { return launch_scene_swept_grid(a, ctx->stream); }));
        return SDFNMPC_OK;
    }
    if (sc->dyn) {
        HIPCHK(timed(ctx, "scene_swept_dyn", [&] { return launch_scene_swept_dyn(a, ctx->stream); }));
        return SDFNMPC_OK;
    }
    HIPCHK(timed(ctx, "scene_swept", [&] { return launch_scene_swept(a, ctx->stream); }));
    return SDFNMPC_OK;
}

extern "C" int sdfnmpc_scene_speed_bound(const sdfnmpc_scene* sc, double* out) {
    if (!sc || !out) return fail(SDFNMPC_E_ARG, "scene_speed_bound: NULL scene or output");
    std::copy(sc->vmax.begin(), sc->vmax.end(), out);
    return SDFNMPC_OK;
}

// the scene's exact distance as the SDF row (scene_sdf.hip): the option check and the argument block, split from the
// launch as the other scene entry points' are, for the preparation phase (lin_args.sdf_scene) and the solver
int sdfn::scene_sdf_args(sdfnmpc_ctx* ctx, const sdfnmpc_scene_sdf_opts* o, int B, int N, int np, const double* x,
                         const double* p, double* h, double* Jh, SceneSdfArgs& out) {
    if (!ctx || !o || !o->scene) return fail(SDFNMPC_E_ARG, "scene_sdf_rows: NULL context, options or scene");
    if (B < 0 || N < 1 || np < 17) return fail(SDFNMPC_E_ARG, "scene_sdf_rows: B >= 0, N >= 1 and np >= 17 required");
    if (!(o->max_df > 0.0) || !std::isfinite(o->max_df))
        return fail(SDFNMPC_E_ARG, "scene_sdf_rows: max_df must be positive and finite");
    if (!std::isfinite(o->t0)) return fail(SDFNMPC_E_ARG, "scene_sdf_rows: the time t0 must be finite");
    if (o->scene->ctx != ctx) return fail(SDFNMPC_E_ARG, "scene_sdf_rows: the scene lives on another context");
    if (o->scene->is_mesh && !o->scene->sdf_source)  // a mesh set is a source only when it was created as one
        return fail(SDFNMPC_E_UNSUPPORTED, "scene_sdf_rows: a mesh set cannot be the SDF source (meshes are rendered and "
                                           "measured, not linearised)");
    if (o->scene->is_inst && !o->scene->sdf_source)
        return fail(SDFNMPC_E_UNSUPPORTED, "scene_sdf_rows: an instanced set created with sdf_source = 0 cannot be the "
                                           "SDF source");
    if (B > 0 && (!x || !p || !h || !Jh)) return fail(SDFNMPC_E_ARG, "scene_sdf_rows: NULL x, p, h or Jh");
    SceneSdfArgs a{};
    a.sc = o->scene->dev; a.dyn = o->scene->dyn; a.mcount = o->scene->mcount; a.scene_of = o->scene_of;
    a.rows = (long long)B * (N + 1); a.N1 = N + 1; a.np = np;
    a.x = x; a.p = p; a.h = h; a.Jh = Jh;
    a.max_df = o->max_df; a.t0 = o->t0; a.tau = o->tau;
    if (o->scene->is_mesh || o->scene->is_inst) a.mesh = o->scene->mesh;
    out = a;
    return SDFNMPC_OK;
}

extern "C" int sdfnmpc_scene_sdf_rows(sdfnmpc_ctx* ctx, const sdfnmpc_scene_sdf_opts* o, int B, int N, int np,
                                      const double* x, const double* p, double* h, double* Jh) {
    SceneSdfArgs a{};
    if (int rc = scene_sdf_args(ctx, o, B, N, np, x, p, h, Jh, a)) return rc;
    if (B == 0) return SDFNMPC_OK;
    ScopedDevice sd(ctx->device);
    HIPCHK(scene_sdf_rows_enqueue(ctx, a, o->scene));
    return SDFNMPC_OK;
}

// ------------------------------------------------------------------------------------------------
// image morphology (morph.hip) and the sensor-degradation stage (sensor.hip)
static int image_batch_check(const char* who, int B, int H, int W) {
    const std::string w(who);
    if (B < 0 || B > 65535) return fail(SDFNMPC_E_ARG, w + ": B must be 0..65535");
    if (H < 1 || W < 1) return fail(SDFNMPC_E_ARG, w + ": bad image size");
    if ((long long)H * W > 2147483647LL || (long long)B * H * W > 2147483647LL)
        return fail(SDFNMPC_E_ARG, w + ": more than 2^31 - 1 pixels");
    return SDFNMPC_OK;
}

static int morph_args(int op, const unsigned char* kernel, int k_h, int k_w, int ignore_zeros, const float* in, int B,
                      int H, int W, float* out, MorphArgs* a) {
    if (op != MORPH_DILATE && op != MORPH_ERODE) return fail(SDFNMPC_E_ARG, "morph: op must be 0 (dilate) or 1 (erode)");
    if (!kernel) return fail(SDFNMPC_E_ARG, "morph: NULL structuring element");
    if (k_h < 1 || k_h > MORPH_K_MAX || k_w < 1 || k_w > MORPH_K_MAX)
        return fail(SDFNMPC_E_ARG, "morph: the structuring element must be 1..21 x 1..21");
    if (int rc = image_batch_check("morph", B, H, W)) return rc;
    if (B > 0 && (!in || !out)) return fail(SDFNMPC_E_ARG, "morph: NULL image");
    if (B > 0 && in == out) return fail(SDFNMPC_E_ARG, "morph: in and out must differ");
    a->in = in; a->out = out; a->B = B; a->H = H; a->W = W;
    a->k_h = k_h; a->k_w = k_w; a->oh = k_h / 2; a->ow = k_w / 2;
    a->op = op; a->ignore_zeros = ignore_zeros != 0;
    a->border = op == MORPH_DILATE ? -2.f : 2.f;
    if (morph_build_taps(op, kernel, k_h, k_w, &a->taps) < 1)
        return fail(SDFNMPC_E_ARG, "morph: the structuring element has no 1");
    return SDFNMPC_OK;
}

extern "C" int sdfnmpc_morph(sdfnmpc_ctx* ctx, int op, const unsigned char* kernel, int k_h, int k_w, int ignore_zeros,
                             const float* in, int B, int H, int W, float* out) {
    if (!ctx) return fail(SDFNMPC_E_ARG, "morph: NULL context");
    MorphArgs a{};
    if (int rc = morph_args(op, kernel, k_h, k_w, ignore_zeros, in, B, H, W, out, &a)) return rc;
    if (B == 0) return SDFNMPC_OK;
    ScopedDevice sd(ctx->device);
    HIPCHK(timed(ctx, "morph", [&] { return launch_morph(a, ctx->stream); }));
    return SDFNMPC_OK;
}

// the fused launch's option check, split from the launch as the scene kernels' are (the rollout repeats the launch)
static int outlier_args(float min_range, const float* in, int B, int H, int W, float* out, OutlierArgs* a) {
    if (int rc = image_batch_check("outlier_rm", B, H, W)) return rc;
    if (!std::isfinite(min_range)) return fail(SDFNMPC_E_ARG, "outlier_rm: min_range must be finite");
    if (B > 0 && (!in || !out)) return fail(SDFNMPC_E_ARG, "outlier_rm: NULL image");
    if (B > 0 && in == out) return fail(SDFNMPC_E_ARG, "outlier_rm: in and out must differ");
    *a = OutlierArgs{in, out, B, H, W, min_range};
    return SDFNMPC_OK;
}

extern "C" int sdfnmpc_outlier_rm(sdfnmpc_ctx* ctx, int kernel_size, float min_range, const float* in, int B, int H,
                                  int W, float* out) {
    if (!ctx) return fail(SDFNMPC_E_ARG, "outlier_rm: NULL context");
    if (kernel_size < 1 || kernel_size > MORPH_K_MAX) return fail(SDFNMPC_E_ARG, "outlier_rm: kernel_size must be 1..21");
    OutlierArgs oa{};
    if (int rc = outlier_args(min_range, in, B, H, W, out, &oa)) return rc;
    if (B == 0) return SDFNMPC_OK;
    ScopedDevice sd(ctx->device);
    if (kernel_size == 3) {
        HIPCHK(timed(ctx, "outlier_rm", [&] { return launch_outlier_rm(oa, ctx->stream); }));
        return SDFNMPC_OK;
    }
    // threshold -> t; erode t -> e; dilate e -> out; out = out > 0 ? t : out
    const long long n = (long long)B * H * W;
    HIPCHK(ctx->morph_t.ensure((size_t)n * sizeof(float)));
    HIPCHK(ctx->morph_e.ensure((size_t)n * sizeof(float)));
    float *t = (float*)ctx->morph_t.p, *e = (float*)ctx->morph_e.p;
    unsigned char ones[MORPH_K_MAX * MORPH_K_MAX];
    memset(ones, 1, sizeof(ones));
    MorphArgs er{}, di{};
    if (int rc = morph_args(MORPH_ERODE, ones, kernel_size, kernel_size, 0, t, B, H, W, e, &er)) return rc;
    if (int rc = morph_args(MORPH_DILATE, ones, kernel_size, kernel_size, 0, e, B, H, W, out, &di)) return rc;
    HIPCHK(timed(ctx, "morph_threshold", [&] { return launch_morph_threshold(in, t, n, min_range, ctx->stream); }));
    HIPCHK(timed(ctx, "morph", [&] { return launch_morph(er, ctx->stream); }));
    HIPCHK(timed(ctx, "morph", [&] { return launch_morph(di, ctx->stream); }));
    HIPCHK(timed(ctx, "morph_restore", [&] { return launch_morph_restore(out, t, n, ctx->stream); }));
    return SDFNMPC_OK;
}

// sdfnmpc_sensor_apply in two halves (solver.hip repeats the second inside a rollout): sensor_args refuses or fills the
// two kernels' argument blocks, sensor_launch enqueues them for a frame
int sdfn::sensor_args(const sdfnmpc_sensor_opts* o, float* img, int B, int H, int W, float* scratch, SensorArgs& sa,
                      OutlierArgs& oa) {
    if (!o) return fail(SDFNMPC_E_ARG, "sensor: NULL options");
    if (int rc = image_batch_check("sensor", B, H, W)) return rc;
    if (!(std::isfinite(o->a) && o->a >= 0.f && std::isfinite(o->b) && o->b >= 0.f))
        return fail(SDFNMPC_E_ARG, "sensor: a and b must be finite and not negative");
    if (!(o->vmax > 0.f && std::isfinite(o->vmax))) return fail(SDFNMPC_E_ARG, "sensor: vmax must be positive and finite");
    if (o->boxes && (o->n_frames < 1 || o->max_boxes < 0 || o->max_boxes > SENSOR_MAX_BOXES))
        return fail(SDFNMPC_E_ARG, "sensor: a box table needs n_frames >= 1 and max_boxes in 0..8");
    if (B > 0 && !img) return fail(SDFNMPC_E_ARG, "sensor: NULL image");
    if (o->outlier_rm) {
        if (B > 0 && !scratch) return fail(SDFNMPC_E_ARG, "sensor: outlier_rm needs the scratch image");
        if (int rc = outlier_args(o->min_range, img, B, H, W, scratch, &oa)) return rc;
    }
    SensorArgs a{};
    a.img = img; a.B = B; a.H = H; a.W = W;
    a.key0 = (unsigned)(o->seed & 0xffffffffull); a.key1 = (unsigned)(o->seed >> 32);
    a.a = o->a; a.b = o->b; a.vmax = o->vmax; a.p_thresh = o->p_thresh; a.miss_invalid = o->miss_invalid != 0;
    a.boxes = (o->boxes && o->max_boxes > 0) ? o->boxes : nullptr;
    a.n_frames = o->n_frames; a.max_boxes = o->max_boxes; a.stream_id = o->stream_id;
    sa = a;
    return SDFNMPC_OK;
}

int sdfn::sensor_launch(sdfnmpc_ctx* ctx, const SensorArgs& sa, const OutlierArgs& oa, int outlier_rm, int frame) {
    if (sa.B == 0) return SDFNMPC_OK;
    SensorArgs a = sa;
    a.frame = (unsigned)frame;
    ScopedDevice sd(ctx->device);
    HIPCHK(timed(ctx, "sensor_degrade", [&] { return launch_sensor_degrade(a, ctx->stream); }));
    if (outlier_rm) {
        HIPCHK(timed(ctx, "outlier_rm", [&] { return launch_outlier_rm(oa, ctx->stream); }));
        HIPCHK(hipMemcpyAsync(a.img, oa.out, (size_t)a.B * a.H * a.W * sizeof(float), hipMemcpyDeviceToDevice, ctx->stream));
    }
    return SDFNMPC_OK;
}

extern "C" int sdfnmpc_sensor_apply(sdfnmpc_ctx* ctx, const sdfnmpc_sensor_opts* o, int frame, float* img, int B, int H,
                                    int W, float* scratch) {
    if (!ctx) return fail(SDFNMPC_E_ARG, "sensor: NULL context");
    SensorArgs sa{};
    OutlierArgs oa{};
    if (int rc = sensor_args(o, img, B, H, W, scratch, sa, oa)) return rc;
    if (frame < 0) return fail(SDFNMPC_E_ARG, "sensor: frame must be >= 0");
    return sensor_launch(ctx, sa, oa, o->outlier_rm != 0, frame);
}
