// sdfnmpc_solver: the device-resident SQP-RTI solver object of include/sdfnmpc.h.
//
// It owns everything one batched control step touches -- iterate, parameters, references, the
// preparation-phase outputs, QP results -- on one context (device + stream), so a controller drives
// it with host arrays and no tensor framework: the counterpart of the AcadosOcpSolver object that
// sdf_nmpc/ocp.py:127 builds (solver.set / cost_set / get / solve_for_x0 / reset), batched over B
// instances.  The compute is the lower-level entry points (sdfnmpc_rti_prepare, sdfnmpc_qp_feedback,
// sdfnmpc_rti_apply); this file adds buffer ownership, masked row uploads through a pinned staging
// arena, and the asynchronous step / wait split that lets one host thread keep several devices busy.
#include <cmath>
#include <cstring>

#include "engine.h"
#include "ref_kernels.h"

using namespace sdfn;

namespace {

// rows r of a [rows][width] field receive staged[r'][0..ncol) at columns col0.. (r = idx[r'])
__global__ __launch_bounds__(256) void scatter_rows_kernel(double* dst, int width, int col0, int ncol,
                                                           const double* staged, const int* idx, int n_rows) {
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= (long long)n_rows * ncol) return;
    const int r = (int)(i / ncol), c = (int)(i - (long long)r * ncol);
    dst[(long long)idx[r] * width + col0 + c] = staged[i];
}

// x_{i-k} = x_i, u_{i-k} = u_i for i = k..N-1 (ocp.py:152-156): one thread per (instance, column), nodes in
// ascending order, so the overlapping rows are read before they are overwritten
__global__ __launch_bounds__(256) void shift_kernel(int B, int N, int k, double* x, double* u) {
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= (long long)B * 14) return;
    const long long b = i / 14;
    const int j = (int)(i - b * 14);
    if (j < 10) {
        double* xb = x + b * (N + 1) * 10 + j;
        for (int n = k; n < N; ++n) xb[(n - k) * 10] = xb[n * 10];
    } else {
        double* ub = u + b * N * 4 + (j - 10);
        for (int n = k; n < N; ++n) ub[(n - k) * 4] = ub[n * 4];
    }
}

// x[b][k] = x0[b] (k = 0..N), u[b][k] = u_init (k < N)
__global__ __launch_bounds__(256) void init_iterate_kernel(int B, int N, double* x, double* u, const double* x0,
                                                           double u0, double u1, double u2, double u3) {
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    const long long nx = (long long)B * (N + 1) * 10, nu = (long long)B * N * 4;
    if (i < nx) {
        const long long b = i / ((N + 1) * 10), e = i % 10;
        x[i] = x0[b * 10 + e];
    }
    if (i < nu) {
        const int e = (int)(i & 3);
        u[i] = e == 0 ? u0 : e == 1 ? u1 : e == 2 ? u2 : u3;
    }
}

struct Field {
    const char* name;
    void* dev;
    int nodes, width, elem;  // [B][nodes][width] of elem-byte values
};

}  // namespace

struct sdfnmpc_solver {
    sdfnmpc_ctx* ctx = nullptr;
    const sdfnmpc_net* net = nullptr;
    int device = 0;
    hipStream_t stream = nullptr;
    int B = 0, N = 0, np = 0, ny = 0, nyN = 4, latent_mode = 0;
    bool no_sdf = false;  // no constraint row or cost reads the network
    // the SDF source: a scene's exact distance instead of the network (sdfnmpc_solver_set_sdf_scene); sdf_src.scene ==
    // NULL is the network.  tau: the node times of `predict`, built once from the solver's own dt grid
    sdfnmpc_scene_sdf_opts sdf_src{};
    double* tau = nullptr;
    std::vector<double> h_dt;
    // or the field of a camera image (sdfnmpc_solver_set_sdf_image): a copy of the caller's option block, its pointers
    // the caller's.  At most one of the two sources is set.
    sdfnmpc_img_sdf_opts img_src{};
    bool has_img = false;
    sdfnmpc_quad_model model{};
    sdfnmpc_qp_opts qp{};
    std::vector<void*> allocs;
    double *x = nullptr, *u = nullptr, *p = nullptr, *x0 = nullptr, *yref = nullptr, *W = nullptr, *yNref = nullptr,
           *WN = nullptr, *dt = nullptr, *xn = nullptr, *AB = nullptr, *y = nullptr, *Jy = nullptr, *yN = nullptr,
           *JyN = nullptr, *h = nullptr, *Jh = nullptr, *dx = nullptr, *du = nullptr, *res = nullptr, *u0 = nullptr,
           *slack = nullptr, *hE = nullptr, *JhE = nullptr;
    int *status = nullptr, *iters = nullptr;
    // pinned host memory: step outputs and the upload staging arena (reset after every wait)
    double* h_u0 = nullptr;
    int *h_status = nullptr, *h_iters = nullptr;
    char* arena = nullptr;   // pinned host staging
    char* d_arena = nullptr; // its device twin (same offsets): staged rows land here before the scatter
    size_t arena_bytes = 0, arena_used = 0;
    bool pending = false;
    std::vector<Field> fields;

    ~sdfnmpc_solver() {
        int prev = -1;
        (void)hipGetDevice(&prev);
        (void)hipSetDevice(device);
        (void)hipStreamSynchronize(stream);
        for (void* a : allocs) (void)hipFree(a);
        if (d_arena) (void)hipFree(d_arena);
        if (h_u0) (void)hipHostFree(h_u0);  // [u0 | status | iters] in one pinned block
        if (arena) (void)hipHostFree(arena);
        if (prev >= 0) (void)hipSetDevice(prev);
    }

    template <typename T>
    hipError_t alloc(T** out, size_t n) {
        void* q = nullptr;
        hipError_t e = hipMalloc(&q, n * sizeof(T) + 16);
        if (e != hipSuccess) return e;
        allocs.push_back(q);
        e = hipMemsetAsync(q, 0, n * sizeof(T), stream);
        *out = (T*)q;
        return e;
    }
    const Field* field(const char* name) const {
        for (const Field& f : fields)
            if (!strcmp(f.name, name)) return &f;
        return nullptr;
    }
    // n bytes of pinned staging (host pointer *out, device twin *dout), 16-byte aligned; when full the
    // stream is drained (every copy out of the arena has completed) and the arena reused or grown
    hipError_t stage(size_t n, char** out, char** dout = nullptr) {
        n = (n + 15) & ~(size_t)15;
        if (arena_used + n > arena_bytes) {
            hipError_t e = hipStreamSynchronize(stream);
            if (e != hipSuccess) return e;
            arena_used = 0;
            if (n > arena_bytes) {
                if (arena) (void)hipHostFree(arena);
                if (d_arena) (void)hipFree(d_arena);
                arena = d_arena = nullptr;
                arena_bytes = 0;
                const size_t want = n > (1u << 20) ? 2 * n : (1u << 20);
                e = hipHostMalloc((void**)&arena, want, hipHostMallocDefault);
                if (e == hipSuccess) e = hipMalloc((void**)&d_arena, want);
                if (e != hipSuccess) return e;
                arena_bytes = want;
            }
        }
        *out = arena + arena_used;
        if (dout) *dout = d_arena + arena_used;
        arena_used += n;
        return hipSuccess;
    }
};

extern "C" int sdfnmpc_solver_create(sdfnmpc_ctx* ctx, const sdfnmpc_net* net, const sdfnmpc_solver_opts* o,
                                     sdfnmpc_solver** out) {
    if (!ctx || !o || !out) return fail(SDFNMPC_E_ARG, "NULL argument to sdfnmpc_solver_create");
    *out = nullptr;
    if (o->B < 1 || o->N < 1 || o->np < 17 || (o->ny != 11 && o->ny != 12) || !o->dt ||
        (o->latent_mode != 0 && o->latent_mode != 1) || o->qp.ny != o->ny)
        return fail(SDFNMPC_E_ARG, "solver opts: B, N >= 1, np >= 17, ny in {11, 12} == qp.ny, dt required");
    if (o->qp.nyN != 4 && o->qp.nyN != 5)
        return fail(SDFNMPC_E_ARG, "solver opts: qp.nyN must be 4 or 5");
    // the model kinds the preparation phase is built for (sdfnmpc_quad_model.kind), refused here and not at the first step
    if (o->model.kind != SDFNMPC_MODEL_ATT && o->model.kind != SDFNMPC_MODEL_ATT_TAU)
        return fail(SDFNMPC_E_UNSUPPORTED, "solver opts: model.kind: only 0 ('att') and 1 ('att_tau') are built");
    if (o->model.kind == SDFNMPC_MODEL_ATT_TAU && (o->model.rec_feas || o->model.stability))
        return fail(SDFNMPC_E_UNSUPPORTED, "solver opts: model.kind 1 ('att_tau') with rec_feas / stability");
    bool need_sdf = o->ny == 12;  // the constraint set or the cost reads the network
    for (int j = 0; j < o->qp.nh && j < 3; ++j) need_sdf = need_sdf || o->qp.h_col[j] == 2;
    for (int j = 0; j < o->qp.nhN && j < SDFNMPC_NHN_MAX; ++j) need_sdf = need_sdf || o->qp.hN_col[j] == 2;
    if (need_sdf && !net)
        return fail(SDFNMPC_E_ARG, "solver: the constraint set / cost reads the SDF but the network is NULL");
    if (net && o->np < 17 + sdfnmpc_net_size_latent(net))  // the stage parameters end with the network's latent
        return fail(SDFNMPC_E_ARG, "solver opts: np = " + std::to_string(o->np) + " < 17 + latent size " +
                                       std::to_string(sdfnmpc_net_size_latent(net)) + " of this network");
    auto* s = new sdfnmpc_solver();
    s->ctx = ctx;
    s->net = net;
    s->device = sdfnmpc_ctx_device(ctx);
    s->stream = (hipStream_t)sdfnmpc_ctx_stream(ctx);
    s->B = o->B; s->N = o->N; s->np = o->np; s->ny = o->ny; s->latent_mode = o->latent_mode;
    s->nyN = o->qp.nyN;
    s->no_sdf = !need_sdf;
    s->model = o->model;
    s->qp = o->qp;
    s->h_dt.assign(o->dt, o->dt + o->N);
    ScopedDevice sd(s->device);
    const size_t B = o->B, N = o->N, N1 = N + 1;
    hipError_t e = hipSuccess;
    auto A = [&](auto** p, size_t n) { if (e == hipSuccess) e = s->alloc(p, n); };
    A(&s->x, B * N1 * 10); A(&s->u, B * N * 4); A(&s->p, B * N1 * o->np); A(&s->x0, B * 10);
    const size_t nyN = s->nyN;
    A(&s->yref, B * N * o->ny); A(&s->W, B * N * o->ny); A(&s->yNref, B * nyN); A(&s->WN, B * nyN); A(&s->dt, N);
    A(&s->xn, B * N * 10); A(&s->AB, B * N * 140); A(&s->y, B * N * 11); A(&s->Jy, B * N * 154); A(&s->yN, B * nyN);
    A(&s->JyN, B * 10 * nyN); A(&s->h, B * N1 * 3); A(&s->Jh, B * N1 * 30); A(&s->dx, B * N1 * 10); A(&s->du, B * N * 4);
    A(&s->res, B * 2); A(&s->slack, B * N1 * 6); A(&s->hE, B * 6); A(&s->JhE, B * 60);
    // [u0 (B x 4 doubles) | status (B ints) | iters (B ints)] contiguous on both sides: one copy back per step
    A(&s->u0, B * 5);
    if (e == hipSuccess) {
        s->status = (int*)(s->u0 + B * 4);
        s->iters = s->status + B;
        e = hipHostMalloc((void**)&s->h_u0, B * 5 * sizeof(double), hipHostMallocDefault);
    }
    if (e == hipSuccess) {
        s->h_status = (int*)(s->h_u0 + B * 4);
        s->h_iters = s->h_status + B;
    }
    if (e == hipSuccess) e = hipMemcpyAsync(s->dt, o->dt, N * sizeof(double), hipMemcpyHostToDevice, s->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(s->stream);
    if (e != hipSuccess) {
        delete s;
        return fail(SDFNMPC_E_HIP, std::string("solver buffers: ") + hipGetErrorString(e));
    }
    const int n = (int)N, n1 = (int)N1, d = 8, w = (int)nyN;
    s->fields = {{"x", s->x, n1, 10, d},       {"u", s->u, n, 4, d},          {"p", s->p, n1, o->np, d},
                 {"x0", s->x0, 1, 10, d},      {"yref", s->yref, n, o->ny, d}, {"W", s->W, n, o->ny, d},
                 {"yNref", s->yNref, 1, w, d}, {"WN", s->WN, 1, w, d},         {"u0", s->u0, 1, 4, d},
                 {"dx", s->dx, n1, 10, d},     {"du", s->du, n, 4, d},         {"xn", s->xn, n, 10, d},
                 {"AB", s->AB, n, 140, d},     {"y", s->y, n, 11, d},          {"Jy", s->Jy, n, 154, d},
                 {"yN", s->yN, 1, w, d},       {"JyN", s->JyN, 1, 10 * w, d},  {"h", s->h, n1, 3, d},
                 {"Jh", s->Jh, n1, 30, d},     {"hE", s->hE, 1, 6, d},         {"JhE", s->JhE, 1, 60, d},
                 {"res", s->res, 1, 2, d},     {"slack", s->slack, n1, 6, d},  {"status", s->status, 1, 1, 4},
                 {"iters", s->iters, 1, 1, 4}};
    *out = s;
    return SDFNMPC_OK;
}

extern "C" void sdfnmpc_solver_destroy(sdfnmpc_solver* s) { delete s; }

extern "C" int sdfnmpc_solver_field(sdfnmpc_solver* s, const char* name, void** dev, int* nodes, int* width) {
    if (!s || !name) return fail(SDFNMPC_E_ARG, "NULL argument to sdfnmpc_solver_field");
    const Field* f = s->field(name);
    if (!f) return fail(SDFNMPC_E_ARG, std::string("no solver field ") + name);
    if (dev) *dev = f->dev;
    if (nodes) *nodes = f->nodes;
    if (width) *width = f->width;
    return SDFNMPC_OK;
}

extern "C" int sdfnmpc_solver_upload(sdfnmpc_solver* s, const char* name, int col0, int ncol, const unsigned char* mask,
                                     const double* host) {
    if (!s || !name || !host) return fail(SDFNMPC_E_ARG, "NULL argument to sdfnmpc_solver_upload");
    const Field* f = s->field(name);
    if (!f || f->elem != 8) return fail(SDFNMPC_E_ARG, std::string("no fp64 solver field ") + name);
    if (col0 < 0 || ncol < 1 || col0 + ncol > f->width) return fail(SDFNMPC_E_ARG, "upload columns out of range");
    ScopedDevice sd(s->device);
    const int rows = s->B * f->nodes;
    if (!mask && col0 == 0 && ncol == f->width) {  // the whole field: one staged copy
        char* st = nullptr;
        const size_t bytes = (size_t)rows * f->width * 8;
        HIPCHK(s->stage(bytes, &st));
        memcpy(st, host, bytes);
        HIPCHK(hipMemcpyAsync(f->dev, st, bytes, hipMemcpyHostToDevice, s->stream));
        return SDFNMPC_OK;
    }
    int n_rows = 0;
    for (int r = 0; r < rows; ++r) n_rows += (!mask || mask[r]) ? 1 : 0;
    if (n_rows == 0) return SDFNMPC_OK;
    // values and row indices in ONE reservation: a second stage() call could drain and reset the arena
    // and hand out a block overlapping the first
    char *vals = nullptr, *dvals = nullptr;
    const size_t vbytes = ((size_t)n_rows * ncol * 8 + 15) & ~(size_t)15;
    HIPCHK(s->stage(vbytes + (size_t)n_rows * 4, &vals, &dvals));
    char *idx = vals + vbytes, *didx = dvals + vbytes;
    double* v = (double*)vals;
    int* ix = (int*)idx;
    for (int r = 0, q = 0; r < rows; ++r)
        if (!mask || mask[r]) {
            memcpy(v + (size_t)q * ncol, host + (size_t)r * f->width + col0, (size_t)ncol * 8);
            ix[q++] = r;
        }
    HIPCHK(hipMemcpyAsync(dvals, vals, (size_t)n_rows * ncol * 8, hipMemcpyHostToDevice, s->stream));
    HIPCHK(hipMemcpyAsync(didx, idx, (size_t)n_rows * 4, hipMemcpyHostToDevice, s->stream));
    const long long n = (long long)n_rows * ncol;
    hipLaunchKernelGGL(scatter_rows_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s->stream, (double*)f->dev,
                       f->width, col0, ncol, (const double*)dvals, (const int*)didx, n_rows);
    HIPCHK(hipGetLastError());
    return SDFNMPC_OK;
}

extern "C" int sdfnmpc_solver_download(sdfnmpc_solver* s, const char* name, void* host) {
    if (!s || !name || !host) return fail(SDFNMPC_E_ARG, "NULL argument to sdfnmpc_solver_download");
    const Field* f = s->field(name);
    if (!f) return fail(SDFNMPC_E_ARG, std::string("no solver field ") + name);
    ScopedDevice sd(s->device);
    HIPCHK(hipMemcpyAsync(host, f->dev, (size_t)s->B * f->nodes * f->width * f->elem, hipMemcpyDeviceToHost, s->stream));
    HIPCHK(hipStreamSynchronize(s->stream));
    return SDFNMPC_OK;
}

extern "C" int sdfnmpc_solver_init(sdfnmpc_solver* s, const double* x0, const double* u_init) {
    if (!s || !x0 || !u_init) return fail(SDFNMPC_E_ARG, "NULL argument to sdfnmpc_solver_init");
    ScopedDevice sd(s->device);
    int rc = sdfnmpc_solver_upload(s, "x0", 0, 10, nullptr, x0);
    if (rc) return rc;
    const long long n = (long long)s->B * (s->N + 1) * 10;
    hipLaunchKernelGGL(init_iterate_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s->stream, s->B, s->N, s->x,
                       s->u, (const double*)s->x0, u_init[0], u_init[1], u_init[2], u_init[3]);
    HIPCHK(hipGetLastError());
    HIPCHK(hipMemsetAsync(s->dx, 0, (size_t)s->B * (s->N + 1) * 10 * 8, s->stream));
    HIPCHK(hipMemsetAsync(s->du, 0, (size_t)s->B * s->N * 4 * 8, s->stream));
    return SDFNMPC_OK;
}

extern "C" int sdfnmpc_solver_shift(sdfnmpc_solver* s, int k) {
    if (!s) return fail(SDFNMPC_E_ARG, "NULL solver");
    if (k <= 0 || k >= s->N) return SDFNMPC_OK;  // ocp.py:153: k > 0 shifts nodes k..N-1 down by k
    ScopedDevice sd(s->device);
    // one launch (it was four strided copies through a scratch buffer: launch latency on the C1 path)
    const long long n = (long long)s->B * 14;
    hipLaunchKernelGGL(shift_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s->stream, s->B, s->N, k, s->x,
                       s->u);
    HIPCHK(hipGetLastError());
    return SDFNMPC_OK;
}

// one SQP-RTI iteration on the solver's buffers, enqueued; u0 / status / iters stay on the device
static int step_enqueue(sdfnmpc_solver* s) {
    const size_t n1 = s->N + 1;
    // x_0 of the iterate = the measured state (Ocp.solve: solver.set(0, 'x', x0), ocp.py:161)
    HIPCHK(hipMemcpy2DAsync(s->x, n1 * 80, s->x0, 80, 80, s->B, hipMemcpyDeviceToDevice, s->stream));
    sdfnmpc_lin_args la{};
    la.B = s->B; la.N = s->N; la.np = s->np; la.latent_mode = s->latent_mode;
    la.x = s->x; la.u = s->u; la.p = s->p; la.dt = s->dt;
    la.xn = s->xn; la.AB = s->AB; la.y = s->y; la.Jy = s->Jy; la.yN = s->yN; la.JyN = s->JyN; la.h = s->h; la.Jh = s->Jh;
    la.nyN = s->nyN; la.no_sdf = s->no_sdf ? 1 : 0; la.hE = s->hE; la.JhE = s->JhE;
    if (s->sdf_src.scene) la.sdf_scene = &s->sdf_src;  // t0: the solver's scene time (sdfnmpc_solver_set_scene_time)
    if (s->has_img) la.sdf_image = &s->img_src;
    sdfnmpc_qp_args qa{};
    qa.B = s->B; qa.N = s->N;
    qa.xn = s->xn; qa.AB = s->AB; qa.y = s->y; qa.Jy = s->Jy; qa.yN = s->yN; qa.JyN = s->JyN; qa.h = s->h; qa.Jh = s->Jh;
    qa.hE = s->hE; qa.JhE = s->JhE;
    qa.x = s->x; qa.u = s->u; qa.x0 = s->x0; qa.yref = s->yref; qa.W = s->W; qa.yNref = s->yNref; qa.WN = s->WN;
    qa.dt = s->dt; qa.dx = s->dx; qa.du = s->du; qa.slack = s->slack; qa.status = s->status; qa.iters = s->iters;
    qa.res = s->res;
    int rc = sdfnmpc_rti_prepare(s->ctx, s->net, &s->model, &la, &s->qp, &qa);  // preparation (+ stage records)
    if (rc) return rc;
    rc = sdfnmpc_qp_feedback(s->ctx, &s->qp, &qa);                             // feedback
    if (rc) return rc;
    rc = sdfnmpc_rti_apply(s->ctx, s->B, s->N, s->x, s->u, s->dx, s->du, s->u0, s->status);
    return rc;
}

extern "C" int sdfnmpc_solver_step(sdfnmpc_solver* s) {
    if (!s) return fail(SDFNMPC_E_ARG, "NULL solver");
    ScopedDevice sd(s->device);
    if (int rc = step_enqueue(s)) return rc;
    HIPCHK(hipMemcpyAsync(s->h_u0, s->u0, (size_t)s->B * 40, hipMemcpyDeviceToHost, s->stream));  // u0, status, iters
    s->pending = true;
    return SDFNMPC_OK;
}

// The vehicle model of a rollout (sdfnmpc_rollout_args.vehicle).  on: the plant call of every step is the vehicle's,
// on its own true state, and x0 receives the estimate.  neutral: a model with everything off -- the plant runs on x0
// as without a vehicle, and the end of the rollout copies the logs and the final state the vehicle would have written.
struct VehicleRun {
    bool on = false, neutral = false, body = false;
    sdfn::VehicleArgs va{};
    double *x_true = nullptr, *scratch = nullptr;
};

// What a rollout does around the bare step [ref pack, shift, step, plant], as data: every flavour of rollout fills one
// plan and rollout_run is the only loop.  Before step k with (k + phase) % every == 0 the stages that are switched on
// run in the order they are declared in, the pack always last:
//   flavour (entry point)             scene clock  pose     render into    sensor  encode  decode  pool      pack
//   plain (perc == NULL)              -            -        -              -       -       -       -         -
//   latent (_perceive_sensor)         -            vehicle  camera buffer  if set  yes     -       -         mode -1
//   scene source (_scene_sdf)         every step   x0       -              -       -       -       -         mode -2
//   image source (_image_sdf)         -            vehicle  the source     if set  -       -       unsigned  mode -2
//   reconstruction (_image_recon)     -            vehicle  camera buffer  if set  yes     source  unsigned  mode -2
struct RolloutPlan {
    // every step (rollout_args): the plant's block, the reference pack when args->ref is set, the vehicle
    sdfn::PlantArgs pa{};
    sdfnmpc_ref_args ra{};
    VehicleRun vr{};
    // schedule and clock: step k happens at t = t0 + (phase + k) dt; every == 0: no stage ever runs
    int every = 0, phase = 0;
    double t0 = 0.0, dt = 0.0;
    bool scene_clock = false;  // the solver's own scene time (sdf_src.t0) is set to t before every step, and stays
    // pose: one launch from x0 (the estimate, also under a vehicle), or rollout_pose (camera from the true state)
    enum { POSE_NONE, POSE_X0, POSE_VEHICLE } pose = POSE_NONE;
    sdfn::ScenePoseArgs spa{};
    // render at t into sra's image, when scene is set
    const sdfnmpc_scene* scene = nullptr;
    sdfn::SceneRenderArgs sra{};
    // sensor on that image as frame phase + k, when sensor is set
    const sdfnmpc_sensor_opts* sensor = nullptr;
    sdfn::SensorArgs sna{};
    sdfn::OutlierArgs ora{};
    // encode cam into latent / latent64, when vae is set
    sdfnmpc_vae* vae = nullptr;
    sdfnmpc_vae_opts vo{};
    const float* cam = nullptr;
    float* latent = nullptr;
    double* latent64 = nullptr;
    // decode latent into the image source's images when dec is set; min-pool the source when pool is
    sdfnmpc_vae_dec* dec = nullptr;
    const sdfnmpc_img_sdf_opts* src = nullptr;
    bool pool = false;
    // pack the pose (mode -2), or the latent and the pose (mode -1), into p
    sdfnmpc_ref_opts po{};
    sdfnmpc_ref_args pra{};
};

static int rollout_clock(double t0, double dt) {
    if (!std::isfinite(t0) || !std::isfinite(dt) || dt < 0.0)
        return fail(SDFNMPC_E_ARG, "rollout: the scene clock needs a finite t0 and a finite dt >= 0");
    return SDFNMPC_OK;
}

static int rollout_schedule(int every, int phase) {
    if (every < 1 || phase < 0)
        return fail(SDFNMPC_E_ARG, "rollout: perceive needs every >= 1 and phase >= 0");
    return SDFNMPC_OK;
}

// what every rollout refuses before its first launch: the step count and logs, the plant's options (pl.pa is filled),
// then what sdfnmpc_pack_refs would refuse (pl.ra is filled when args->ref is set)
static int rollout_args(sdfnmpc_solver* s, const sdfnmpc_rollout_args* a, RolloutPlan& pl) {
    sdfn::PlantArgs& pa = pl.pa;
    sdfnmpc_ref_args& ra = pl.ra;
    VehicleRun& vr = pl.vr;
    if (a->steps < 1) return fail(SDFNMPC_E_ARG, "rollout: steps must be >= 1");
    if (!a->x_log || !a->u_log) return fail(SDFNMPC_E_ARG, "rollout: x_log and u_log are required");
    if (int rc = plant_args(&a->plant, s->B, s->x0, s->u0, s->x0, pa)) return rc;
    if (!a->vehicle) {
        if (a->xhat_log || a->uapp_log)
            return fail(SDFNMPC_E_ARG, "rollout: xhat_log and uapp_log need a vehicle");
        if (a->omega_log || a->rotor_log)
            return fail(SDFNMPC_E_ARG, "rollout: omega_log and rotor_log need a vehicle with a body");
    } else {
        int neutral = 0;
        if (int rc = vehicle_info(a->vehicle, s->ctx, s->B, &neutral, &vr.x_true, &vr.scratch)) return rc;
        if (a->frame0 < 0 || (long long)a->frame0 + a->steps > 2147483647LL)
            return fail(SDFNMPC_E_ARG, "rollout: the vehicle's frame counter (frame0 + steps) overflows or frame0 < 0");
        vr.neutral = neutral != 0;
        vr.on = !vr.neutral;
        vr.body = a->vehicle->body;
        if (!vr.body && (a->omega_log || a->rotor_log))
            return fail(SDFNMPC_E_ARG, "rollout: omega_log and rotor_log need a vehicle with a body");
        if (vr.on)
            if (int rc = vehicle_args(a->vehicle, pa, s->x0, vr.va)) return rc;
    }
    if (a->ref) {
        const int mode = a->ref->mode;
        if (mode < 0 || mode > 2) return fail(SDFNMPC_E_ARG, "rollout: ref->mode must be 0, 1 or 2");
        if (!a->wrow) return fail(SDFNMPC_E_ARG, "rollout: ref needs wrow");
        if (mode == 0 && (a->n_wp < 1 || a->n_wp > sdfn::RP_MAX_WP || !a->wp_p || !a->wp_q))
            return fail(SDFNMPC_E_ARG, "rollout: ref mode 0 needs 1..32 waypoints (wp_p, wp_q)");
        if (mode == 1 && !a->vw) return fail(SDFNMPC_E_ARG, "rollout: ref mode 1 needs vw");
        ra.B = s->B; ra.N = s->N; ra.np = s->np; ra.ny = s->ny; ra.n_wp = mode == 0 ? a->n_wp : 0;
        ra.x0 = s->x0; ra.x0_stride = 10;
        ra.wp_p = a->wp_p; ra.wp_q = a->wp_q; ra.vw = a->vw; ra.wrow = a->wrow;
        ra.p = s->p; ra.yref = s->yref; ra.W = s->W; ra.yNref = s->yNref; ra.WN = s->WN; ra.nyN = s->nyN;
    }
    return SDFNMPC_OK;
}

// step k's plant call: the plant on x0, or the vehicle at frame frame0 + k (pa carries the log pointers either way)
static int rollout_plant(sdfnmpc_solver* s, const sdfnmpc_rollout_args* a, sdfn::PlantArgs& pa, const VehicleRun& vr, int k) {
    pa.k = k;
    if (!vr.on) return plant_launch(s->ctx, pa);
    sdfn::VehicleArgs va = vr.va;
    va.P = pa;
    va.P.x = va.P.x_next = vr.x_true;
    va.frame = (unsigned)(a->frame0 + k);
    va.xhat_log = a->xhat_log;
    va.uapp_log = a->uapp_log;
    if (vr.body) return vehicle_launch_body(s->ctx, a->vehicle, va, a->omega_log, a->rotor_log);
    return vehicle_launch(s->ctx, va);
}

// the poses of a perceiving step: the camera sees from where the vehicle is (its true state), the body pose the
// controller is given comes from its estimate in x0 -- two launches, the unused pair of each into the vehicle's scratch
static int rollout_pose(sdfnmpc_solver* s, const sdfn::ScenePoseArgs& spa, const VehicleRun& vr) {
    if (!vr.on) return scene_pose_launch(s->ctx, spa);
    sdfn::ScenePoseArgs cam = spa, body = spa;
    cam.x = vr.x_true; cam.W_p_Bo = vr.scratch; cam.W_R_Bo = vr.scratch + (size_t)s->B * 3;
    if (int rc = scene_pose_launch(s->ctx, cam)) return rc;
    body.W_p_C = vr.scratch; body.W_R_C = vr.scratch + (size_t)s->B * 3;
    return scene_pose_launch(s->ctx, body);
}

// after the last step: a neutral vehicle receives what its own kernel would have written
static int rollout_end(sdfnmpc_solver* s, const sdfnmpc_rollout_args* a, const VehicleRun& vr) {
    if (!vr.neutral) return SDFNMPC_OK;
    const size_t B = s->B, K = a->steps;
    HIPCHK(hipMemcpyAsync(vr.x_true, s->x0, B * 80, hipMemcpyDeviceToDevice, s->stream));
    if (a->xhat_log) HIPCHK(hipMemcpyAsync(a->xhat_log, a->x_log, B * (K + 1) * 80, hipMemcpyDeviceToDevice, s->stream));
    if (a->uapp_log) HIPCHK(hipMemcpyAsync(a->uapp_log, a->u_log, B * K * 32, hipMemcpyDeviceToDevice, s->stream));
    return SDFNMPC_OK;
}

// the pack stage: the extrinsics into the options, and what sdfnmpc_pack_refs (mode -1 / -2) needs of the solver
static void rollout_pack(const sdfnmpc_solver* s, int mode, const double* B_p_C, const double* B_R_C, const double* W_p_Bo,
                         const double* W_R_Bo, RolloutPlan& pl) {
    pl.po.mode = mode;
    for (int i = 0; i < 3; ++i) pl.po.B_p_C[i] = B_p_C[i];
    for (int i = 0; i < 9; ++i) pl.po.B_R_C[i] = B_R_C[i];
    sdfnmpc_ref_args& pra = pl.pra;
    pra.B = s->B; pra.N = s->N; pra.np = s->np; pra.ny = s->ny; pra.nyN = s->nyN;
    pra.W_p_Bo = W_p_Bo; pra.W_R_Bo = W_R_Bo; pra.p = s->p;
}

// the stages every perceiving flavour has: perc's schedule, the vehicle's pose pair, the render into img, the pack
static int rollout_camera(sdfnmpc_solver* s, const sdfnmpc_perceive_args* pc, float* img, int mode, RolloutPlan& pl) {
    if (int rc = scene_pose_args(pc->B_p_C, pc->B_R_C, s->B, s->x0, pc->W_p_Bo, pc->W_R_Bo, pc->W_p_C, pc->W_R_C, pl.spa))
        return rc;
    if (int rc = scene_render_args(s->ctx, pc->scene, pc->scene_of, &pc->img, pc->h, pc->w, pc->scale, s->B, pc->W_p_C,
                                   pc->W_R_C, img, pl.sra))
        return rc;
    pl.every = pc->every; pl.phase = pc->phase;
    pl.pose = RolloutPlan::POSE_VEHICLE;
    pl.scene = pc->scene;
    rollout_pack(s, mode, pc->B_p_C, pc->B_R_C, pc->W_p_Bo, pc->W_R_Bo, pl);
    return SDFNMPC_OK;
}

// the sensor stage on img [B][h][w]: frame = phase + k must not overflow
static int rollout_sensor(sdfnmpc_solver* s, const sdfnmpc_rollout_args* a, const sdfnmpc_sensor_opts* sensor, float* img,
                          int h, int w, float* scratch, RolloutPlan& pl) {
    if ((long long)pl.phase + a->steps > 2147483647LL)
        return fail(SDFNMPC_E_ARG, "rollout: the sensor's frame counter (phase + steps) overflows");
    pl.sensor = sensor;
    return sensor_args(sensor, img, s->B, h, w, scratch, pl.sna, pl.ora);
}

// The one rollout loop: nothing in here refuses, the plan has been checked.  Per step [pose, render, sensor, encode,
// decode, pool, pack] when the schedule says so, then ref pack, shift, step, plant; a plain launch sequence.
static int rollout_run(sdfnmpc_solver* s, const sdfnmpc_rollout_args* a, RolloutPlan& pl) {
    sdfn::PlantArgs& pa = pl.pa;
    pa.K = a->steps;
    pa.x_log = a->x_log; pa.u_log = a->u_log; pa.status_log = a->status_log; pa.iters_log = a->iters_log;
    pa.pts_log = a->pts_log;
    pa.status = s->status; pa.iters = s->iters;
    pa.p = s->p; pa.p_stride = (long long)(s->N + 1) * s->np;
    ScopedDevice sd(s->device);
    for (int k = 0; k < a->steps; ++k) {
        // the time of step k, t0 + (phase + k) dt: the product is rounded on its own (a volatile temporary keeps the
        // compiler from contracting it into a fused multiply-add), as a host loop forms it
        volatile double steps_dt = (double)(pl.phase + k) * pl.dt;
        const double t = pl.t0 + steps_dt;
        if (pl.scene_clock) s->sdf_src.t0 = t;
        if (pl.every > 0 && (k + pl.phase) % pl.every == 0) {  // a new view from the current state
            if (pl.pose == RolloutPlan::POSE_X0)
                if (int rc = scene_pose_launch(s->ctx, pl.spa)) return rc;
            if (pl.pose == RolloutPlan::POSE_VEHICLE)
                if (int rc = rollout_pose(s, pl.spa, pl.vr)) return rc;
            if (pl.scene)
                if (int rc = scene_render_launch(s->ctx, *pl.scene, pl.sra, t)) return rc;
            if (pl.sensor)  // what the camera makes of the exact image: frame = phase + k, as a chunked or host loop counts
                if (int rc = sensor_launch(s->ctx, pl.sna, pl.ora, pl.sensor->outlier_rm != 0, pl.phase + k))
                    return rc;
            if (pl.vae)
                if (int rc = sdfnmpc_vae_encode(s->ctx, pl.vae, &pl.vo, pl.cam, pl.latent, pl.latent64)) return rc;
            if (pl.dec)
                if (int rc = sdfnmpc_vae_decode(s->ctx, pl.dec, s->B, pl.latent, pl.src->H, pl.src->W,
                                                const_cast<float*>(pl.src->images), nullptr))
                    return rc;
            if (pl.pool)
                if (int rc = sdfnmpc_img_sdf_pool(s->ctx, pl.src, s->B)) return rc;
            if (int rc = sdfnmpc_pack_refs(s->ctx, &pl.po, &pl.pra)) return rc;
        }
        if (a->ref)
            if (int rc = sdfnmpc_pack_refs(s->ctx, a->ref, &pl.ra)) return rc;
        if (int rc = sdfnmpc_solver_shift(s, a->shift)) return rc;
        if (int rc = step_enqueue(s)) return rc;
        if (int rc = rollout_plant(s, a, pa, pl.vr, k)) return rc;
    }
    if (int rc = rollout_end(s, a, pl.vr)) return rc;
    HIPCHK(hipMemcpyAsync(s->h_u0, s->u0, (size_t)s->B * 40, hipMemcpyDeviceToHost, s->stream));  // the last step's
    s->pending = true;
    return SDFNMPC_OK;
}

extern "C" int sdfnmpc_solver_rollout(sdfnmpc_solver* s, const sdfnmpc_rollout_args* a) {
    return sdfnmpc_solver_rollout_perceive(s, a, nullptr);
}

extern "C" int sdfnmpc_solver_rollout_perceive(sdfnmpc_solver* s, const sdfnmpc_rollout_args* a,
                                               const sdfnmpc_perceive_args* pc) {
    return sdfnmpc_solver_rollout_perceive_at(s, a, pc, 0.0, 0.0);
}

extern "C" int sdfnmpc_solver_rollout_perceive_at(sdfnmpc_solver* s, const sdfnmpc_rollout_args* a,
                                                  const sdfnmpc_perceive_args* pc, double t0, double dt) {
    return sdfnmpc_solver_rollout_perceive_sensor(s, a, pc, t0, dt, nullptr, nullptr);
}

extern "C" int sdfnmpc_solver_rollout_perceive_sensor(sdfnmpc_solver* s, const sdfnmpc_rollout_args* a,
                                                      const sdfnmpc_perceive_args* pc, double t0, double dt,
                                                      const sdfnmpc_sensor_opts* sensor, float* scratch) {
    if (!s || !a) return fail(SDFNMPC_E_ARG, "NULL argument to sdfnmpc_solver_rollout");
    if (sensor && !pc) return fail(SDFNMPC_E_ARG, "rollout: a sensor model needs perception (perc)");
    if (int rc = rollout_clock(t0, dt)) return rc;
    RolloutPlan pl;
    pl.t0 = t0; pl.dt = dt;
    if (int rc = rollout_args(s, a, pl)) return rc;
    if (pc) {  // what sdfnmpc_vae_encode / sdfnmpc_pack_refs (mode -1) would refuse; the image goes into the camera buffer
        if (int rc = rollout_schedule(pc->every, pc->phase)) return rc;
        if (!pc->scene || !pc->vae) return fail(SDFNMPC_E_ARG, "rollout: perception needs a scene and an encoder");
        if (pc->scene->ctx != s->ctx || pc->vae->ctx != s->ctx)
            return fail(SDFNMPC_E_ARG, "rollout: the scene and the encoder must live on the solver's context");
        if (!pc->images || !pc->latent || !pc->latent64 || !pc->W_p_Bo || !pc->W_R_Bo || !pc->W_p_C || !pc->W_R_C)
            return fail(SDFNMPC_E_ARG, "rollout: perception needs its workspaces (images, latents, poses)");
        const int L = sdfnmpc_vae_size_latent(pc->vae);
        if (L < 1 || 17 + L > s->np)
            return fail(SDFNMPC_E_ARG, "rollout: the encoder's latent does not fit the parameter row");
        if (!(pc->vae_opts.clip > 0.f)) return fail(SDFNMPC_E_ARG, "rollout: vae_opts.clip must be > 0");
        if (int rc = rollout_camera(s, pc, pc->images, -1, pl)) return rc;
        pl.pra.L = L; pl.pra.latent = pc->latent64;
        pl.vae = pc->vae; pl.cam = pc->images; pl.latent = pc->latent; pl.latent64 = pc->latent64;
        pl.vo = pc->vae_opts;
        pl.vo.B = s->B; pl.vo.in_h = pc->h; pl.vo.in_w = pc->w; pl.vo.dtype = 0;
        if (sensor)
            if (int rc = rollout_sensor(s, a, sensor, pc->images, pc->h, pc->w, scratch, pl)) return rc;
    }
    return rollout_run(s, a, pl);
}

extern "C" int sdfnmpc_solver_set_sdf_scene(sdfnmpc_solver* s, const sdfnmpc_scene* scene, const int* scene_of,
                                            double max_df, int predict) {
    if (!s) return fail(SDFNMPC_E_ARG, "NULL solver");
    if (!scene) {  // back to the network, from either source; the scene time stays
        s->sdf_src = sdfnmpc_scene_sdf_opts{nullptr, nullptr, 0.0, s->sdf_src.t0, nullptr};
        s->has_img = false;
        return SDFNMPC_OK;
    }
    if (s->no_sdf)
        return fail(SDFNMPC_E_ARG, "set_sdf_scene: no row or cost of the solver's constraint set reads the SDF");
    if (scene->ctx != s->ctx)
        return fail(SDFNMPC_E_ARG, "set_sdf_scene: the scene must live on the solver's context");
    if (scene->is_mesh && !scene->sdf_source)  // a mesh set is a source only when it was created as one
        return fail(SDFNMPC_E_UNSUPPORTED, "set_sdf_scene: a mesh set cannot be the SDF source (meshes are rendered and "
                                           "measured, not linearised)");
    if (scene->is_inst && !scene->sdf_source)
        return fail(SDFNMPC_E_UNSUPPORTED, "set_sdf_scene: an instanced set created with sdf_source = 0 cannot be the SDF "
                                           "source");
    if (!(max_df > 0.0) || !std::isfinite(max_df))
        return fail(SDFNMPC_E_ARG, "set_sdf_scene: max_df must be positive and finite");
    ScopedDevice sd(s->device);
    if (predict && !s->tau) {  // tau[0] = 0, tau[k] = tau[k-1] + dt[k-1], summed in that order
        std::vector<double> tau(s->N + 1, 0.0);
        for (int k = 1; k <= s->N; ++k) tau[k] = tau[k - 1] + s->h_dt[k - 1];
        double* d = nullptr;
        HIPCHK(s->alloc(&d, (size_t)s->N + 1));
        HIPCHK(hipMemcpyAsync(d, tau.data(), tau.size() * sizeof(double), hipMemcpyHostToDevice, s->stream));
        HIPCHK(hipStreamSynchronize(s->stream));  // tau is a host temporary
        s->tau = d;
    }
    const double t = s->sdf_src.t0;  // the scene time survives a change of source
    s->sdf_src = sdfnmpc_scene_sdf_opts{scene, scene_of, max_df, t, predict ? s->tau : nullptr};
    s->has_img = false;  // setting either source replaces the other
    return SDFNMPC_OK;
}

extern "C" int sdfnmpc_solver_set_sdf_image(sdfnmpc_solver* s, const sdfnmpc_img_sdf_opts* o) {
    if (!s) return fail(SDFNMPC_E_ARG, "NULL solver");
    if (!o) return sdfnmpc_solver_set_sdf_scene(s, nullptr, nullptr, 0.0, 0);  // back to the network
    if (s->no_sdf)
        return fail(SDFNMPC_E_ARG, "set_sdf_image: no row or cost of the solver's constraint set reads the SDF");
    sdfn::ImgSdfArgs ia{};
    if (int rc = img_sdf_args(s->ctx, o, s->B, s->N, s->np, s->x, s->p, s->h, s->Jh, nullptr, ia)) return rc;
    s->img_src = *o;
    s->has_img = true;
    s->sdf_src = sdfnmpc_scene_sdf_opts{nullptr, nullptr, 0.0, s->sdf_src.t0, nullptr};
    return SDFNMPC_OK;
}

extern "C" int sdfnmpc_solver_set_scene_time(sdfnmpc_solver* s, double t) {
    if (!s) return fail(SDFNMPC_E_ARG, "NULL solver");
    if (!std::isfinite(t)) return fail(SDFNMPC_E_ARG, "set_scene_time: the time must be finite");
    s->sdf_src.t0 = t;
    return SDFNMPC_OK;
}

extern "C" int sdfnmpc_solver_rollout_scene_sdf(sdfnmpc_solver* s, const sdfnmpc_rollout_args* a,
                                                const sdfnmpc_pose_refresh_args* pose, int phase, double t0, double dt) {
    if (!s || !a) return fail(SDFNMPC_E_ARG, "NULL argument to sdfnmpc_solver_rollout_scene_sdf");
    if (!s->sdf_src.scene)
        return fail(SDFNMPC_E_ARG, "rollout_scene_sdf: no scene source set (sdfnmpc_solver_set_sdf_scene)");
    if (int rc = rollout_clock(t0, dt)) return rc;
    if (phase < 0) return fail(SDFNMPC_E_ARG, "rollout_scene_sdf: phase must be >= 0");
    RolloutPlan pl;
    pl.t0 = t0; pl.dt = dt; pl.phase = phase;
    pl.scene_clock = true;  // from the first step on, so after the last refusal
    if (int rc = rollout_args(s, a, pl)) return rc;
    if (pose) {  // the camera pose the FOV rows read, from x0: the pose block, and what sdfnmpc_pack_refs (mode -2) would refuse
        if (pose->every < 1) return fail(SDFNMPC_E_ARG, "rollout_scene_sdf: pose->every must be >= 1");
        if (!pose->W_p_Bo || !pose->W_R_Bo || !pose->W_p_C || !pose->W_R_C)
            return fail(SDFNMPC_E_ARG, "rollout_scene_sdf: the pose refresh needs its workspaces");
        if (int rc = scene_pose_args(pose->B_p_C, pose->B_R_C, s->B, s->x0, pose->W_p_Bo, pose->W_R_Bo, pose->W_p_C,
                                     pose->W_R_C, pl.spa))
            return rc;
        pl.every = pose->every;
        pl.pose = RolloutPlan::POSE_X0;
        rollout_pack(s, -2, pose->B_p_C, pose->B_R_C, pose->W_p_Bo, pose->W_R_Bo, pl);
    }
    return rollout_run(s, a, pl);
}

extern "C" int sdfnmpc_solver_rollout_image_sdf(sdfnmpc_solver* s, const sdfnmpc_rollout_args* a,
                                                const sdfnmpc_perceive_args* pc, double t0, double dt,
                                                const sdfnmpc_sensor_opts* sensor, float* scratch) {
    if (!s || !a) return fail(SDFNMPC_E_ARG, "NULL argument to sdfnmpc_solver_rollout_image_sdf");
    if (!s->has_img)
        return fail(SDFNMPC_E_ARG, "rollout_image_sdf: no image source set (sdfnmpc_solver_set_sdf_image)");
    if (sensor && !pc) return fail(SDFNMPC_E_ARG, "rollout: a sensor model needs perception (perc)");
    if (int rc = rollout_clock(t0, dt)) return rc;
    RolloutPlan pl;
    pl.t0 = t0; pl.dt = dt;
    if (int rc = rollout_args(s, a, pl)) return rc;
    const sdfnmpc_img_sdf_opts& src = s->img_src;
    if (pc) {  // re-imaging: rendered into the source itself; NULL keeps the image and the pose as set
        if (int rc = rollout_schedule(pc->every, pc->phase)) return rc;
        if (!pc->scene || pc->scene->ctx != s->ctx)
            return fail(SDFNMPC_E_ARG, "rollout_image_sdf: re-imaging needs a scene on the solver's context");
        if (pc->h != src.H || pc->w != src.W)
            return fail(SDFNMPC_E_ARG, "rollout_image_sdf: the render size must equal the source's H x W");
        if (src.img_of)
            return fail(SDFNMPC_E_ARG, "rollout_image_sdf: re-imaging renders one image per instance (img_of must be NULL)");
        if (!pc->W_p_Bo || !pc->W_R_Bo || !pc->W_p_C || !pc->W_R_C)
            return fail(SDFNMPC_E_ARG, "rollout_image_sdf: re-imaging needs the pose workspaces");
        float* img = const_cast<float*>(src.images);
        if (int rc = rollout_camera(s, pc, img, -2, pl)) return rc;
        pl.src = &src; pl.pool = !src.is_signed;
        if (sensor)
            if (int rc = rollout_sensor(s, a, sensor, img, pc->h, pc->w, scratch, pl)) return rc;
    }
    return rollout_run(s, a, pl);
}

extern "C" int sdfnmpc_solver_rollout_image_recon(sdfnmpc_solver* s, const sdfnmpc_rollout_args* a,
                                                  const sdfnmpc_perceive_args* pc, double t0, double dt,
                                                  const sdfnmpc_sensor_opts* sensor, float* scratch, sdfnmpc_vae_dec* dec) {
    if (!s || !a) return fail(SDFNMPC_E_ARG, "NULL argument to sdfnmpc_solver_rollout_image_recon");
    if (!s->has_img)
        return fail(SDFNMPC_E_ARG, "rollout_image_recon: no image source set (sdfnmpc_solver_set_sdf_image)");
    if (!pc) return fail(SDFNMPC_E_ARG, "rollout_image_recon: perception (perc) is required");
    if (!dec) return fail(SDFNMPC_E_ARG, "rollout_image_recon: no decoder");
    if (int rc = rollout_clock(t0, dt)) return rc;
    RolloutPlan pl;
    pl.t0 = t0; pl.dt = dt;
    if (int rc = rollout_args(s, a, pl)) return rc;
    const sdfnmpc_img_sdf_opts& src = s->img_src;
    if (int rc = rollout_schedule(pc->every, pc->phase)) return rc;
    if (!pc->scene || pc->scene->ctx != s->ctx)
        return fail(SDFNMPC_E_ARG, "rollout_image_recon: re-imaging needs a scene on the solver's context");
    if (!pc->vae || pc->vae->ctx != s->ctx || dec->ctx != s->ctx)
        return fail(SDFNMPC_E_ARG, "rollout_image_recon: the encoder and the decoder must live on the solver's context");
    if (sdfnmpc_vae_size_latent(pc->vae) != sdfnmpc_vae_dec_size_latent(dec))
        return fail(SDFNMPC_E_ARG, "rollout_image_recon: the encoder and the decoder have different latent sizes");
    if (pc->h != src.H || pc->w != src.W)
        return fail(SDFNMPC_E_ARG, "rollout_image_recon: the render size must equal the source's H x W");
    if (src.img_of)
        return fail(SDFNMPC_E_ARG, "rollout_image_recon: re-imaging renders one image per instance (img_of must be NULL)");
    if (!pc->images || !pc->latent || !pc->W_p_Bo || !pc->W_R_Bo || !pc->W_p_C || !pc->W_R_C)
        return fail(SDFNMPC_E_ARG, "rollout_image_recon: perception needs its workspaces (camera images, latent, poses)");
    if (pc->images == src.images)
        return fail(SDFNMPC_E_ARG, "rollout_image_recon: the camera buffer must not be the source's images");
    if (pc->img.is_depth && !pc->vae_opts.yz)
        return fail(SDFNMPC_E_ARG, "rollout_image_recon: a depth camera needs the Depth2Range table (vae_opts.yz)");
    // rendered into the camera buffer, encoded, the reconstruction decoded into the source
    if (int rc = rollout_camera(s, pc, pc->images, -2, pl)) return rc;
    pl.vae = pc->vae; pl.cam = pc->images; pl.latent = pc->latent; pl.latent64 = pc->latent64;
    // the images are normalised: clip = 1, and Depth2Range exactly when the camera measures depth
    pl.vo = sdfnmpc_vae_opts{s->B, pc->h, pc->w, 0, 1.0f, pc->img.is_depth ? pc->vae_opts.yz : nullptr};
    pl.dec = dec; pl.src = &src; pl.pool = !src.is_signed;
    if (sensor)
        if (int rc = rollout_sensor(s, a, sensor, pc->images, pc->h, pc->w, scratch, pl)) return rc;
    return rollout_run(s, a, pl);
}

extern "C" int sdfnmpc_solver_wait(sdfnmpc_solver* s, double* u0, int* status, int* iters) {
    if (!s) return fail(SDFNMPC_E_ARG, "NULL solver");
    ScopedDevice sd(s->device);
    HIPCHK(hipStreamSynchronize(s->stream));
    s->arena_used = 0;  // every staged upload has landed
    if (!s->pending && (u0 || status || iters))
        return fail(SDFNMPC_E_ARG, "sdfnmpc_solver_wait: no step was enqueued");
    s->pending = false;
    if (u0) memcpy(u0, s->h_u0, (size_t)s->B * 32);
    if (status) memcpy(status, s->h_status, (size_t)s->B * 4);
    if (iters) memcpy(iters, s->h_iters, (size_t)s->B * 4);
    return SDFNMPC_OK;
}
