// What the host files of libsdfnmpc.so share (engine.cpp and solver.hip); internal, not installed.
//
// The error message, the device guard, the context and the timed launch helper; the opaque objects of
// include/sdfnmpc.h that both files look inside; and the helpers engine.cpp offers the solver's rollouts,
// each declared here once, in namespace sdfn.
#pragma once
#include <hip/hip_runtime.h>

#include <chrono>
#include <map>
#include <mutex>
#include <string>
#include <vector>

#include "../../include/sdfnmpc.h"
#include "sdf_kernels.h"
#include "vae_kernels.h"
#include "df_kernels.h"
#include "plant_kernels.h"
#include "scene_kernels.h"
#include "sensor_kernels.h"
#include "vehicle_kernels.h"

namespace sdfn {

// ------------------------------------------------------------------------------------------------
// errors: sets the thread-local message of sdfnmpc_last_error (engine.cpp) and returns the code
int fail(int code, const std::string& msg);
int fail(int code, const char* msg);  // a literal message: no std::string built at the call site
#define HIPCHK(expr)                                                                              \
    do {                                                                                          \
        hipError_t e_ = (expr);                                                                   \
        if (e_ != hipSuccess) return sdfn::fail(SDFNMPC_E_HIP, std::string(#expr) + ": " + hipGetErrorString(e_)); \
    } while (0)

struct DevBuf {
    void* p = nullptr;
    size_t bytes = 0;
    unsigned long long gen = 0;  // reallocations so far (a captured step graph holds the pointer of its time)
    hipError_t ensure(size_t n) {
        if (n <= bytes) return hipSuccess;
        if (p) (void)hipFree(p);
        p = nullptr;
        bytes = 0;
        ++gen;
        hipError_t e = hipMalloc(&p, n);
        if (e == hipSuccess) bytes = n;
        return e;
    }
    ~DevBuf() {
        if (p) (void)hipFree(p);
    }
};

struct KStat {
    std::vector<std::pair<hipEvent_t, hipEvent_t>> pending;
    double ms = 0.0;
    long long n = 0;
};

struct ScopedDevice {
    int prev = -1;
    explicit ScopedDevice(int d) {
        (void)hipGetDevice(&prev);
        if (prev != d) (void)hipSetDevice(d);
    }
    ~ScopedDevice() {
        int cur = -1;
        (void)hipGetDevice(&cur);
        if (prev >= 0 && cur != prev) (void)hipSetDevice(prev);
    }
};

struct VaeLayer {
    const float* w = nullptr;
    const float* b = nullptr;
    const unsigned short* wpl = nullptr;  // convolutions: w split into bf16 planes (VaeConvArgs::wpl)
    int cin = 0, cout = 0, ks = 0, stride = 0;
};

struct VaeDecOp {
    size_t wpl_off = 0, b_off = 0;  // in floats from the device block
    const unsigned short* wpl = nullptr;
    const float* b = nullptr;
    size_t wps = 0;
    int cin = 0, cout = 0, nphase = 0;
    int ntaps[4] = {0}, py[4] = {0}, px[4] = {0};
    unsigned woff[4] = {0};
    signed char dy[4][VAE_DEC_TAPS] = {{0}}, dx[4][VAE_DEC_TAPS] = {{0}};
};

}  // namespace sdfn

// ------------------------------------------------------------------------------------------------
// context
struct sdfnmpc_ctx {
    int device = 0;
    hipStream_t stream = nullptr;
    bool own_stream = false;
    hipStream_t aux = nullptr;                       // low-priority side stream (fork/join per call)
    hipEvent_t ev_fork = nullptr, ev_join = nullptr;
    bool serial_prep = false;  // diagnostic (SDFNMPC_SERIAL_PREP=1): linearize after the SDF kernel, same stream
    int qp_kernel = SDFNMPC_QP_AUTO;  // SDFNMPC_QP_KERNEL=serial|segmented, or sdfnmpc_ctx_set_qp_kernel
    int tile_rows = 32;
    int n_cu = 0;              // compute units of the device (hipDeviceProp_t::multiProcessorCount)
    size_t lds_per_cu = 0;     // LDS bytes per CU (hipDeviceProp_t::maxSharedMemoryPerMultiProcessor)
    bool timing = false;
    sdfn::DevBuf c13, sdf4, lat, out4, glat, qpw, qpst, wws;
    sdfn::DevBuf dfpool;  // sdfnmpc_udf: the 5x5 min-pooled images
    sdfn::DevBuf imgpts;  // sdfnmpc_img_sdf_rows without the caller's pts: the camera-frame points of the rows
    sdfn::DevBuf morph_t, morph_e;  // sdfnmpc_outlier_rm with kernel_size != 3: the thresholded image and its erosion
    // host-pointer path (sdf_eval_host, the CasADi external): pinned staging, its own hoist buffer and
    // the latents it was computed for (consecutive acados calls share one latent: the hoist is reused)
    float* h_pin = nullptr;
    size_t h_pin_bytes = 0;
    sdfn::DevBuf hin, hout, hc13;
    std::vector<float> h_lat;
    uint64_t h_net = 0;  // uid of the network the cached hoist belongs to
    // resident SDF server of the host path (sdf_row.hip, SdfMbox): mailbox in pinned coherent memory, its
    // own stream, the network it serves, the last request number, and whether it may still be running
    struct {
        int mode = -1;                // -1: from SDFNMPC_SDF_SERVER (default on), 0 off, 1 on
        sdfn::SdfMbox* mb = nullptr;
        sdfn::SdfMbox* mb_dev = nullptr;
        hipStream_t stream = nullptr;
        uint64_t net = 0;
        unsigned long long seq = 0;
        bool live = false;
        long long idle_ticks = 0, life_ticks = 0;
        double idle_s = 0.001, life_s = 0.0008;  // SDFNMPC_SDF_SERVER_IDLE_MS / _LIFE_MS
        unsigned long long epoch = 0;           // launches so far; the live server's is in `gone` once it left
        bool abandoned = false;                 // a server that would not stop: its mailbox is never reused
        double khz = 100000.0;
        std::chrono::steady_clock::time_point last{};
        double acc[4] = {0, 0, 0, 0};  // diagnostics: us staging, computing, host round trip; calls
        double ph[14] = {};            // diagnostics: us per row_eval phase
    } srv;
    std::map<std::string, sdfn::KStat> stats;
    std::mutex mu;  // serialises the host-pointer path (CasADi externals may be called concurrently)
    // stage records packed by sdfnmpc_rti_prepare, consumed by the next sdfnmpc_qp_feedback
    struct {
        bool valid = false;
        int B = 0, N = 0;
        const double* xn = nullptr;  // the lin outputs they were packed from
        const void* work = nullptr;
        bool sdf_row_patch = false;  // the feedback's QP kernel copies the sdf row of C^T into them
        int ny = 0, cost_scaling = 0, lm_scaling = 0;  // the qp options the records were packed under
        double lm = 0.0;
        long long cset = 0;  // and their constraint set (cset_key)
    } prep;
};

// ------------------------------------------------------------------------------------------------
// the objects both files look inside
// the vehicle model around the plant (vehicle.hip).  The object owns the hidden states of B instances in one
// device block; a model with everything off is `neutral` and every entry point runs the plant's own kernel (or a copy).
struct sdfnmpc_vehicle {
    sdfnmpc_ctx* ctx = nullptr;
    int device = 0;
    int B = 0;
    sdfnmpc_vehicle_opts o{};
    bool neutral = false;
    double* block = nullptr;  // [x_true B*10 | gamma_act B | w B*3 | ring B*d*4 | pose scratch B*12]
    double *x_true = nullptr, *gamma_act = nullptr, *w = nullptr, *ring = nullptr, *scratch = nullptr;
    // the rigid body (sdfnmpc_vehicle_set_body): its options, and [omega B*3 | rotor B*4], allocated with the first body
    bool body = false;
    sdfnmpc_body_opts bo{};
    double* body_block = nullptr;
};

struct sdfnmpc_vae {
    int device = 0;
    const sdfnmpc_ctx* ctx = nullptr;  // the context it was loaded on (sdfnmpc_solver_rollout_perceive asks)
    int L = 0, H = 0, W = 0;
    int Hc = 0, Wc = 0, Hp = 0, Wp = 0;
    int bh[4] = {0}, bw[4] = {0};  // block output maps
    void* dmem = nullptr;
    sdfn::VaeLayer stem, conv[11], head;  // conv: b0a b0s b0b b1a b1s b1b b2a b2s b2b b3a b3b
    const unsigned short* stem_wpl = nullptr;  // the stem weights split into bf16 planes (VaeStemArgs::wpl)
    const float* zero16 = nullptr;              // 16 zero floats (VaeConvArgs::zero: a tap outside the map)
    sdfn::DevBuf ws;
    int ws_B = 0;
};

struct sdfnmpc_vae_dec {
    int device = 0;
    const sdfnmpc_ctx* ctx = nullptr;
    int L = 0;
    void* dmem = nullptr;
    const float *head_w = nullptr, *head_b = nullptr, *tail_w = nullptr, *tail_b = nullptr;
    sdfn::VaeDecOp up[4], sc[4], cv[4];  // per ResBlockDeconv: the stride-2 3x3, the shortcut, the stride-1 3x3
    sdfn::DevBuf ws;
};

struct sdfnmpc_scene {
    int device = 0;
    const sdfnmpc_ctx* ctx = nullptr;
    int S = 0;
    void* dmem = nullptr;  // count [S] | ScenePrimD [S][32] | ScenePrimF [S][32] | dynamic: ScenePrimDyn [S][32] | vmax [S]
    sdfn::SceneDev dev{};
    const sdfn::ScenePrimDyn* dyn = nullptr;  // non-NULL: a dynamic set (some primitive is oriented or moves)
    const int* mcount = nullptr;              // [S]: with dev.ghdr and dyn, the movers per scene of a mixed set
    std::vector<double> vmax;                 // [S]: the bound on the speed of any surface point of a mover (0: none moves)
    const double* dvmax = nullptr;            // the same on the device, at the end of the image of a set with dyn
    // an indexed set (sdfnmpc_scene_create_large; dev.ghdr != nullptr): count [S] | SceneGridHdr [S] | ScenePrimD [total]
    // | ScenePrimF [total] | cell_start | cell_items, every block at a multiple of 16 bytes; a mixed set
    // (sdfnmpc_scene_create_mixed; dev.ghdr and dyn both non-NULL) appends mcount [S] | ScenePrimDyn [S][32] | vmax [S]
    // a mesh set (sdfnmpc_scene_create_mesh): MeshHdr [S] | MeshNode [nodes] | MeshTriF [tris] | MeshTriD [tris] | closed:
    // MeshTriN [tris], every block at a multiple of 16 bytes; dev carries S alone, dyn and mcount stay NULL; a mesh set
    // with movers (sdfnmpc_scene_create_mesh_mixed; is_mesh and dyn non-NULL) appends mcount [S] | ScenePrimDyn [S][32] |
    // vmax [S]
    bool is_mesh = false;
    bool sdf_source = false;  // a mesh set created with sdfnmpc_mesh_opts.sdf_source = 1: accepted as the SDF source
    sdfn::MeshDev mesh{};
    // an instanced set (sdfnmpc_scene_create_instanced): the image of a mesh set over the nparts parts of the pool (mesh:
    // hdr [nparts] | ...), then icount [S] | ioff [S] | ScenePrimDyn [sum of icount] | vmax [S]; is_mesh stays false, dyn
    // and mcount stay NULL, dev carries S alone
    bool is_inst = false;
    bool inst_moves = false;  // some instance has a non-zero v, amp or yaw_rate: the set is dynamic
    sdfn::InstDev inst{};
};

namespace sdfn {

// launch helper with optional HIP-event timing on the context stream
template <typename F>
static hipError_t timed(sdfnmpc_ctx* ctx, const char* name, F&& launch, hipStream_t st = nullptr) {
    if (!ctx->timing) return launch();
    if (!st) st = ctx->stream;
    hipEvent_t a, b;
    hipError_t e = hipEventCreate(&a);
    if (e != hipSuccess) return e;
    e = hipEventCreate(&b);
    if (e != hipSuccess) return e;
    (void)hipEventRecord(a, st);
    e = launch();
    (void)hipEventRecord(b, st);
    ctx->stats[name].pending.emplace_back(a, b);
    return e;
}

// ------------------------------------------------------------------------------------------------
// what engine.cpp offers solver.hip (and uses itself).  An *_args function checks the options and fills a kernel's
// argument block (nothing is launched); its *_launch enqueues a filled block on the context stream, under the stat
// name given.

// the plant ("plant"); the vehicle around a filled plant block, whose x / x_next become the
// vehicle's true state ("plant_vehicle", with a body "plant_vehicle_body").  vehicle_info refuses a vehicle a
// rollout cannot use and tells whether it is neutral and where its true state and pose scratch live.
int plant_args(const sdfnmpc_plant_opts* o, int B, const double* x, const double* u, double* x_next, PlantArgs& out);
int plant_launch(sdfnmpc_ctx* ctx, const PlantArgs& a);
int vehicle_info(const sdfnmpc_vehicle* v, const sdfnmpc_ctx* ctx, int B, int* neutral, double** x_true,
                 double** scratch);
int vehicle_args(const sdfnmpc_vehicle* v, const PlantArgs& pa, double* x_est, VehicleArgs& out);
int vehicle_launch(sdfnmpc_ctx* ctx, const VehicleArgs& a);
int vehicle_launch_body(sdfnmpc_ctx* ctx, const sdfnmpc_vehicle* v, const VehicleArgs& a, double* omega_log,
                        double* rotor_log);

// the render of a scene at time t ("scene_render", "_grid", "_dyn", "_mixed"), the camera and body poses
// ("scene_pose"), and the option check of the scene's exact distance as the SDF row
int scene_render_args(sdfnmpc_ctx* ctx, const sdfnmpc_scene* sc, const int* scene_of, const sdfnmpc_img_opts* o, int H,
                      int W, float scale, int B, const double* W_p_C, const double* W_R_C, float* img,
                      SceneRenderArgs& out);
int scene_render_launch(sdfnmpc_ctx* ctx, const sdfnmpc_scene& sc, const SceneRenderArgs& a, double t);
int scene_pose_args(const double* B_p_C, const double* B_R_C, int B, const double* x, double* W_p_Bo, double* W_R_Bo,
                    double* W_p_C, double* W_R_C, ScenePoseArgs& out);
int scene_pose_launch(sdfnmpc_ctx* ctx, const ScenePoseArgs& a);
int scene_sdf_args(sdfnmpc_ctx* ctx, const sdfnmpc_scene_sdf_opts* o, int B, int N, int np, const double* x,
                   const double* p, double* h, double* Jh, SceneSdfArgs& out);

// the option check of a camera image's field as the SDF row, and the sensor stage of a frame ("sensor_degrade",
// then "outlier_rm")
int img_sdf_args(sdfnmpc_ctx* ctx, const sdfnmpc_img_sdf_opts* o, int B, int N, int np, const double* x, const double* p,
                 double* h, double* Jh, float* pts, ImgSdfArgs& out);
int sensor_args(const sdfnmpc_sensor_opts* o, float* img, int B, int H, int W, float* scratch, SensorArgs& sa,
                OutlierArgs& oa);
int sensor_launch(sdfnmpc_ctx* ctx, const SensorArgs& sa, const OutlierArgs& oa, int outlier_rm, int frame);

}  // namespace sdfn
