// The closed-loop plant (plant.hip): argument block shared with the engine and the solver object.
#pragma once
#include <hip/hip_runtime.h>

namespace sdfn {

constexpr int PLANT_MAX_SUBSTEPS = 64;

struct PlantArgs {
    int B;
    int kind;                       // 0 'att', 1 'att_tau' (sdfnmpc_plant_opts.kind): which plant_advance_kernel runs
    int substeps;                   // RK4 steps of dt / substeps per call, 1..PLANT_MAX_SUBSTEPS
    double gamma, roll, pitch, wz;  // input scalings u -> (thrust/m, roll, pitch, yaw rate)
    double g;
    double itau_roll, itau_pitch;   // 'att_tau': 1 / tau of the roll and pitch lags
    double dt;                      // control period
    const double* x;                // [B][10]
    const double* u;                // [B][4]
    double* x_next;                 // [B][10], may alias x (a lane reads its row before it writes it)
    const double* acc_dist;         // [B][3] or NULL: world-frame acceleration added to dv/dt
    const double* gamma_scale;      // [B] or NULL: factor on the thrust input
    // ---- the rollout's log (sdfnmpc_rollout_args); x_log == NULL: no logging, the rest is ignored
    int K, k;                       // steps of the rollout, this step
    double* x_log;                  // [B][K+1][10]: row k + 1 (and row 0, the state before the step, at k == 0)
    double* u_log;                  // [B][K][4]
    int* status_log;                // [B][K] or NULL, from status
    int* iters_log;                 // [B][K] or NULL, from iters
    float* pts_log;                 // [B][K+1][3] or NULL: camera-frame positions W_R_Co^T (x[:3] - W_p_Co)
    const int* status;              // [B] the step's QP status / iterations
    const int* iters;
    const double* p;                // [B][p_stride]: node 0's parameter row of each instance (pose at [1..12])
    long long p_stride;
};

hipError_t launch_plant(const PlantArgs& a, hipStream_t s);

}  // namespace sdfn
