// The plant of a closed loop (fp64): x_next = RK4^substeps(x, u) of the 'att' model
// (quad_rollpitchyawrate.py:19-55) or the 'att_tau' model (quad_rollpitchyawrate_tau.py:19-58), one instance
// per lane -- what a simulator does between two control steps, so that K steps of Monte-Carlo closed loops
// stay on the device (sdfnmpc_solver_rollout).  The reference has no counterpart: its plant is the
// simulator outside the controller.
//
// f_expl is evaluated value-only (no dual numbers), in the operation order of linearize.hip's quad_f /
// quad_f_tau, and integrated with the Butcher tableau and the accumulation order linearize_kernel documents:
// at substeps = 1 and without mismatch the result is the preparation phase's x_{k+1} up to the compiler's
// contraction choices (a few ulp; tests/test_gpu_plant.py pins 1e-13).  The plant may differ from the
// controller's model: another kind, a finer step, a constant world-frame acceleration (wind, a payload's
// weight error) and a thrust-gain error per instance.  No input clipping and no quaternion renormalisation
// (both models normalise internally).
//
// The same launch writes the rollout's log: the next measured state in place, x / u / status / iterations
// rows, and the camera-frame position Nmpc.check_openloop_traj would check.
#include <hip/hip_runtime.h>

#include "plant_dev.h"
#include "plant_kernels.h"

namespace sdfn {

// One instance per lane, 64-thread blocks: B = 1024 spreads over 16 CUs, and the kernel is a chain of
// dependent fp64 operations per lane either way.
template <int KIND>
__global__ __launch_bounds__(64) void plant_advance_kernel(PlantArgs A) {
    const long long b = (long long)blockIdx.x * 64 + threadIdx.x;
    if (b >= A.B) return;
    double x[10], u[4];
#pragma unroll
    for (int i = 0; i < 10; ++i) x[i] = A.x[b * 10 + i];
#pragma unroll
    for (int i = 0; i < 4; ++i) u[i] = A.u[b * 4 + i];

    const bool log = A.x_log != nullptr;
    const double* pr = A.p + b * A.p_stride;
    if (log && A.k == 0) {  // row 0: the state the rollout starts from
        double* xl = A.x_log + b * (A.K + 1) * 10;
#pragma unroll
        for (int i = 0; i < 10; ++i) xl[i] = x[i];
        if (A.pts_log) log_point(pr, x, A.pts_log + b * (A.K + 1) * 3);
    }

    PlantIn in{};
    in.gamma = u[0] * A.gamma;
    if (A.gamma_scale) in.gamma = in.gamma * A.gamma_scale[b];
    in.wz = u[3] * A.wz;
    in.g = A.g;
    in.dist = A.acc_dist != nullptr;
    if (in.dist) {
        in.ad0 = A.acc_dist[b * 3 + 0];
        in.ad1 = A.acc_dist[b * 3 + 1];
        in.ad2 = A.acc_dist[b * 3 + 2];
    }
    if constexpr (KIND == 0) {  // sin / cos of roll and pitch depend on u only: once per call
        double sr, cr, sp, cp;
        sincos(u[1] * A.roll, &sr, &cr);
        sincos(u[2] * A.pitch, &sp, &cp);
        in.b0 = cr * sp * in.gamma;
        in.b1 = -sr * in.gamma;
        in.b2 = cr * cp * in.gamma;
    } else {
        in.roll_des = u[1] * A.roll;
        in.pitch_des = u[2] * A.pitch;
        in.itau_roll = A.itau_roll;
        in.itau_pitch = A.itau_pitch;
    }
    auto f_expl = [&](const double* xs, double* f) {
        if constexpr (KIND == 0)
            plant_f_att(in, xs, f);
        else
            plant_f_tau(in, xs, f);
        if (in.dist) {
            f[7] = f[7] + in.ad0;
            f[8] = f[8] + in.ad1;
            f[9] = f[9] + in.ad2;
        }
    };

    // ---- ERK4 (Butcher c = [0, 1/2, 1/2, 1], b = [1/6, 1/3, 1/3, 1/6]), linearize_kernel's accumulation:
    //      x_out = x + (h b_1) k_1 + ... + (h b_4) k_4, stage input x + (h a_s) k_{s-1}
    const double h = A.dt / (double)A.substeps;
    const double hb[4] = {h / 6, h / 3, h / 3, h / 6}, ha[4] = {0.0, h / 2, h / 2, h};
    for (int sub = 0; sub < A.substeps; ++sub) {
        double xo[10], kk[10], tmp[10];
        f_expl(x, kk);
#pragma unroll
        for (int i = 0; i < 10; ++i) xo[i] = x[i] + kk[i] * hb[0];
#pragma unroll
        for (int st = 1; st < 4; ++st) {
#pragma unroll
            for (int i = 0; i < 10; ++i) tmp[i] = x[i] + kk[i] * ha[st];
            f_expl(tmp, kk);
#pragma unroll
            for (int i = 0; i < 10; ++i) xo[i] = xo[i] + kk[i] * hb[st];
        }
#pragma unroll
        for (int i = 0; i < 10; ++i) x[i] = xo[i];
    }

#pragma unroll
    for (int i = 0; i < 10; ++i) A.x_next[b * 10 + i] = x[i];
    if (log) {
        const long long row = b * A.K + A.k;
        double* xl = A.x_log + (b * (A.K + 1) + A.k + 1) * 10;
#pragma unroll
        for (int i = 0; i < 10; ++i) xl[i] = x[i];
#pragma unroll
        for (int i = 0; i < 4; ++i) A.u_log[row * 4 + i] = u[i];
        if (A.status_log) A.status_log[row] = A.status[b];
        if (A.iters_log) A.iters_log[row] = A.iters[b];
        if (A.pts_log) log_point(pr, x, A.pts_log + (b * (A.K + 1) + A.k + 1) * 3);
    }
}

hipError_t launch_plant(const PlantArgs& a, hipStream_t s) {
    if (a.B <= 0) return hipSuccess;
    const dim3 grid((unsigned)((a.B + 63) / 64));
    if (a.kind == 1)
        hipLaunchKernelGGL(plant_advance_kernel<1>, grid, dim3(64), 0, s, a);
    else
        hipLaunchKernelGGL(plant_advance_kernel<0>, grid, dim3(64), 0, s, a);
    return hipGetLastError();
}

}  // namespace sdfn
