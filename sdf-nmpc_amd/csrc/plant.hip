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

#include "plant_kernels.h"

namespace sdfn {

namespace {

// 1 / sqrt(a), a > 0: the hardware estimate and two Newton steps (linearize.hip's drsqrt, value only)
__device__ __forceinline__ double prsqrt(double a) {
    double r = __builtin_amdgcn_rsq(a);
#pragma unroll
    for (int it = 0; it < 2; ++it) {
        const double e = __builtin_fma(-(a * r), r, 1.0);
        r = __builtin_fma(0.5 * r, e, r);
    }
    return r;
}

// what of the inputs is constant over the stages and substeps
struct PlantIn {
    double gamma, wz;
    double b0, b1, b2;          // 'att': V_R_B e_z gamma = [cr sp, -sr, cr cp] gamma (sin / cos of the commands)
    double roll_des, pitch_des; // 'att_tau'
    double itau_roll, itau_pitch, g;
    double ad0, ad1, ad2;       // acc_dist
    bool dist;
};

// 'att' (linearize.hip quad_f): (cos, sin)(theta_z) = (x3, x6) / |(x3, x6)|, W_R_V = quat2rot([c, 0, 0, s])
__device__ __forceinline__ void plant_f_att(const PlantIn& in, const double* x, double* f) {
    const double inv = prsqrt(x[3] * x[3] + x[4] * x[4] + (x[5] * x[5] + x[6] * x[6]));
    const double s03 = x[3] * x[3] + x[6] * x[6];
    double c = 1.0, s = 0.0;  // atan2(0, 0) = 0
    if (s03 > 0.0) {
        const double r = prsqrt(s03);
        c = x[3] * r;
        s = x[6] * r;
    }
    const double r11 = c * c - s * s, r21 = (c * s) * 2.0, r33 = c * c + s * s;
    const double hw = (in.wz * inv) * 0.5;  // hamilton_prod(q, [0, 0, 0, wz]) / 2 with q = x * inv
    f[0] = x[7];
    f[1] = x[8];
    f[2] = x[9];
    f[3] = -(x[6] * hw);
    f[4] = x[5] * hw;
    f[5] = -(x[4] * hw);
    f[6] = x[3] * hw;
    f[7] = r11 * in.b0 - r21 * in.b1;
    f[8] = r21 * in.b0 + r11 * in.b1;
    f[9] = r33 * in.b2 - in.g;
}

// 'att_tau' (linearize.hip quad_f_tau): roll = atan2(ay, ax), pitch = asin(sp) = atan2(sp, cos(pitch)); the
// angles' sines and cosines from the same arguments.  No guard at |pitch| = pi / 2, as there.
__device__ __forceinline__ void plant_f_tau(const PlantIn& in, const double* x, double* f) {
    const double inv = prsqrt(x[3] * x[3] + x[4] * x[4] + (x[5] * x[5] + x[6] * x[6]));
    const double q0 = x[3] * inv, q1 = x[4] * inv, q2 = x[5] * inv, q3 = x[6] * inv;
    const double ay = (q0 * q1 + q2 * q3) * 2.0, ax = 1.0 - (q1 * q1 + q2 * q2) * 2.0;
    const double sp = (q0 * q2 - q3 * q1) * 2.0;
    const double cp2 = (1.0 - sp) * (1.0 + sp);
    const double icp = prsqrt(cp2);  // 1 / cos(pitch)
    const double rr = prsqrt(ax * ax + ay * ay);
    const double sr = ay * rr, cr = ax * rr;
    const double roll = atan2(ay, ax), pitch = atan2(sp, cp2 * icp);
    const double dr = (in.roll_des - roll) * in.itau_roll, dp = (in.pitch_des - pitch) * in.itau_pitch;
    const double w0 = dr + ((sp * sr) * icp) * dp, w1 = cr * dp;
    const double wz = in.wz, gamma = in.gamma;
    f[0] = x[7];
    f[1] = x[8];
    f[2] = x[9];
    f[3] = (-(q1 * w0) - q2 * w1 - q3 * wz) * 0.5;
    f[4] = (q0 * w0 + q2 * wz - q3 * w1) * 0.5;
    f[5] = (q0 * w1 - q1 * wz + q3 * w0) * 0.5;
    f[6] = (q0 * wz + q1 * w1 - q2 * w0) * 0.5;
    f[7] = ((q1 * q3 + q0 * q2) * 2.0) * gamma;
    f[8] = ((q2 * q3 - q0 * q1) * 2.0) * gamma;
    f[9] = (q0 * q0 - q1 * q1 - q2 * q2 + q3 * q3) * gamma - in.g;
}

// Co_p = W_R_Co^T (x[:3] - W_p_Co) with the pose of a parameter row (p_idx: W_p_Co at 1, W_R_Co row-major at 4)
__device__ __forceinline__ void log_point(const double* pr, const double* x, float* out) {
    const double e0 = x[0] - pr[1], e1 = x[1] - pr[2], e2 = x[2] - pr[3];
    const double* R = pr + 4;
#pragma unroll
    for (int i = 0; i < 3; ++i) out[i] = (float)((e0 * R[i] + e1 * R[3 + i]) + e2 * R[6 + i]);
}

}  // namespace

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
