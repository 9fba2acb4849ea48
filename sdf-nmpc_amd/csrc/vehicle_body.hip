// The rigid-body vehicle of a closed loop (fp64): the controller's command (thrust, roll, pitch, yaw rate) is the
// setpoint of an on-board attitude and rate controller, which drives four rotors with a first-order speed lag, which
// move a rigid body -- the 13-state physics of the reference's model/quad_props.py:41-48 with a continuous inner loop
// around it, one instance per lane.  Delay, gust, drag and the estimate are vehicle.hip's (steps 1, 2, 4 and 6 of
// include/sdfnmpc.h's description); this file replaces its steps 3 and 5.
//
// Hidden state per instance: x_true [10] = (p, q, v) with the full attitude in q, the body rate omega [3] in the body
// frame and the rotor speeds Omega [4] -- 17 states under the plant's RK4 (substeps, tableau, accumulation order).
// With F = m u_0 gamma and (roll_d, pitch_d, wz_d) from the applied input, at every stage:
//   q <- q / |q|, psi = quat2yaw(q), q_d = q_z(psi) (x) q_y(pitch_d) (x) q_x(roll_d)    (the 'att' model's W_R_V V_R_B)
//   q_e = q^-1 (x) q_d, negated when q_e[0] < 0;  omega_sp = (2 q_e[1] / tau_att, 2 q_e[2] / tau_att, wz_d)
//   tau = J k_rate (omega_sp - omega) + omega x J omega;  s = clip(M [F; tau], wp_idle^2, wp_max^2);  Omega_cmd = sqrt(s)
//   dOmega/dt = (Omega_cmd - Omega) / tau_mot          (tau_mot = 0: Omega = Omega_cmd, also in what is stored)
//   dp/dt = v;  dq/dt = q (x) (0, omega) / 2
//   dv/dt = R(q) Gf Omega^2 gamma_scale / m - g e_z + acc_dist + gust - R diag(drag) R^T v
//   domega/dt = (Gt Omega^2 - omega x J omega) / J
// Gf, Gt and the mixer M come by value in the argument block; the kernel knows nothing of motor geometry.  No LDS.
// Four 17-double arrays are 136 VGPRs: one wave per SIMD's budget holds them without scratch.
#include <hip/hip_runtime.h>

#include "plant_dev.h"
#include "vehicle_dev.h"
#include "vehicle_kernels.h"

namespace sdfn {

__global__ __launch_bounds__(64) void plant_vehicle_body_kernel(VehicleBodyArgs W) {
    const VehicleArgs& V = W.V;
    const PlantArgs& A = V.P;
    const long long b = (long long)blockIdx.x * 64 + threadIdx.x;
    if (b >= A.B) return;
    double x[17], u[4], ucmd[4];  // p, q, v | omega | Omega
#pragma unroll
    for (int i = 0; i < 10; ++i) x[i] = A.x[b * 10 + i];
#pragma unroll
    for (int i = 0; i < 3; ++i) x[10 + i] = W.omega[b * 3 + i];
#pragma unroll
    for (int i = 0; i < 4; ++i) x[13 + i] = W.rotor[b * 4 + i];
#pragma unroll
    for (int i = 0; i < 4; ++i) ucmd[i] = u[i] = A.u[b * 4 + i];

    const bool log = A.x_log != nullptr;
    const double* pr = A.p + b * A.p_stride;
    if (log && A.k == 0) {  // row 0: the states and the estimate the rollout starts from
        double* xl = A.x_log + b * (A.K + 1) * 10;
#pragma unroll
        for (int i = 0; i < 10; ++i) xl[i] = x[i];
        if (A.pts_log) log_point(pr, x, A.pts_log + b * (A.K + 1) * 3);
        if (V.xhat_log) {
            double* hl = V.xhat_log + b * (A.K + 1) * 10;
#pragma unroll
            for (int i = 0; i < 10; ++i) hl[i] = V.x_est[b * 10 + i];
        }
        if (W.omega_log) {
#pragma unroll
            for (int i = 0; i < 3; ++i) W.omega_log[b * (A.K + 1) * 3 + i] = x[10 + i];
        }
        if (W.rotor_log) {
#pragma unroll
            for (int i = 0; i < 4; ++i) W.rotor_log[b * (A.K + 1) * 4 + i] = x[13 + i];
        }
    }

    // ---- 1. input delay and 2. gust, as plant_vehicle_kernel
    if (V.delay > 0) {
        double* slot = V.ring + (b * V.delay + (long long)(V.frame % (unsigned)V.delay)) * 4;
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            u[i] = slot[i];
            slot[i] = ucmd[i];
        }
    }
    double w0 = 0.0, w1 = 0.0, w2 = 0.0;
    if (V.has_gust) {
        double n0, n1, n2, skip;
        const unsigned st = vstream(V, b);
        vnormal_pair(V, 0u, V.frame, st, n0, n1);
        vnormal_pair(V, 1u, V.frame, st, n2, skip);
        w0 = V.gust_phi * V.w[b * 3 + 0] + V.gust_amp * n0;
        w1 = V.gust_phi * V.w[b * 3 + 1] + V.gust_amp * n1;
        w2 = V.gust_phi * V.w[b * 3 + 2] + V.gust_amp * n2;
        V.w[b * 3 + 0] = w0;
        V.w[b * 3 + 1] = w1;
        V.w[b * 3 + 2] = w2;
    }

    // ---- 3. the setpoints of the inner loop, constant over the call
    const double F = (W.m * u[0]) * A.gamma, wz_d = u[3] * A.wz;
    double sr, cr, sp, cp;
    sincos((u[1] * A.roll) * 0.5, &sr, &cr);
    sincos((u[2] * A.pitch) * 0.5, &sp, &cp);
    const double a0 = cp * cr, a1 = cp * sr, a2 = sp * cr, a3 = -(sp * sr);  // q_y(pitch_d) (x) q_x(roll_d)
    const double fscale = A.gamma_scale ? A.gamma_scale[b] * W.im : W.im;
    const bool dist = A.acc_dist != nullptr;
    double ad0 = 0.0, ad1 = 0.0, ad2 = 0.0;
    if (dist) {
        ad0 = A.acc_dist[b * 3 + 0];
        ad1 = A.acc_dist[b * 3 + 1];
        ad2 = A.acc_dist[b * 3 + 2];
    }
    const bool lagged = W.itau_mot > 0.0;
    const double dr0 = V.drag[0], dr1 = V.drag[1], dr2 = V.drag[2];

    // f = f_expl(xs) on the 17 states; oc = the rotor speeds the inner loop commands at xs
    auto f_expl = [&](const double* xs, double* f, double* oc) {
        const double inv = prsqrt(xs[3] * xs[3] + xs[4] * xs[4] + (xs[5] * xs[5] + xs[6] * xs[6]));
        const double q0 = xs[3] * inv, q1 = xs[4] * inv, q2 = xs[5] * inv, q3 = xs[6] * inv;
        const double o0 = xs[10], o1 = xs[11], o2 = xs[12];
        // attitude loop
        const double psi = atan2((q0 * q3 + q1 * q2) * 2.0, 1.0 - (q2 * q2 + q3 * q3) * 2.0);
        double sy, cy;
        sincos(psi * 0.5, &sy, &cy);
        const double d0 = cy * a0 - sy * a3, d1 = cy * a1 - sy * a2, d2 = cy * a2 + sy * a1, d3 = cy * a3 + sy * a0;
        const double e0 = q0 * d0 + q1 * d1 + q2 * d2 + q3 * d3;  // q^-1 (x) q_d
        const double e1 = q0 * d1 - q1 * d0 - q2 * d3 + q3 * d2;
        const double e2 = q0 * d2 + q1 * d3 - q2 * d0 - q3 * d1;
        const double sg = e0 < 0.0 ? -W.katt : W.katt;
        const double ws0 = e1 * sg, ws1 = e2 * sg;
        // rate loop and mixer
        const double j0 = W.J[0] * o0, j1 = W.J[1] * o1, j2 = W.J[2] * o2;
        const double c0 = o1 * j2 - o2 * j1, c1 = o2 * j0 - o0 * j2, c2 = o0 * j1 - o1 * j0;  // omega x J omega
        const double t0 = W.J[0] * (W.k_rate[0] * (ws0 - o0)) + c0;
        const double t1 = W.J[1] * (W.k_rate[1] * (ws1 - o1)) + c1;
        const double t2 = W.J[2] * (W.k_rate[2] * (wz_d - o2)) + c2;
        double s2[4];
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const double s = W.M[i * 4] * F + W.M[i * 4 + 1] * t0 + W.M[i * 4 + 2] * t1 + W.M[i * 4 + 3] * t2;
            oc[i] = sqrt(fmin(fmax(s, W.s_min), W.s_max));
            const double om = lagged ? xs[13 + i] : oc[i];
            s2[i] = om * om;
            f[13 + i] = lagged ? (oc[i] - xs[13 + i]) * W.itau_mot : 0.0;
        }
        // rotors -> body force and torque
        double fb[3], tb[3];
#pragma unroll
        for (int r = 0; r < 3; ++r) {
            fb[r] = (W.Gf[r * 4] * s2[0] + W.Gf[r * 4 + 1] * s2[1] + W.Gf[r * 4 + 2] * s2[2] + W.Gf[r * 4 + 3] * s2[3]) * fscale;
            tb[r] = W.Gt[r * 4] * s2[0] + W.Gt[r * 4 + 1] * s2[1] + W.Gt[r * 4 + 2] * s2[2] + W.Gt[r * 4 + 3] * s2[3];
        }
        const double r11 = q0 * q0 + q1 * q1 - q2 * q2 - q3 * q3, r12 = (q1 * q2 - q0 * q3) * 2.0,
                     r13 = (q1 * q3 + q0 * q2) * 2.0;
        const double r21 = (q1 * q2 + q0 * q3) * 2.0, r22 = q0 * q0 - q1 * q1 + q2 * q2 - q3 * q3,
                     r23 = (q2 * q3 - q0 * q1) * 2.0;
        const double r31 = (q1 * q3 - q0 * q2) * 2.0, r32 = (q2 * q3 + q0 * q1) * 2.0,
                     r33 = q0 * q0 - q1 * q1 - q2 * q2 + q3 * q3;
        f[0] = xs[7];
        f[1] = xs[8];
        f[2] = xs[9];
        f[3] = (-(q1 * o0) - q2 * o1 - q3 * o2) * 0.5;
        f[4] = (q0 * o0 + q2 * o2 - q3 * o1) * 0.5;
        f[5] = (q0 * o1 - q1 * o2 + q3 * o0) * 0.5;
        f[6] = (q0 * o2 + q1 * o1 - q2 * o0) * 0.5;
        f[7] = r11 * fb[0] + r12 * fb[1] + r13 * fb[2];
        f[8] = r21 * fb[0] + r22 * fb[1] + r23 * fb[2];
        f[9] = (r31 * fb[0] + r32 * fb[1] + r33 * fb[2]) - A.g;
        if (dist) {
            f[7] = f[7] + ad0;
            f[8] = f[8] + ad1;
            f[9] = f[9] + ad2;
        }
        if (V.has_gust) {
            f[7] = f[7] + w0;
            f[8] = f[8] + w1;
            f[9] = f[9] + w2;
        }
        // ---- 4. rotor drag -R diag(d) R^T v
        if (V.has_drag) {
            const double vx = xs[7], vy = xs[8], vz = xs[9];
            const double b0 = (r11 * vx + r21 * vy + r31 * vz) * dr0;
            const double b1 = (r12 * vx + r22 * vy + r32 * vz) * dr1;
            const double b2 = (r13 * vx + r23 * vy + r33 * vz) * dr2;
            f[7] = f[7] - (r11 * b0 + r12 * b1 + r13 * b2);
            f[8] = f[8] - (r21 * b0 + r22 * b1 + r23 * b2);
            f[9] = f[9] - (r31 * b0 + r32 * b1 + r33 * b2);
        }
        f[10] = (tb[0] - c0) * W.iJ[0];
        f[11] = (tb[1] - c1) * W.iJ[1];
        f[12] = (tb[2] - c2) * W.iJ[2];
    };

    // ---- 5. ERK4 with plant_advance_kernel's tableau and accumulation order, on seventeen states
    const double h = A.dt / (double)A.substeps;
    const double hb[4] = {h / 6, h / 3, h / 3, h / 6}, ha[4] = {0.0, h / 2, h / 2, h};
    double oc[4];
    for (int sub = 0; sub < A.substeps; ++sub) {
        double xo[17], kk[17], tmp[17];
        f_expl(x, kk, oc);
#pragma unroll
        for (int i = 0; i < 17; ++i) xo[i] = x[i] + kk[i] * hb[0];
#pragma unroll
        for (int st = 1; st < 4; ++st) {
#pragma unroll
            for (int i = 0; i < 17; ++i) tmp[i] = x[i] + kk[i] * ha[st];
            f_expl(tmp, kk, oc);
#pragma unroll
            for (int i = 0; i < 17; ++i) xo[i] = xo[i] + kk[i] * hb[st];
        }
#pragma unroll
        for (int i = 0; i < 17; ++i) x[i] = xo[i];
    }
    if (!lagged) {  // the rotors are where the inner loop commands them at the new state
        double kk[17];
        f_expl(x, kk, oc);
#pragma unroll
        for (int i = 0; i < 4; ++i) x[13 + i] = oc[i];
    }

#pragma unroll
    for (int i = 0; i < 10; ++i) A.x_next[b * 10 + i] = x[i];
#pragma unroll
    for (int i = 0; i < 3; ++i) W.omega[b * 3 + i] = x[10 + i];
#pragma unroll
    for (int i = 0; i < 4; ++i) W.rotor[b * 4 + i] = x[13 + i];

    // ---- 6. the estimate the next frame's controller step reads
    double xe[10];
    vehicle_estimate(V, b, V.frame + 1u, x, xe);
#pragma unroll
    for (int i = 0; i < 10; ++i) V.x_est[b * 10 + i] = xe[i];

    if (log) {
        const long long row = b * A.K + A.k, row1 = b * (A.K + 1) + A.k + 1;
        double* xl = A.x_log + row1 * 10;
#pragma unroll
        for (int i = 0; i < 10; ++i) xl[i] = x[i];
#pragma unroll
        for (int i = 0; i < 4; ++i) A.u_log[row * 4 + i] = ucmd[i];
        if (A.status_log) A.status_log[row] = A.status[b];
        if (A.iters_log) A.iters_log[row] = A.iters[b];
        if (A.pts_log) log_point(pr, x, A.pts_log + row1 * 3);
        if (V.xhat_log) {
            double* hl = V.xhat_log + row1 * 10;
#pragma unroll
            for (int i = 0; i < 10; ++i) hl[i] = xe[i];
        }
        if (V.uapp_log) {
#pragma unroll
            for (int i = 0; i < 4; ++i) V.uapp_log[row * 4 + i] = u[i];
        }
        if (W.omega_log) {
#pragma unroll
            for (int i = 0; i < 3; ++i) W.omega_log[row1 * 3 + i] = x[10 + i];
        }
        if (W.rotor_log) {
#pragma unroll
            for (int i = 0; i < 4; ++i) W.rotor_log[row1 * 4 + i] = x[13 + i];
        }
    }
}

__global__ __launch_bounds__(64) void vehicle_body_reset_kernel(VehicleBodyArgs W) {
    const long long b = (long long)blockIdx.x * 64 + threadIdx.x;
    if (b >= W.V.P.B) return;
#pragma unroll
    for (int i = 0; i < 3; ++i) W.omega[b * 3 + i] = 0.0;
#pragma unroll
    for (int i = 0; i < 4; ++i) W.rotor[b * 4 + i] = W.hover[i];
}

hipError_t launch_vehicle_body(const VehicleBodyArgs& a, hipStream_t s) {
    if (a.V.P.B <= 0) return hipSuccess;
    hipLaunchKernelGGL(plant_vehicle_body_kernel, dim3((unsigned)((a.V.P.B + 63) / 64)), dim3(64), 0, s, a);
    return hipGetLastError();
}

hipError_t launch_vehicle_body_reset(const VehicleBodyArgs& a, hipStream_t s) {
    if (a.V.P.B <= 0) return hipSuccess;
    hipLaunchKernelGGL(vehicle_body_reset_kernel, dim3((unsigned)((a.V.P.B + 63) / 64)), dim3(64), 0, s, a);
    return hipGetLastError();
}

}  // namespace sdfn
