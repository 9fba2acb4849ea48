// Device code shared by the two plant kernels (plant.hip, vehicle.hip): the value-only f_expl of both models, in
// the operation order of linearize.hip's quad_f / quad_f_tau, and the camera-frame log point.
#pragma once
#include <hip/hip_runtime.h>

namespace sdfn {

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

}  // namespace sdfn
