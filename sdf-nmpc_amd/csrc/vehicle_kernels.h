// The vehicle model of a closed loop (vehicle.hip): argument block shared with the engine and the solver object.
#pragma once
#include <hip/hip_runtime.h>

#include "plant_kernels.h"

namespace sdfn {

constexpr int VEHICLE_MAX_DELAY = 8;

struct VehicleArgs {
    // the plant's block: x = x_next = the vehicle's true state, u = the command, the log rows as in a rollout
    PlantArgs P;
    unsigned frame;                 // f: the gust's frame; the estimate written is that of frame f + 1
    unsigned key0, key1;            // the seed's two words
    int delay;                      // d control periods, 0..VEHICLE_MAX_DELAY
    double itau_m;                  // 1 / tau_m, 0: no thrust lag
    double drag[3];
    bool has_drag;
    double gust_phi, gust_amp;      // exp(-dt / tau_g) and sigma_g sqrt(1 - phi^2)
    bool has_gust;
    double est_std_p, est_std_v, est_std_yaw;
    bool est_noise;                 // any of the three > 0
    const double* est_bias;         // [B][7] (p, v, yaw) or NULL
    const int* stream_id;           // [B] or NULL: the instance index
    double* gamma_act;              // [B]
    double* w;                      // [B][3]
    double* ring;                   // [B][delay][4]
    double* x_est;                  // [B][10]: the estimate (row 0 of xhat_log is read from it at k == 0)
    double* xhat_log;               // [B][K+1][10] or NULL
    double* uapp_log;               // [B][K][4] or NULL
    double g, hover_u0;             // vehicle_reset: gamma_act and the ring's thrust input
};

// The rigid-body vehicle (vehicle_body.hip): the vehicle's block and the body's constants by value, its hidden states
// and logs.  The kernel knows nothing of motor geometry: the matrices come from the caller.
struct VehicleBodyArgs {
    VehicleArgs V;                  // delay, gust, drag and estimate as in plant_vehicle_kernel; itau_m is unused
    double m, im;                   // mass and 1 / mass
    double J[3], iJ[3];             // inertia diagonal and its reciprocals
    double Gf[12], Gt[12];          // [3][4] row-major: force and torque of the squared rotor speeds
    double M[16];                   // [4][4] row-major: squared speeds = M [F; tau]
    double s_min, s_max;            // wp_idle^2, wp_max^2
    double katt;                    // 2 / tau_att
    double k_rate[3];
    double itau_mot;                // 1 / tau_mot, 0: the rotors follow their command algebraically
    double hover[4];                // vehicle_body_reset: sqrt(M [m g; 0; 0; 0])
    double* omega;                  // [B][3] body rate, body frame
    double* rotor;                  // [B][4] rotor speeds
    double* omega_log;              // [B][K+1][3] or NULL
    double* rotor_log;              // [B][K+1][4] or NULL
};

hipError_t launch_vehicle(const VehicleArgs& a, hipStream_t s);
hipError_t launch_vehicle_body(const VehicleBodyArgs& a, hipStream_t s);
// omega <- 0, rotor <- hover
hipError_t launch_vehicle_body_reset(const VehicleBodyArgs& a, hipStream_t s);
// x_true = P.x_next <- x_est; x_est <- est(x_true, frame)
hipError_t launch_vehicle_begin(const VehicleArgs& a, hipStream_t s);
// ring <- hover, gamma_act <- g, w <- 0
hipError_t launch_vehicle_reset(const VehicleArgs& a, hipStream_t s);

}  // namespace sdfn
