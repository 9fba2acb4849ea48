/* sdfnmpc.h -- C ABI of the MI355X-native neural-SDF NMPC evaluator (libsdfnmpc.so).
 *
 * Plain pointers and sizes only: no torch types, no C++ types.  Every entry point returns
 * SDFNMPC_OK (0) or a negative error code and never throws; sdfnmpc_last_error() gives the message
 * (thread-local).  Device pointers are HIP device pointers on the context's device; work is enqueued
 * on the context's stream (asynchronous unless stated otherwise).
 *
 * Which reference interface each entry point replaces (paths relative to the reference checkout):
 *
 *   sdfnmpc_net_load / _load_file      torch.jit.load(sdf weights) + .to(device) + .eval()
 *                                      (sdf_nmpc/gen_model.py:32-34); weights as a packed .sdfw blob
 *   sdfnmpc_net_siren                  NeuralDF(...) + init_linear_layer_sine (df_train.py:109-110,
 *                                      layer_init.py:15-25) with a counter-based PRNG
 *   sdfnmpc_sdf_eval                   NeuralDF.forward (network/neural_df.py:91-103) + autograd
 *                                      d df / d input, batched over rows -- what L4CasADi's
 *                                      sdf_l4c / jac_sdf_l4c compute one row at a time
 *                                      (gen_model.py:39,60)
 *   sdfnmpc_linearize                  the per-node evaluations acados performs in the SQP-RTI
 *                                      preparation phase of Ocp.solve (ocp.py:159-170, rti_phase 0):
 *                                      ERK4 + forward sensitivities (ocp.py:106), NONLINEAR_LS residual
 *                                      and Jacobian (model/quad_rollpitchyawrate.py:48-55), and the
 *                                      constraint vector h = [hfov, vfov, sdf] with its Jacobian
 *                                      (model/cost_const_helpers.py:48-75, gen_model.py:46-70)
 *   sdfnmpc_qp_solve                   the feedback phase of the same SQP-RTI step: the QP acados
 *                                      builds (NONLINEAR_LS Gauss-Newton + levenberg_marquardt, soft
 *                                      h rows, input boxes, ocp.py:54-120) and hands to HPIPM
 *                                      (FULL_CONDENSING_HPIPM, ocp.py:113-116), batched over instances
 *   sdfnmpc_rti_apply                  the SQP-RTI full step x <- x + dx, u <- u + du and u_0
 *                                      (solve_for_x0's return value, ocp.py:169)
 *   sdfnmpc_shooting_grid              Ocp.__init__ shooting nodes / time steps (ocp.py:18-27)
 *   sdfnmpc_solver_*                   the AcadosOcpSolver object Ocp builds (ocp.py:127) and drives:
 *                                      solver.set(k, 'x'|'u'|'p') / cost_set(k, 'yref'|'W') (ocp.py:
 *                                      146-170) -> _upload; solver.get -> _download; reset + init
 *                                      (ocp.py:144-149) -> _init; shift (ocp.py:152-156) -> _shift;
 *                                      solve_for_x0 (ocp.py:169) -> _step + _wait.  It owns the device
 *                                      workspace of B instances, so a controller needs no tensor library
 *
 *   sdfnmpc_plant_step                 (no reference interface: the reference's plant is the simulator it is run against)
 *                                      x_next = RK4^substeps of the 'att' / 'att_tau' f_expl (model/
 *                                      quad_rollpitchyawrate.py:19-55, quad_rollpitchyawrate_tau.py:19-58) per
 *                                      instance, optionally with a disturbance acceleration and a thrust-gain error
 *   sdfnmpc_solver_rollout             K iterations of the loop a user of Nmpc writes around it (controller.py:
 *                                      65-81 set_x0 + solve, with RefGen before and the simulator after), enqueued
 *                                      without a host round trip: references from x0, shift, RTI step, plant
 *   sdfnmpc_vehicle_* / sdfnmpc_plant_step_vehicle
 *                                      (no reference interface) an imperfect vehicle and estimator around the plant:
 *                                      input delay, thrust lag, rotor drag, gusts, bias and noise on the state
 *                                      estimate, reproducible per (seed, instance, frame); sdfnmpc_rollout_args.vehicle
 *                                      carries it through every rollout; sdfnmpc_vehicle_set_body makes it a rigid
 *                                      body (model/quad_props.py:41-48) under an attitude and rate loop and rotors
 *                                      with a speed lag
 *
 *   sdfnmpc_colcheck                   ColChecker.check_image_points (utils/collision_checker.py:23-125)
 *   sdfnmpc_udf / sdfnmpc_sdf_truth    DfComputer.get_udf / get_sdf (utils/df_computer.py:85-221): the distance
 *                                      field the image itself implies, to label data and to score a network
 *
 *   sdfnmpc_scene_*                    (no reference interface: the reference's images come from the simulator it is
 *                                      run against) range / depth images of an analytic scene from a camera pose,
 *                                      the camera pose of a state (controller.py:52-53), the exact signed distance;
 *                                      primitives may be oriented and may move (_create_moving, _render_at,
 *                                      _distance_at, sdfnmpc_solver_rollout_perceive_at)
 *   sdfnmpc_solver_rollout_perceive    sdfnmpc_solver_rollout with the perception a user wraps around it every
 *                                      control period: VaeWrapper.set_img / encode (sdf_nmpc/vae.py:29-40) of a new
 *                                      image and Nmpc.set_latent (controller.py:50-54) with the pose at image time
 *   sdfnmpc_scene_sdf_rows             (no reference interface: the reference's SDF is always the network) what the
 *                                      network's epilogue writes as the sdf row of h / J_h (gen_model.py:46-61),
 *                                      from the scene's exact distance; sdfnmpc_lin_args.sdf_scene, sdfnmpc_solver_
 *                                      set_sdf_scene and sdfnmpc_solver_rollout_scene_sdf carry it through the step
 *   sdfnmpc_img_sdf_rows               DfComputer.get_df (utils/df_computer.py:152-221), the network's training target
 *                                      (scripts/neural_nets/df_train.py:52,123,168), under the same epilogue at the
 *                                      node positions of the batch: the field the camera image itself implies, in
 *                                      the frame of the image; sdfnmpc_lin_args.sdf_image, sdfnmpc_solver_set_sdf_image
 *                                      and sdfnmpc_solver_rollout_image_sdf carry it through the step
 *   sdfnmpc_vae_decode                 VaeWrapper.decode (sdf_nmpc/vae.py:42-45): Decoder.forward (network/vae.py:63-90),
 *                                      the image a latent retains; sdfnmpc_solver_rollout_image_recon flies on it (the
 *                                      image source holds the reconstruction of every new camera image)
 *   sdfnmpc_morph / sdfnmpc_outlier_rm Dilate / Erode (and with them Open / Close) and RemoveCloseOutliers
 *                                      (utils/preprocessing.py:100-259), batched
 *   sdfnmpc_sensor_apply               ImageAugmenter's noise and erasing (utils/data.py:11-108) as a reproducible
 *                                      sensor model, also inside the rollout (sdfnmpc_solver_rollout_perceive_sensor)
 *
 * The CasADi external-function symbols that acados links (sdf_l4c, jac_sdf_l4c, ...) are in
 * sdf_l4c.h / libsdf_l4c.so.
 */
#ifndef SDFNMPC_H
#define SDFNMPC_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define SDFNMPC_ABI_VERSION 19

enum {
    SDFNMPC_OK = 0,
    SDFNMPC_E_ARG = -1,          /* invalid argument / shape */
    SDFNMPC_E_HIP = -2,          /* HIP runtime error (message has the HIP error string) */
    SDFNMPC_E_FORMAT = -3,       /* malformed weight blob */
    SDFNMPC_E_UNSUPPORTED = -4,  /* network architecture / model option not built for */
    SDFNMPC_E_NODEVICE = -5      /* no HIP device visible */
};

typedef struct sdfnmpc_ctx sdfnmpc_ctx;
typedef struct sdfnmpc_net sdfnmpc_net;
typedef struct sdfnmpc_scene sdfnmpc_scene;

/* An analytic scene as the source of the SDF row (csrc/scene_sdf.hip, sdfnmpc_scene_sdf_rows below): the scene
 * set, the scene of each instance, the truncation distance and the scene's time at the nodes. */
typedef struct {
    const sdfnmpc_scene* scene;  /* on the caller's context */
    const int* scene_of;         /* device [B] or NULL (scene 0); entries clamped into [0, S) as by every scene kernel */
    double max_df;               /* > 0, finite: distances are truncated there (df_train.py:50) */
    double t0;                   /* finite: the scene's time at node 0 */
    const double* tau;           /* device [N+1] or NULL: node k sees the scene at t0 + tau[k]; NULL: every node at t0 */
} sdfnmpc_scene_sdf_opts;
/* A camera image as the source of the SDF row (sdfnmpc_img_sdf_rows, defined with the image ground truth below) */
typedef struct sdfnmpc_img_sdf_opts sdfnmpc_img_sdf_opts;

#define SDFNMPC_POLY_DEG_MAX 6 /* braking-distance polynomial: degree bound ... */
#define SDFNMPC_POLY_MAX 84    /* ... and its coefficient count (deg + 3 choose 3) */
#define SDFNMPC_NHN_MAX 8      /* terminal constraint rows (soft <= 3, hard <= 6) */
#define SDFNMPC_NHE 6          /* terminal extra functions hE (sdfnmpc_lin_args) */

/* 'att' / 'att_tau' model constants (model/quad_rollpitchyawrate.py; config robot.limits / sensor / mpc) and the
 * terminal ingredients of flags.recursive_feasibility / flags.stability (gen_model.py:72-149) */
typedef struct {
    double gamma, roll, pitch, wz; /* robot.limits.{gamma, roll, pitch, wz}: u -> physical inputs */
    double g;                      /* gravity, 9.81 (model/base_model.py:10) */
    double B_p_C[3];               /* sensor.B_p_C (utils/config.py:43) */
    double B_R_C[9];               /* sensor.B_R_C, row-major (utils/config.py:44) */
    double fov_const_offset;       /* mpc.fov_const_offset (cost_const_helpers.py:65) */
    int rec_feas;                  /* 1: the preparation phase evaluates the terminal extras hE[0..2] (below) */
    int stability;                 /* 1: hE[3..5] = v_N, and the terminal residual y_N is scaled by the flag and
                                      gains the row flag |v|^2 (quad_rollpitchyawrate.py:52-55, gen_model.py:
                                      142-149): nyN = 5 */
    int poly_deg;                  /* braking-distance polynomial degree (mpc.braking_dist.degree, <= 6) */
    double poly[SDFNMPC_POLY_MAX]; /* its coefficients in polynomial_3variate's term order (utils/math.py:
                                      307-314: total degree 0..deg, then x exponent a, then y exponent b) */
    int kind;                      /* mpc.model: SDFNMPC_MODEL_ATT (0) or SDFNMPC_MODEL_ATT_TAU (1, model/
                                      quad_rollpitchyawrate_tau.py: roll and pitch follow their commands with a
                                      first-order lag; same dimensions, residual layout and bounds).  Any other
                                      value, and kind 1 with rec_feas or stability (gen_model.py:74: "only for
                                      'att'"), is refused with SDFNMPC_E_UNSUPPORTED */
    double tau_roll, tau_pitch;    /* kind 1: the lags' time constants in seconds, > 0 (the reference's 0.12) */
} sdfnmpc_quad_model;

#define SDFNMPC_MODEL_ATT 0
#define SDFNMPC_MODEL_ATT_TAU 1

/* Batched preparation phase: B instances x (N+1) shooting nodes, fp64, row-major C arrays.
 * Jacobian blocks are column-major (column j contiguous), j over (x[0..9], u[0..3]). */
typedef struct {
    int B, N;         /* instances, horizon */
    int np;           /* parameters per node, >= 17 + 128 (p layout: default.yaml mpc.p_idx) */
    int latent_mode;  /* 0: latent shared per instance (node 0's, as Nmpc.set_latent writes all
                         rows, controller.py:50-54); 1: latent read per node */
    const double* x;  /* [B][N+1][10] current iterate */
    const double* u;  /* [B][N][4] */
    const double* p;  /* [B][N+1][np] stage parameters (Ocp.solve p[k], ocp.py:165,168) */
    const double* dt; /* [N] time steps (sdfnmpc_shooting_grid) */
    double* xn;       /* [B][N][10]      x_{k+1} = RK4(x_k, u_k, dt_k) */
    double* AB;       /* [B][N][14][10]  [A_k | B_k] column-major */
    double* y;        /* [B][N][11]      NONLINEAR_LS residual */
    double* Jy;       /* [B][N][14][11]  column-major */
    double* yN;       /* [B][4]          terminal residual */
    double* JyN;      /* [B][10][4]      column-major */
    double* h;        /* [B][N+1][3]     the three node functions [hfov, vfov, sdf] in fixed columns: which
                                            of them are rows of the OCP is the QP's constraint set
                                            (sdfnmpc_qp_opts.nh / h_col) */
    double* Jh;       /* [B][N+1][10][3] column-major, d h / d x (d h / d u == 0) */
    float* sdf;       /* [B][N+1][4]     optional: (df, d df / d Co_p_B); NULL = internal buffer */
    int nyN;          /* terminal residual rows: 4, or 5 with sdfnmpc_quad_model.stability (yN [B][nyN],
                         JyN [B][10][nyN]) */
    int no_sdf;       /* 1: no constraint or cost uses the network (enable_sdf False, or neither sdf_constraint,
                         sdf_cost nor rec_feas): the SDF kernels are skipped, h[.][2] is not written and
                         net may be NULL */
    double* hE;       /* [B][6]          terminal extras (NULL unless rec_feas / stability): [-flag poly(v),
                         flag atan2(E_y, E_x), flag atan2(E_z, |E_xy|), v_x, v_y, v_z] with E = Co_p_E, the
                         camera-frame point at the braking distance ahead (gen_model.py:98-112); the
                         rec_feas constraint value is h[N][2] + hE[0] (gen_model.py:94-95) */
    double* JhE;      /* [B][10][6]      column-major d hE / d x_N */
    const sdfnmpc_scene_sdf_opts* sdf_scene; /* NULL: the network.  Else the SDF row h[.][2] / J_h[.][.][2] is the
                         exact distance of this scene (sdfnmpc_scene_sdf_rows on x, p, h, Jh): net may be NULL and no
                         network is evaluated; linearize, then the rows kernel, then the record pack, on the context
                         stream.  Refused together with no_sdf (SDFNMPC_E_ARG), and by sdfnmpc_step_create
                         (SDFNMPC_E_UNSUPPORTED) */
    const sdfnmpc_img_sdf_opts* sdf_image; /* NULL: the network.  Else the SDF row is the field of this camera image
                         (sdfnmpc_img_sdf_rows on x, p, h, Jh), with the semantics of sdf_scene: net may be NULL;
                         linearize, then the rows kernel, then the record pack, on the context stream, no fork.  Refused
                         together with no_sdf and together with sdf_scene (SDFNMPC_E_ARG), and by sdfnmpc_step_create
                         (SDFNMPC_E_UNSUPPORTED) */
} sdfnmpc_lin_args;

/* QP model data and solver options (defaults in sdf-nmpc_amd/model.py / ocp.py) */
typedef struct {
    double lbu[4], ubu[4]; /* input box (model/quad_rollpitchyawrate.py:58-59) */
    double lh[3], uh[3];   /* h bounds: +-fov_ratio*fov, [size.xy+bound_margin, max_df+0.2] */
    double zl[3], Zl[3];   /* L1 / L2 slack penalties of the soft h rows, lower == upper (ocp.py:85-92) */
    double lm;             /* levenberg_marquardt (ocp.py:120, mpc.lm_reg) */
    int cost_scaling;      /* 1: stage cost and slack penalties x dt_k, terminal x 1 (acados default) */
    int max_iter;          /* qp_solver_iter_max (ocp.py:115) */
    double tol;            /* IPM stop: max complementarity max_i t_i lambda_i and max primal residual below
                              tol (HPIPM's res_m / res_b tests) */
    int ny;                /* stage residuals: 11, or 12 with flags.sdf_cost (gen_model.py:65-66): the 12th,
                              (1 - s/2)^4 of the flagged SDF value s = h[2], and its Jacobian
                              -2 (1 - s/2)^3 J_h[2] are formed from h / J_h by the QP (yref, W: [B][N][ny]) */
    int lm_scaling;        /* 1: Levenberg-Marquardt term lm dt_k at stages k < N and lm at N (acados adds
                              Ts[k] * levenberg_marquardt); 0: lm at every node */
    int warm_start;        /* qp_solver_warm_start (ocp.py:116, HPIPM's primal warm start): 1 = the IPM starts
                              from the du found in sdfnmpc_qp_args.du on entry (the previous QP's solution --
                              the solver object keeps it between steps; zero after init), dx rolled out from
                              x0 under it, t / lambda by the cold start's rule; 0 = du = 0 (cold) */
    /* The constraint set (gen_model.py:26-149 under flags.enable_sdf / sdf_constraint / vfov_constraint /
     * recursive_feasibility / stability and sensor.hfov < 3.14; sdf-nmpc_amd/model.py builds it).
     * Stage rows k < N: nh rows, row j = column h_col[j] of h / J_h, with bounds / slack weights lh[j], uh[j],
     * zl[j], Zl[j] above; the first nh - nhs soft, the last nhs hard (slack weight None: add_const_stage,
     * base_model.py:142-155; zl / Zl unused).  Terminal rows: nhN rows, the first nsN soft
     * (lhN / uhN, slack weights zlN / ZlN, not cost-scaled), the rest hard; row j's value is
     * h[N][hN_col[j]] (if >= 0) + hE[hE_col[j]] (if >= 0), its Jacobian the same sum of columns. */
    int nh;                /* 0..3 (3: [hfov, vfov, sdf], the default flags) */
    int h_col[3];          /* distinct columns 0..2 */
    int nhN, nsN;          /* nhN <= SDFNMPC_NHN_MAX, nsN <= min(nhN, 3), nhN - nsN <= 6 */
    int hN_col[SDFNMPC_NHN_MAX], hE_col[SDFNMPC_NHN_MAX];
    double lhN[SDFNMPC_NHN_MAX], uhN[SDFNMPC_NHN_MAX], zlN[3], ZlN[3];
    int nyN;               /* terminal residual rows (yNref / WN [B][nyN]): 4, or 5 with flags.stability */
    int nhs;               /* hard stage rows (the last nhs of the nh), 0..nh: mpc.weights.slack_fov / slack_df
                              None (the terminal copies of those rows are then hard rows of the nhN too) */
} sdfnmpc_qp_opts;

/* Batched QP of the RTI feedback phase, built from sdfnmpc_linearize outputs. */
typedef struct {
    int B, N;
    const double *xn, *AB, *y, *Jy, *yN, *JyN, *h, *Jh; /* sdfnmpc_lin_args outputs */
    const double *hE, *JhE; /* sdfnmpc_lin_args outputs (NULL when no terminal row reads them) */
    const double* x;     /* [B][N+1][10] iterate the QP was built at */
    const double* u;     /* [B][N][4] */
    const double* x0;    /* [B][10] measured state (Ocp.solve x0) */
    const double* yref;  /* [B][N][ny] stage references (Ocp.solve y[k]) */
    const double* W;     /* [B][N][ny] diagonal weights (Ocp.solve W[k], set as np.diag) */
    const double* yNref; /* [B][nyN] */
    const double* WN;    /* [B][nyN] */
    const double* dt;    /* [N] */
    double* dx;          /* [B][N+1][10] solution: the RTI step */
    double* du;          /* [B][N][4] */
    double* slack;       /* [B][N+1][3][2] optional: (sl, su) of the soft rows (row j of node k < N; terminal
                            soft row j at node N; unused entries 0) */
    int* status;         /* [B] optional: 0 converged, 1 max_iter reached (acados status 2: the step is
                            kept), 2 numerical failure -- a NaN / Inf in the data (acados QP failure,
                            status 4: sdfnmpc_rti_apply given this array keeps the instance's iterate) */
    int* iters;          /* [B] optional */
    double* res;         /* [B][2] optional: (max complementarity, max primal residual) */
} sdfnmpc_qp_args;

/* Batched reference / parameter packing: RefGen (ref_gen.py:17-130) ->
 * formate_ref (quad_rollpitchyawrate.py:62-65) -> Nmpc.set_ref / set_latent / set_sdf_flag
 * (controller.py:45-54,133-142) for B instances x (N+1) nodes on the device. */
typedef struct {
    int mode;              /* 0 gen_ref_list_wps, 1 gen_ref_joystick, 2 from_x0, -1 latent / flag only, -2 pose only:
                              p[:, :, 1:13] of every node from W_p_Bo / W_R_Bo (required) and the extrinsics, the
                              bits mode -1 writes there; flag and latent columns untouched (latent / flag ignored) */
    int yaw_mode;          /* path samples: 0 identity, 1 'ref', 2 'align', 3 x0 quaternion ('curent', sic) */
    int st_enable;         /* ref.stop_and_turn.enable */
    int st_mode;           /* stop-and-turn yaw: 0 current, 1 'topic', 2 'align' */
    double st_dang;        /* ref.stop_and_turn.dang_min */
    double align_off;      /* ref.align_yaw_offset */
    double dmin;           /* ref.yaw_align_dmin */
    double vref, wzref;    /* ref.vref, ref.wzref */
    double T;              /* mpc.T */
    double B_p_C[3], B_R_C[9]; /* sensor extrinsics (config.py) */
} sdfnmpc_ref_opts;

typedef struct {
    int B, N, np, ny;      /* np = 17 + latent size; ny = 11 or 12 (sdf_cost) */
    int n_wp;              /* waypoints per instance (mode 0), <= 32 */
    int L;                 /* latent size (when latent != NULL) */
    const double* x0;      /* [B][x0_stride] current state */
    int x0_stride;
    const double* wp_p;    /* [B][n_wp][3] (mode 0) */
    const double* wp_q;    /* [B][n_wp][4] (mode 0) */
    const double* vw;      /* [B][4] (vx, vy, vz, wz) in [-1, 1] (mode 1) */
    const double* wrow;    /* [ny] the W row formate_ref builds from the caller's weight set */
    const double* latent;  /* [B][L] or NULL (then W_p_Bo / W_R_Bo are ignored) */
    const double* W_p_Bo;  /* [B][3] body position at image time */
    const double* W_R_Bo;  /* [B][9] body attitude at image time, row-major */
    const double* flag;    /* [B] sdf flag or NULL */
    double* p;             /* [B][N+1][np] OCP parameters */
    double* yref;          /* [B][N][ny] */
    double* W;             /* [B][N][ny] */
    double* yNref;         /* [B][nyN] */
    double* WN;            /* [B][nyN] */
    int nyN;               /* terminal residual rows: 4, or 5 with flags.stability (y[:nyN] / W[:nyN] of the
                              last node, controller.py:141-142; 0 is taken as 4) */
} sdfnmpc_ref_args;

int sdfnmpc_abi_version(void);
const char* sdfnmpc_last_error(void);

/* ---- context: one device + one stream (+ workspaces, kernel timing) ---- */
int sdfnmpc_ctx_create(int device, void* hip_stream /* NULL: create a non-blocking stream */, sdfnmpc_ctx** out);
void sdfnmpc_ctx_destroy(sdfnmpc_ctx* ctx);
int sdfnmpc_ctx_set_stream(sdfnmpc_ctx* ctx, void* hip_stream);
/* launch on the legacy null stream (handle 0, e.g. PyTorch's default stream) */
int sdfnmpc_ctx_use_null_stream(sdfnmpc_ctx* ctx);
void* sdfnmpc_ctx_stream(sdfnmpc_ctx* ctx);
int sdfnmpc_ctx_device(const sdfnmpc_ctx* ctx);
int sdfnmpc_ctx_synchronize(sdfnmpc_ctx* ctx);
/* the feedback-phase IPM kernel: SEGMENTED runs every instance on one workgroup of four wavefronts with a
 * partitioned (parallel-in-time) Riccati recursion (csrc/rti_qp_seg.hip); SERIAL on one wavefront
 * (csrc/rti_qp.hip).  AUTO (default) = SEGMENTED for batches of at most SDFNMPC_QP_SEG_AUTO_MAX_B
 * instances (twice that from N = 48) at horizons SDFNMPC_QP_SEG_AUTO_MIN_N <= N <= 63 (8-10 % faster
 * at N = 40, 21-24 % at N = 60 up to B = 512), SERIAL otherwise (large batches at N < 48: one wavefront
 * per SIMD is the throughput regime; short horizons, where the couplings outweigh the segments).  Both solve the same QP to the same stop test; their iterates
 * agree to rounding, not bitwise.  SDFNMPC_QP_KERNEL=serial|segmented sets the default of new contexts. */
#define SDFNMPC_QP_AUTO 0
#define SDFNMPC_QP_SERIAL 1
#define SDFNMPC_QP_SEGMENTED 2
#define SDFNMPC_QP_SEG_AUTO_MAX_B 256
#define SDFNMPC_QP_SEG_AUTO_MIN_N 36
int sdfnmpc_ctx_set_qp_kernel(sdfnmpc_ctx* ctx, int kernel);
/* the kernel a QP batch of B instances at horizon N runs on this context (SDFNMPC_QP_SERIAL or
 * _SEGMENTED; -1 on bad arguments) */
int sdfnmpc_ctx_qp_kernel(const sdfnmpc_ctx* ctx, int N, int B);
/* the same for the constraint set of opts (NULL: the default set; -1 on a malformed set).  Both kernels serve
 * every constraint set sdfnmpc_qp_opts describes (soft / hard stage rows, rec_feas and stability terminal
 * rows), so the choice is the batch / horizon policy above.  Replaces acados' one HPIPM instance per solver
 * (ocp.py:113-120). */
int sdfnmpc_ctx_qp_kernel_for(const sdfnmpc_ctx* ctx, int N, int B, const sdfnmpc_qp_opts* opts);
/* segments (wavefronts) per instance of the SEGMENTED kernel at horizon N: 4 for 7 <= N <= 63, 3 for N = 5, 6,
 * 2 for N = 3, 4; 0 where it does not serve N (the SERIAL kernel runs then).  Read-only; follows the
 * diagnostic SDFNMPC_QP_NSEG as the launch does. */
int sdfnmpc_qp_seg_count(int N);
/* LDS bytes one instance of the serial QP kernel holds at horizon N (-1: N < 1) */
long long sdfnmpc_qp_lds_bytes(int N);
/* the occupancy gate of SURVEY.md §8(e): instances the context's device solves in one wave of QP
 * workgroups at horizon N = CUs x min(LDS per CU / LDS per instance, the runtime's occupancy of the
 * kernel sdfnmpc_ctx_qp_kernel picks -- registers and waves included), from hipDeviceProp_t and
 * hipOccupancyMaxActiveBlocksPerMultiprocessor (1024 at N = 20 and 40 on an MI355X: the serial kernel's
 * registers allow four instances per CU); 0 when N does not fit one CU, -1 on bad arguments.  Replaces the reference's single acados solver per process
 * (controller.py:16 builds one Ocp): a batch larger than this is split over devices (shard.plan). */
long long sdfnmpc_qp_capacity(const sdfnmpc_ctx* ctx, int N);
/* the same for the constraint set of opts (its rows change the LDS per instance; NULL: the default set) */
long long sdfnmpc_qp_capacity_for(const sdfnmpc_ctx* ctx, int N, const sdfnmpc_qp_opts* opts);
/* rows per SDF workgroup: 32 (2 workgroups / CU) or 64 (1 workgroup / CU); default 32 */
int sdfnmpc_ctx_set_tile_rows(sdfnmpc_ctx* ctx, int rows);
/* per-kernel HIP-event timing on the context stream (off by default) */
int sdfnmpc_ctx_enable_timing(sdfnmpc_ctx* ctx, int on);
/* kernel: "sdf_mlp", "sdf_hoist", "linearize", "rti_qp", "plant", "scene_render", "scene_pose", "scene_dist",
 * "scene_render_dyn", "scene_dist_dyn", "scene_render_grid", "scene_dist_grid", "scene_sdf_rows_grid", "morph", "outlier_rm", "sensor_degrade",
 * "plant_vehicle", "plant_vehicle_body", "vehicle_begin", "vehicle_reset", ...; synchronizes the stream(s) */
int sdfnmpc_ctx_kernel_stats(sdfnmpc_ctx* ctx, const char* kernel, double* total_ms, long long* launches);
int sdfnmpc_ctx_reset_stats(sdfnmpc_ctx* ctx);

/* ---- network ---- */
int sdfnmpc_net_load(sdfnmpc_ctx* ctx, const void* blob, size_t bytes, sdfnmpc_net** out);
int sdfnmpc_net_load_file(sdfnmpc_ctx* ctx, const char* path, sdfnmpc_net** out);
int sdfnmpc_net_siren(sdfnmpc_ctx* ctx, uint64_t seed, float weight_gain, float bias_gain, sdfnmpc_net** out);
void sdfnmpc_net_free(sdfnmpc_net* net);
float sdfnmpc_net_max_df(const sdfnmpc_net* net);
int sdfnmpc_net_size_latent(const sdfnmpc_net* net);
/* FNV-1a of the fp32 parameters in torch order (identity check across ranks / files) */
uint64_t sdfnmpc_net_fingerprint(const sdfnmpc_net* net);

/* ---- SDF evaluation, device pointers ----
 * pos4[rows][4] = (Co_p_B, unused); latent[n_inst][128] fp32 with row r -> instance r / rows_per_inst;
 * out4[rows][4] = (df, d df / d pos); grad_latent[rows][128] optional (NULL to skip). */
int sdfnmpc_sdf_eval(sdfnmpc_ctx* ctx, const sdfnmpc_net* net, long long rows, const float* pos4,
                     const float* latent, int rows_per_inst, float* out4, float* grad_latent);

/* ---- SDF evaluation, host pointers, synchronous (the CasADi external path) ----
 * in[rows][3+128] doubles (the L4CasADi input vertcat(Co_p_B, latent), gen_model.py:60) ->
 * df[rows], grad[rows][3+128] (optional). Computed in fp32 on the device, returned as fp64. */
int sdfnmpc_sdf_eval_host(sdfnmpc_ctx* ctx, const sdfnmpc_net* net, int rows, const double* in, double* df,
                          double* grad);
/* Calls of sdfnmpc_sdf_eval_host with at most 16 rows (the CasADi external's one row per node) are
 * served by a resident server kernel: one persistent workgroup on its own stream polls a mailbox in
 * pinned host memory, so a call costs no launch, no copies and no stream synchronisation.  It exits
 * after SDFNMPC_SDF_SERVER_IDLE_MS (default 20) without a request, on sdfnmpc_ctx_destroy, or after 10 s
 * (relaunched on the next call).  on = 0 stops it and returns to one launch per call (also
 * SDFNMPC_SDF_SERVER=0); results are bitwise the same either way. */
int sdfnmpc_ctx_set_sdf_server(sdfnmpc_ctx* ctx, int on);
/* diagnostics: mean microseconds per served request since the last call -- out18[0] staging the request,
 * [1] evaluating it, [2] the caller's wait from posting to the answer; out18[3] = requests;
 * out18[4..17] the evaluation's phases (embedding, 4 x (layer GEMV, sine), the last sine, 4 backward
 * GEMVs, outputs) */
int sdfnmpc_ctx_sdf_server_stats(sdfnmpc_ctx* ctx, double* out18);

/* ---- batched preparation phase ---- */
int sdfnmpc_linearize(sdfnmpc_ctx* ctx, const sdfnmpc_net* net, const sdfnmpc_quad_model* model,
                      const sdfnmpc_lin_args* args);

/* ---- batched QP (feedback phase) and the RTI step ---- */
int sdfnmpc_qp_solve(sdfnmpc_ctx* ctx, const sdfnmpc_qp_opts* opts, const sdfnmpc_qp_args* args);
/* The same SQP-RTI step split the way acados splits it (rti_phase 1 / 2, ocp.py:110): everything that
 * does not depend on x0 -- the linearisation and the QP's stage records (H, g, dynamics, constraint
 * rows) -- in the preparation phase, the IPM alone in the feedback phase.  sdfnmpc_rti_prepare =
 * sdfnmpc_linearize + the record pack (qp_args must name lin_args' iterate and outputs; the pack runs
 * beside the SDF kernel); sdfnmpc_qp_feedback = the IPM on those records, once per preparation
 * (SDFNMPC_E_ARG without a matching sdfnmpc_rti_prepare).  Results are bitwise those of
 * sdfnmpc_linearize + sdfnmpc_qp_solve. */
int sdfnmpc_rti_prepare(sdfnmpc_ctx* ctx, const sdfnmpc_net* net, const sdfnmpc_quad_model* model,
                        const sdfnmpc_lin_args* lin_args, const sdfnmpc_qp_opts* opts, const sdfnmpc_qp_args* qp_args);
int sdfnmpc_qp_feedback(sdfnmpc_ctx* ctx, const sdfnmpc_qp_opts* opts, const sdfnmpc_qp_args* args);
/* x[B][N+1][10] += dx, u[B][N][4] += du, u0[B][4] = u[:, 0] (u0 may be NULL).  status [B] (may be NULL):
 * instances with status >= 2 (QP failure) keep x and u; their u0 is the unchanged u[:, 0]. */
int sdfnmpc_rti_apply(sdfnmpc_ctx* ctx, int B, int N, double* x, double* u, const double* dx, const double* du,
                      double* u0, const int* status);

/* One whole SQP-RTI control step -- sdfnmpc_rti_prepare + sdfnmpc_qp_feedback + sdfnmpc_rti_apply on
 * fixed buffers -- captured once into a HIP graph and replayed by sdfnmpc_step_launch with one host call
 * (the latency path: the per-call form spends its host time in ≈10 runtime calls per step).  create runs the
 * step once eagerly (workspaces allocated, arguments checked), then captures it on a private stream; launch
 * enqueues the graph on the context stream.  The buffers named in the arguments must stay allocated at the
 * same addresses; results are bitwise those of the three calls.  The graph also addresses the context's own
 * workspaces: a later call on the context that grows them (a larger B or N) reallocates them, and launch then
 * fails with SDFNMPC_E_ARG instead of running on freed memory (destroy and create the step again).  Timing (sdfnmpc_ctx_enable_timing) does not
 * see graph launches.  (Not a reference interface: the acados solver object's solve() is one call too.) */
typedef struct sdfnmpc_step sdfnmpc_step;
int sdfnmpc_step_create(sdfnmpc_ctx* ctx, const sdfnmpc_net* net, const sdfnmpc_quad_model* model,
                        const sdfnmpc_lin_args* lin_args, const sdfnmpc_qp_opts* opts, const sdfnmpc_qp_args* qp_args,
                        double* u0, const int* status, sdfnmpc_step** out);
int sdfnmpc_step_launch(sdfnmpc_ctx* ctx, sdfnmpc_step* step);
void sdfnmpc_step_destroy(sdfnmpc_step* step);

/* ---- batched reference / parameter packing into the OCP device buffers (sdfnmpc_ref_args) ---- */
int sdfnmpc_pack_refs(sdfnmpc_ctx* ctx, const sdfnmpc_ref_opts* opts, const sdfnmpc_ref_args* args);

/* ---- in-loop VAE encoder ----
 * Replaces VaeWrapper.set_img + VaeWrapper.encode (sdf_nmpc/vae.py:29-40): preprocessing
 * (vae.py:15-24: float32 cast, Reshape's bilinear resize, ClipDistance, Depth2Range) and
 * Encoder.forward (network/vae.py:39-43, eval mode) for B images in one call on the context stream.
 * The encoder is the reference architecture (1 channel, conv7x7/2 + ELU + maxpool, ResBlocks
 * 64/128/256/512, avgpool 2x2, mean Linear); weights come as a `.vaew` blob (sdf-nmpc_amd/vae.py:pack)
 * with every BatchNorm folded into its convolution. */
typedef struct sdfnmpc_vae sdfnmpc_vae;

typedef struct {
    int B;                 /* images */
    int in_h, in_w;        /* raw image size; resized bilinearly to the encoder's H x W when different */
    int dtype;             /* 0 float32, 1 uint16 (ToDevice casts to float32) */
    float clip;            /* ClipDistance.dmax = sensor.dmax / sensor.mm_resolution * 1000 */
    const float* yz;       /* device [H][W] Depth2Range.yz_sqrt (sdf-nmpc_amd/vae.py:depth2range_table),
                              NULL when sensor.is_depth is false */
} sdfnmpc_vae_opts;

int sdfnmpc_vae_load(sdfnmpc_ctx* ctx, const void* vaew_blob, size_t bytes, sdfnmpc_vae** out);
void sdfnmpc_vae_free(sdfnmpc_vae* vae);
int sdfnmpc_vae_size_latent(const sdfnmpc_vae* vae);
/* img: device [B][in_h][in_w]; latent: device [B][L] float32; latent64: optional device [B][L] float64
 * (the precision Nmpc.set_latent stores into p).  The activation workspace (~5.7 MB per 270x480 image)
 * is owned by the encoder object and grows with B. */
int sdfnmpc_vae_encode(sdfnmpc_ctx* ctx, sdfnmpc_vae* vae, const sdfnmpc_vae_opts* opts, const void* img,
                       float* latent, double* latent64);

/* ---- VAE decoder (csrc/vae_dec.hip) ----
 * Replaces VaeWrapper.decode (sdf_nmpc/vae.py:42-45): Decoder.forward (network/vae.py:63-90, eval mode) for B
 * latents in one call on the context stream: Linear(L, 512*8*15) + ELU, four ResBlockDeconvs (512 -> 32 channels,
 * 8x15 -> 128x240), ConvTranspose2d(32, 1, 5), a bilinear resize (align_corners false) to out_h x out_w, sigmoid.
 * The result is a normalised RANGE image in [0, 1] whatever sensor.is_depth says (the encoder's input is
 * Depth2Range'd).  Weights come as a `.vaed` blob of their own (sdf-nmpc_amd/vae.py:pack_decoder) with every
 * BatchNorm folded into its transposed convolution; the encoder's `.vaew` layout is unchanged.
 * latent: device [B][L] float32; img: device [B][out_h][out_w] float32; logits: optional device [B][128][240]
 * float32, the values before the resize and the sigmoid.  Asynchronous; B == 0 is a no-op.  An image does not
 * depend on its batch neighbours (bitwise).  The activation workspace (about 22 MB an image, for at most 64
 * images: larger batches are decoded in passes of 64) is owned by the decoder object and grows with B.
 * The workspace ties the object to the context it was loaded on (one stream orders its calls): decode on any other
 * context is refused.  SDFNMPC_E_ARG with nothing launched: a NULL context / decoder / latent / img, B < 0, out_h or
 * out_w < 1, a decoder loaded on another context. */
typedef struct sdfnmpc_vae_dec sdfnmpc_vae_dec;
int sdfnmpc_vae_dec_load(sdfnmpc_ctx* ctx, const void* vaed_blob, size_t bytes, sdfnmpc_vae_dec** out);
void sdfnmpc_vae_dec_free(sdfnmpc_vae_dec* dec);
int sdfnmpc_vae_dec_size_latent(const sdfnmpc_vae_dec* dec);
int sdfnmpc_vae_decode(sdfnmpc_ctx* ctx, sdfnmpc_vae_dec* dec, int B, const float* latent, int out_h, int out_w,
                       float* img, float* logits);

/* ---- ground truth from range images (csrc/df_truth.hip) ----
 * What the image itself says about a point: the reference's Warp kernels ColChecker._kernel_colcheck
 * (utils/collision_checker.py:23-90) and DfComputer._kernel_pixel_wise_udf / get_sdf (utils/df_computer.py:
 * 85-221), restated as written in fp32.  img: device [n_img][H][W] float32, normalised by dmax; points: device
 * [n][3] float32, unnormalised camera-frame coordinates; p_to_i: device [n] int32, the image of each point, or
 * NULL for the reference's default ordering, point j -> image j / (n / n_img) (n must then be a multiple of
 * n_img).  The entries of p_to_i must lie in [0, n_img): they are the caller's responsibility and are not
 * checked on the device.  Launches are ordered on the context stream; n == 0 is a no-op.  SDFNMPC_E_ARG (nothing
 * is launched, outputs untouched): outside not 0 / 1 / 2, non-positive dmax / hfov / vfov, n_img <= 0, H or W
 * < 1, NULL p_to_i with n % n_img != 0, n < 0 or beyond 2^31 - 1, and for sdfnmpc_udf an H or W that is not a
 * multiple of 5. */
typedef struct {
    float dmax, hfov, vfov;      /* sensor.dmax, half fields of view in radians */
    int is_depth, is_spherical;  /* pixel value is depth (x) instead of range; spherical pixel coordinates */
} sdfnmpc_img_opts;

/* out[j] = 1 where point j collides: farther than its pixel, or past dmax; 0 inside the safe ball.  outside:
 * what holds beyond the field of view -- 0 free, 1 collision, 2 extrapolate (angles clamped to the border). */
int sdfnmpc_colcheck(sdfnmpc_ctx* ctx, const sdfnmpc_img_opts* opts, int outside, float safe_ball, const float* img,
                     int n_img, int H, int W, const float* points, const int* p_to_i, long long n,
                     unsigned char* out);
/* Unsigned distance to the nearest pixel of the 5x5 min-pooled image (zeros skipped) or to the virtual wall at
 * dmax, clamped to [0, max_df]; grad [n][3] = minus the unit direction to that pixel, 0 where udf == max_df;
 * pix_idx [n] (may be NULL) = the pooled pixel chosen (row-major, ties to the lowest index).  The pooled image
 * lives in a workspace of the context. */
int sdfnmpc_udf(sdfnmpc_ctx* ctx, const sdfnmpc_img_opts* opts, float max_df, const float* img, int n_img, int H,
                int W, const float* points, const int* p_to_i, long long n, float* udf, float* grad, int* pix_idx);
/* Signed distance over a voxel grid around each point (grid [G][3] offsets, dist [G] their norms, device
 * float32): the sign is the point's collision label (mode extrapolate, safe ball 0); a voxel counts when its own
 * label differs from the point's; sdf = clamp(sign * min dist over counting voxels (max_df if none), min_df,
 * max_df); grad [n][3] = -sign * grid[g] / |grid[g]| of that voxel g, 0 where sdf equals either clamp; ties go to
 * the lowest voxel index; vox_idx [n] (may be NULL) = g, -1 where no voxel counts.  orig_idx NULL: the grid in any
 * order, every voxel visited.  orig_idx [G] (device int32): the grid sorted by dist ascending, orig_idx the
 * voxel's index before sorting (ties are decided on it and vox_idx reports it); the scan then stops early.  Both
 * give bitwise the same outputs. */
int sdfnmpc_sdf_truth(sdfnmpc_ctx* ctx, const sdfnmpc_img_opts* opts, float min_df, float max_df, const float* grid,
                      const float* dist, const int* orig_idx, int G, const float* img, int n_img, int H, int W,
                      const float* points, const int* p_to_i, long long n, float* sdf, float* grad, int* vox_idx);

/* ---- the camera image's own field as the controller's SDF (csrc/df_truth.hip: img_sdf_rows_kernel) ----
 * The network's training target is DfComputer.get_df(img, points) (df_train.py:52,123,168, signed_df = True): the
 * distance and gradient the camera image itself implies -- limited to what the camera saw, quantised by the voxel
 * grid, in the frame of the image.  sdfnmpc_img_sdf_rows evaluates that field at the node positions of a batch and
 * writes what the network kernels' epilogue writes (gen_model.py:46-61): a controller flying on its own labels, the
 * perfect network with the learned one's partial observability and image staleness and no approximation error.
 * One 256-lane workgroup per node row r = b (N+1) + k:
 *   flag = p[r][0];  Co_p_B = W_R_Co^T (x[r][0:3] - W_p_Co) in fp64 from the row's own parameters (W_p_Co = p[r][1:4],
 *   W_R_Co = p[r][4:13] row-major), the network kernels' statements, rounded to fp32 (stored into pts[r], device float32
 *   [B][N+1][3], when pts != NULL -- for every row);
 *   (df, g) = the field at that point against image b (img_of[b] when img_of != NULL; the entries are the caller's to
 *   keep in range): is_signed -- exactly sdfnmpc_sdf_truth (sign from the collision test in mode extrapolate with safe
 *   ball 0, the distance-sorted voxel scan with its early stop, ties on the original voxel index, clamp to [min_df,
 *   max_df] with a zero gradient where saturated); else exactly sdfnmpc_udf's scan of `pooled` (the virtual wall at
 *   dmax, clamp to [0, max_df]).  Bitwise what those two return for the same fp32 point and image;
 *   h[r][2] = flag df + (1 - flag) max_df,  Jh[r][j][2] = flag ((R[j][0] g0 + R[j][1] g1) + R[j][2] g2) for j < 3 with
 *   R = W_R_Co, in that association, 0 for j = 3..9 -- fp64 on the widened fp32 values, no fused multiply-add.
 * Where flag == 0 exactly the scan is skipped: h[r][2] = max_df, Jh[r][.][2] = 0 (what the epilogue gives, the field
 * being finite).  Columns 0 and 1 of h and Jh are not touched; a row does not depend on its place in the batch.
 * "img_sdf_rows" in sdfnmpc_ctx_kernel_stats.  x [B][N+1][10], p [B][N+1][np], h [B][N+1][3], Jh [B][N+1][10][3] device
 * float64.  Asynchronous on the context stream; B == 0 is a no-op.  SDFNMPC_E_ARG (nothing is launched, outputs
 * untouched): NULL arguments (pts may be NULL), B < 0, N < 1, np < 17, non-positive dmax / hfov / vfov, H or W < 1, a
 * non-finite or non-positive max_df, min_df >= max_df, NULL images; signed without grid / dist or with G < 1; unsigned
 * with an H or W that is not a multiple of 5 or without pooled. */
struct sdfnmpc_img_sdf_opts {
    sdfnmpc_img_opts img;      /* the sensor */
    int H, W;                  /* image size */
    const float* images;       /* device [n_img][H][W] float32, normalised by dmax */
    const int* img_of;         /* device [B] int32 or NULL: instance b reads image b */
    int is_signed;             /* 1: get_sdf over the voxel grid; 0: get_udf over the pooled image */
    float min_df, max_df;      /* the clamps (DfComputer: -0.3 and 1) */
    const float* grid;         /* signed: device [G][3], [G], [G] as sdfnmpc_sdf_truth takes them (orig_idx NULL: */
    const float* dist;         /*   any order, full scan; else sorted by dist with the original indices) */
    const int* orig_idx;
    int G;
    const float* pooled;       /* unsigned: device [n_img][H/5][W/5], the 5x5 min-pool of images (sdfnmpc_img_sdf_pool) */
};
int sdfnmpc_img_sdf_rows(sdfnmpc_ctx* ctx, const sdfnmpc_img_sdf_opts* opts, int B, int N, int np, const double* x,
                         const double* p, double* h, double* Jh, float* pts);
/* The zero-skipping 5x5 min-pool sdfnmpc_udf runs in front of its scan, of opts->images [n_img] into opts->pooled
 * ("minpool5" in the kernel stats).  SDFNMPC_E_ARG: NULL arguments, n_img < 0, H or W not a positive multiple of 5. */
int sdfnmpc_img_sdf_pool(sdfnmpc_ctx* ctx, const sdfnmpc_img_sdf_opts* opts, int n_img);

/* ---- device memory on a context (inputs of the device-side setters without a tensor library) ----
 * memcpy kind: 1 host -> device, 2 device -> host, 3 device -> device; ordered on the context stream,
 * synchronous (returns when the copy has completed). */
int sdfnmpc_dev_alloc(sdfnmpc_ctx* ctx, size_t bytes, void** out);
void sdfnmpc_dev_free(sdfnmpc_ctx* ctx, void* ptr);
int sdfnmpc_memcpy(sdfnmpc_ctx* ctx, void* dst, const void* src, size_t bytes, int kind);

/* ---- the batched SQP-RTI solver object (owns its device workspace) ----
 * Fields (name: [B][nodes][width] fp64 unless noted): x [N+1][10], u [N][4], p [N+1][np], x0 [1][10],
 * yref / W [N][ny], yNref / WN [1][nyN], u0 [1][4], dx [N+1][10], du [N][4], the sdfnmpc_lin_args outputs
 * xn, AB, y, Jy, yN [1][nyN], JyN [1][10 nyN], h, Jh, hE [1][6], JhE [1][60], res [1][2], slack [N+1][6]
 * ((sl, su) per soft row), status / iters [1][1] int32.  A field's device pointer may be handed to the
 * lower-level entry points (e.g. sdfnmpc_pack_refs or sdfnmpc_vae_encode writing p).  The network may be
 * NULL when the constraint set (qp.nh / h_col, qp.hN_col) and the cost (ny == 11) never read the SDF. */
typedef struct sdfnmpc_solver sdfnmpc_solver;

typedef struct {
    int B, N, np, ny;          /* instances, horizon, parameters per node, stage residuals (11 / 12) */
    int latent_mode;           /* as sdfnmpc_lin_args.latent_mode */
    const double* dt;          /* [N] shooting-grid steps (host; copied) */
    sdfnmpc_quad_model model;
    sdfnmpc_qp_opts qp;        /* qp.ny == ny */
} sdfnmpc_solver_opts;

int sdfnmpc_solver_create(sdfnmpc_ctx* ctx, const sdfnmpc_net* net, const sdfnmpc_solver_opts* opts,
                          sdfnmpc_solver** out);
void sdfnmpc_solver_destroy(sdfnmpc_solver* s);
int sdfnmpc_solver_field(sdfnmpc_solver* s, const char* name, void** dev, int* nodes, int* width);
/* host [B][nodes][width] (the caller's full mirror of the field): columns [col0, col0 + ncol) of the rows
 * r = b * nodes + k with row_mask[r] != 0 (row_mask NULL: every row) -> device.  Asynchronous: the data
 * is staged in pinned memory before the call returns, so host may be reused at once. */
int sdfnmpc_solver_upload(sdfnmpc_solver* s, const char* name, int col0, int ncol, const unsigned char* row_mask,
                          const double* host);
/* the whole field -> host [B][nodes][width] (synchronous) */
int sdfnmpc_solver_download(sdfnmpc_solver* s, const char* name, void* host);
/* reset + init (ocp.py:144-153): x0 = x_k = x0[b] for k = 0..N, u_k = u_init[4], dx = du = 0 */
int sdfnmpc_solver_init(sdfnmpc_solver* s, const double* x0, const double* u_init);
/* shift (ocp.py:152-156): x_{i-k} = x_i, u_{i-k} = u_i for i = k..N-1 (k <= 0 or k >= N: no-op) */
int sdfnmpc_solver_shift(sdfnmpc_solver* s, int k);
/* enqueue one SQP-RTI iteration: x_0 = x0, preparation phase, QP, full step (failed instances keep their
 * iterate), then u_0 / status / iterations into pinned host memory.  Asynchronous. */
int sdfnmpc_solver_step(sdfnmpc_solver* s);
/* wait for the stream; copy the last step's u0 [B][4], status [B], iters [B] (each may be NULL) */
int sdfnmpc_solver_wait(sdfnmpc_solver* s, double* u0, int* status, int* iters);

/* ---- the plant of a closed loop (csrc/plant.hip) ----
 * One control period of the vehicle, integrated with `substeps` RK4 steps of dt / substeps (the Butcher tableau and
 * accumulation order of the preparation phase: with the controller's kind, substeps = 1, dt = dt_k and no mismatch,
 * x_next is sdfnmpc_lin_args.xn up to rounding).  The plant may differ from the controller's model: the other kind,
 * a finer step, and per instance a constant world-frame acceleration added to dv/dt and a factor on the thrust
 * input.  Inputs are not clipped and the quaternion is not renormalised (both models normalise internally). */
typedef struct {
    int kind;                      /* SDFNMPC_MODEL_ATT / _ATT_TAU: the plant's model, may differ from the controller's */
    double gamma, roll, pitch, wz, g, tau_roll, tau_pitch; /* as sdfnmpc_quad_model (tau_*: kind 1 only, > 0) */
    double dt;                     /* control period, s (> 0) */
    int substeps;                  /* RK4 steps per period, 1..64 */
    const double* acc_dist;        /* device [B][3] or NULL */
    const double* gamma_scale;     /* device [B] or NULL */
} sdfnmpc_plant_opts;

/* x_next[B][10] = plant(x[B][10], u[B][4]); device pointers, x_next may alias x.  Asynchronous on the context
 * stream.  SDFNMPC_E_ARG (nothing is launched, x_next untouched): NULL arguments, B < 0, substeps outside 1..64,
 * dt <= 0, kind 1 with a tau <= 0; SDFNMPC_E_UNSUPPORTED: an unknown kind.  B == 0 is a no-op. */
int sdfnmpc_plant_step(sdfnmpc_ctx* ctx, const sdfnmpc_plant_opts* opts, int B, const double* x, const double* u,
                       double* x_next);

/* ---- the vehicle model of a closed loop (csrc/vehicle.hip) ----
 * What stands between the controller's command and the state it is told about.  The vehicle object owns, per instance,
 * the true state x_true [10], the actual specific thrust gamma_act, the gust acceleration w [3] and a ring of the last
 * d commands.  One plant call at frame f with the command u_cmd does, in this order:
 *   1. input delay: u_app = ring[f % d], ring[f % d] <- u_cmd (d = 0: u_app = u_cmd);
 *   2. gust: w <- phi w + gust_std sqrt(1 - phi^2) xi(f), phi = exp(-dt / gust_tau) (gust_tau = 0: phi = 0), held over
 *      the period and added to dv/dt beside acc_dist;
 *   3. thrust lag: d(gamma_act)/dt = (gamma_cmd - gamma_act) / tau_m, gamma_cmd = u_app[0] gamma gamma_scale, an 11th
 *      RK4 state whose stage value is the thrust of f_expl (tau_m = 0: the thrust is gamma_cmd);
 *   4. rotor drag: dv/dt gains -R diag(drag) R^T v, R the body rotation the model's thrust uses;
 *   5. RK4 with the plant's substeps, tableau and accumulation order: x_true, gamma_act;
 *   6. the estimate of frame f + 1: p + bias_p + est_std_p n_p, v + bias_v + est_std_v n_v, the attitude turned about
 *      world z by bias_yaw + est_std_yaw n_yaw (no noise and no bias: a copy of x_true).
 * Random numbers: Philox4x32-10 under the key seed with the counter (j, frame, stream, 1), j = 0..4, stream =
 * stream_id[b] or b; call j gives the normals n[2j] = N(w0, w1), n[2j+1] = N(w2, w3), Box-Muller's cosine branch on
 * the 24-bit uniforms ((w >> 8) + 1) 2^-24 in fp64; n[0..2] -> xi, n[3..5] -> n_p, n[6..8] -> n_v, n[9] -> n_yaw.
 * A model with everything off (d = 0, gust_std = 0, tau_m = 0, no drag, no estimate error) runs the plant's own
 * kernel: the bits of sdfnmpc_plant_step. */
typedef struct {
    uint64_t seed;
    int d;                         /* input delay in control periods, 0..8 */
    double tau_m;                  /* thrust lag, s (0: none) */
    double drag[3];                /* rotor drag coefficients in the body frame, 1/s */
    double gust_std, gust_tau;     /* stationary standard deviation (m/s^2) and correlation time (s) of the gust */
    double est_std_p, est_std_v, est_std_yaw; /* estimate noise: m, m/s, rad */
    const double* est_bias;        /* device [B][7] (p, v, yaw) or NULL */
    const int* stream_id;          /* device [B] or NULL: the instance index */
    double g, gamma;               /* what a reset writes: gamma_act = g, every ring slot the hover input (g / gamma, 0, 0,
                                      0); g > 0, gamma > 0 */
} sdfnmpc_vehicle_opts;
typedef struct sdfnmpc_vehicle sdfnmpc_vehicle;

/* SDFNMPC_E_ARG: NULL arguments, B < 0, d outside 0..8, a negative or non-finite tau, std or drag coefficient, g or
 * gamma not positive and finite.  The new vehicle is reset and its true state is zero until _begin. */
int sdfnmpc_vehicle_create(sdfnmpc_ctx* ctx, const sdfnmpc_vehicle_opts* opts, int B, sdfnmpc_vehicle** out);
void sdfnmpc_vehicle_destroy(sdfnmpc_vehicle* v);
/* ring <- hover, gamma_act <- g, w <- 0 (asynchronous on the context stream) */
int sdfnmpc_vehicle_reset(sdfnmpc_vehicle* v);
/* x_true <- x0; x0 <- est(x_true, frame): the one launch before a loop's first step.  x0: device [B][10], in the
 * truth, out the estimate.  est is a pure function, so the begin of a second chunk writes what the first chunk's last
 * plant call wrote. */
int sdfnmpc_vehicle_begin(sdfnmpc_ctx* ctx, sdfnmpc_vehicle* v, double* x0, int frame);
/* the vehicle's true state, device [B][10] (owned by the vehicle) */
double* sdfnmpc_vehicle_x_true(sdfnmpc_vehicle* v);
/* one plant call (above) on the vehicle's own true state under the command u [B][4] at `frame`; x_est_out [B][10]
 * receives the estimate of frame + 1.  SDFNMPC_E_ARG: the plant's refusals, a vehicle of another context or batch
 * size, frame < 0 or frame + 1 overflowing.  B == 0 is a no-op. */
int sdfnmpc_plant_step_vehicle(sdfnmpc_ctx* ctx, const sdfnmpc_plant_opts* opts, sdfnmpc_vehicle* v, int B,
                               const double* u, int frame, double* x_est_out);

/* ---- the rigid-body vehicle (csrc/vehicle_body.hip) ----
 * With a body the command (thrust, roll, pitch, yaw rate) is the setpoint of an on-board attitude and rate controller
 * that drives four rotors with a first-order speed lag, which move a rigid body by model/quad_props.py:41-48.  It
 * replaces steps 3 and 5 of the plant call above; delay, gust, drag and the estimate stay.  The plant options' kind
 * only supplies the limits.  Hidden state per instance: x_true [10] = (p, q, v) with the full attitude in q, the body
 * rate omega [3] (body frame) and the rotor speeds Omega [4] (the reference's unit, u robot.limits.wp).  With the applied
 * input u: F = mass u[0] gamma, roll_d = u[1] roll, pitch_d = u[2] pitch, wz_d = u[3] wz; at every RK4 stage (a
 * continuous controller, no sample-and-hold), with q normalised:
 *   psi = quat2yaw(q), q_d = q_z(psi) (x) q_y(pitch_d) (x) q_x(roll_d), q_e = q^-1 (x) q_d, negated if q_e[0] < 0
 *   omega_sp = (2 q_e[1] / tau_att, 2 q_e[2] / tau_att, wz_d)
 *   tau = J k_rate (omega_sp - omega) + omega x J omega
 *   s = mixer [F; tau], each clipped to [wp_idle^2, wp_max^2];  Omega_cmd = sqrt(s)
 *   dOmega/dt = (Omega_cmd - Omega) / tau_mot      (tau_mot = 0: Omega = Omega_cmd)
 *   dp/dt = v;  dq/dt = q (x) (0, omega) / 2;  domega/dt = (Gt Omega^2 - omega x J omega) / J
 *   dv/dt = R(q) Gf Omega^2 gamma_scale / mass - g e_z + acc_dist + gust - R diag(drag) R^T v
 * integrated on the 17 states with the plant's substeps, tableau and accumulation order.  A reset writes omega = 0 and
 * Omega = sqrt(mixer [mass g; 0; 0; 0]), the hover speeds.  The matrices come from the caller (vehicle.RigidBody forms
 * them from the motor geometry as quad_props.py:20-27 does): the kernel knows nothing of motor geometry. */
typedef struct {
    double mass;                   /* kg */
    double inertia[3];             /* the diagonal of J, kg m^2 */
    double Gf[12], Gt[12];         /* [3][4] row-major: body force and torque = G Omega^2 */
    double mixer[16];              /* [4][4] row-major: inv([Gf row z; Gt]) */
    double wp_max, wp_idle;        /* the rotor speed's range, 0 < wp_idle < wp_max */
    double tau_att;                /* attitude loop time constant, s */
    double k_rate[3];              /* rate loop gains, 1/s */
    double tau_mot;                /* rotor speed lag, s (0: none) */
} sdfnmpc_body_opts;
/* opts: the vehicle becomes a rigid body (and is never neutral), its omega and Omega reset; NULL: the plain vehicle
 * again, with the bits it had.  SDFNMPC_E_ARG (nothing is launched or allocated, the vehicle stays as it was): a
 * non-finite or non-positive mass, inertia, wp_max, tau_att or k_rate, wp_idle outside (0, wp_max), tau_mot < 0 or
 * non-finite, a non-finite matrix entry, a vehicle with tau_m > 0 (the rotor lag replaces the thrust lag).  With a
 * body sdfnmpc_plant_step_vehicle and the rollouts also refuse (SDFNMPC_E_ARG, nothing launched) a step with
 * (dt / substeps) max(1 / tau_mot, max k_rate, 2 / tau_att) > 1: RK4's real-axis stability limit is 2.78, and a batch
 * that silently blows up is worse than a refusal. */
int sdfnmpc_vehicle_set_body(sdfnmpc_vehicle* v, const sdfnmpc_body_opts* opts);
/* the body's hidden states, device [B][3] and [B][4] (owned by the vehicle; each out pointer may be NULL).
 * SDFNMPC_E_ARG: a NULL vehicle or one without a body. */
int sdfnmpc_vehicle_body_state(sdfnmpc_vehicle* v, double** omega, double** rotor);

/* K closed-loop steps of the solver's B instances without a host round trip.  Per step, in the order Nmpc.solve
 * uses: (1) with ref: sdfnmpc_pack_refs from the current x0 into the solver's p / yref / W / yNref / WN; (2) with
 * shift > 0: sdfnmpc_solver_shift(shift); (3) the SQP-RTI step of sdfnmpc_solver_step; (4) the plant on the solver's
 * x0 and u0 fields: x0 <- plant(x0, u0) in place -- the next measured state -- and the log rows.  Everything is
 * enqueued on the solver's stream as a plain launch sequence; sdfnmpc_solver_wait finishes it and returns the last
 * step's u0 / status / iters.  The arrays named here (and by ref and plant) must stay alive until then.
 * An instance whose QP fails (status >= 2) keeps its iterate and is advanced with the u0 sdfnmpc_rti_apply leaves,
 * the unchanged u[:, 0] (Ocp.solve on the host substitutes the previous call's u instead).
 * SDFNMPC_E_ARG (nothing is launched): NULL arguments, steps < 1, a missing x_log or u_log, the plant's refusals,
 * ref->mode outside 0..2 or without its inputs (wrow; mode 0: wp_p, wp_q, 1 <= n_wp <= 32; mode 1: vw);
 * SDFNMPC_E_UNSUPPORTED: an unknown plant kind. */
typedef struct {
    int steps;                     /* K >= 1 */
    int shift;                     /* sdfnmpc_solver_shift(k) before every step (mpc.shift) */
    const sdfnmpc_ref_opts* ref;   /* NULL: references and q_d stay as they are; else sdfnmpc_pack_refs from the
                                      current x0 before every step (modes 0 / 1 / 2), with: */
    const double *wp_p, *wp_q, *vw, *wrow; /* device, as sdfnmpc_ref_args */
    int n_wp;
    sdfnmpc_plant_opts plant;
    double* x_log;                 /* device [B][K+1][10]; row 0 = the starting x0 */
    double* u_log;                 /* device [B][K][4] */
    int *status_log, *iters_log;   /* device [B][K], each may be NULL */
    float* pts_log;                /* device [B][K+1][3] or NULL: the fp32 camera-frame position W_R_Co^T (x[:3] -
                                      W_p_Co) of every logged state, the pose from node 0 of the instance's p row */
    /* ---- the vehicle model (all NULL / 0: the plant on x0, as above).  With a vehicle (after sdfnmpc_vehicle_begin on
     * the solver's x0 field) step (4) is sdfnmpc_plant_step_vehicle at frame frame0 + k: the true state lives in the
     * vehicle, x0 receives the estimate; x_log and pts_log log the true state, u_log the command.  In the rollouts
     * that render, the camera pose comes from the true state and the body pose written into p from the estimate;
     * references and sdfnmpc_solver_rollout_scene_sdf's pose refresh read the estimate.  SDFNMPC_E_ARG: a vehicle of
     * another context or batch size, frame0 < 0 or frame0 + steps overflowing, xhat_log / uapp_log without a vehicle. */
    sdfnmpc_vehicle* vehicle;
    int frame0;
    double* xhat_log;              /* device [B][K+1][10] or NULL: the estimates; row 0 = what _begin wrote */
    double* uapp_log;              /* device [B][K][4] or NULL: the applied (delayed) inputs */
    /* a vehicle with a body (else SDFNMPC_E_ARG): its body rates and rotor speeds, row 0 before the first step */
    double* omega_log;             /* device [B][K+1][3] or NULL */
    double* rotor_log;             /* device [B][K+1][4] or NULL */
} sdfnmpc_rollout_args;

int sdfnmpc_solver_rollout(sdfnmpc_solver* s, const sdfnmpc_rollout_args* args);

/* ---- analytic scenes (csrc/scene.hip) ----
 * A scene is a union of up to SDFNMPC_SCENE_MAX_PRIMS primitives (sdfnmpc_scene_create_large below: up to
 * SDFNMPC_SCENE_LARGE_MAX_PRIMS static ones, with a grid index) in the world frame (z up, as in the models):
 *   SDFNMPC_PRIM_SPHERE    a = (cx, cy, cz, r)
 *   SDFNMPC_PRIM_BOX       a = (lo_x, lo_y, lo_z, hi_x, hi_y, hi_z), axis-aligned
 *   SDFNMPC_PRIM_CYLINDER  a = (cx, cy, r, z0, z1), capped, along z
 * sdfnmpc_scene_create copies S scenes to the context's device (host arrays: count [S] primitives per scene, prims
 * [sum of count] scene after scene; synchronous).  It is where a scene is checked -- SDFNMPC_E_ARG for S < 1, a
 * count outside 0..32, an unknown kind, a radius <= 0, lo >= hi or z0 >= z1, a non-finite value -- so no launch
 * ever sees a malformed scene.  A launch names the scene of each instance by scene_of [B] (device int32; NULL: every
 * instance uses scene 0).  Its entries are the caller's responsibility, as p_to_i above (a kernel clamps them into
 * [0, S)). */
#define SDFNMPC_SCENE_MAX_PRIMS 32
#define SDFNMPC_PRIM_SPHERE 0
#define SDFNMPC_PRIM_BOX 1
#define SDFNMPC_PRIM_CYLINDER 2
typedef struct {
    int kind;
    double a[6];
} sdfnmpc_prim;
int sdfnmpc_scene_create(sdfnmpc_ctx* ctx, int S, const int* count, const sdfnmpc_prim* prims, sdfnmpc_scene** out);
void sdfnmpc_scene_free(sdfnmpc_scene* scene);

/* img [B][H][W] (device float32) = the image instance b's camera takes of its scene: per pixel the nearest hit t >= 0
 * of the ray through the pixel centre of colcheck's pixel grid (collision_checker.py:80-84; camera frame x forward,
 * y left, z up) -- pinhole d_c ~ (1, tan(hfov) (1 - (2u+1)/W), tan(vfov) (1 - (2v+1)/H)), spherical azimuth hfov (1 -
 * (2u+1)/W) and elevation vfov (1 - (2v+1)/H) -- written as min(val, dmax) * scale with val = t (range) or, with
 * opts->is_depth, t d_c.x for unit d_c; a miss gives dmax * scale.  scale = 1 / dmax: the normalised image
 * sdfnmpc_colcheck / sdfnmpc_udf read; scale = 1000 / mm_resolution: the raw sensor image sdfnmpc_vae_encode expects.
 * A camera inside a primitive sees t = 0 everywhere: the all-zero image colcheck reads as collision.  The pose
 * W_p_C [B][3], W_R_C [B][9] (device float64, row-major: world = W_R_C cam + W_p_C) is rounded to fp32 once; the
 * image is computed in fp32 without atomics, bitwise reproducible and independent of the instance's place in the
 * batch.  Asynchronous on the context stream; B == 0 is a no-op.  SDFNMPC_E_ARG (nothing is launched, img untouched):
 * NULL arguments, B < 0 or > 65535, H or W < 1 (or H W beyond 2^31 - 1), non-positive or non-finite dmax / hfov / vfov
 * / scale, pinhole with hfov or vfov >= pi / 2, a spherical image with H + W > 6144, a scene on another device. */
int sdfnmpc_scene_render(sdfnmpc_ctx* ctx, const sdfnmpc_scene* scene, const int* scene_of, const sdfnmpc_img_opts* opts,
                         int H, int W, float scale, int B, const double* W_p_C, const double* W_R_C, float* img);
/* The poses of B states x [B][10] (device float64; position x[0..2], quaternion x[3..6] = (w, x, y, z), not
 * necessarily normalised): W_p_Bo [B][3] = x[0..2], W_R_Bo [B][9] = quat2rot(q / |q|) (utils/math.py:7-23), and the
 * camera pose W_p_C = W_R_Bo B_p_C + W_p_Bo, W_R_C = W_R_Bo B_R_C (controller.py:52-53; B_p_C [3], B_R_C [9] host,
 * row-major).  fp64, asynchronous; B == 0 is a no-op.  SDFNMPC_E_ARG: NULL arguments, B < 0. */
int sdfnmpc_scene_pose(sdfnmpc_ctx* ctx, const double* B_p_C, const double* B_R_C, int B, const double* x, double* W_p_Bo,
                       double* W_R_Bo, double* W_p_C, double* W_R_C);
/* out [n] (device float64) = the signed distance from world point points [n][3] (device float64) to its scene: the
 * minimum over the primitives of the closed-form sphere, box and capped-cylinder distances, negative inside (exact
 * outside the union).  p_to_scene [n] (device int32) names each point's scene; NULL: the default ordering of
 * sdfnmpc_colcheck's p_to_i, point j -> scene j / (n / S) (n must then be a multiple of S).  A scene without
 * primitives gives +inf.  fp64, asynchronous; n == 0 is a no-op.  SDFNMPC_E_ARG: NULL arguments, n < 0 or beyond
 * 2^31 - 1, NULL p_to_scene with n % S != 0. */
int sdfnmpc_scene_distance(sdfnmpc_ctx* ctx, const sdfnmpc_scene* scene, const double* points, const int* p_to_scene,
                           long long n, double* out);

/* ---- moving and oriented primitives ----
 * Every primitive has a reference point c0 -- sphere: its centre; box: (lo + hi) / 2; cylinder: (cx, cy, (z0 + z1) /
 * 2) -- and an optional motion record that gives its rigid frame at time t:
 *   c(t) = c0 + v t + amp sin(omega t + phase)      (amp component-wise)
 *   R(t) = Rz(yaw_rate t) R(q)                      q = (w, x, y, z) of any non-zero norm, normalised at creation
 * The primitive is its canonical shape (centred, axes as given) placed at (R(t), c(t)): a box with q != identity is
 * an oriented box, a cylinder with q != identity a tilted capped cylinder.  R(q) is formed once in fp64 when the
 * scene is created and kept on the device beside the primitives.
 * sdfnmpc_scene_create_moving is sdfnmpc_scene_create with motion [sum of count] beside prims; motion == NULL gives
 * exactly what sdfnmpc_scene_create gives.  In addition to that function's checks it refuses (SDFNMPC_E_ARG, before
 * anything is allocated) a non-finite motion value and a zero quaternion.
 * A scene set is dynamic (sdfnmpc_scene_is_dynamic: 1, else 0) when some primitive of it has a q that is not the
 * identity rotation or a non-zero yaw_rate, v or amp.  A set that is not dynamic is rendered and measured by the
 * static kernels whatever time is given: the same bits as sdfnmpc_scene_render / sdfnmpc_scene_distance.  A dynamic
 * set takes the dynamic kernels ("scene_render_dyn", "scene_dist_dyn" in sdfnmpc_ctx_kernel_stats) for every scene
 * of it; a primitive without motion is the case R = I, v = 0 of the same path. */
typedef struct {
    double q[4];                   /* orientation (w, x, y, z); (1, 0, 0, 0): none */
    double yaw_rate;               /* rad / s about the world z axis */
    double v[3];                   /* m / s */
    double amp[3];                 /* m, harmonic term */
    double omega, phase;           /* rad / s, rad */
} sdfnmpc_prim_motion;
int sdfnmpc_scene_create_moving(sdfnmpc_ctx* ctx, int S, const int* count, const sdfnmpc_prim* prims,
                                const sdfnmpc_prim_motion* motion, sdfnmpc_scene** out);
int sdfnmpc_scene_is_dynamic(const sdfnmpc_scene* scene);
/* sdfnmpc_scene_render of the scene at time t (sdfnmpc_scene_render is t = 0).  For a dynamic set each block forms
 * its primitives' frames at t in fp64 -- the camera origin and axes in the primitive's frame -- rounds them to fp32
 * once and runs the interval tests of sdfnmpc_scene_render on the canonical shapes; hit rule, depth / range,
 * clipping and scale are the same.  Also refused (SDFNMPC_E_ARG, nothing launched): a non-finite t. */
int sdfnmpc_scene_render_at(sdfnmpc_ctx* ctx, const sdfnmpc_scene* scene, const int* scene_of,
                            const sdfnmpc_img_opts* opts, int H, int W, float scale, int B, const double* W_p_C,
                            const double* W_R_C, double t, float* img);
/* sdfnmpc_scene_distance with point j measured against the scene at times [j] (device float64 [n]; NULL: t = 0).
 * The times are the caller's to keep finite, as the points are. */
int sdfnmpc_scene_distance_at(sdfnmpc_ctx* ctx, const sdfnmpc_scene* scene, const double* points, const int* p_to_scene,
                              const double* times, long long n, double* out);

/* ---- swept clearance: the minimum distance over a segment of space-time (csrc/scene_swept.hip) ----
 * Segment j runs from (p0[j], t0[j]) to (p1[j], t1[j]): p(s) = p0 + s (p1 - p0), t(s) = t0 + s (t1 - t0), s in [0, 1],
 * and D(s) is what sdfnmpc_scene_distance_at returns for the point p(s) at the time t(s).  The call returns the minimum
 * of D over s with a certificate:
 *   dmin [n]   the smallest value found, a value of D at an actual point
 *   s [n]      the parameter of that point (the smaller one on a tie)
 *   gap [n]    the true minimum lies in [dmin - gap, dmin]
 *   evals [n]  evaluations of D used (int32)
 * by a deterministic Lipschitz branch and bound on dyadic intervals.  D is Lipschitz in s with L = |p1 - p0| +
 * V |t1 - t0|, where V bounds the speed of any surface point of any mover of the scene: the maximum over its movers of
 * |v| + |omega| |amp| + |yaw_rate| rho in Euclidean norms (rho: 0 for a sphere, the half diagonal of a box, sqrt(r^2 +
 * hz^2) for a cylinder), formed in fp64 when the scene is created and inflated by 1 + 1e-12; 0 for a set that is not
 * dynamic.  sdfnmpc_scene_speed_bound copies V of the S scenes to out (host [S]).  An interval [a, b] of width w holds
 * no value below lb = (D(a) + D(b) - L w) / 2; one with lb >= best - eps is dropped, any other is halved at its midpoint,
 * the left half first, down to a width of 2^-20 and until max_evals evaluations are used.  gap = max(0, dmin - the
 * smallest lb of any interval dropped), so gap <= eps when neither limit was met, and larger -- never wrong -- when one
 * was.  Every loop's trip count is fixed by max_evals before it starts.  A zero-length segment of one time gives one
 * evaluation, s = 0 and gap 0; a non-finite coordinate or time gives NaN in dmin, s and gap and 0 in evals for that
 * segment alone; a scene without primitives gives +inf and gap 0.
 * All arrays are device arrays; p_to_scene as for sdfnmpc_scene_distance (segment j -> scene); t0 and t1 may both be
 * NULL (t = 0), and a set that is not dynamic does not read them; s, gap and evals may be NULL.  The kernels are
 * "scene_swept", "scene_swept_dyn", "scene_swept_grid" and "scene_swept_mixed" in sdfnmpc_ctx_kernel_stats, one thread
 * per segment over the device functions of the distance kernels.  fp64, asynchronous; n == 0 is a no-op.
 * SDFNMPC_E_ARG (nothing launched, no output written): NULL ctx, scene, p0, p1 or dmin, n < 0 or beyond 2^31 - 1, NULL
 * p_to_scene with n % S != 0, one of t0 and t1 NULL alone, eps not finite or below 1e-6, max_evals outside 2..65536, a
 * scene of another context. */
int sdfnmpc_scene_swept_distance(sdfnmpc_ctx* ctx, const sdfnmpc_scene* scene, const double* p0, const double* p1,
                                 const int* p_to_scene, const double* t0, const double* t1, long long n, double eps,
                                 int max_evals, double* dmin, double* s, double* gap, int* evals);
int sdfnmpc_scene_speed_bound(const sdfnmpc_scene* scene, double* out);

/* ---- scenes of many primitives: a uniform-grid index (csrc/scene_grid.hip) ----
 * sdfnmpc_scene_create_large is sdfnmpc_scene_create for S scenes of 0..SDFNMPC_SCENE_LARGE_MAX_PRIMS static
 * primitives each (the same kinds, checks and fp32 rounding; no motion records), with a uniform grid per scene built
 * on the host inside the call (synchronous).  cell > 0: the grid's cell edge in metres (rounded to fp32).  cell <= 0:
 * the default, a function of the scene's primitives only -- cbrt(V / (4 n)) for the volume V of the n primitives'
 * bounding box, about 4 cells per primitive, and not below (E + R / 1024) / 250 for the box's longest edge E and the
 * largest absolute coordinate R, which keeps every axis at 1..256 cells; a forest of upright cylinders gets a few
 * layers in z.  A primitive is listed in every cell that its bounding box inflated by cell / 1024 + R / 4096 overlaps;
 * the grid's box is the bounding box padded by twice that.  A scene without primitives gets an empty grid.
 * The handle is used like any other: sdfnmpc_scene_render(_at), sdfnmpc_scene_distance(_at), sdfnmpc_scene_sdf_rows,
 * sdfnmpc_lin_args.sdf_scene, sdfnmpc_solver_set_sdf_scene and every rollout that takes a scene dispatch on it
 * (sdfnmpc_scene_is_indexed: 1, else 0) and launch the grid kernels -- "scene_render_grid", "scene_dist_grid",
 * "scene_sdf_rows_grid" in sdfnmpc_ctx_kernel_stats -- which visit only the cells along a ray or around a point and
 * return, bit for bit, what the brute-force kernels would return over all primitives of the scene, for a camera
 * within about 100 times the scene's size of it (farther away a pixel may differ; no read leaves the scene's arrays
 * for any pose or point).  An indexed set is static: times are ignored, sdfnmpc_scene_is_dynamic is 0.
 * SDFNMPC_E_ARG (nothing is allocated): what sdfnmpc_scene_create refuses, a count above
 * SDFNMPC_SCENE_LARGE_MAX_PRIMS, a non-finite cell, a grid of more than SDFNMPC_SCENE_GRID_MAX_AXIS cells along an
 * axis or SDFNMPC_SCENE_GRID_MAX_CELLS cells in a scene, or more than SDFNMPC_SCENE_GRID_MAX_ITEMS cells plus
 * cell-list entries in the set. */
#define SDFNMPC_SCENE_LARGE_MAX_PRIMS 65536
#define SDFNMPC_SCENE_GRID_MAX_AXIS 1024
#define SDFNMPC_SCENE_GRID_MAX_CELLS (1 << 22)
#define SDFNMPC_SCENE_GRID_MAX_ITEMS (1 << 26)
int sdfnmpc_scene_create_large(sdfnmpc_ctx* ctx, int S, const int* count, const sdfnmpc_prim* prims, double cell,
                               sdfnmpc_scene** out);
int sdfnmpc_scene_is_indexed(const sdfnmpc_scene* scene);

/* ---- a large static world with a few moving obstacles: mixed sets (csrc/scene_grid.hip) ----
 * sdfnmpc_scene_create_mixed is sdfnmpc_scene_create_large (count, prims, cell: the same arguments, checks and grid,
 * which covers these static primitives only) with a mover set beside every scene: mcount [S] primitives per scene,
 * 0..SDFNMPC_SCENE_MAX_PRIMS, mprims [sum of mcount] and mmotion [sum of mcount] as sdfnmpc_scene_create_moving takes
 * and checks them (mmotion == NULL: no motion; such movers still take the mover path).  The movers are not in the
 * grid: they may leave its box, overlap static primitives, or be all a scene has (count[s] == 0).
 * Every query of such a handle is the minimum over both sets at the query's time, bit for bit the elementwise minimum
 * of the indexed static set's result and of the movers' as a dynamic set of their own: sdfnmpc_scene_render(_at),
 * sdfnmpc_scene_distance(_at) (times [j] per point), sdfnmpc_scene_sdf_rows, sdfnmpc_lin_args.sdf_scene,
 * sdfnmpc_solver_set_sdf_scene (predict as for a dynamic set) and every rollout that takes a scene.  In the SDF row
 * the gradient is that of the nearest primitive; on a tie a static primitive comes before a mover, and within each
 * set the lowest index wins.  The kernels are "scene_render_mixed", "scene_dist_mixed" and "scene_sdf_rows_mixed" in
 * sdfnmpc_ctx_kernel_stats: they evaluate the movers first and start the grid's search from that bound.
 * With a mover in some scene both sdfnmpc_scene_is_indexed and sdfnmpc_scene_is_dynamic are 1.  With every mcount[s]
 * == 0 the handle is what sdfnmpc_scene_create_large returns (not dynamic, the grid kernels).
 * SDFNMPC_E_ARG (nothing is allocated): what sdfnmpc_scene_create_large refuses of count, prims and cell, what
 * sdfnmpc_scene_create_moving refuses of the movers, an mcount[s] outside 0..SDFNMPC_SCENE_MAX_PRIMS, NULL mcount. */
int sdfnmpc_scene_create_mixed(sdfnmpc_ctx* ctx, int S, const int* count, const sdfnmpc_prim* prims, double cell,
                               const int* mcount, const sdfnmpc_prim* mprims, const sdfnmpc_prim_motion* mmotion,
                               sdfnmpc_scene** out);

/* ---- triangle-mesh scenes: mesh sets (csrc/scene_mesh.hip, csrc/mesh_bvh.h) ----
 * sdfnmpc_scene_create_mesh makes S scenes, each a static triangle mesh behind a bounding-volume hierarchy built on the
 * host inside the call (synchronous): nvert [S] and ntri [S] per scene, verts [sum of nvert][3] and tris [sum of
 * ntri][3] scene after scene, the indices local to their scene.  Vertices are rounded to fp32 once, as primitives are;
 * normals and boxes are formed in fp64 from the rounded values.  A scene with no triangles is allowed (a miss
 * everywhere, distance +inf).
 * The hierarchy: top-down, split at the median of the triangle centroids along the longest axis of the centroid bounds,
 * ordered by (centroid coordinate, triangle index), down to leaf_size triangles per leaf; nodes in depth-first preorder
 * with a skip index each, so the kernels walk it without a stack.  A box is the fp32 bounds of its fp32 vertices widened
 * by R / 4096 (R: the scene's largest absolute coordinate); the kernels' results do not depend on the hierarchy, bit for
 * bit (leaf_size = -1 is the brute-force yardstick through the same kernels).
 * The handle is used like any other by sdfnmpc_scene_render(_at), sdfnmpc_scene_distance(_at),
 * sdfnmpc_scene_swept_distance and every rollout that renders a scene; they dispatch on it (sdfnmpc_scene_is_mesh: 1,
 * else 0) and launch "scene_render_mesh", "scene_dist_mesh" and "scene_swept_mesh" (sdfnmpc_ctx_kernel_stats).  A mesh
 * set is static: times are ignored, sdfnmpc_scene_is_dynamic and sdfnmpc_scene_is_indexed are 0 and
 * sdfnmpc_scene_speed_bound gives 0.
 *   render    the pixel grid, pose rounding, values, clipping and scale of sdfnmpc_scene_render; fp32, one lane per pixel,
 *             bitwise reproducible.  A mesh is a surface: hits are double-sided with t >= 0, and a camera inside a
 *             closed mesh sees its inner walls -- there is no "camera inside sees zero" convention here.  The hit test
 *             evaluates each edge with its endpoints in ascending vertex-index order and accepts inclusively, so no
 *             ray passes between two triangles that share an edge (by index).
 *   distance  fp64: the distance to the nearest triangle, ties between triangles to the lower index.  closed = 0: unsigned.
 *             closed = 1: negative inside, by the sign of (p - c) . n at the closest point c for the angle-weighted
 *             pseudonormal n of the feature c lies on (face, edge or vertex); a point on the surface counts as outside.
 * SDFNMPC_E_ARG (nothing is allocated on the device): NULL ctx, nvert, ntri or out, S < 1, a negative count or one over
 * the limits below, more than 2^24 triangles in the set, a non-finite vertex, an index outside [0, nvert[s]), a
 * triangle whose area is zero after rounding, a leaf_size outside the values below, and with closed = 1 an edge that is
 * not shared by exactly two triangles traversing it in opposite directions.
 *   SDF rows  a set created with sdf_source = 1 is accepted by sdfnmpc_scene_sdf_rows, sdfnmpc_lin_args.sdf_scene and
 *             sdfnmpc_solver_set_sdf_scene (and so by every step and rollout of a solver with that source) and launches
 *             "scene_sdf_rows_mesh": the value of `distance` above, bit for bit, and its world gradient (see
 *             sdfnmpc_scene_sdf_rows).  sdfnmpc_scene_is_sdf_source: 1 for such a set and for every set that is not a
 *             mesh set, else 0.
 * The triangle-mesh work first shipped with a mesh set refused as an SDF source, and that refusal is pinned by a test of
 * the project that must keep passing as it is: a set created with sdf_source = 0 -- every caller from before the field
 * existed -- is still refused with the same code and message.  That, and nothing about the kernels, is why a mesh set
 * becomes a source only when it is created as one.
 * SDFNMPC_E_ARG (nothing is allocated on the device) also: a sdf_source other than 0 or 1.
 * SDFNMPC_E_UNSUPPORTED, nothing launched, outputs untouched: a mesh set created with sdf_source = 0 given to
 * sdfnmpc_scene_sdf_rows, sdfnmpc_lin_args.sdf_scene or sdfnmpc_solver_set_sdf_scene.  Movers beside a mesh:
 * sdfnmpc_scene_create_mesh_mixed below.  Moving meshes, several meshes in one scene and more than 32 moving objects:
 * sdfnmpc_scene_create_instanced below.  Not built: deforming or scaled meshes, meshes mixed with static primitives in
 * one scene, a walk pruned at max_df (or at the movers' distance) for closed sets, a hierarchy over the instances of an
 * instanced set (or more than SDFNMPC_SCENE_MAX_INSTANCES of them per scene). */
#define SDFNMPC_MESH_MAX_TRIS (1 << 20)  /* per scene */
#define SDFNMPC_MESH_MAX_VERTS (1 << 21) /* per scene */
typedef struct {
    int leaf_size; /* 1..8 triangles per leaf; 0: the default (4); -1: no hierarchy, one leaf holding every
                      triangle of the scene -- the brute-force yardstick through the same kernels */
    int closed;    /* 0: open surfaces, unsigned distance; 1: every scene must be a closed, consistently oriented
                      manifold (else SDFNMPC_E_ARG) and the distance is signed, negative inside */
    int sdf_source; /* 0: the set is refused as the controller's SDF source (SDFNMPC_E_UNSUPPORTED), as every mesh set
                      was before this field; 1: it is accepted.  Nothing else about the set depends on it */
} sdfnmpc_mesh_opts;
int sdfnmpc_scene_create_mesh(sdfnmpc_ctx* ctx, int S, const int* nvert, const double* verts, const int* ntri,
                              const int* tris, const sdfnmpc_mesh_opts* opts, sdfnmpc_scene** out);
int sdfnmpc_scene_is_mesh(const sdfnmpc_scene* scene);
int sdfnmpc_scene_is_sdf_source(const sdfnmpc_scene* scene);

/* ---- a mesh world with a few moving obstacles: mesh sets with movers (csrc/scene_mesh.hip) ----
 * sdfnmpc_scene_create_mesh_mixed is sdfnmpc_scene_create_mesh (nvert, verts, ntri, tris, opts: the same arguments,
 * checks, rounding and hierarchy) with a mover set beside every scene, exactly as sdfnmpc_scene_create_mixed puts one
 * beside a grid: mcount [S] primitives per scene, 0..SDFNMPC_SCENE_MAX_PRIMS, mprims [sum of mcount] and mmotion [sum
 * of mcount] as sdfnmpc_scene_create_moving takes and checks them (mmotion == NULL: no motion; such primitives are
 * still movers).  The movers are not in the hierarchy: they may be anywhere, overlap the mesh, or be all a scene has
 * (ntri[s] == 0).
 * Every query of such a handle is the minimum over the mesh and the movers at the query's time, bit for bit the
 * combination of the mesh set alone (sdfnmpc_scene_create_mesh, the same options) and of the movers as a dynamic set
 * of their own (sdfnmpc_scene_create_moving): the pixelwise minimum of the images, the minimum of the distances
 * (times [j] per point), and in the SDF row the movers' (h, J_h) only where their h is strictly below the mesh's -- on
 * a tie the mesh comes before a mover; within the mesh the lowest original triangle index wins, within the movers the
 * lowest mover index.  A closed mesh gives a signed value, a point inside a mover a negative one: the minimum is the
 * union.  sdfnmpc_scene_render(_at), sdfnmpc_scene_distance(_at), sdfnmpc_scene_swept_distance (its Lipschitz constant
 * takes the movers' speed bound), and for a set created with opts->sdf_source = 1 sdfnmpc_scene_sdf_rows,
 * sdfnmpc_lin_args.sdf_scene, sdfnmpc_solver_set_sdf_scene (predict as for a dynamic set) and every rollout of such a
 * solver take the handle; with sdf_source = 0 those three refuse it as they refuse a mesh set.  The kernels are
 * "scene_render_mesh_mixed", "scene_dist_mesh_mixed", "scene_sdf_rows_mesh_mixed" and "scene_swept_mesh_mixed" in
 * sdfnmpc_ctx_kernel_stats: they evaluate the movers first and start the walk of the hierarchy from what they give (an
 * open set's distance walk is pruned at the movers' distance; a closed set takes the full walk, for the sign).
 * With a mover in some scene sdfnmpc_scene_is_mesh and sdfnmpc_scene_is_dynamic are 1, sdfnmpc_scene_is_indexed is 0 and
 * sdfnmpc_scene_speed_bound gives the movers' bound per scene.  With every mcount[s] == 0 the handle is what
 * sdfnmpc_scene_create_mesh returns (not dynamic, the mesh kernels under their names).
 * SDFNMPC_E_ARG (nothing is allocated on the device): what sdfnmpc_scene_create_mesh refuses of the mesh arguments, what
 * sdfnmpc_scene_create_moving refuses of the movers, an mcount[s] outside 0..SDFNMPC_SCENE_MAX_PRIMS, NULL mcount.
 * Not built: more than 32 movers per scene. */
int sdfnmpc_scene_create_mesh_mixed(sdfnmpc_ctx* ctx, int S, const int* nvert, const double* verts, const int* ntri,
                                    const int* tris, const sdfnmpc_mesh_opts* opts, const int* mcount,
                                    const sdfnmpc_prim* mprims, const sdfnmpc_prim_motion* mmotion, sdfnmpc_scene** out);

/* ---- instanced mesh scenes: rigid, moving copies of shared meshes (csrc/scene_inst.hip, csrc/inst_dev.h) ----
 * sdfnmpc_scene_create_instanced makes a pool of nparts parts and S scenes of instances that place them.  A part is a
 * triangle mesh in its own coordinates, given, checked, rounded to fp32 and put behind a hierarchy exactly as a scene of
 * sdfnmpc_scene_create_mesh is (nvert [nparts], verts, ntri [nparts], tris: that function's arguments with nparts for
 * S; opts: closed, leaf_size and sdf_source mean what they mean there), and stored once however often it is placed.
 * Scene s holds icount[s] instances, 0..SDFNMPC_SCENE_MAX_INSTANCES, instances [sum of icount] scene after scene.
 * Instance i is a part under the rigid frame of sdfnmpc_scene_create_moving about the part's origin,
 *   c(t) = p + v t + amp sin(omega t + phase),   R(t) = Rz(yaw_rate t) R(q),
 * formed in fp64; there is no scale.  With x' = R(t)^T (x - c(t)):
 *   distance  min over i of the part's distance at x'_i, fp64: unsigned for closed = 0; for closed = 1 every part must be
 *             a closed, consistently oriented manifold and the value is the minimum of the instances' signed distances,
 *             the union -- instances may overlap.
 *   render    the smallest hit t >= 0 over the instances, fp32; instance i's ray has the origin R(t)^T (W_p_C - c(t))
 *             and the axes R(t)^T W_R_C, formed in fp64 and rounded to fp32 once per image.  Hit rule (double-sided,
 *             edge-consistent, no "inside sees zero"), pixel grid, clipping, depth / range and scale: a mesh set's.
 *   SDF rows  (sdf_source = 1) the value and the gradient R(t) g' of the minimising instance, g' the mesh row's gradient
 *             in the part's frame; the lowest instance index wins a tie, within a part the lowest original triangle
 *             index.  Truncation, flag and row contract: a mesh set's.  Node k of a source with tau at t0 + tau[k].
 *   swept     sdfnmpc_scene_swept_distance over the distance above; the speed bound V of a scene is the maximum over its
 *             instances of |v| + |omega| |amp| + |yaw_rate| rho, rho the largest |vertex| of the part, inflated by
 *             1 + 1e-12 (sdfnmpc_scene_speed_bound).
 * A scene without instances renders a miss everywhere and is at distance +inf.  Results depend neither on the parts'
 * hierarchies (leaf_size) nor on the order of the instances or on which of them a query skips, bit for bit, except for
 * the tie rule of the rows.  An instance with p = 0, q = identity and no motion gives the bits of the mesh set of its
 * part.  The top level is a linear pass over the scene's instances in every query.
 * For such a handle sdfnmpc_scene_is_instanced is 1, sdfnmpc_scene_is_mesh and sdfnmpc_scene_is_indexed are 0,
 * sdfnmpc_scene_is_dynamic is 1 exactly when some instance has a non-zero v, amp or yaw_rate, and
 * sdfnmpc_scene_is_sdf_source is opts->sdf_source.  sdfnmpc_scene_render(_at), sdfnmpc_scene_distance(_at),
 * sdfnmpc_scene_swept_distance and every rollout that renders a scene take it, and with sdf_source = 1
 * sdfnmpc_scene_sdf_rows, sdfnmpc_lin_args.sdf_scene and sdfnmpc_solver_set_sdf_scene; with sdf_source = 0 those three
 * refuse it (SDFNMPC_E_UNSUPPORTED, nothing launched, outputs untouched).  The kernels are "scene_render_inst",
 * "scene_dist_inst", "scene_sdf_rows_inst" and "scene_swept_inst" in sdfnmpc_ctx_kernel_stats.  A spherical image of
 * an instanced set needs H + W <= 4096 (SDFNMPC_E_ARG otherwise).
 * SDFNMPC_E_ARG (nothing is allocated on the device): nparts or S outside 1..2^20, a part index outside [0, nparts), an
 * icount[s] outside 0..SDFNMPC_SCENE_MAX_INSTANCES, a zero quaternion, a non-finite position or motion value, what
 * sdfnmpc_scene_create_mesh refuses of a part (closed = 1 with a part that is not closed among it), a NULL argument.
 * Not built: a hierarchy over the instances, scaled or deforming instances, primitives in an instanced set. */
#define SDFNMPC_SCENE_MAX_INSTANCES 256
typedef struct {
    int part;                      /* index into the pool, 0..nparts-1 */
    double p[3];                   /* the position of the part's origin at t = 0 (without the harmonic term) */
    sdfnmpc_prim_motion motion;    /* q, yaw_rate, v, amp, omega, phase */
} sdfnmpc_mesh_instance;
int sdfnmpc_scene_create_instanced(sdfnmpc_ctx* ctx, int nparts, const int* nvert, const double* verts, const int* ntri,
                                   const int* tris, const sdfnmpc_mesh_opts* opts, int S, const int* icount,
                                   const sdfnmpc_mesh_instance* instances, sdfnmpc_scene** out);
int sdfnmpc_scene_is_instanced(const sdfnmpc_scene* scene);

/* sdfnmpc_solver_rollout with perception inside the loop.  Before step k with (k + phase) % every == 0 it enqueues, on the
 * solver's stream and in this order: (a) sdfnmpc_scene_pose from the solver's x0 field; (b) sdfnmpc_scene_render of
 * every instance's scene from that camera pose; (c) sdfnmpc_vae_encode of the images; (d) sdfnmpc_pack_refs in mode -1
 * with that latent and body pose (Nmpc.set_latent on the device; the sdf flag is untouched).  Then the step's
 * sequence of sdfnmpc_solver_rollout.  Still a plain launch sequence: no graph, no host synchronisation and no copy
 * inside the loop.  perc == NULL is sdfnmpc_solver_rollout.  The workspaces are the caller's and hold the last
 * perception afterwards.  pts_log keeps its meaning, the camera frame of node 0's pose parameters at the time of
 * logging: with perception that is the frame of the latest image (row k + 1 is logged after step k, in the frame of
 * the image taken at or before step k).
 * SDFNMPC_E_ARG, all before the first launch: what sdfnmpc_solver_rollout, sdfnmpc_scene_render, sdfnmpc_scene_pose,
 * sdfnmpc_vae_encode and sdfnmpc_pack_refs refuse, every < 1, phase < 0, a NULL workspace, an encoder or a scene that does not
 * live on the solver's context, a latent size that does not fit the solver's parameter row (17 + L > np). */
typedef struct {
    const sdfnmpc_scene* scene;
    const int* scene_of;           /* device [B] or NULL */
    sdfnmpc_img_opts img;          /* the sensor */
    int h, w;                      /* rendered image size (the encoder resizes when its own differs) */
    float scale;                   /* as sdfnmpc_scene_render: the raw sensor image, 1000 / mm_resolution */
    double B_p_C[3], B_R_C[9];     /* sensor extrinsics */
    sdfnmpc_vae* vae;              /* loaded on the solver's context */
    sdfnmpc_vae_opts vae_opts;     /* clip and yz; B, in_h, in_w and dtype are set by the rollout (B, h, w, float32) */
    int every;                     /* >= 1: a new image before every `every`-th step, starting with step 0 */
    int phase;                     /* >= 0: steps already taken since the schedule began -- a new image before step k
                                      when (k + phase) % every == 0, so that a rollout cut into chunks perceives
                                      where the uncut one does (0: before step 0) */
    float* images;                 /* device workspaces: [B][h][w] */
    float* latent;                 /* [B][L] */
    double* latent64;              /* [B][L] */
    double *W_p_Bo, *W_R_Bo, *W_p_C, *W_R_C; /* [B][3], [B][9], [B][3], [B][9] */
} sdfnmpc_perceive_args;

int sdfnmpc_solver_rollout_perceive(sdfnmpc_solver* s, const sdfnmpc_rollout_args* args,
                                    const sdfnmpc_perceive_args* perc);
/* sdfnmpc_solver_rollout_perceive of a scene that moves: the image before step k is rendered at the time
 * t = t0 + (double)(perc->phase + k) * dt, one multiplication and one addition in fp64 (never a fused multiply-add),
 * so that a host loop that calls sdfnmpc_scene_render_at with the same expression gets the same bits.
 * sdfnmpc_solver_rollout_perceive is _at(..., 0, 0).  Also refused, before the first launch: a non-finite t0 or dt,
 * dt < 0. */
int sdfnmpc_solver_rollout_perceive_at(sdfnmpc_solver* s, const sdfnmpc_rollout_args* args,
                                       const sdfnmpc_perceive_args* perc, double t0, double dt);

/* ---- the scene's exact distance as the controller's SDF (csrc/scene_sdf.hip) ----
 * sdfnmpc_scene_sdf_rows writes what the network kernels' epilogue writes (gen_model.py:46-61), from the closed forms of
 * sdfnmpc_scene_distance(_at): for node row r = b (N+1) + k with the world position x[r][0..2], the instance's scene
 * and the time t0 + tau[k],
 *   h[r][2] = flag df + (1 - flag) max_df,   Jh[r][j][2] = flag grad_j (j < 3), 0 (j = 3..9),   flag = p[r][0]
 * where df = d and grad = the world gradient of d where the signed distance d < max_df, else (and for a scene without
 * primitives) df = max_df and grad = 0.  The gradient is that of the primitive attaining the minimum (the lowest index
 * on a tie), taken in the primitive's frame and rotated by R(t): sphere q / |q|; box and capped cylinder the normalised
 * positive excesses outside and the axis of the largest excess inside.  At a kink it is one of the one-sided values,
 * finite and of norm <= 1.  Columns 0 and 1 of h and Jh are not touched.  A set that is not dynamic takes the static
 * kernel whatever the time.  fp64, no atomics: a row does not depend on its place in the batch.  "scene_sdf_rows" in
 * sdfnmpc_ctx_kernel_stats.
 * A mesh set created with sdfnmpc_mesh_opts.sdf_source = 1 ("scene_sdf_rows_mesh"; t0 and tau are accepted and not
 * read): d is the value sdfnmpc_scene_distance returns for the position, bit for bit, from the same search.  grad =
 * (p - c) / |p - c| for the closest point c of the nearest triangle (the lowest index on a tie), negated where a closed
 * set's d is negative: a unit vector away from the surface outside, towards it inside.  At d = 0: the normalised
 * pseudonormal of the feature c lies on (closed sets), the winning triangle's unit face normal (open sets), one-sided
 * values.  A row whose position is not finite gives (max_df, 0).  The rows of an open set are searched only within
 * max_df (the same bits as the full search followed by the truncation); a closed set takes the full search.
 * x [B][N+1][10], p [B][N+1][np], h [B][N+1][3], Jh [B][N+1][10][3] device float64.
 * Asynchronous on the context stream; B == 0 is a no-op.  SDFNMPC_E_ARG (nothing is launched, outputs untouched): NULL
 * arguments, B < 0, N < 1, np < 17, max_df not > 0 or not finite, a non-finite t0, a scene on another context.
 * SDFNMPC_E_UNSUPPORTED (the same): a mesh set created with sdf_source = 0. */
int sdfnmpc_scene_sdf_rows(sdfnmpc_ctx* ctx, const sdfnmpc_scene_sdf_opts* opts, int B, int N, int np, const double* x,
                           const double* p, double* h, double* Jh);

/* The solver's SDF source.  scene != NULL: every later step evaluates the scene's exact distance instead of the
 * network (sdfnmpc_lin_args.sdf_scene), truncated at max_df, for scene_of [B] (device, NULL: scene 0; the caller's to
 * keep alive), at the solver's scene time; with predict node k sees the scene at that time + tau[k], tau[0] = 0,
 * tau[k] = tau[k-1] + dt[k-1] of the solver's own grid.  scene == NULL returns to the network.  The solver keeps the
 * two pointers, not copies: the scene, like scene_of, must stay alive while it is the source -- call this with NULL
 * before sdfnmpc_scene_free (sdf_nmpc_amd.scene.Scene.close does).  SDFNMPC_E_ARG: no row
 * or cost of the solver's constraint set reads the SDF, a scene on another context, max_df not > 0 or not finite. */
int sdfnmpc_solver_set_sdf_scene(sdfnmpc_solver* s, const sdfnmpc_scene* scene, const int* scene_of, double max_df,
                                 int predict);
/* The scene time the next steps pass as sdfnmpc_scene_sdf_opts.t0 (0 at creation).  SDFNMPC_E_ARG: a non-finite t. */
int sdfnmpc_solver_set_scene_time(sdfnmpc_solver* s, double t);

/* sdfnmpc_solver_rollout for a solver with a scene source.  Before step k the solver's scene time is set to
 * t0 + (double)(phase + k) * dt (the product rounded on its own, as sdfnmpc_solver_rollout_perceive_at forms it), and
 * with pose != NULL and (k + phase) % pose->every == 0 the camera pose the field-of-view rows read is refreshed:
 * sdfnmpc_scene_pose from the solver's x0 field into the caller's workspaces, then sdfnmpc_pack_refs in mode -2.  A
 * plain launch sequence.  SDFNMPC_E_ARG, all before the first launch: what sdfnmpc_solver_rollout refuses, no source
 * set on the solver, every < 1, phase < 0, a missing workspace, a non-finite t0 or dt, dt < 0. */
typedef struct {
    int every;                     /* >= 1 */
    double B_p_C[3], B_R_C[9];     /* sensor extrinsics */
    double *W_p_Bo, *W_R_Bo, *W_p_C, *W_R_C; /* device workspaces [B][3], [B][9], [B][3], [B][9] */
} sdfnmpc_pose_refresh_args;
int sdfnmpc_solver_rollout_scene_sdf(sdfnmpc_solver* s, const sdfnmpc_rollout_args* args,
                                     const sdfnmpc_pose_refresh_args* pose, int phase, double t0, double dt);

/* The solver's SDF source, an image: opts != NULL -- every later step evaluates sdfnmpc_img_sdf_rows instead of the
 * network (sdfnmpc_lin_args.sdf_image) with the camera pose that is in p.  NULL returns to the network.  Setting either
 * source (scene or image) replaces the other.  The solver copies the option block but keeps its pointers, not what they
 * point to: images, img_of, grid and pooled stay the caller's and must stay alive while they are the source.
 * SDFNMPC_E_ARG: no row or cost of the solver's constraint set reads the SDF, what sdfnmpc_img_sdf_rows refuses. */
int sdfnmpc_solver_set_sdf_image(sdfnmpc_solver* s, const sdfnmpc_img_sdf_opts* opts);

/* ---- image morphology (csrc/morph.hip) ----
 * The reference's Dilate / Erode (utils/preprocessing.py:100-199) on images in / out [B][H][W] (device float32, in !=
 * out) with a structuring element kernel [k_h][k_w] (host bytes, row-major; a tap is included where the byte is not
 * 0), as the reference writes them: the image is padded by origin = (k_h / 2, k_w / 2) on the top / left and by k -
 * origin - 1 on the bottom / right with the border value -2 (dilate, op 0) or +2 (erode, op 1); the erosion of a pixel
 * is the minimum over all k_h k_w taps (i, j) of padded[y + i][x + j] + bias(i, j), the bias 0 where the tap is
 * included and +2 where it is not; the dilation is the maximum with the bias 0 / -2 of the *flipped* element (tap
 * (i, j) is included where kernel[k_h-1-i][k_w-1-j] is) on the same, unflipped padding -- for an even-sized or
 * asymmetric element not a textbook dilation.  While an included tap reads a value of the image (the reference's
 * modules assume images normalised by dmax, in [0, 1]) the result is the plain min / max over the included taps; where
 * every included tap reads the border value, an erosion of a non-negative image gives the border value 2 itself and a
 * dilation the largest excluded value minus 2, as the reference's does.  ignore_zeros: zeros count as the border value
 * during the scan, and a result equal to the border value becomes 0; the input is not modified (the reference's
 * module overwrites its input).  The results are the reference's bit for bit.  Asynchronous on the context stream;
 * B == 0 is a no-op.  SDFNMPC_E_ARG (nothing is launched, out untouched): NULL arguments, in == out, op not 0 / 1, B < 0 or > 65535,
 * H or W < 1 (or B H W beyond 2^31 - 1), k_h or k_w outside 1..21, an element without a 1. */
#define SDFNMPC_MORPH_DILATE 0
#define SDFNMPC_MORPH_ERODE 1
#define SDFNMPC_MORPH_K_MAX 21
int sdfnmpc_morph(sdfnmpc_ctx* ctx, int op, const unsigned char* kernel, int k_h, int k_w, int ignore_zeros,
                  const float* in, int B, int H, int W, float* out);
/* RemoveCloseOutliers(kernel_size, min_range) (utils/preprocessing.py:241-259): t = in < min_range ? 0 : in, the
 * opening of t (erosion, then dilation, by a kernel_size x kernel_size element of ones, ignore_zeros off), and the
 * value of t restored where the opening is > 0.  min_range is in the image's own units.  kernel_size 3 is one fused
 * launch ("outlier_rm" in sdfnmpc_ctx_kernel_stats) without an intermediate image in device memory; any other size
 * takes a threshold launch, two sdfnmpc_morph launches and a restore launch through workspaces of the context.  Both
 * give what the composition of the reference's modules gives.  SDFNMPC_E_ARG (nothing is launched): NULL arguments,
 * in == out, B < 0 or > 65535, H or W < 1 (or B H W beyond 2^31 - 1), kernel_size outside 1..21, a non-finite min_range. */
int sdfnmpc_outlier_rm(sdfnmpc_ctx* ctx, int kernel_size, float min_range, const float* in, int B, int H, int W,
                       float* out);

/* ---- sensor degradation (csrc/sensor.hip) ----
 * What a real depth camera does to the exact image sdfnmpc_scene_render gives, in place on img [B][H][W] (device
 * float32) in the image's own units (raw or normalised; vmax is the image's value at dmax).  Per pixel with value v:
 *   1. miss     with miss_invalid, v >= vmax -> 0 (no return)
 *   2. noise    v == 0 stays 0 (utils/data.py:67); else v <- clamp(v + (a + b v^2) z, 0, vmax), z ~ N(0, 1)
 *   3. dropout  with probability p_thresh / 2^32 the pixel becomes 0
 *   4. boxes    the pixel becomes 0 inside any of the image's erased rectangles
 * The randomness is counter-based: one Philox4x32-10 call per pixel with the 64-bit seed as the key (low word first)
 * and the counter (pixel index y W + x, frame, stream, 0), stream = stream_id[b] (device int32 [B]; NULL: b).  Words 0
 * and 1 give u = ((w >> 8) + 1) 2^-24 in (0, 1] and z = sqrtf(-2 logf(u1)) cosf(2 pi u2); word 2 < p_thresh (unsigned)
 * is the dropout decision.  No atomics, no state: the result depends on (seed, stream, frame, pixel, v) only, not on
 * the instance's place in the batch, the launch shape or earlier launches.
 * boxes: device int16 [n_frames][B][max_boxes][4] = (y0, x0, h, w) per box, h == 0: none; the launch reads the
 * entries of frame % n_frames and of instance b.  NULL: no boxes (n_frames and max_boxes are then ignored).
 * outlier_rm: after the degradation, sdfnmpc_outlier_rm(3, min_range) of the image through the caller's workspace
 * scratch [B][H][W] (required exactly then), and the result copied back into img.
 * SDFNMPC_E_ARG (nothing is launched, img untouched): NULL ctx / opts / img, B < 0 or > 65535, H or W < 1 (or B H W
 * beyond 2^31 - 1), a non-finite or negative a or b, vmax not positive and finite, frame < 0, a box table with n_frames
 * < 1 or max_boxes outside 0..8, outlier_rm without scratch or with a non-finite min_range.  B == 0 is a no-op. */
typedef struct {
    uint64_t seed;
    float a, b;                    /* noise standard deviation a + b v^2, image units */
    float vmax;
    uint32_t p_thresh;             /* floor(p 2^32) */
    int miss_invalid;
    int outlier_rm;
    float min_range;               /* image units (outlier_rm) */
    const int16_t* boxes;
    int n_frames, max_boxes;
    const int* stream_id;
} sdfnmpc_sensor_opts;
int sdfnmpc_sensor_apply(sdfnmpc_ctx* ctx, const sdfnmpc_sensor_opts* opts, int frame, float* img, int B, int H, int W,
                         float* scratch);

/* sdfnmpc_solver_rollout_perceive_at with a sensor model between the renderer and the encoder: at a perceiving step k
 * the sequence is pose, render, sdfnmpc_sensor_apply(sensor, frame = perc->phase + k, perc->images, scratch), encode,
 * pack -- so a rollout cut into chunks degrades as the uncut one does, and a host loop that calls sdfnmpc_sensor_apply
 * with that frame between the render and the encoder gets the same bits.  perc->images holds the degraded image
 * afterwards.  sensor == NULL is exactly sdfnmpc_solver_rollout_perceive_at (scratch is ignored).  Also refused, before
 * the first launch: a sensor without perc, what sdfnmpc_sensor_apply refuses, phase + steps beyond 2^31 - 1. */
int sdfnmpc_solver_rollout_perceive_sensor(sdfnmpc_solver* s, const sdfnmpc_rollout_args* args,
                                           const sdfnmpc_perceive_args* perc, double t0, double dt,
                                           const sdfnmpc_sensor_opts* sensor, float* scratch);

/* sdfnmpc_solver_rollout for a solver with an image source.  With perc != NULL (scene, scene_of, img, h, w, extrinsics,
 * scale, every, phase and the four pose workspaces are read; no encoder: vae, vae_opts, images and the latents are
 * ignored), before step k with (k + perc->phase) % perc->every == 0 it enqueues, in this order: (1) sdfnmpc_scene_pose
 * from the solver's x0 field; (2) sdfnmpc_scene_render_at of the normalised image (perc->scale = 1 / dmax, the scale
 * ColChecker takes) into the source's images, at t0 + (double)(phase + k) * dt formed as sdfnmpc_solver_rollout_perceive_at forms
 * it; (3) with sensor != NULL sdfnmpc_sensor_apply as frame phase + k (its vmax and min_range in normalised units);
 * (4) in unsigned mode sdfnmpc_img_sdf_pool; (5) sdfnmpc_pack_refs in mode -2 (the pose columns of p).  Then the step's
 * sequence of sdfnmpc_solver_rollout.  perc == NULL keeps the image and the pose as they are set.  A plain launch
 * sequence.  SDFNMPC_E_ARG, all before the first launch: what the other rollouts refuse, no image source set on the
 * solver, a render size other than the source's H x W, a source that maps instances to images (img_of) with perc, a
 * sensor without perc. */
int sdfnmpc_solver_rollout_image_sdf(sdfnmpc_solver* s, const sdfnmpc_rollout_args* args,
                                     const sdfnmpc_perceive_args* perc, double t0, double dt,
                                     const sdfnmpc_sensor_opts* sensor, float* scratch);

/* sdfnmpc_solver_rollout_image_sdf for an image source that holds the RECONSTRUCTION of the camera image: what the
 * VAE's latent retains of it (encode, decode), the rung between the camera image and the network.  perc is required
 * and names, beside what sdfnmpc_solver_rollout_image_sdf reads, the encoder (perc->vae), the camera buffer
 * perc->images [B][h][w] float32 (not the source's images), perc->latent [B][L] float32, optionally perc->latent64, and
 * perc->vae_opts.yz, the Depth2Range table, required when perc->img.is_depth.  Before step k with (k + perc->phase) %
 * perc->every == 0 it enqueues, in this order: (1) sdfnmpc_scene_pose; (2) sdfnmpc_scene_render_at of the normalised
 * image (perc->scale = 1 / dmax) into the camera buffer; (3) with sensor != NULL sdfnmpc_sensor_apply on that buffer as
 * frame phase + k, in normalised units; (4) sdfnmpc_vae_encode with clip = 1 and the yz table exactly when the camera
 * measures depth; (5) sdfnmpc_vae_decode of that latent into the source's images at the source's H x W (a range image:
 * set the source's img.is_depth = 0); (6) in unsigned mode sdfnmpc_img_sdf_pool; (7) sdfnmpc_pack_refs in mode -2.
 * Then the step's sequence.  The latent columns of p are not written: no network is evaluated.  A plain launch
 * sequence.  SDFNMPC_E_ARG, all before the first launch: what sdfnmpc_solver_rollout_image_sdf refuses, perc == NULL,
 * no decoder, no encoder, either on another context, different latent sizes, missing workspaces, a camera buffer that
 * is the source's, a depth camera without the table. */
int sdfnmpc_solver_rollout_image_recon(sdfnmpc_solver* s, const sdfnmpc_rollout_args* args,
                                       const sdfnmpc_perceive_args* perc, double t0, double dt,
                                       const sdfnmpc_sensor_opts* sensor, float* scratch, sdfnmpc_vae_dec* dec);

/* ---- shooting grid (host, bit-exact numpy.linspace/diff semantics of ocp.py:21-27) ---- */
int sdfnmpc_shooting_grid(int N, double T, int uniform, int nb_short_nodes, double dt_short, double* nodes,
                          double* dt);

#ifdef __cplusplus
}
#endif
#endif /* SDFNMPC_H */
