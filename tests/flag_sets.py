"""TEST INFRASTRUCTURE: the flag sets of default.yaml:16-23 the parity tests run (gen_model.py:26-149).

Each entry: name -> (Config overrides, expected stage columns, expected terminal rows as (hN_col, hE_col,
soft)).  'lidar' is sensor.hfov >= 3.14 (gen_model.py:42: no hfov row), with a spherical sensor so that
Config's fov consistency check (utils/config.py:39-41) holds."""
import numpy as np

LIDAR = dict(sensor__hfov=3.1416, sensor__is_spherical=True, sensor__aspect_ratio=3.1416 / 0.4903)
RF = dict(flags__recursive_feasibility=True)
ST = dict(flags__recursive_feasibility=True, flags__stability=True)
# hard stage rows (slack weight None: add_const_stage / add_const_term without slack, base_model.py:142-168)
HARD_FOV = dict(mpc__weights__slack_fov=None)
HARD_DF = dict(mpc__weights__slack_df=None)

FLAG_SETS = {
    "default": ({}, [0, 1, 2], [(0, -1, True), (1, -1, True), (2, -1, True)]),
    "no_sdf": (dict(flags__enable_sdf=False), [], []),
    "no_sdf_constraint": (dict(flags__sdf_constraint=False), [0, 1], [(0, -1, True), (1, -1, True)]),
    "sdf_cost_only": (dict(flags__sdf_constraint=False, flags__sdf_cost=True), [0, 1], [(0, -1, True), (1, -1, True)]),
    "no_vfov": (dict(flags__vfov_constraint=False), [0, 2], [(0, -1, True), (2, -1, True)]),
    "lidar": (LIDAR, [1, 2], [(1, -1, True), (2, -1, True)]),
    "lidar_sdf_only": (dict(LIDAR, flags__vfov_constraint=False), [2], [(2, -1, True)]),
    "rec_feas": (RF, [0, 1, 2], [(0, -1, True), (1, -1, True), (2, 0, False), (-1, 1, False), (-1, 2, False)]),
    "rec_feas_soft_brake": (dict(RF, mpc__weights__slack_brake=[50.0, 10.0]), [0, 1, 2],
                            [(0, -1, True), (1, -1, True), (2, 0, True), (-1, 1, False), (-1, 2, False)]),
    # the network read by terminal rows only (the braking row), no stage sdf row: need_sdf with sdf_row == -1
    "rec_feas_no_sdf_row": (dict(RF, flags__sdf_constraint=False), [0, 1],
                            [(0, -1, True), (1, -1, True), (2, 0, False), (-1, 1, False), (-1, 2, False)]),
    "rec_feas_lidar_no_rows": (dict(RF, **LIDAR, flags__sdf_constraint=False, flags__vfov_constraint=False), [],
                               [(2, 0, False), (-1, 1, False)]),
    "stability": (ST, [0, 1, 2], [(0, -1, True), (1, -1, True), (2, 0, False), (-1, 1, False), (-1, 2, False),
                                  (-1, 3, False), (-1, 4, False), (-1, 5, False)]),
    "stability_lidar_no_vfov": (dict(ST, **LIDAR, flags__vfov_constraint=False), [2],
                                [(2, 0, False), (-1, 1, False), (-1, 3, False), (-1, 4, False), (-1, 5, False)]),
    # stage rows ordered soft first (model.Quad.h_cols), terminal rows soft first
    "hard_fov": (HARD_FOV, [2, 0, 1], [(2, -1, True), (0, -1, False), (1, -1, False)]),
    "hard_df": (HARD_DF, [0, 1, 2], [(0, -1, True), (1, -1, True), (2, -1, False)]),
    "hard_all": (dict(HARD_FOV, **HARD_DF), [0, 1, 2], [(0, -1, False), (1, -1, False), (2, -1, False)]),
    "hard_fov_lidar": (dict(LIDAR, **HARD_FOV), [2, 1], [(2, -1, True), (1, -1, False)]),
    "hard_df_rec_feas": (dict(RF, **HARD_DF), [0, 1, 2],
                         [(0, -1, True), (1, -1, True), (2, 0, False), (-1, 1, False), (-1, 2, False)]),
}
HARD_SETS = [n for n in FLAG_SETS if n.startswith("hard")]

# Edges of the segmented QP kernel's horizon / segment-count space as (N, SDFNMPC_QP_NSEG set, segments P): the
# partition is a_i = i (N + 1) / P.  Without the variable: N = 7 (P = 4, two nodes per segment), 36 (AUTO's lower
# bound), 37 (38 nodes: segments of 9, 10, 9, 10), 63 (16 nodes per segment, the kernel's largest horizon), 5
# (the smallest N with P = 3), 3 (the smallest with P = 2).  With it: the three- and two-segment instantiations at
# a mid horizon and at their largest one (47, 31: 16 nodes per segment).
SEG_EDGES = [(7, False, 4), (36, False, 4), (37, False, 4), (63, False, 4), (5, False, 3), (30, True, 3), (47, True, 3),
             (3, False, 2), (20, True, 2), (31, True, 2)]


# The phase-split runs (test_gpu_flags.test_phase_split_bitwise_per_flag_set) as (B, N, kernel, seed): the serial
# kernel under AUTO; the segmented one under AUTO; the segmented one forced at a short horizon.  The test asks for
# status 0 everywhere, so each seed is one at which every QP of every set below is feasible -- the C IPM on the
# oracle linearisation converges on all of them (test_flags.test_phase_split_problems_converge_in_the_c_ipm).  At
# (8, 20) seeds 13 and 14 each give hard_df_rec_feas one instance whose hard sdf row is infeasible (status 2 from
# the C IPM as from both kernels): the next seed, 15.
PHASE_SPLIT_SETS = ["no_vfov", "lidar_sdf_only", "sdf_cost_only", "no_sdf", "rec_feas", "stability", "hard_fov",
                    "hard_df_rec_feas", "stability_lidar_no_vfov", "rec_feas_no_sdf_row", "rec_feas_lidar_no_rows"]
# The last three are short horizons on the serial kernel, 96, 48 and 8 rows of the linearisation: both sides of the
# 64-row line below which the preparation runs its few-row path, with the sdf-row patch at N + 1 = 3, 6, 2 nodes.
PHASE_SPLIT_RUNS = [(24, 20, "auto", 13), (8, 40, "auto", 13), (8, 20, "segmented", 15),
                    (32, 2, "auto", 13), (8, 5, "auto", 13), (4, 1, "auto", 13)]

# ---- the serial QP kernel's horizon edges (rti_qp.hip; test_gpu_flags.test_serial_qp_horizon_edges)
# The kernel's LDS per instance, csrc/qp_kernels.h qp_lds_doubles restated (rows: (ns, nhN, nsN, nhs)), with the
# constants the edge table below assumes: a ring of QP_RING = 3 stream positions (QP_RING_DEPTH's default; the
# tests hold the library's sdfnmpc_qp_lds_bytes to this formula, whose QP_RING * 168 term moves with the depth).
QP_RING, QP_SLOT, QP_NHN, QP_N_MAX = 3, 5, 8, 200
LDS_PER_CU = 160 * 1024  # bytes of LDS per compute unit of the MI355X (CDNA4)


def qp_rows(name):
    """(ns, nhN, nsN, nhs) of a flag set, from its FLAG_SETS entry (QpRows of csrc/qp_kernels.h)."""
    over, cols, rows = FLAG_SETS[name]
    hard = [c for c in cols if (c < 2 and "mpc__weights__slack_fov" in over) or (c == 2 and "mpc__weights__slack_df" in over)]
    return len(cols), len(rows), sum(1 for r in rows if r[2]), len(hard)


def qp_lds_doubles(N, rows):
    ns, nhN, nsN, nhs = rows
    even = lambda n: (n + 1) & ~1
    N1, G = N + 1, N * ns + nhN
    m = 8 * N + 4 * (N * (ns - nhs) + nsN) + 2 * ((N - 1) * nhs + nhN - nsN)
    return (2 * even(m) + 2 * even(N1 * 10) + 3 * even(N * 4) + 2 * even(G) + QP_SLOT * 64 + QP_RING * 168 + 48 + 2
            + even(N * 4) + even(G) + even(N1) + 2 * even(G) + 2 * even(N * 4) + 8 + 4 * (3 + QP_NHN) + even(nhN * 10))


def serial_max_horizon(name, limit=LDS_PER_CU):
    """The largest horizon (<= the ABI's 200) at which one instance of the set fits `limit` bytes of LDS."""
    return max(N for N in range(1, QP_N_MAX + 1) if qp_lds_doubles(N, qp_rows(name)) * 8 <= limit)


# (N, flag sets), PD = QP_RING.  Every sweep of the kernel is unrolled by PD over NP = ceil((N + 1) / PD) PD
# positions:
#   1   N + 1 < PD: the single-trip branch with one dead position, one stage; every factor row from fsave; the HARD
#       instantiation with zero hard stage rows (node 0's zero folds are its only stage groups); nhN = 8 (stability)
#   2   N + 1 = PD: the single trip with no dead position; the NSS = 0 instantiation (no_sdf)
#   3   N + 1 = PD + 1: a first and a last trip, no middle one, two dead tail positions
#   4   one dead tail position; hard stage rows at nodes 1..3 only
#   5   N + 1 = 2 PD: no tail, no middle trip
#   8   N + 1 = 3 PD: the middle loop runs exactly once
#   35  AUTO's last serial horizon below the segmented range
#   64  the first horizon beyond the segmented kernel
#   the largest horizon of the widest row set (stability, nhN = 8) and of the default rows (193 and 194 with 160 KiB
#   of LDS per CU: one instance fills a CU's LDS), computed from the formula above
_E2 = ["default", "rec_feas_no_sdf_row"]
SERIAL_EDGES = [(1, _E2 + ["hard_df_rec_feas", "stability", "no_sdf"]), (2, _E2 + ["no_sdf"]), (3, _E2),
                (4, _E2 + ["hard_df_rec_feas"]), (5, _E2), (8, _E2), (35, _E2 + ["hard_df_rec_feas"]), (64, _E2),
                (serial_max_horizon("stability"), ["stability"]), (serial_max_horizon("default"), _E2)]
# B = 16, seed 12; test_flags.test_serial_edges_references holds the references to the GPU test's bars on the CPU.
# (1, stability) at seed 12 has one instance on which the C IPM's stopped point misses the exact solution's
# objective bound (4.3e-5 against 1.1e-5), at seed 13 one that runs to max_iter: the next seed that meets the bars.
SERIAL_EDGE_SEEDS = {(1, "stability"): 14}
SERIAL_LONG_N = 100    # from here on no dense solve (one exact solve at N = 194 takes over a minute)
# The per-iteration pin (du after max_iter = 1 and 2 against the C IPM at the same max_iter).  Up to N = 64 the
# bar test_qp_warm_start_matches_riccati_oracle holds at N = 40.  At the long horizons max(1e-9, 10 x the reference
# against itself): the C IPM's serial recursion against its recursion over four segments (another evaluation
# order of the same Newton steps) at the same N, B = 16, seed 12, measured on the CPU: 1.3e-15 after one iteration,
# 4.2e-15 after two (193 stability; 2.9e-15 and 3.7e-15 at 194), with |du| up to 0.9.  The factor 10 covers the
# GPU's fused multiply-adds and summation order; 10 x 4.2e-15 is far below 1e-9, so the long horizons keep the
# short ones' bar.  test_flags.test_serial_edges_references holds the references to a tenth of the bar.
SERIAL_STEP_ATOL = 1e-9
SERIAL_STEP_SELF_LONG = 4.2e-15
SERIAL_STEP_ATOL_LONG = max(1e-9, 10 * SERIAL_STEP_SELF_LONG)


def serial_edge_sets(N):
    return dict(SERIAL_EDGES)[N]


def serial_edge_seed(N, name):
    return SERIAL_EDGE_SEEDS.get((N, name), 12)


def seg_edge_sets(N, P):
    """The flag sets run at an edge: the default rows and the set with no stage sdf row everywhere, a set with a
    hard stage row at P = 4's largest horizon and at one P = 3 case."""
    return ["default", "rec_feas_no_sdf_row"] + (["hard_df_rec_feas"] if (N, P) in ((63, 4), (30, 3)) else [])


def config(name, **more):
    from sdf_nmpc_amd.config import Config
    over, _, _ = FLAG_SETS[name]
    return Config(**{**over, **more})


def quad(name, cfg=None, seed=0, coeffs=None):
    """coeffs: the braking polynomial of a rec_feas set (default: braking(cfg), the four-term physical law)."""
    from sdf_nmpc_amd import synth
    from sdf_nmpc_amd.model import Quad
    cfg = cfg or config(name)
    if not cfg.flags.recursive_feasibility:
        coeffs = None
    elif coeffs is None:
        coeffs = braking(cfg)
    return Quad(cfg, braking_coeffs=coeffs)


def uses_scene(q):
    """Sets with a hard row (stage rows with slack None, the rec_feas braking / Co_p_E rows, stability's
    velocity box) are run on the fitted obstacle-scene network (tests/golden/scene.sdfw, scene_setup.py) at
    the reference's own bounds: on the SIREN initialisation (df ~ 0 everywhere, every point inside an
    obstacle) a hard sdf or braking row demands moves no input sequence gives, and the QP is infeasible
    or degenerate -- for the reference's HPIPM as much as here."""
    return q.nhN > q.nsN or q.nhs > 0


def braking(cfg):
    """The braking polynomial of a physical braking law: d(v) = 0.05 + |v|^2 / (2 a_b_min) in the basis of
    polynomial_3variate (utils/math.py:307-314), a_b_min = mpc.stability.a_b_min (default.yaml:73-74)."""
    from sdf_nmpc_amd import synth
    return synth.braking_coeffs(int(cfg.mpc.braking_dist.degree), noise=0.0, a_brake=float(cfg.mpc.stability.a_b_min))


def dense_braking(deg):
    """The reference-pinned dense coefficients of polynomial_3variate at degree deg (flags_golden.npz
    poly/deg*/coeffs, every monomial ~ N(0, 1): test_flags.test_poly_term_order_and_values_match_reference)."""
    import os
    with np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "flags_golden.npz")) as f:
        return f[f"poly/deg{deg}/coeffs"].copy()


# The coefficient seed of noisy_braking per (flag set, degree, N) where seed 1 does not converge everywhere in
# the C IPM (test_flags.test_noisy_braking_is_seen_and_converges); none so far.
NOISY_SEEDS = {}
NOISY_SETS = ["rec_feas", "rec_feas_soft_brake", "stability", "hard_df_rec_feas"]
# the QP runs of test_gpu_lin_general.test_qp_with_noisy_braking as (set, degree, B, N, kernel); problem seed 11
NOISY_QP_RUNS = [("rec_feas_soft_brake", 4, 8, 20, "serial"), ("rec_feas_soft_brake", 6, 8, 20, "serial"),
                 ("stability", 4, 8, 20, "serial"), ("stability", 6, 8, 20, "serial"),
                 ("hard_df_rec_feas", 6, 8, 20, "serial"), ("stability", 6, 8, 40, "segmented")]


def noisy_braking(cfg, deg, seed=1):
    """The physical braking law of braking(cfg) at degree deg with N(0, 2e-3) on every monomial
    (synth.braking_coeffs' noise argument): mixed terms and every degree's coefficients are live."""
    from sdf_nmpc_amd import synth
    return synth.braking_coeffs(int(deg), seed=seed, noise=2e-3, a_brake=float(cfg.mpc.stability.a_b_min))


def degree_of(coeffs):
    """The degree whose polynomial_3variate has len(coeffs) monomials ((d + 1)(d + 2)(d + 3) / 6: 1, 4, .., 84)."""
    return {(d + 1) * (d + 2) * (d + 3) // 6: d for d in range(7)}[len(coeffs)]


def config_for(name, coeffs=None, **more):
    """config(name) with mpc.braking_dist.degree set to the degree of the given coefficients."""
    if coeffs is not None:
        more = dict(more, mpc__braking_dist__degree=degree_of(coeffs))
    return config(name, **more)


def problem(cfg, q, B, N, seed):
    """The synthetic problem of a set (synth.make_problem), its velocity along the camera's view (the braking
    point and the trajectory inside the field of view), and with uses_scene the scene latent in p."""
    from sdf_nmpc_amd import synth
    prob = synth.make_problem(cfg, B, N, seed=seed, sdf_cost=q.sdf_cost, nyN=q.nyN, v_forward=True)
    if uses_scene(q):
        import scene_setup as S
        prob["p"][..., 17:17 + 128] = S.scene_latent()
        # the image taken 1 m behind the start (camera moved back along the body's x axis): the start lies
        # inside the field of view, not at the camera's origin where the fov functions (atan2 of a few
        # centimetres) swing through the whole range -- a hard fov row would be infeasible at node 1
        fwd = synth.quat2rot(prob["x"][:, 0, 3:7])[:, :, 0]
        prob["p"][..., 1:4] -= fwd[:, None, :]
    return prob
