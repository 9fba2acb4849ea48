"""The flag space of default.yaml:16-23 on the CPU (gen_model.py:26-149): the constraint set the host builds
for every flag combination, the reference-pinned pieces of recursive_feasibility / stability, and the two
CPU QP checkers (oracle/qp_ipm.c, the structured Riccati IPM with the kernel's row semantics; oracle/
qp_oracle.py, the dense KKT IPM + active-set polish) against each other on every flag set.

Pins (tests/golden/flags_golden.npz, made by tests/golden/make_golden.py flags from the reference itself):
  * polynomial_3variate's term order and values (utils/math.py:294-321), degrees 0..6;
  * stability.get_r_tilde_max (utils/stability.py:44-75) under a seeded np.random;
  * Nmpc.set_ref at the terminal node with the stability row (nyN = 5: WN = W[:5], controller.py:141-142).
The row sets themselves (tests/flag_sets.py) restate gen_model.py:41-70,98-126 and cost_const_helpers.py:
70-102; acados is absent, so the QP they make is pinned to its exact solution, not to HPIPM.
"""
import os

import numpy as np
import pytest

import flag_sets as F
from sdf_nmpc_amd import synth, weights as W
from sdf_nmpc_amd.model import Quad, UnsupportedConfig, poly_eval, poly_terms, r_tilde_max

HERE = os.path.dirname(os.path.abspath(__file__))
QP_TOL = 1e-8
SOL_ATOL = 2e-6  # C IPM at QP_TOL vs the exact solution on well-posed instances (measured <= 4e-7)


@pytest.fixture(scope="module")
def fg():
    return np.load(os.path.join(HERE, "golden", "flags_golden.npz"))


@pytest.mark.parametrize("deg", range(7))
def test_poly_term_order_and_values_match_reference(fg, deg):
    np.testing.assert_array_equal(np.array(poly_terms(deg)), fg[f"poly/deg{deg}/exps"])
    val, grad = poly_eval(fg[f"poly/deg{deg}/coeffs"], deg, fg[f"poly/deg{deg}/v"])
    np.testing.assert_allclose(val, fg[f"poly/deg{deg}/val"], rtol=1e-12, atol=1e-12)
    # the gradient (the Jacobian the kernel forms with dual numbers) against central differences
    v = fg[f"poly/deg{deg}/v"]
    for i in range(3):
        d = np.zeros(3); d[i] = 1e-6
        fd = (poly_eval(fg[f"poly/deg{deg}/coeffs"], deg, v + d)[0] - poly_eval(fg[f"poly/deg{deg}/coeffs"], deg, v - d)[0]) / 2e-6
        np.testing.assert_allclose(grad[:, i], fd, rtol=1e-6, atol=1e-6)


@pytest.mark.parametrize("N,T", [(20, 1.5), (40, 1.5), (30, 2.0)])
def test_r_tilde_matches_reference(fg, N, T):
    """get_r_tilde_max restated in closed form (the sympy solve is linear in r~) with the reference's SLSQP
    start drawn from np.random: the same seed gives the same maximum (SLSQP stops at ~1e-8 relative)."""
    from sdf_nmpc_amd.config import Config
    cfg = Config(mpc__N=N, mpc__T=T)
    for seed in (0, 1, 2):
        np.random.seed(seed)
        got = r_tilde_max(cfg)
        want = float(fg[f"rtilde/N{N}_T{T}/seed{seed}"])
        assert abs(got - want) <= 1e-6 * abs(want), (seed, got, want)


@pytest.mark.parametrize("name", list(F.FLAG_SETS))
def test_constraint_set_of_each_flag_set(name):
    cfg = F.config(name)
    q = F.quad(name, cfg)
    _, cols, rows = F.FLAG_SETS[name]
    assert q.h_cols == cols and q.nh == len(cols)
    assert [r[:3] for r in q.term_rows] == rows and q.nhN == len(rows)
    assert q.nsN == sum(1 for r in rows if r[2]) and all(r[2] for r in q.term_rows[:q.nsN])
    # hard stage rows: the columns whose slack weight is None (fov: 0, 1; sdf: 2), after the soft ones
    hard = {0: cfg.mpc.weights.slack_fov is None, 1: cfg.mpc.weights.slack_fov is None, 2: cfg.mpc.weights.slack_df is None}
    assert q.nhs == sum(hard[c] for c in cols) and all(hard[c] for c in cols[q.nh - q.nhs:])
    assert all((q.zl[j], q.Zl[j]) == (0.0, 0.0) for j in range(q.nh - q.nhs, q.nh))
    # bounds: fov rows +-fov_ratio fov, the sdf row [size.xy + bound_margin, max_df + 0.2] (gen_model.py:35),
    # the braking row [size.xy, max_df] (gen_model.py:118), the velocity bounds +-limits (add_vel_const)
    lims = {0: cfg.sensor.hfov * cfg.mpc.fov_ratio, 1: cfg.sensor.vfov * cfg.mpc.fov_ratio}
    for j, c in enumerate(cols):
        lo, hi = (-lims[c], lims[c]) if c < 2 else (cfg.robot.size.xy + cfg.mpc.bound_margin, q.max_df + 0.2)
        assert (q.lh[j], q.uh[j]) == pytest.approx((lo, hi))
    for (c1, c2, soft, lo, hi, zl, Zl) in q.term_rows:
        if c2 == 0:
            assert (lo, hi) == pytest.approx((cfg.robot.size.xy, q.max_df))
        elif c2 in (1, 2):
            assert (lo, hi) == pytest.approx((-lims[c2 - 1], lims[c2 - 1]))
        elif c2 >= 3:
            v = [cfg.robot.limits.vx, cfg.robot.limits.vy, cfg.robot.limits.vz][c2 - 3]
            assert (lo, hi) == (-v, v)
    assert q.nyN == (5 if cfg.flags.get("stability") and cfg.flags.get("recursive_feasibility") else 4)
    assert q.need_sdf == (2 in cols or q.sdf_cost or q.rec_feas)
    assert q.name.endswith("_sdf") == bool(cfg.flags.enable_sdf)


def test_unbuilt_models_are_refused():
    with pytest.raises(UnsupportedConfig):
        Quad(F.config("default", mpc__model="acc"))
    with pytest.raises(UnsupportedConfig):  # rec_feas without coefficients (no file in the cache dir)
        os.environ["SDFNMPC_CACHE"] = os.path.join(HERE, "_nonexistent_cache")
        try:
            Quad(F.config("rec_feas"))
        finally:
            os.environ.pop("SDFNMPC_CACHE")


def test_stability_terminal_reference_matches_reference(fg):
    """Nmpc.set_ref(ref, N) with the stability row: WN = W[:5], yN = y[:5] (controller.py:141-142) -- the 5th
    weight is the x velocity weight, not the reference's unused p_term (extra_WN, gen_model.py:149)."""
    from sdf_nmpc_amd.controller import Nmpc
    from sdf_nmpc_amd.reference import Ref

    cfg = F.config("stability", mpc__N=20)
    q = F.quad("stability", cfg)

    class StubOcp:
        model = q

    n = Nmpc(cfg, ocp=StubOcp())
    a = fg["setref5/ref"]
    r = Ref(cfg)
    r.p, r.q, r.v, r.wz = a[0:3], a[3:7], a[7:10], a[10]
    r.Wp, r.Wq, r.Wv, r.Ww, r.Wa = a[11:14], a[14:17], a[17:20], a[20:23], a[23]
    n.set_ref(r, cfg.mpc.N)
    np.testing.assert_array_equal(n.yN, fg["setref5/yN"])
    np.testing.assert_array_equal(n.WN, fg["setref5/WN"])
    assert q.extra_WN.shape == (1,) and q.extra_WN[0] > 0


def test_terminal_extras_oracle(oracle_lib):
    """orc_quad_term (the checker of the kernel's terminal extras): values against a numpy restatement of
    gen_model.py:81-121 built on the reference-pinned poly_eval, Jacobians against central differences."""
    cfg = F.config("stability")
    q = F.quad("stability", cfg)
    m = oracle_lib.quad_model(cfg)
    rng = np.random.default_rng(2)
    R_off = np.asarray(cfg.sensor.B_R_C).T @ np.asarray(cfg.sensor.B_p_C) + np.array([cfg.mpc.fov_const_offset, 0, 0])
    for _ in range(8):
        x = np.concatenate([rng.uniform(-2, 2, 3), synth.euler2quat(rng.uniform(-0.5, 0.5, 3)), rng.uniform(-3, 3, 3)])
        p = np.zeros(145)
        p[0] = rng.choice([0.0, 1.0, 0.3])
        R = synth.quat2rot(synth.euler2quat(rng.uniform(-1, 1, 3)))
        p[1:4], p[4:13] = rng.uniform(-1, 1, 3), R.ravel()
        hE, JhE, yN5, JyN5 = oracle_lib.term_extras(m, x, p, q)
        v = x[7:]
        pv, _ = poly_eval(q.poly, q.poly_deg, v)
        E = R.T @ (x[:3] + pv * v / np.sqrt(v @ v + 1e-4) - p[1:4]) + R_off
        want = [-p[0] * pv, p[0] * np.arctan2(E[1], E[0]), p[0] * np.arctan2(E[2], np.hypot(E[0], E[1])), *v]
        np.testing.assert_allclose(hE, want, rtol=1e-12, atol=1e-12)
        _, _, yN4, _ = oracle_lib.cost(m, x, np.zeros(4), p)
        np.testing.assert_allclose(yN5, p[0] * np.concatenate([yN4, [v @ v]]), rtol=1e-13, atol=1e-13)
        for j in range(10):
            d = np.zeros(10); d[j] = 1e-6
            hp, _, yp, _ = oracle_lib.term_extras(m, x + d, p, q)
            hm, _, ym, _ = oracle_lib.term_extras(m, x - d, p, q)
            np.testing.assert_allclose(JhE[:, j], (hp - hm) / 2e-6, rtol=1e-5, atol=1e-6)
            np.testing.assert_allclose(JyN5[:, j], (yp - ym) / 2e-6, rtol=1e-5, atol=1e-6)


def _net(oracle_lib, q):
    if F.uses_scene(q):
        import scene_setup as S
        with open(S.SCENE, "rb") as f:
            return oracle_lib.Net(*W.unpack(f.read()))
    return oracle_lib.Net(W.DEFAULT_SPEC, W.siren_weights(W.DEFAULT_SPEC, 0))


def _problem(oracle_lib, name, B, N, seed, noise=0.05, coeffs=None):
    cfg = F.config_for(name, coeffs, mpc__N=N)
    q = F.quad(name, cfg, coeffs=coeffs)
    # the flight along the camera's view (hard fov rows: random v0 can leave the cone before any input acts,
    # which makes a hard row infeasible -- for the reference's HPIPM too); sets with hard rows on the scene net
    prob = F.problem(cfg, q, B, N, seed)
    x0 = prob["x"][:, 0] + np.random.default_rng(seed).normal(0, noise, (B, 10))
    net = _net(oracle_lib, q)
    lin = oracle_lib.linearize_batch(oracle_lib.quad_model(cfg), net, prob["x"], prob["u"], prob["p"], prob["dt"], model=q)
    return cfg, q, prob, x0, lin


@pytest.mark.parametrize("name", list(F.FLAG_SETS))
def test_riccati_ipm_matches_exact_solution_per_flag_set(oracle_lib, name):
    """The C restatement of the kernel's IPM (soft stage rows of the set, soft + hard terminal rows) against the
    exact QP solution: status 0; the objective within the duality gap m tol of F*; (dx, du) inside the
    strong-convexity ball sqrt(2 (F - F*) / mu); 2e-6 absolute where the instance is well posed (a hard
    terminal row far outside its bounds at the linearisation point -- the synthetic camera pose puts the
    braking point anywhere -- flattens the objective, as for the reference's HPIPM)."""
    import qp_oracle
    cfg, q, prob, x0, lin = _problem(oracle_lib, name, 3, 20, seed=3)
    r = oracle_lib.qp_ipm_batch(lin, prob, x0, q, tol=QP_TOL)
    assert (r["status"] == 0).all(), r["iters"]
    close = hard_active = 0
    for b in range(3):
        qq = qp_oracle.stage_qp({k: v[b] for k, v in lin.items() if k != "sdf"}, prob["x"][b], prob["u"][b], x0[b],
                                prob["yref"][b], prob["W"][b], prob["yN"][b], prob["WN"][b], prob["dt"], q, 10.0)
        H, g, E, e, G, d = qp_oracle.dense_problem(qq)
        ex = qp_oracle.polish_active_set(qq, qp_oracle.solve_dense(qq))
        assert ex["max_violation"] < 1e-9 and ex["min_dual"] > -1e-9
        sol = dict(dx=r["dx"][b], du=r["du"][b], sl=r["slack"][b][..., 0], su=r["slack"][b][..., 1])
        z, zs = qp_oracle.z_of(qq, sol), qp_oracle.z_of(qq, ex)
        Fz, Fs = 0.5 * z @ H @ z + g @ z, 0.5 * zs @ H @ zs + g @ zs
        assert (G @ z + d).min() > -1e-7 and np.abs(E @ z - e).max() < 1e-8  # feasible
        m = G.shape[0]
        assert Fz - Fs <= qp_oracle.objective_bound(m, QP_TOL, ex["lam_l1"], r["res"][b, 1]), (b, Fz - Fs)
        n_xu = 10 * (cfg.mpc.N + 1) + 4 * cfg.mpc.N
        mu = np.linalg.eigvalsh(H[:n_xu, :n_xu]).min()
        ball = np.sqrt(2 * max(Fz - Fs, 0.0) / mu) + 1e-6  # + the exact solution's own rounding level
        assert np.linalg.norm(z[:n_xu] - zs[:n_xu]) <= ball
        close += np.abs(sol["du"] - ex["du"]).max() <= SOL_ATOL
        if q.nhs:  # hard stage rows: some bind at the exact solution, none is violated by the C IPM's point
            nb = 8 * cfg.mpc.N + 4 * (cfg.mpc.N * (q.nh - q.nhs) + q.nsN)
            hard_active += int(((G @ zs + d)[nb:] < 1e-7).sum())
    assert close >= (1 if q.nhN > q.nsN else 2)
    if q.nhs:
        assert hard_active > 0


@pytest.mark.parametrize("name", ["no_vfov", "lidar_sdf_only", "rec_feas", "rec_feas_soft_brake", "hard_fov", "hard_df_rec_feas"])
def test_segments_match_serial_riccati(oracle_lib, name):
    """The C restatement's partitioned Riccati (P = 4) on the terminal rows of a flag set: the same iterates
    as the serial recursion (the terminal node is in the last, serial segment)."""
    cfg, q, prob, x0, lin = _problem(oracle_lib, name, 2, 40, seed=5)
    a = oracle_lib.qp_ipm_batch(lin, prob, x0, q, tol=QP_TOL)
    b = oracle_lib.qp_ipm_batch(lin, prob, x0, q, tol=QP_TOL, start=dict(seg=4))
    assert np.abs(a["iters"] - b["iters"]).max() <= 1
    np.testing.assert_allclose(a["du"], b["du"], rtol=0, atol=1e-6)  # rounding-level differences, amplified near tol


@pytest.mark.parametrize("B,N,kernel,seed", F.PHASE_SPLIT_RUNS)
def test_phase_split_problems_converge_in_the_c_ipm(oracle_lib, B, N, kernel, seed):
    """The problems of test_gpu_flags.test_phase_split_bitwise_per_flag_set, which asks for status 0 on every
    instance, are feasible: the C IPM (the recursion of the kernel the run uses) converges on all of them."""
    for name in F.PHASE_SPLIT_SETS:
        cfg, q, prob, x0, lin = _problem(oracle_lib, name, B, N, seed=seed)
        seg = kernel == "segmented" or N >= 36
        r = oracle_lib.qp_ipm_batch(lin, prob, x0, q, tol=QP_TOL, start=dict(seg=4) if seg else None)
        assert (r["status"] == 0).all(), (name, r["status"])


def test_serial_edge_table_and_lds_formula():
    """flag_sets' restatement of the serial kernel's LDS formula: the row counts it reads from FLAG_SETS are the
    model's, and the long-horizon edges are the largest horizons that fit 160 KiB (the next one does not)."""
    for name in F.FLAG_SETS:
        q = F.quad(name)
        assert F.qp_rows(name) == (q.nh, q.nhN, q.nsN, q.nhs), name
    for name in ("default", "stability"):
        n = F.serial_max_horizon(name)
        assert F.qp_lds_doubles(n, F.qp_rows(name)) * 8 <= F.LDS_PER_CU < F.qp_lds_doubles(n + 1, F.qp_rows(name)) * 8
    for name in ("no_sdf", "hard_all", "rec_feas_no_sdf_row"):  # the ABI's limit, not the LDS, bounds these
        assert F.serial_max_horizon(name) == F.QP_N_MAX
    Ns = [N for N, _ in F.SERIAL_EDGES]
    assert Ns[:8] == [1, 2, 3, 4, 5, 8, 35, 64] and Ns[8] < Ns[9] == F.serial_max_horizon("default") < F.QP_N_MAX
    assert all(N < 36 or N >= 64 for N in Ns)  # horizons AUTO gives the serial kernel at every batch size
    assert sum(len(s) for _, s in F.SERIAL_EDGES) == 25


@pytest.mark.parametrize("N,name", [(N, name) for N, sets in F.SERIAL_EDGES for name in sets])
def test_serial_edges_references(oracle_lib, N, name):
    """The references of test_gpu_flags.test_serial_qp_horizon_edges meet its bars among themselves, on that test's
    problems (B = 16, flag_sets.serial_edge_seed).  The C IPM's serial recursion converges on every instance.  Up
    to N = 8 every instance has an exact solution (the dense KKT solve + active-set polish), the C IPM's point is
    inside the objective bound and the strong-convexity ball around it, and within SOL_ATOL of its du on >= 90 %
    of the instances (test_gpu_qp._agree's share; a degenerate instance moves along its flat direction).  From
    N = 35 on there is no dense solve: the serial recursion against the recursion over four segments (which the C
    code, unlike rti_qp_seg.hip, runs at any horizon), to test_segment_edges_serial_vs_segmented_c_ipm's bars.
    At the long horizons the same pair after one and two iterations is the yardstick of the GPU test's
    per-iteration bar (flag_sets.SERIAL_STEP_ATOL_LONG, at least 10 x the measured flag_sets.SERIAL_STEP_SELF_LONG):
    the references meet a tenth of that bar."""
    import qp_oracle
    B = 16
    cfg, q, prob, x0, lin = _problem(oracle_lib, name, B, N, seed=F.serial_edge_seed(N, name))
    r = oracle_lib.qp_ipm_batch(lin, prob, x0, q, tol=QP_TOL)
    assert (r["status"] == 0).all(), (r["status"], r["iters"])
    if N <= 8:
        close = 0
        for b in range(B):
            qq = qp_oracle.stage_qp({k: v[b] for k, v in lin.items() if k != "sdf"}, prob["x"][b], prob["u"][b], x0[b],
                                    prob["yref"][b], prob["W"][b], prob["yN"][b], prob["WN"][b], prob["dt"], q, 10.0)
            H, g, E, e, G, d = qp_oracle.dense_problem(qq)
            ex = qp_oracle.polish_active_set(qq, qp_oracle.solve_dense(qq))
            assert ex["max_violation"] < 1e-9 and ex["min_dual"] > -1e-9, (b, ex["max_violation"], ex["min_dual"])
            sol = dict(dx=r["dx"][b], du=r["du"][b], sl=r["slack"][b][..., 0], su=r["slack"][b][..., 1])
            z, zs = qp_oracle.z_of(qq, sol), qp_oracle.z_of(qq, ex)
            Fz, Fs = 0.5 * z @ H @ z + g @ z, 0.5 * zs @ H @ zs + g @ zs
            assert Fz - Fs <= qp_oracle.objective_bound(G.shape[0], QP_TOL, ex["lam_l1"], r["res"][b, 1]), (b, Fz - Fs)
            n_xu = 10 * (N + 1) + 4 * N
            mu = np.linalg.eigvalsh(H[:n_xu, :n_xu]).min()
            assert np.linalg.norm(z[:n_xu] - zs[:n_xu]) <= np.sqrt(2 * max(Fz - Fs, 0.0) / mu) + 1e-6
            close += np.abs(sol["du"] - ex["du"]).max() <= SOL_ATOL
        print(f"\nserial edge N={N} {name}: {close} of {B} within {SOL_ATOL:g} of the exact du, iters {r['iters'].tolist()}")
        assert close >= 0.9 * B
        return
    s = oracle_lib.qp_ipm_batch(lin, prob, x0, q, tol=QP_TOL, start=dict(seg=4))
    assert (s["status"] == 0).all(), s["status"]
    assert np.abs(r["iters"] - s["iters"]).max() <= 1, (r["iters"], s["iters"])
    gap = np.abs(r["du"] - s["du"]).max(axis=(1, 2))
    print(f"\nserial edge N={N} {name}: serial vs 4 segments, worst |du - du| {gap.max():.2e}, iters {r['iters'].tolist()}")
    assert (gap <= 5e-6).mean() >= 0.9, gap
    if N >= F.SERIAL_LONG_N:
        for it in (1, 2):
            a = oracle_lib.qp_ipm_batch(lin, prob, x0, q, tol=QP_TOL, max_iter=it)
            b = oracle_lib.qp_ipm_batch(lin, prob, x0, q, tol=QP_TOL, max_iter=it, start=dict(seg=4))
            self_err = np.abs(a["du"] - b["du"]).max()
            print(f"  max_iter={it}: serial vs 4 segments |du - du| = {self_err:.3e}, |du| max {np.abs(a['du']).max():.3e}")
            assert (a["iters"] == it).all() and (a["status"] == 1).all()
            assert 10 * self_err <= F.SERIAL_STEP_ATOL_LONG


@pytest.mark.parametrize("N,P", [(N, P) for N, _, P in F.SEG_EDGES])
def test_segment_edges_serial_vs_segmented_c_ipm(oracle_lib, N, P):
    """The references of test_gpu_flags.test_segmented_qp_horizon_and_segment_edges meet its bars among
    themselves: at every (N, P) edge, on that test's problems (B = 16, seed 12), the C IPM's serial recursion
    and its recursion over P segments both converge everywhere, stop within one iteration of each other, and
    agree in du to 5e-6 on >= 90 % of the instances (a degenerate instance -- one of 16 at (37, 4) default
    and at (63, 4) hard_df_rec_feas, 7e-6 and 1.5e-5 -- moves along its flat direction)."""
    for name in F.seg_edge_sets(N, P):
        cfg, q, prob, x0, lin = _problem(oracle_lib, name, 16, N, seed=12)
        a = oracle_lib.qp_ipm_batch(lin, prob, x0, q, tol=QP_TOL)
        b = oracle_lib.qp_ipm_batch(lin, prob, x0, q, tol=QP_TOL, start=dict(seg=P))
        assert (a["status"] == 0).all() and (b["status"] == 0).all(), (name, a["status"], b["status"])
        assert np.abs(a["iters"] - b["iters"]).max() <= 1, (name, a["iters"], b["iters"])
        gap = np.abs(a["du"] - b["du"]).max(axis=(1, 2))
        assert (gap <= 5e-6).mean() >= 0.9, (name, gap)


# ---- the references of tests/test_gpu_lin_general.py, held on the CPU before the GPU sees them
LIN_GEN_RTOL, LIN_GEN_ATOL = 1e-9, 1e-11   # the GPU bars there (test_gpu_flags.test_linearisation_per_flag_set's)
FLAG_VALUES = (0.0, 1.0, 0.3)


@pytest.mark.parametrize("deg", range(7))
def test_terminal_extras_oracle_dense_polynomial(oracle_lib, fg, deg):
    """orc_quad_term with every monomial of polynomial_3variate live, degrees 0..6 (the reference-pinned dense
    coefficients and velocities of flags_golden.npz, |v| up to 4 m/s, poly up to 8.9e3) and flags {0, 1, 0.3}:
    values against the numpy restatement on the reference-pinned poly_eval, and the polynomial's gradient columns
    of JhE[0] against poly_eval's analytic gradient, to a tenth of the GPU test's bars (relative 1e-10, absolute
    1e-12 max(1, |poly|)); JhE against central differences at test_terminal_extras_oracle's bars.  Measured worst
    value error 3e-15 max(1, |poly|) (printed)."""
    coeffs = F.dense_braking(deg)
    cfg = F.config_for("stability", coeffs)
    q = F.quad("stability", cfg, coeffs=coeffs)
    assert q.poly_deg == deg and len(q.poly) == len(poly_terms(deg)) and np.array_equal(q.poly, fg[f"poly/deg{deg}/coeffs"])
    m = oracle_lib.quad_model(cfg)
    rng = np.random.default_rng(20 + deg)
    R_off = np.asarray(cfg.sensor.B_R_C).T @ np.asarray(cfg.sensor.B_p_C) + np.array([cfg.mpc.fov_const_offset, 0, 0])
    worst = worst_g = 0.0
    for i, v in enumerate(fg[f"poly/deg{deg}/v"]):
        x = np.concatenate([rng.uniform(-2, 2, 3), synth.euler2quat(rng.uniform(-0.5, 0.5, 3)), v])
        p = np.zeros(145)
        p[0] = flag = FLAG_VALUES[i % 3]
        R = synth.quat2rot(synth.euler2quat(rng.uniform(-1, 1, 3)))
        p[1:4], p[4:13] = rng.uniform(-1, 1, 3), R.ravel()
        hE, JhE, yN5, JyN5 = oracle_lib.term_extras(m, x, p, q)
        pv, gv = poly_eval(q.poly, deg, v)
        np.testing.assert_allclose(pv, fg[f"poly/deg{deg}/val"][i], rtol=1e-12, atol=1e-12)
        sc = max(1.0, abs(pv))
        E = R.T @ (x[:3] + pv * v / np.sqrt(v @ v + 1e-4) - p[1:4]) + R_off
        want = np.array([-flag * pv, flag * np.arctan2(E[1], E[0]), flag * np.arctan2(E[2], np.hypot(E[0], E[1])), *v])
        worst = max(worst, np.abs(hE - want).max() / sc)
        np.testing.assert_allclose(hE, want, rtol=LIN_GEN_RTOL / 10, atol=LIN_GEN_ATOL / 10 * sc)
        gs = max(1.0, np.abs(gv).max())
        worst_g = max(worst_g, np.abs(JhE[0, 7:] + flag * gv).max() / gs)
        np.testing.assert_allclose(JhE[0, 7:], -flag * gv, rtol=LIN_GEN_RTOL / 10, atol=LIN_GEN_ATOL / 10 * gs)
        assert (JhE[0, :7] == 0).all() and np.array_equal(JhE[3:], np.eye(10)[7:])
        if flag == 0:
            assert (hE[:3] == 0).all() and (JhE[:3] == 0).all() and (yN5 == 0).all() and (JyN5 == 0).all()
            assert np.array_equal(hE[3:], v)
        for j in range(10):
            d = np.zeros(10); d[j] = 1e-6
            hp, _, yp, _ = oracle_lib.term_extras(m, x + d, p, q)
            hm, _, ym, _ = oracle_lib.term_extras(m, x - d, p, q)
            np.testing.assert_allclose(JhE[:, j], (hp - hm) / 2e-6, rtol=1e-5, atol=1e-6)
            np.testing.assert_allclose(JyN5[:, j], (yp - ym) / 2e-6, rtol=1e-5, atol=1e-6)
    print(f"\ndense polynomial deg {deg}: worst |hE - numpy| / max(1, |poly|) = {worst:.2e}, "
          f"worst |dpoly/dv - poly_eval's| / max(1, |grad|) = {worst_g:.2e}")


def test_noisy_braking_is_seen_and_converges(oracle_lib):
    """The problems of test_gpu_lin_general's QP, phase-split and controller runs (flag_sets.noisy_braking: the
    physical law plus N(0, 2e-3) on every monomial; B = 8, N = 20, seed 11) at degrees 2, 4 and 6 on the four
    rec_feas sets: the C IPM on the checker's linearisation converges on every instance (the GPU tests ask for
    status 0), and at degree 4 the noise is visible in the solution -- du differs from the noise-free
    polynomial's by more than 1e-3, two hundred times the GPU bar (measured 0.02; 0.18 for stability).  The
    segmented run's problem (flag_sets.NOISY_QP_RUNS, N = 40) converges in the four-segment recursion."""
    B, N, seed = 8, 20, 11
    for name in F.NOISY_SETS:
        base = oracle_lib.qp_ipm_batch(*_lin_prob(oracle_lib, name, B, N, seed, None), tol=QP_TOL)
        assert (base["status"] == 0).all(), (name, base["status"])
        for deg in (2, 4, 6):
            cfg = F.config(name)
            coeffs = F.noisy_braking(cfg, deg, F.NOISY_SEEDS.get((name, deg, N), 1))
            r = oracle_lib.qp_ipm_batch(*_lin_prob(oracle_lib, name, B, N, seed, coeffs), tol=QP_TOL)
            assert (r["status"] == 0).all(), (name, deg, r["status"], r["iters"])
            if deg == 4:
                gap = np.abs(r["du"] - base["du"]).max()
                print(f"\nnoisy braking {name} deg 4: |du - du_noise_free| = {gap:.3e}, iters {r['iters'].tolist()}")
                assert gap > 1e-3, (name, gap)
    for name, deg, B, N, kernel in F.NOISY_QP_RUNS:
        if kernel != "segmented":
            assert (name, deg, B, N) in [(n, d, 8, 20) for n in F.NOISY_SETS for d in (2, 4, 6)]  # shown above
            continue
        coeffs = F.noisy_braking(F.config(name), deg, F.NOISY_SEEDS.get((name, deg, N), 1))
        r = oracle_lib.qp_ipm_batch(*_lin_prob(oracle_lib, name, B, N, seed, coeffs), tol=QP_TOL, start=dict(seg=4))
        assert (r["status"] == 0).all(), (name, deg, N, r["status"], r["iters"])


def _lin_prob(oracle_lib, name, B, N, seed, coeffs):
    """qp_ipm_batch's leading arguments for a flag set's problem with the given braking coefficients."""
    cfg, q, prob, x0, lin = _problem(oracle_lib, name, B, N, seed, coeffs=coeffs)
    return lin, prob, x0, q


ATT_WIDE_SHAPES = [(1, 20, True), (7, 40, False), (3, 60, True)]  # (B, N, uniform grid)


def att_wide_problem(cfg, B, N, seed, dt=None):
    """synth.make_problem's problem for the 'att' model away from the hover-ish iterate: at every node roll and
    pitch within +-1.2 rad and any yaw, the quaternion scaled by U(0.5, 2) and by +-1 (f_expl normalises it;
    the sign leaves the yaw's rotation as it is); commands alternately at a corner of the input box (thrust 0 or 1,
    the others +-1) and drawn from U(box); the flag off at every third node."""
    prob = synth.make_problem(cfg, B, N, seed=seed, dt=dt)
    rng = np.random.default_rng(2000 + seed)
    eul = np.stack([rng.uniform(-1.2, 1.2, (B, N + 1)), rng.uniform(-1.2, 1.2, (B, N + 1)),
                    rng.uniform(-np.pi, np.pi, (B, N + 1))], -1)
    prob["x"][..., 3:7] = (synth.euler2quat(eul) * rng.uniform(0.5, 2.0, (B, N + 1, 1))
                           * rng.choice([-1.0, 1.0], (B, N + 1, 1)))
    lbu, ubu = Quad(cfg).lbu, Quad(cfg).ubu
    corner = np.where(rng.integers(0, 2, (B, N, 4)) == 1, ubu, lbu)
    inside = rng.uniform(lbu, ubu, (B, N, 4))
    at_corner = (np.arange(B * N).reshape(B, N) % 2 == 0)[..., None]
    prob["u"] = np.where(at_corner, corner, inside)
    prob["p"][:, ::3, 0] = 0.0
    return prob


@pytest.mark.parametrize("B,N,uniform", ATT_WIDE_SHAPES)
def test_att_wide_problem_referees(oracle_lib, cfg, B, N, uniform):
    """The checker on test_gpu_lin_general's widened 'att' inputs (att_wide_problem at that test's shapes and
    seeds): orc_quad_rk4 against synth.rk4 (independent numpy) to a tenth of lin_close's bar, its [A | B] against
    central differences at this module's FD bars (the differences' own limit, ~3e-10, is far inside them); and the
    problem holds what it promises (commands at the box, non-unit and sign-flipped quaternions, the grid)."""
    from tolerances import LIN_RTOL, lin_close
    _, dt = oracle_lib.shooting_grid(N, float(cfg.mpc.T), uniform)
    prob = att_wide_problem(cfg, B, N, seed=B * 100 + N, dt=dt)
    m, lim = oracle_lib.quad_model(cfg), cfg.robot.limits
    x, u = prob["x"], prob["u"]
    nrm = np.linalg.norm(x[..., 3:7], axis=-1)
    assert nrm.min() < 0.7 and nrm.max() > 1.5 and (x[..., 3] < 0).any() and (x[..., 3] > 0).any()
    at_box = ((u == Quad(cfg).lbu) | (u == Quad(cfg).ubu)).all(-1)
    assert at_box[:, ::2].any() and not at_box.all() and (prob["p"][:, ::3, 0] == 0).all() and (prob["p"][:, 1::3, 0] == 1).all()
    assert uniform == (np.ptp(prob["dt"]) < 1e-12)
    want = np.stack([synth.rk4(x[:, k], u[:, k], prob["dt"][k], lim) for k in range(N)], 1)
    got, worst_fd = np.empty_like(want), 0.0
    for b in range(B):
        for k in range(N):
            got[b, k], AB = oracle_lib.rk4(m, x[b, k], u[b, k], prob["dt"][k])
            if (b * N + k) % 7:  # central differences on every seventh row
                continue
            z = np.concatenate([x[b, k], u[b, k]])
            fd = np.empty((10, 14))
            for j in range(14):
                d = np.zeros(14); d[j] = 1e-6
                fd[:, j] = (synth.rk4((z + d)[:10], (z + d)[10:], prob["dt"][k], lim)
                            - synth.rk4((z - d)[:10], (z - d)[10:], prob["dt"][k], lim)) / 2e-6
            worst_fd = max(worst_fd, np.abs(AB - fd).max())
            np.testing.assert_allclose(AB, fd, rtol=1e-5, atol=1e-6)
    err = np.abs(got - want).max() / max(1.0, np.abs(want).max())
    print(f"\natt wide ({B}, {N}): |rk4_C - rk4_numpy| / max(1, |x+|) = {err:.2e}, worst |AB - FD| = {worst_fd:.2e}")
    assert lin_close(got, want, rtol=LIN_RTOL / 10)


def s03_zero_problem(cfg):
    """Rows of the 'att' model with x3 = x6 = 0 (q = [0, qx, qy, 0]: a half turn about a horizontal axis, where
    the yaw atan2(q3, q0) is atan2(0, 0) = 0): B = 6 instances of N = 2 nodes on dt = 0.075, instance 0 the point
    x = [0, 0, 1, 0, 0.6, 0.8, 0, 1, 0, 0], u = [0.5, 0.1, 0.1, 0.2], the others with (qx, qy) at any angle, unit
    (instances 0..2) and scaled by U(0.5, 2) (3..5), and synth.make_problem's commands."""
    B, N = 6, 2
    prob = synth.make_problem(cfg, B, N, seed=61, dt=np.full(N, 0.075))
    rng = np.random.default_rng(62)
    ang = rng.uniform(-np.pi, np.pi, (B, N + 1))
    scale = np.where(np.arange(B) < 3, 1.0, rng.uniform(0.5, 2.0, B))[:, None]
    prob["x"][..., 3], prob["x"][..., 6] = 0.0, 0.0
    prob["x"][..., 4], prob["x"][..., 5] = np.cos(ang) * scale, np.sin(ang) * scale
    prob["x"][0, 0] = [0, 0, 1, 0, 0.6, 0.8, 0, 1, 0, 0]
    prob["u"][0, 0] = [0.5, 0.1, 0.1, 0.2]
    return prob


def test_s03_zero_point_in_the_checker(oracle_lib, cfg):
    """At x3 = x6 = 0 the checker's x+ and y are numpy's (atan2(0, 0) = 0 on both sides), to a tenth of lin_close's
    bar; its [A | B] is not finite there (the derivative of atan2 at (0, 0) is 0 / 0), so it referees values only:
    test_gpu_lin_general.test_att_s03_zero_branch claims nothing about the kernel's q and u columns."""
    from tolerances import LIN_RTOL, lin_close
    prob = s03_zero_problem(cfg)
    m, lim = oracle_lib.quad_model(cfg), cfg.robot.limits
    B, N = prob["u"].shape[:2]
    for b in range(B):
        for k in range(N):
            x, u = prob["x"][b, k], prob["u"][b, k]
            xn, AB = oracle_lib.rk4(m, x, u, prob["dt"][k])
            assert lin_close(xn, synth.rk4(x, u, prob["dt"][k], lim), rtol=LIN_RTOL / 10)
            assert xn[3] == 0 and xn[6] == 0  # the whole step stays on the branch
            assert not np.isfinite(AB[:, 3:7]).all()
            y = oracle_lib.cost(m, x, u, prob["p"][b, k])[0]
            f = synth.f_expl(x, u, lim)
            want = np.concatenate([x[:3], [y[3]], x[7:], [u[1] * lim.roll, u[2] * lim.pitch, u[3] * lim.wz, f[9]]])  # y[10] = W_a[2]
            assert np.isfinite(y).all() and lin_close(y, want, rtol=LIN_RTOL / 10), (y, want)
