"""The flag space of default.yaml:16-23 on the GPU (gen_model.py:26-149): for every flag set of
tests/flag_sets.py the preparation phase (linearize.hip + the SDF kernels only where a row or the cost reads
the network) against the oracle, the QP kernel (the stage row count as a template parameter; soft rows, hard
stage rows (slack None), soft / hard terminal rows) against the structured C IPM and the exact QP solution,
the acados-style phase split, and the whole controller (Nmpc / Ocp over the solver object) against the
oracle pipeline.  Sets with a hard row run on the fitted scene net at the reference's own bounds
(flag_sets.uses_scene); tests/test_gpu_scene.py flies them in closed loop past the pillar."""
import numpy as np
import pytest

import flag_sets as F
from sdf_nmpc_amd import _lib, synth, weights as W

pytestmark = pytest.mark.gpu

QP_TOL = 1e-8
ORC_ATOL = 5e-6   # GPU vs the C restatement of the same IPM (same iterations; rounding differences)
LIN_RTOL = 1e-9   # fp64 linearisation

LIN = ("xn", "AB", "y", "Jy", "yN", "JyN", "h", "Jh", "hE", "JhE")
OUT = LIN + ("dx", "du", "slack", "status", "iters", "res")


def _config(name, N, coeffs=None):
    """The flag set's config at horizon N, at the reference's bounds (default.yaml); with braking coefficients,
    at their degree."""
    return F.config_for(name, coeffs, mpc__N=N)


def _setup(gpu_ctx, name, B, N, seed, noise=0.05, coeffs=None):
    """coeffs: the braking polynomial of a rec_feas set (default: flag_sets.braking, four non-zero terms)."""
    import torch
    cfg = _config(name, N, coeffs)
    q = F.quad(name, cfg, coeffs=coeffs)
    dev = torch.device("cuda", gpu_ctx.device)
    # v0 along the camera's view: the braking point of the rec_feas rows lies in the field of view; sets with
    # a hard row carry the scene latent (flag_sets.problem)
    prob = F.problem(cfg, q, B, N, seed)
    x0 = prob["x"][:, 0] + np.random.default_rng(seed).normal(0, noise, (B, 10))
    t = {k: torch.from_numpy(np.ascontiguousarray(v)).to(dev) for k, v in
         dict(x=prob["x"], u=prob["u"], p=prob["p"], dt=prob["dt"], x0=x0, yref=prob["yref"], W=prob["W"],
              yNref=prob["yN"], WN=prob["WN"]).items()}
    sh = dict(xn=(B, N, 10), AB=(B, N, 14, 10), y=(B, N, 11), Jy=(B, N, 14, 11), yN=(B, q.nyN), JyN=(B, 10, q.nyN),
              h=(B, N + 1, 3), Jh=(B, N + 1, 10, 3), hE=(B, 6), JhE=(B, 10, 6), dx=(B, N + 1, 10), du=(B, N, 4),
              slack=(B, N + 1, 3, 2), res=(B, 2))
    for k, s in sh.items():
        t[k] = torch.full(s, float("nan"), dtype=torch.float64, device=dev)
    t["status"] = torch.full((B,), -1, dtype=torch.int32, device=dev)
    t["iters"] = torch.full((B,), -1, dtype=torch.int32, device=dev)
    torch.cuda.synchronize()
    return cfg, q, prob, x0, t


def _net(gpu_ctx, q):
    if not q.enable_sdf:
        return None
    if F.uses_scene(q):
        import scene_setup as S
        return _lib.Net.from_file(gpu_ctx, S.SCENE)
    return _lib.Net.siren(gpu_ctx, 0)


def _onet(oracle_lib, q):
    if F.uses_scene(q):
        import scene_setup as S
        with open(S.SCENE, "rb") as f:
            return oracle_lib.Net(*W.unpack(f.read()))
    return oracle_lib.Net(W.DEFAULT_SPEC, W.siren_weights(W.DEFAULT_SPEC, 0))


def _np(t, keys):
    return {k: t[k].cpu().numpy() for k in keys}


@pytest.mark.parametrize("name", list(F.FLAG_SETS))
def test_linearisation_per_flag_set(gpu_ctx, oracle_lib, name):
    """sdfnmpc_linearize with the flag set's terminal extras (hE: braking row add-on, fov at Co_p_E, v_N),
    residual width (nyN 5 with the flag-scaled stability residual) and no network where nothing reads it."""
    B, N = 6, 20
    cfg, q, prob, x0, t = _setup(gpu_ctx, name, B, N, seed=11)
    _lib.linearize(gpu_ctx, _net(gpu_ctx, q), _lib.quad_model(cfg, q), B, N, q.np, t, nyN=q.nyN, no_sdf=not q.need_sdf)
    gpu_ctx.synchronize()
    got = _np(t, LIN)
    onet = _onet(oracle_lib, q)
    ref = oracle_lib.linearize_batch(oracle_lib.quad_model(cfg), onet, prob["x"], prob["u"], prob["p"], prob["dt"], model=q)
    for k in ("xn", "AB", "y", "Jy", "yN", "JyN"):
        np.testing.assert_allclose(got[k], ref[k], rtol=LIN_RTOL, atol=1e-12 * max(1.0, np.abs(ref[k]).max()), err_msg=k)
    for c in (0, 1):  # the fov functions are computed for every set (cheap), whichever are rows
        np.testing.assert_allclose(got["h"][..., c], ref["h"][..., c], rtol=LIN_RTOL, atol=1e-12)
        np.testing.assert_allclose(got["Jh"][..., c], ref["Jh"][..., c], rtol=LIN_RTOL, atol=1e-12)
    if q.need_sdf:  # fp32 network: the SURVEY §8(d) bar
        np.testing.assert_allclose(got["h"][..., 2], ref["h"][..., 2], rtol=0, atol=1e-5 * max(1.0, np.abs(ref["h"][..., 2]).max()))
        np.testing.assert_allclose(got["Jh"][..., 2], ref["Jh"][..., 2], rtol=0, atol=1e-4 * max(1.0, np.abs(ref["Jh"][..., 2]).max()))
    else:  # the SDF kernels did not run: the sdf column stays as it was (NaN here)
        assert np.isnan(got["h"][..., 2]).all()
    if q.rec_feas or q.stability:
        for k in ("hE", "JhE"):
            cols = slice(0, 6) if q.rec_feas else slice(3, 6)
            np.testing.assert_allclose(got[k][..., cols], ref[k][..., cols], rtol=LIN_RTOL, atol=1e-11, err_msg=k)


@pytest.mark.parametrize("name", list(F.FLAG_SETS))
def test_qp_per_flag_set_vs_c_ipm_and_exact(gpu_ctx, oracle_lib, name):
    """The QP kernel on the GPU linearisation of each flag set: the same iterations as the C restatement
    (oracle/qp_ipm.c) up to one; du within 5e-6 of it on >= 90 % of the instances and, on the rest (degenerate
    rows whose slack and dual both -> 0, where a stopped IPM iterate moves along the flat direction),
    the same objective to the duality-gap bound and both points feasible (test_gpu_qp._agree, the main QP
    suite's bar); dx within 5e-6 on the same instances; every instance within the exact solution's objective
    / convexity-ball bounds; and with hard stage rows, some of them binding at the solution."""
    _check_qp(gpu_ctx, oracle_lib, name, 16, 20, "serial")


@pytest.mark.parametrize("name", list(F.FLAG_SETS))
def test_segmented_qp_per_flag_set(gpu_ctx, oracle_lib, name):
    """VERDICT r5 missing 2: the segmented kernel (rti_qp_seg.hip, four wavefronts per instance, the B = 1
    latency kernel) on every flag set -- 0..3 stage rows of hfov / vfov / sdf, soft or hard (slack None; the
    hard sets on the scene net), and the terminal rows (the rec_feas braking and Co_p_E rows, stability's
    velocity box) -- at N = 40, to the same bar as the serial kernel against the C IPM and the exact
    solution."""
    # (whether a hard row binds is the problem's property: at N = 40 the hard fov rows of this seed stay
    # inactive; test_gpu_scene.py's closed loops, on this kernel at B = 64, assert that they bind.)  B = 32:
    # at N = 40 two instances of hard_df_rec_feas's first 16 are degenerate -- the serial kernel, the C IPM's
    # serial and segmented recursions and this kernel all stop 2e-6..9e-5 in du from the exact solution and
    # from each other, inside the objective bound (profiles/r06/seg_flag_probe_hard_df_rec_feas.txt,
    # tools/seg_flag_probe.py) -- 12.5 % of a 16-instance sample against the >= 90 % bar
    # (the same degeneracy moves a stop by more than one iteration on one instance in 32 (hard_df: 16 vs 14):
    # iterations within one of the C IPM on >= 90 % of the instances; every instance meets the exact-solution
    # bounds below)
    _check_qp(gpu_ctx, oracle_lib, name, 32, 40, "segmented", need_active=False, iters_frac=0.9, n_exact=4)


def test_segmented_kernel_row_sets(gpu_ctx):
    """The kernel each flag set's QP runs when the context asks for the segmented one
    (sdfnmpc_ctx_qp_kernel_for): every flag set gets it."""
    gpu_ctx.set_qp_kernel("segmented")
    try:
        for name in F.FLAG_SETS:
            assert gpu_ctx.qp_kernel(40, 1, _lib.qp_opts(F.quad(name), tol=QP_TOL)) == "segmented", name
    finally:
        gpu_ctx.set_qp_kernel("auto")


@pytest.mark.parametrize("N,nseg_env,nseg,name", [
    pytest.param(N, env, P, name, id=f"N{N}-P{P}{'env' if env else ''}-{name}")
    for N, env, P in F.SEG_EDGES for name in F.seg_edge_sets(N, P)])
def test_segmented_qp_horizon_and_segment_edges(gpu_ctx, oracle_lib, monkeypatch, N, nseg_env, nseg, name):
    """The segmented kernel's three instantiations (<2,31>, <3,47>, <4,63>) at the edges of the horizon and
    segment-count space (flag_sets.SEG_EDGES: two-node segments, AUTO's lower bound N = 36, the one-node
    remainder at N = 37, sixteen-node segments at each instantiation's largest N -- the lane-ownership and
    LDS limit -- and the smallest horizons that reach P = 3 and P = 2), against the C IPM's recursion over
    the same partition a_i = i (N + 1) / P and the exact solution, to _check_qp's bars.  B = 16, seed 12:
    test_flags.test_segment_edges_serial_vs_segmented_c_ipm holds the references to those bars on the CPU."""
    if nseg_env:
        monkeypatch.setenv("SDFNMPC_QP_NSEG", str(nseg))
    else:
        monkeypatch.delenv("SDFNMPC_QP_NSEG", raising=False)
    assert _lib.qp_seg_count(N) == nseg  # the instantiation under test; 0 would run the serial kernel
    _check_qp(gpu_ctx, oracle_lib, name, 16, N, "segmented", need_active=False, iters_frac=0.9,
              n_exact=1 if N >= 47 else 2, nseg=nseg)


def _solve_again(gpu_ctx, w, B, N, du0=None, **opts):
    """Another serial-kernel solve on the buffers of a _check_qp run (du0: the du buffer's entry values)."""
    import torch
    t = w["t"]
    for k in ("dx", "du", "slack", "res"):
        t[k].fill_(float("nan"))
    if du0 is not None:
        t["du"].copy_(torch.from_numpy(np.ascontiguousarray(du0)))
    t["status"].fill_(-1)
    t["iters"].fill_(-1)
    torch.cuda.synchronize()
    gpu_ctx.set_qp_kernel("serial")
    try:
        _lib.qp_solve(gpu_ctx, _lib.qp_opts(w["q"], tol=QP_TOL, **opts), B, N, t)
        gpu_ctx.synchronize()
    finally:
        gpu_ctx.set_qp_kernel("auto")
    return _np(t, ("dx", "du", "slack", "status", "iters", "res"))


@pytest.mark.parametrize("N,name", [pytest.param(N, name, id=f"N{N}-{name}") for N, sets in F.SERIAL_EDGES for name in sets])
def test_serial_qp_horizon_edges(gpu_ctx, oracle_lib, N, name):
    """The serial kernel (rti_qp.hip, one wavefront per instance) where its control flow depends on the horizon
    (flag_sets.SERIAL_EDGES: the single-trip branch at N + 1 <= 3 ring positions, a first and a last trip with
    two, one and no dead tail position at N = 3, 4, 5, one middle trip at N = 8, AUTO's serial horizons next to
    the segmented range, and the largest horizon whose instance fits a CU's LDS), on the GPU linearisation of
    each set -- so linearize and the pack kernel run at 2 .. 195 nodes too -- to _check_qp's bars against the C
    IPM's serial recursion.  Up to N = 8 every instance against the exact solution, at 35 and 64 the first one,
    at the long horizons none (dense=False: the point itself is checked).  B = 16;
    test_flags.test_serial_edges_references holds the references to these bars on the CPU.

    Per-iteration pin: du after max_iter = 1 and 2 from a cold start equals the C IPM's at the same max_iter to
    flag_sets.SERIAL_STEP_ATOL (1e-9; SERIAL_STEP_ATOL_LONG at the long horizons, from the reference's own
    rounding there).  After one or two Newton steps no flat direction has opened: a wrong stage, a missed node
    or a stale factor row shows at the size of the step.  Warm start at N = 1 and 3 (default): a zero du
    reproduces the cold solve bit for bit, one iteration from a random du equals the C IPM's from the same du.
    Determinism at N = 2, 4 and the largest default horizon: a second solve agrees bit for bit."""
    B = 16
    rows = F.qp_rows(name)
    long_n = N >= F.SERIAL_LONG_N
    # the LDS formula the table's horizons come from is the library's (its QP_RING * 168 term: a ring of 3)
    assert _lib.load().sdfnmpc_qp_lds_bytes(N) == F.qp_lds_doubles(N, F.qp_rows("default")) * 8
    opts = _lib.qp_opts(F.quad(name, _config(name, N)), tol=QP_TOL)
    assert gpu_ctx.qp_capacity(N, opts) > 0
    if long_n and F.serial_max_horizon(name) == N:
        assert F.qp_lds_doubles(N + 1, rows) * 8 > F.LDS_PER_CU and gpu_ctx.qp_capacity(N + 1, opts) == 0
    w = _check_qp(gpu_ctx, oracle_lib, name, B, N, "serial", need_active=False, n_exact=None if N <= 8 else 1,
                  seed=F.serial_edge_seed(N, name), dense=not long_n)
    q, prob, x0, lin, full = w["q"], w["prob"], w["x0"], w["lin"], w["got"]
    atol = F.SERIAL_STEP_ATOL_LONG if long_n else F.SERIAL_STEP_ATOL
    for it in (1, 2):
        g = _solve_again(gpu_ctx, w, B, N, max_iter=it)
        c = oracle_lib.qp_ipm_batch(lin, prob, x0, q, tol=QP_TOL, max_iter=it)
        print(f"serial edge N={N} {name} max_iter={it}: |du - du_C| = {np.nan_to_num(np.abs(g['du'] - c['du']), nan=np.inf).max():.3e}, "
              f"|du_C| max {np.abs(c['du']).max():.3e}")
        assert (c["status"] == 1).all() and (c["iters"] == it).all()
        assert (g["status"] == 1).all() and (g["iters"] == it).all(), (g["status"], g["iters"])
        assert np.isfinite(g["res"]).all()
        np.testing.assert_allclose(g["du"], c["du"], rtol=0, atol=atol)
    if name == "default" and N in (1, 3):
        g = _solve_again(gpu_ctx, w, B, N, du0=np.zeros((B, N, 4)), warm_start=True)
        for k in ("du", "dx", "iters", "status"):
            np.testing.assert_array_equal(g[k], full[k], err_msg=k)
        du_ws = np.random.default_rng(14).normal(0, 0.1, (B, N, 4))
        g = _solve_again(gpu_ctx, w, B, N, du0=du_ws, warm_start=True, max_iter=1)
        c = oracle_lib.qp_ipm_batch(lin, prob, x0, q, tol=QP_TOL, max_iter=1, du_ws=du_ws)
        assert np.abs(c["du"] - oracle_lib.qp_ipm_batch(lin, prob, x0, q, tol=QP_TOL, max_iter=1)["du"]).max() > 1e-3  # the start is live
        np.testing.assert_allclose(g["du"], c["du"], rtol=0, atol=F.SERIAL_STEP_ATOL)
    if N in (2, 4) or (name == "default" and long_n):
        g = _solve_again(gpu_ctx, w, B, N)
        for k in ("du", "dx", "slack", "iters", "status", "res"):
            np.testing.assert_array_equal(g[k], full[k], err_msg=k)


def test_serial_qp_upper_end_refusals(gpu_ctx, oracle_lib):
    """The upper end of the serial kernel's horizon range.  The default rows at the first horizon that does not
    fit a CU's LDS and at the ABI's largest, 200: qp_solve and rti_prepare refuse (SDFNMPC_E_UNSUPPORTED, -4,
    "horizon too long") with nothing enqueued -- every output buffer keeps its fill -- and qp_capacity is 0.
    no_sdf (no stage row) fits at 200: solved, status 0, du within ORC_ATOL of the C IPM.  N = 201 and N = 0 are
    argument errors (SDFNMPC_E_ARG, -1)."""
    B = 4
    for N in (F.serial_max_horizon("default") + 1, F.QP_N_MAX):
        cfg, q, prob, x0, t = _setup(gpu_ctx, "default", B, N, seed=12)
        opts = _lib.qp_opts(q, tol=QP_TOL)
        assert gpu_ctx.qp_capacity(N, opts) == 0
        with pytest.raises(_lib.SdfnmpcError, match=r"error -4: .*horizon too long"):
            _lib.rti_prepare(gpu_ctx, _net(gpu_ctx, q), _lib.quad_model(cfg, q), opts, B, N, q.np, t)
        with pytest.raises(_lib.SdfnmpcError, match=r"error -4: .*horizon too long"):
            _lib.qp_solve(gpu_ctx, opts, B, N, t)
        gpu_ctx.synchronize()
        got = _np(t, OUT)
        assert all(np.isnan(got[k]).all() for k in OUT if k not in ("status", "iters")), "a refused call wrote an output"
        assert (got["status"] == -1).all() and (got["iters"] == -1).all()
    for N in (F.QP_N_MAX + 1, 0):  # (the buffers of the last setup: the horizon is refused before anything is read)
        with pytest.raises(_lib.SdfnmpcError, match="error -1: "):
            _lib.qp_solve(gpu_ctx, opts, B, N, t)
    N = F.QP_N_MAX
    assert F.serial_max_horizon("no_sdf") == N
    cfg, q, prob, x0, t = _setup(gpu_ctx, "no_sdf", B, N, seed=12)
    opts = _lib.qp_opts(q, tol=QP_TOL)
    assert gpu_ctx.qp_capacity(N, opts) > 0 and gpu_ctx.qp_kernel(N, B, opts) == "serial"
    _lib.linearize(gpu_ctx, None, _lib.quad_model(cfg, q), B, N, q.np, t, nyN=q.nyN, no_sdf=True)
    _lib.qp_solve(gpu_ctx, opts, B, N, t)
    gpu_ctx.synchronize()
    got = _np(t, OUT)
    c = oracle_lib.qp_ipm_batch({k: got[k] for k in LIN}, prob, x0, q, tol=QP_TOL)
    assert (c["status"] == 0).all() and (got["status"] == 0).all(), (got["status"], got["iters"])
    assert np.abs(got["iters"] - c["iters"]).max() <= 1
    np.testing.assert_allclose(got["du"], c["du"], rtol=0, atol=ORC_ATOL)
    _check_point(prob, x0, {k: got[k] for k in LIN}, q, got)


def _check_qp(gpu_ctx, oracle_lib, name, B, N, kernel, need_active=True, iters_frac=1.0, n_exact=None, nseg=4, seed=12,
              dense=True, coeffs=None):
    """n_exact: the exact solution (a dense KKT solve, ~2 s per instance at N = 40) for the first n_exact
    instances and every instance whose du is off the C IPM's by more than the bar (None: all).  nseg: the
    segments of the segmented kernel at this N (the C IPM runs lqr_seg over the same partition).  dense=False
    (long horizons, where one dense solve takes a minute): no exact solution at all -- an instance off the C IPM
    is held to _agree's m tol gap bound, and every instance's point to the x0 row, the linearised dynamics and
    the input boxes directly.  Returns the problem, its device buffers and the C IPM's result (whole batch)."""
    import qp_oracle
    from test_gpu_qp import _agree
    cfg, q, prob, x0, t = _setup(gpu_ctx, name, B, N, seed=seed, coeffs=coeffs)
    _lib.linearize(gpu_ctx, _net(gpu_ctx, q), _lib.quad_model(cfg, q), B, N, q.np, t, nyN=q.nyN, no_sdf=not q.need_sdf)
    opts = _lib.qp_opts(q, tol=QP_TOL)
    gpu_ctx.set_qp_kernel(kernel)
    try:
        assert gpu_ctx.qp_kernel(N, B, opts) == kernel
        _lib.qp_solve(gpu_ctx, opts, B, N, t)
        gpu_ctx.synchronize()
    finally:
        gpu_ctx.set_qp_kernel("auto")
    got = _np(t, OUT)
    lin = {k: got[k] for k in LIN}
    # the segmented kernel against the C IPM's segmented recursion (oracle/qp_ipm.c lqr_seg: the same
    # segments and couplings), the serial one against the serial recursion
    c = oracle_lib.qp_ipm_batch(lin, prob, x0, q, tol=QP_TOL, start=dict(seg=nseg) if kernel == "segmented" else None)
    whole = dict(cfg=cfg, q=q, prob=prob, x0=x0, t=t, opts=opts, lin=lin, got=got, c=c)
    gap = np.abs(got["du"] - c["du"]).max(axis=(1, 2))[(c["status"] == 0) & (got["status"] == 0)]
    print(f"\n_check_qp {name} B={B} N={N} {kernel}" + (f" P={nseg}" if kernel == "segmented" else "") +
          f": worst |du - du_C| = {gap.max() if gap.size else float('nan'):.2e}, share within {ORC_ATOL:g}: "
          f"{(gap <= ORC_ATOL).mean() if gap.size else float('nan'):.3f}, iters GPU {got['iters'].tolist()} C {c['iters'].tolist()}")
    # a set with hard rows can make an instance's QP infeasible (the scene problems fly straight at the pillar:
    # a hard sdf row linearised inside it may demand more than the inputs give -- HPIPM fails there too);
    # the two solvers must agree on which instances fail, and the rest are compared
    conv = c["status"] == 0
    assert ((got["status"] == 0) == conv).all(), (got["status"], c["status"], got["iters"], c["iters"])
    assert conv.all() or (q.nhs > 0 and conv.mean() >= 0.75), c["status"]
    sel = np.flatnonzero(conv)
    got = {k: v[sel] for k, v in got.items()}
    c = {k: (v[sel] if isinstance(v, np.ndarray) and v.shape[:1] == (B,) else v) for k, v in c.items()}
    lin = {k: v[sel] for k, v in lin.items()}
    prob = {k: (v if k == "dt" else v[sel]) for k, v in prob.items()}
    x0, B = x0[sel], len(sel)
    assert (np.abs(got["iters"] - c["iters"]) <= 1).mean() >= iters_frac, (got["iters"], c["iters"])
    off = np.abs(got["du"] - c["du"]).max(axis=(1, 2)) > ORC_ATOL
    exact = {}
    for b in range(B if dense else 0):
        if n_exact is None or b < n_exact or off[b]:
            qq = qp_oracle.stage_qp({k: v[b] for k, v in lin.items()}, prob["x"][b], prob["u"][b], x0[b], prob["yref"][b],
                                    prob["W"][b], prob["yN"][b], prob["WN"][b], prob["dt"], q, 10.0)
            exact[b] = (qq, qp_oracle.polish_active_set(qq, qp_oracle.solve_dense(qq)))
    _agree(prob, x0, lin, q, got, c, atol=ORC_ATOL,
           lam_l1=[exact[b][1]["lam_l1"] if b in exact else None for b in range(B)] if dense else None)
    ok = np.abs(got["du"] - c["du"]).max(axis=(1, 2)) <= ORC_ATOL
    # dx accumulates du through the dynamics: 4x the du bar where du agrees
    assert (np.abs(got["dx"] - c["dx"]).max(axis=(1, 2))[ok] <= 4 * ORC_ATOL).all()
    hard_active = 0
    for b, (qq, ex) in exact.items():
        H, g, E, e, G, d = qp_oracle.dense_problem(qq)
        sol = dict(dx=got["dx"][b], du=got["du"][b], sl=got["slack"][b][..., 0], su=got["slack"][b][..., 1])
        z, zs = qp_oracle.z_of(qq, sol), qp_oracle.z_of(qq, ex)
        Fz, Fs = 0.5 * z @ H @ z + g @ z, 0.5 * zs @ H @ zs + g @ zs
        assert (G @ z + d).min() > -1e-7 and np.abs(E @ z - e).max() < 1e-8
        assert Fz - Fs <= qp_oracle.objective_bound(G.shape[0], QP_TOL, ex["lam_l1"], got["res"][b, 1]), (b, Fz - Fs)
        n_xu = 10 * (N + 1) + 4 * N
        mu = np.linalg.eigvalsh(H[:n_xu, :n_xu]).min()
        assert np.linalg.norm(z[:n_xu] - zs[:n_xu]) <= np.sqrt(2 * max(Fz - Fs, 0.0) / mu) + 1e-6
        nb = 8 * N + 4 * (N * (q.nh - q.nhs) + q.nsN)  # hard rows follow the box rows and the soft groups
        hard_active += int(((G @ z + d)[nb:] < 1e-6).sum())
    if q.nhs and need_active:
        assert hard_active > 0
    # unused slack entries are zero: stage rows past nh, terminal rows past nsN
    assert (got["slack"][:, :N, q.nh:] == 0).all() and (got["slack"][:, N, q.nsN:] == 0).all()
    if not dense:
        _check_point(prob, x0, lin, q, got)
    return whole


def _check_point(prob, x0, lin, q, got):
    """The returned point itself: the x0 row, the linearised dynamics and the input boxes (the bars of
    test_gpu_qp.test_qp_full_size_feasibility_and_determinism)."""
    dx, du = got["dx"], got["du"]
    np.testing.assert_allclose(dx[:, 0], x0 - prob["x"][:, 0], rtol=0, atol=1e-12)
    cc = lin["xn"] - prob["x"][:, 1:]
    pred = np.einsum("bkji,bkj->bki", lin["AB"][:, :, :10], dx[:, :-1]) + np.einsum("bkji,bkj->bki", lin["AB"][:, :, 10:], du) + cc
    np.testing.assert_allclose(dx[:, 1:], pred, rtol=0, atol=1e-9)
    u_new = prob["u"] + du
    assert (u_new >= np.asarray(q.lbu) - 1e-7).all() and (u_new <= np.asarray(q.ubu) + 1e-7).all()


@pytest.mark.parametrize("name,B,N,kernel,seed", [
    pytest.param(name, B, N, kernel, seed, id=name if (B, N, kernel) == F.PHASE_SPLIT_RUNS[0][:3] else f"{name}-{B}-{N}-{kernel}")
    for B, N, kernel, seed in F.PHASE_SPLIT_RUNS for name in F.PHASE_SPLIT_SETS])
def test_phase_split_bitwise_per_flag_set(gpu_ctx, name, B, N, kernel, seed):
    """rti_prepare (records packed beside the SDF kernel; the sdf row of C^T -- row 1 with no_vfov, row 0 with
    lidar_sdf_only, none (sdf_row == -1) where only the terminal braking row reads the network -- patched by
    the QP kernel) + qp_feedback == linearize + qp_solve, bit for bit, on the serial and the segmented kernel
    (flag_sets.PHASE_SPLIT_RUNS).  (A segmented kernel that patches with sdf_row == -1 writes J_h[:, 2] over
    g_x[4..9] and g_u of every stage record: status 0 everywhere and du off by 0.39 on the two rec_feas sets
    without a stage sdf row.)"""
    _phase_split(gpu_ctx, name, B, N, kernel, seed)


def _phase_split(gpu_ctx, name, B, N, kernel, seed, coeffs=None):
    cfg, q, prob, x0, ta = _setup(gpu_ctx, name, B, N, seed=seed, coeffs=coeffs)
    _, _, _, _, tb = _setup(gpu_ctx, name, B, N, seed=seed, coeffs=coeffs)
    net, qm, opts = _net(gpu_ctx, q), _lib.quad_model(cfg, q), _lib.qp_opts(q)
    gpu_ctx.set_qp_kernel(kernel)
    try:
        want = "segmented" if (kernel == "segmented" or N >= 36) else "serial"
        assert gpu_ctx.qp_kernel(N, B, opts) == want
        _lib.linearize(gpu_ctx, net, qm, B, N, q.np, ta, nyN=q.nyN, no_sdf=not q.need_sdf)
        _lib.qp_solve(gpu_ctx, opts, B, N, ta)
        _lib.rti_prepare(gpu_ctx, net, qm, opts, B, N, q.np, tb, no_sdf=not q.need_sdf)
        _lib.qp_feedback(gpu_ctx, opts, B, N, tb)
        gpu_ctx.synchronize()
    finally:
        gpu_ctx.set_qp_kernel("auto")
    a, b = _np(ta, OUT), _np(tb, OUT)
    print(f"\nphase split {name} B={B} N={N} {want}: max |du_split - du_whole| = {np.nan_to_num(np.abs(a['du'] - b['du']), nan=np.inf).max():.3e}, "
          f"status whole {a['status'].tolist()} split {b['status'].tolist()}")
    assert (a["status"] == 0).all()
    for k in OUT:
        np.testing.assert_array_equal(a[k], b[k], err_msg=k)


def test_capacity_and_refusals(gpu_ctx):
    """The occupancy gate per constraint set (LDS per instance follows the rows), and the ABI's refusals."""
    base = gpu_ctx.qp_capacity(40)
    assert gpu_ctx.qp_capacity(40, _lib.qp_opts(F.quad("default"))) == base
    assert gpu_ctx.qp_capacity(40, _lib.qp_opts(F.quad("no_sdf"))) >= base
    assert gpu_ctx.qp_capacity(40, _lib.qp_opts(F.quad("stability"))) >= 256
    bad = _lib.qp_opts(F.quad("default"))
    bad.h_col[1] = 0  # a column twice
    with pytest.raises(_lib.SdfnmpcError):
        gpu_ctx.qp_capacity(40, bad)
    B, N = 2, 20
    cfg, q, prob, x0, t = _setup(gpu_ctx, "stability", B, N, seed=1)
    with pytest.raises(_lib.SdfnmpcError, match="nyN"):  # stability needs the 5-row terminal residual
        _lib.linearize(gpu_ctx, _net(gpu_ctx, q), _lib.quad_model(cfg, q), B, N, q.np, t, nyN=4)
    cfg, q, prob, x0, t = _setup(gpu_ctx, "default", B, N, seed=1)
    with pytest.raises(_lib.SdfnmpcError, match="NULL network"):
        _lib.linearize(gpu_ctx, None, _lib.quad_model(cfg, q), B, N, q.np, t)


def _nmpc(name, B, N, seed, coeffs=None):
    from sdf_nmpc_amd.controller import Nmpc
    from sdf_nmpc_amd.reference import Ref, yaw2quat
    cfg = _config(name, N, coeffs)
    q = F.quad(name, cfg, coeffs=coeffs)
    scene = F.uses_scene(q)
    if scene:
        import scene_setup as S
    n = Nmpc(cfg, batch=B, braking_coeffs=q.poly if q.rec_feas else None, weights=S.SCENE if scene else None)
    rng = np.random.default_rng(seed)
    x0 = np.zeros((B, 10))
    x0[:, :3] = rng.uniform(-1, 1, (B, 3))
    x0[:, 3:7] = np.stack([yaw2quat(y) for y in rng.uniform(-0.5, 0.5, B)])
    x0[:, 7] = rng.uniform(0, 1.5, B)  # moving forward: the braking point ahead of the camera
    n.set_sdf_flag(1.0)
    lat = np.broadcast_to(S.scene_latent(), (B, 128)) if scene else rng.normal(size=(B, 128))
    n.set_latent(lat, x0[:, :3], np.stack([np.eye(3)] * B))
    r = Ref(cfg)
    r.p, r.q = np.array([4.0, 0.5, 1.0]), yaw2quat(0.1)
    r.use_weights(r.W_on)
    for k in range(N + 1):
        n.set_ref(r, k)
    n.set_x0(x0)
    return n, q, x0


@pytest.mark.parametrize("name,N", [pytest.param(n, 20, id=n) for n in (
    "no_sdf", "no_sdf_constraint", "lidar", "rec_feas_soft_brake", "stability", "hard_all", "hard_df_rec_feas")] +
    [pytest.param("rec_feas_no_sdf_row", 40, id="rec_feas_no_sdf_row-N40")])
def test_controller_rti_step_per_flag_set(oracle_lib, name, N):
    """Nmpc.solve (host setters, solver object) for a flag set: one SQP-RTI step against the oracle pipeline
    (oracle linearisation + the C IPM) on the same iterate; u0 within 2e-5.  At N = 40 AUTO runs the segmented
    kernel on the solver object's split pack -- for rec_feas_no_sdf_row with no stage sdf row to patch."""
    _controller_step(oracle_lib, name, N)


def _controller_step(oracle_lib, name, N, coeffs=None, check=None):
    """check(n, q, x0, xbar, glin, lin, onet): further assertions on the open controller after its step."""
    B = 6
    n, q, x0 = _nmpc(name, B, N, seed=21, coeffs=coeffs)
    assert n.ocp.ctx.qp_kernel(N, B, _lib.qp_opts(q)) == ("segmented" if N >= 36 else "serial")
    xbar, ubar = n.ocp.download("x").copy(), n.ocp.download("u").copy()
    xbar[:, 0] = x0
    assert n.solve() == 0
    u0 = n.get_u()
    # the step's preparation phase (solver fields) against the oracle linearisation of the same iterate
    glin = {k: n.ocp.download(k).reshape(B, *s) for k, s in dict(
        xn=(N, 10), AB=(N, 14, 10), y=(N, 11), Jy=(N, 14, 11), yN=(q.nyN,), JyN=(10, q.nyN), h=(N + 1, 3),
        Jh=(N + 1, 10, 3), hE=(6,), JhE=(10, 6)).items()}
    onet = _onet(oracle_lib, q)
    lin = oracle_lib.linearize_batch(oracle_lib.quad_model(n.cfg), onet, xbar, ubar, n.p, n.ocp.dt, model=q)
    for k in ("xn", "AB", "y", "Jy", "yN", "JyN"):
        np.testing.assert_allclose(glin[k], lin[k], rtol=LIN_RTOL, atol=1e-12 * max(1.0, np.abs(lin[k]).max()), err_msg=k)
    # the QP of that step against the C restatement on the step's own linearisation
    prob = dict(x=xbar, u=ubar, yref=n.y, W=n.W, yN=n.yN, WN=n.WN, dt=n.ocp.dt)
    r = oracle_lib.qp_ipm_batch(glin, prob, x0, q, tol=QP_TOL)
    assert (r["status"] == 0).all()
    np.testing.assert_allclose(u0, ubar[:, 0] + r["du"][:, 0], rtol=0, atol=2e-5)
    if q.enable_sdf:  # Nmpc.eval: [sdf] (+ [poly(v), sdf - poly(v)] with rec_feas), flag = 1
        ev = n.eval(N)
        assert ev.shape == (B, 3 if q.rec_feas else 1)
    else:
        assert (n.eval(0) == 0).all()
    if check is not None:
        check(n, q, x0, xbar, glin, lin, onet)
    n.ocp.close()
