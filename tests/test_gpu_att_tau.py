"""The 'att_tau' model (first-order roll / pitch lag, sdfnmpc_quad_model.kind = 1) on the GPU: linearize_kernel<1>
against the fixtures recorded from the reference's helpers (tests/golden/tau_golden.npz) and against the torch fp64
restatement (att_tau_ref.py), through every entry point that embeds the model struct (linearize, rti_prepare, the
serial few-row path, the graph step, the solver object), into the QP and around the closed loop; and the ABI's
refusals."""
import os

import numpy as np
import pytest

import att_tau_ref as T
from sdf_nmpc_amd import _lib, synth, weights as W
from sdf_nmpc_amd.config import Config
from sdf_nmpc_amd.controller import Nmpc
from sdf_nmpc_amd.model import Quad
from test_gpu_controller import scenario
from test_gpu_qp import QP_TOL, _agree
from tolerances import lin_close, sdf_df_ok, sdf_grad_ok

pytestmark = [pytest.mark.gpu, pytest.mark.filterwarnings("ignore:no SDF weights")]

HERE = os.path.dirname(os.path.abspath(__file__))
LIN = ("xn", "AB", "y", "Jy", "yN", "JyN", "h", "Jh")
OUT = LIN + ("dx", "du", "slack", "status", "iters", "res")
U0_ATOL = 2e-5   # tests/test_gpu_closed_loop.py
K = 10


@pytest.fixture(scope="module")
def cfg_tau():
    return Config(mpc__model="att_tau")


@pytest.fixture(scope="module")
def onet(oracle_lib):
    return oracle_lib.Net(W.DEFAULT_SPEC, W.siren_weights(W.DEFAULT_SPEC, 0))


@pytest.fixture(scope="module")
def tau_golden():
    return np.load(os.path.join(HERE, "golden", "tau_golden.npz"))


def _dev(ctx):
    import torch
    return torch.device("cuda", ctx.device)


def run_lin(ctx, net, qm, prob, latent_mode=0):
    """sdfnmpc_linearize into NaN-filled outputs."""
    import torch
    dev = _dev(ctx)
    B, N1, _ = prob["x"].shape
    N = N1 - 1
    bufs = {k: torch.from_numpy(np.ascontiguousarray(prob[k])).to(dev) for k in ("x", "u", "p", "dt")}
    shapes = dict(xn=(B, N, 10), AB=(B, N, 14, 10), y=(B, N, 11), Jy=(B, N, 14, 11), yN=(B, 4), JyN=(B, 10, 4),
                  h=(B, N1, 3), Jh=(B, N1, 10, 3))
    for k, s in shapes.items():
        bufs[k] = torch.full(s, float("nan"), dtype=torch.float64, device=dev)
    torch.cuda.synchronize()
    _lib.linearize(ctx, net, qm, B, N, prob["p"].shape[-1], bufs, latent_mode)
    ctx.synchronize()
    return {k: bufs[k].cpu().numpy() for k in LIN}


def check_lin(got, ref):
    """lin_close on every fp64 output; the sdf row (fp32 network) at the SDF bar."""
    for k in LIN:
        assert np.isfinite(got[k]).all(), k
    for k in ("xn", "AB", "y", "Jy", "yN", "JyN"):
        assert lin_close(got[k], ref[k]), (k, np.abs(got[k] - ref[k]).max())
    assert lin_close(got["h"][..., :2], ref["h"][..., :2]) and lin_close(got["Jh"][..., :2], ref["Jh"][..., :2])
    assert sdf_df_ok(got["h"][..., 2], ref["h"][..., 2])
    assert sdf_grad_ok(got["Jh"][..., :3, 2], ref["Jh"][..., :3, 2])
    assert np.all(got["Jh"][..., 3:, 2] == 0)


def tau_problem(cfg, B, N, seed, dt=None):
    """synth.make_problem's positions and velocities; attitudes with roll and pitch in +-0.5 rad at every node,
    non-unit quaternions; the flag off at every third node."""
    prob = synth.make_problem(cfg, B, N, seed=seed, dt=dt)
    rng = np.random.default_rng(1000 + seed)
    eul = np.stack([rng.uniform(-0.5, 0.5, (B, N + 1)), rng.uniform(-0.5, 0.5, (B, N + 1)),
                    rng.uniform(-np.pi, np.pi, (B, N + 1))], -1)
    prob["x"][..., 3:7] = synth.euler2quat(eul) * rng.uniform(0.9, 1.1, (B, N + 1, 1))
    prob["p"][:, ::3, 0] = 0.0
    return prob


def qp_bufs(ctx, prob, x0, node0=True):
    """Device inputs of one RTI step (node0: the iterate's node 0 = x0, as the solver object sets it) and NaN
    outputs."""
    import torch
    dev = _dev(ctx)
    B, N1, _ = prob["x"].shape
    N = N1 - 1
    x = prob["x"].copy()
    if node0:
        x[:, 0] = x0
    t = {k: torch.from_numpy(np.ascontiguousarray(v)).to(dev) for k, v in
         dict(x=x, u=prob["u"], p=prob["p"], dt=prob["dt"], x0=x0, yref=prob["yref"], W=prob["W"], yNref=prob["yN"],
              WN=prob["WN"]).items()}
    sh = dict(xn=(B, N, 10), AB=(B, N, 14, 10), y=(B, N, 11), Jy=(B, N, 14, 11), yN=(B, 4), JyN=(B, 10, 4),
              h=(B, N1, 3), Jh=(B, N1, 10, 3), dx=(B, N1, 10), du=(B, N, 4), slack=(B, N1, 3, 2), res=(B, 2))
    for k, s in sh.items():
        t[k] = torch.full(s, float("nan"), dtype=torch.float64, device=dev)
    t["status"] = torch.full((B,), -1, dtype=torch.int32, device=dev)
    t["iters"] = torch.full((B,), -1, dtype=torch.int32, device=dev)
    torch.cuda.synchronize()
    return t


# ---- 1. the fixtures recorded from the reference's helpers
def _golden_cases(ctx, cfg, L, qm):
    net = _lib.Net.siren(ctx, 0)
    for dtv in np.unique(L["dt"]):
        idx = np.nonzero(L["dt"] == dtv)[0]
        prob = {"x": np.repeat(L["x"][idx][:, None], 2, 1), "u": L["u"][idx][:, None].copy(),
                "p": np.repeat(L["p"][idx][:, None], 2, 1), "dt": np.array([dtv])}
        got = run_lin(ctx, net, qm, prob, latent_mode=1)
        assert lin_close(got["xn"][:, 0], L["xn"][idx])
        assert lin_close(got["AB"][:, 0].transpose(0, 2, 1), np.concatenate([L["A"][idx], L["B"][idx]], 2))
        assert lin_close(got["y"][:, 0], L["y"][idx])
        assert lin_close(got["Jy"][:, 0].transpose(0, 2, 1), L["Jy"][idx])
        assert lin_close(got["yN"], L["yN"][idx]) and lin_close(got["JyN"].transpose(0, 2, 1), L["JyN"][idx])
        assert lin_close(got["h"][:, 0, :2], L["h"][idx][:, :2])
        assert lin_close(got["Jh"][:, 0, :, :2].transpose(0, 2, 1), L["Jh"][idx][:, :2])
        assert sdf_df_ok(got["h"][:, 0, 2], L["h"][idx][:, 2])
        assert sdf_grad_ok(got["Jh"][:, 0, :3, 2], L["Jh"][idx][:, 2, :3])


def test_att_tau_linearize_vs_reference_helper_fixtures(tau_golden, gpu_ctx, cfg_tau):
    """The 64 tau_golden cases (values from the reference's numpy helpers, Jacobians FD-pinned)."""
    _golden_cases(gpu_ctx, cfg_tau, tau_golden, _lib.quad_model(cfg_tau))


# ---- 2. against the helper: a partial last workgroup (21 and 183 rows, 32 nodes per block), more than one
#         block, the terminal two-pass branch, the non-uniform grid
@pytest.mark.parametrize("B,N,uniform", [(1, 20, True), (7, 40, False), (3, 60, True)])
def test_att_tau_linearize_vs_helper(gpu_ctx, oracle_lib, onet, cfg_tau, B, N, uniform):
    _, dt = oracle_lib.shooting_grid(N, float(cfg_tau.mpc.T), uniform)
    prob = tau_problem(cfg_tau, B, N, seed=B * 100 + N, dt=dt)
    got = run_lin(gpu_ctx, _lib.Net.siren(gpu_ctx, 0), _lib.quad_model(cfg_tau), prob)
    check_lin(got, T.lin(oracle_lib, cfg_tau, onet, prob["x"], prob["u"], prob["p"], prob["dt"]))


# ---- 3. the kind is honoured by every entry point that embeds the model struct
@pytest.mark.parametrize("B,N,kernel", [(24, 20, "auto"), (8, 40, "segmented")])
def test_att_tau_through_every_entry_point_bitwise(gpu_ctx, cfg, cfg_tau, B, N, kernel):
    """rti_prepare + qp_feedback == linearize + qp_solve; the graph step and the solver object == the eager phases,
    bit for bit under 'att_tau'; and the linearisation is not the 'att' one."""
    import torch
    net = _lib.Net.siren(gpu_ctx, 0)
    model = Quad(cfg_tau)
    opts, qm = _lib.qp_opts(model), _lib.quad_model(cfg_tau, model)
    prob = synth.make_problem(cfg_tau, B, N, seed=3)
    x0 = prob["x"][:, 0] + np.random.default_rng(3).normal(0, 0.05, (B, 10))
    np_ = prob["p"].shape[-1]
    ta, tb, tc, td, te = (qp_bufs(gpu_ctx, prob, x0) for _ in range(5))
    ua, ub = (torch.empty((B, 4), dtype=torch.float64, device=_dev(gpu_ctx)) for _ in range(2))
    gpu_ctx.set_qp_kernel(kernel)
    try:
        if kernel != "auto":
            assert gpu_ctx.qp_kernel(N, B) == kernel
        _lib.linearize(gpu_ctx, net, qm, B, N, np_, ta)
        _lib.qp_solve(gpu_ctx, opts, B, N, ta)
        _lib.rti_prepare(gpu_ctx, net, qm, opts, B, N, np_, tb)
        _lib.qp_feedback(gpu_ctx, opts, B, N, tb)
        _lib.linearize(gpu_ctx, net, _lib.quad_model(cfg), B, N, np_, tc)  # the same inputs under 'att'
        gpu_ctx.synchronize()
        assert (ta["status"].cpu().numpy() == 0).all()
        for k in OUT:
            np.testing.assert_array_equal(ta[k].cpu().numpy(), tb[k].cpu().numpy(), err_msg=k)
        assert np.abs(ta["AB"].cpu().numpy() - tc["AB"].cpu().numpy()).max() > 1e-3
        assert np.abs(ta["xn"].cpu().numpy() - tc["xn"].cpu().numpy()).max() > 1e-4
        # two control steps: eager phases, the captured graph (its creation runs the first step), the solver object
        for _ in range(2):
            _lib.rti_prepare(gpu_ctx, net, qm, opts, B, N, np_, td)
            _lib.qp_feedback(gpu_ctx, opts, B, N, td)
            _lib.rti_apply(gpu_ctx, B, N, td["x"], td["u"], td["dx"], td["du"], ua, td["status"])
        step = _lib.RtiStep(gpu_ctx, net, qm, opts, B, N, np_, te, u0=ub, graph=True)
        step()
        gpu_ctx.synchronize()
        for k in OUT + ("x", "u"):
            np.testing.assert_array_equal(td[k].cpu().numpy(), te[k].cpu().numpy(), err_msg=f"graph {k}")
        np.testing.assert_array_equal(ua.cpu().numpy(), ub.cpu().numpy())
        del step
        s = _lib.Solver(gpu_ctx, net, qm, opts, B, N, np_, model.ny, prob["dt"])
        xs = prob["x"].copy()
        xs[:, 0] = x0
        for name, v in (("x", xs), ("u", prob["u"]), ("p", prob["p"]), ("x0", x0[:, None]), ("yref", prob["yref"]),
                        ("W", prob["W"]), ("yNref", prob["yN"][:, None]), ("WN", prob["WN"][:, None])):
            s.upload(name, v)
        for _ in range(2):
            s.step()
            u0 = s.wait().copy()
        np.testing.assert_array_equal(u0, ua.cpu().numpy())
        for k in ("x", "u", "xn", "AB", "y", "Jy", "dx", "du"):
            np.testing.assert_array_equal(s.download(k).reshape(td[k].shape), td[k].cpu().numpy(), err_msg=f"solver {k}")
        np.testing.assert_array_equal(s.status, td["status"].cpu().numpy())
        s.close()
    finally:
        gpu_ctx.set_qp_kernel("auto")


def test_att_tau_serial_few_row_path_vs_helper(gpu_ctx, oracle_lib, onet, cfg_tau):
    """B = 1 (41 rows): the preparation phase runs the linearisation after the row kernel on the one stream."""
    B, N = 1, 40
    model = Quad(cfg_tau)
    prob = tau_problem(cfg_tau, B, N, seed=17)
    t = qp_bufs(gpu_ctx, prob, prob["x"][:, 0])
    _lib.rti_prepare(gpu_ctx, _lib.Net.siren(gpu_ctx, 0), _lib.quad_model(cfg_tau, model), _lib.qp_opts(model), B, N,
                     prob["p"].shape[-1], t)
    gpu_ctx.synchronize()
    check_lin({k: t[k].cpu().numpy() for k in LIN},
              T.lin(oracle_lib, cfg_tau, onet, prob["x"], prob["u"], prob["p"], prob["dt"]))


# ---- 4. the QP on the 'att_tau' linearisation (seeds: status 0 for every instance in the C IPM alone)
@pytest.mark.parametrize("B,N,seed", [(8, 20, 3), (8, 40, 4)])
def test_att_tau_qp_matches_riccati_oracle(gpu_ctx, oracle_lib, onet, cfg_tau, B, N, seed):
    net = _lib.Net.siren(gpu_ctx, 0)
    model = Quad(cfg_tau)
    prob = synth.make_problem(cfg_tau, B, N, seed=seed)
    x0 = prob["x"][:, 0] + np.random.default_rng(seed).normal(0, 0.05, (B, 10))
    lin = T.lin(oracle_lib, cfg_tau, onet, prob["x"], prob["u"], prob["p"], prob["dt"])
    ref = oracle_lib.qp_ipm_batch(lin, prob, x0, model, tol=QP_TOL, nthreads=8)
    assert (ref["status"] == 0).all()
    t = qp_bufs(gpu_ctx, prob, x0, node0=False)  # the iterate as generated: x0 enters through the QP only
    _lib.linearize(gpu_ctx, net, _lib.quad_model(cfg_tau, model), B, N, prob["p"].shape[-1], t)
    _lib.qp_solve(gpu_ctx, _lib.qp_opts(model, tol=QP_TOL), B, N, t)
    gpu_ctx.synchronize()
    assert (t["status"].cpu().numpy() == 0).all()
    lin.pop("sdf", None)
    _agree(prob, x0, lin, model, {k: t[k].cpu().numpy() for k in ("du", "dx", "slack")}, ref)
    assert np.abs(t["iters"].cpu().numpy() - ref["iters"]).max() <= 1


# ---- 5. closed loop
def _oracle_loop(O, onet, n, cfg, x0, p, K):
    """tests/test_gpu_closed_loop.py's oracle pipeline with the 'att_tau' linearisation and plant."""
    B, N, dt = x0.shape[0], n.N, n.ocp.dt
    xs = np.repeat(x0[:, None], N + 1, axis=1)
    us = np.broadcast_to(n.model.u_hover, (B, N, 4)).copy()
    prob = {"yref": n.y, "W": n.W, "yN": n.yN, "WN": n.WN, "dt": dt}
    xo, u_hist, du = x0.copy(), [], np.zeros((B, N, 4))
    for _ in range(K):
        xs[:, 0] = xo
        lin = T.lin(O, cfg, onet, xs, us, p, dt)
        r = O.qp_ipm_batch(lin, dict(prob, x=xs, u=us), xo, n.model, nthreads=4, du_ws=du)
        assert (r["status"] == 0).all()
        du = r["du"].copy()
        xs, us = xs + r["dx"], us + r["du"]
        u_hist.append(us[:, 0].copy())
        xo = T.step(cfg, xo, us[:, 0], dt[0])
    return np.array(u_hist), xs, us


@pytest.mark.parametrize("flag,margin", [(0.0, None), (1.0, -0.6)])
def test_att_tau_closed_loop_matches_oracle_pipeline(oracle_lib, onet, flag, margin):
    """K Nmpc.solve steps under 'att_tau', the plant advanced by the helper's RK4, against the oracle pipeline.
    The oracle loop alone is contractive in both settings, so every step is pinned to U0_ATOL (the envelope form of
    tests/test_gpu_closed_loop.py is not needed): its response to a 1e-10 change of x_0 does not grow over the K
    steps (asserted; measured 1.9e-10 at step 1 -> 3.3e-11 at step 10 with the flag off, and with the flag on
    2.2e-7 -> 1.7e-7 with a largest value of 5.9e-7 at step 2: there the soft rows are live and the IPM's stopped
    iterate moves by ~1e-7 under any change of its data, without growth).  Measured |u0 - u0_oracle|: 2e-15 with
    the flag off, 4.5e-6 with it on."""
    O = oracle_lib
    over = {} if margin is None else {"mpc__bound_margin": margin}
    cfg = Config(mpc__N=20, mpc__model="att_tau", **over)
    B = 4
    n = Nmpc(cfg, batch=B)
    assert n.model.kind == "att_tau" and n.ocp.cmodel.kind == 1
    x0 = scenario(n, np.random.default_rng(31))
    n.set_sdf_flag(flag)
    ug, xg = [], x0.copy()
    for _ in range(K):
        n.set_x0(xg)
        assert n.solve() == 0 and (n.ocp.status == 0).all()
        ug.append(n.get_u().copy())
        xg = T.step(cfg, xg, ug[-1], n.ocp.dt[0])
    ug = np.array(ug)
    uo, xs, us = _oracle_loop(O, onet, n, cfg, x0, n.p, K)
    xp = x0.copy()
    xp[:, [0, 4, 8]] += 1e-10
    up, _, _ = _oracle_loop(O, onet, n, cfg, xp, n.p, K)
    growth = np.abs(up - uo).max(axis=(1, 2))
    d = np.abs(ug - uo).max(axis=(1, 2))
    print(f"\natt_tau closed loop, flag {flag}: |u0 - u0_oracle| per step max {d.max():.2e}; oracle's response to a "
          f"1e-10 change of x0 per step {np.array2string(growth, precision=1)}")
    # contractive: the response does not grow over the K steps (a chaotic loop multiplies it step by step,
    # tests/test_gpu_closed_loop.py: about 5x per step), so no envelope is needed
    assert growth[K // 2:].max() <= growth[:K // 2].max() and growth[-1] <= growth[0], growth
    assert d.max() <= U0_ATOL, d
    xgpu, ugpu = n.get_matrices()
    np.testing.assert_allclose(ugpu, us, rtol=0, atol=U0_ATOL)
    np.testing.assert_allclose(xgpu, xs, rtol=0, atol=1e-4)
    n.ocp.close()


# ---- 6. the ABI's refusals, and the default kind through the enlarged struct
def test_model_kind_refusals_and_default_kind(golden, gpu_ctx, cfg, cfg_tau):
    B, N = 2, 20
    net = _lib.Net.siren(gpu_ctx, 0)
    prob = synth.make_problem(cfg, B, N, seed=5)
    t = qp_bufs(gpu_ctx, prob, prob["x"][:, 0])
    np_ = prob["p"].shape[-1]
    qm = _lib.quad_model(cfg)
    qm.kind = 2
    with pytest.raises(_lib.SdfnmpcError, match="error -4"):  # SDFNMPC_E_UNSUPPORTED
        _lib.linearize(gpu_ctx, net, qm, B, N, np_, t)
    with pytest.raises(_lib.SdfnmpcError, match="error -4"):
        _lib.rti_prepare(gpu_ctx, net, qm, _lib.qp_opts(Quad(cfg)), B, N, np_, t)
    with pytest.raises(_lib.SdfnmpcError, match="error -4"):
        _lib.Solver(gpu_ctx, net, qm, _lib.qp_opts(Quad(cfg)), B, N, np_, 11, prob["dt"])
    for field in ("rec_feas", "stability"):
        qm = _lib.quad_model(cfg_tau)
        setattr(qm, field, 1)
        with pytest.raises(_lib.SdfnmpcError, match="error -4"):
            _lib.linearize(gpu_ctx, net, qm, B, N, np_, t)
    gpu_ctx.synchronize()
    assert np.isnan(t["AB"].cpu().numpy()).all()  # nothing ran
    qm = _lib.quad_model(cfg)
    assert qm.kind == 0
    _golden_cases(gpu_ctx, cfg, golden["lin"], qm)
