"""Closed-loop rollouts of a controller whose SDF is the exact distance of the scene it flies in (Nmpc.set_sdf_scene,
sdfnmpc_solver_rollout_scene_sdf): bitwise against the host-driven loop set_x0 / scene.pose + set_pose_device /
set_scene_time / gen_refs_device / solve / plant_step (static and moving scenes, `predict`, chunks), against the CPU
oracle pipeline with the SDF row replaced by tests/scene_sdf_ref.py on the pillar-and-box world of tests/scene_setup.py,
the way back to the network, and the API contract.  N = 10, B = 3, K <= 12."""
import numpy as np
import pytest

import scene_dyn_ref as D
import scene_ref as R
import scene_sdf_ref as SR
import scene_setup as S
from sdf_nmpc_amd import _lib
from sdf_nmpc_amd import weights as W
from sdf_nmpc_amd.config import Config
from sdf_nmpc_amd.controller import Nmpc
from sdf_nmpc_amd.reference import Ref, yaw2quat
from sdf_nmpc_amd.scene import Scene
from test_gpu_closed_loop import U0_ATOL
from test_gpu_rollout import _setup

pytestmark = [pytest.mark.gpu, pytest.mark.filterwarnings("ignore:no SDF weights"),
              pytest.mark.filterwarnings("ignore:QP reached")]

B, K = 3, 6
SCENE_OF = np.array([1, 0, 1], np.int32)
OTHER = [("sphere", [1.5, 0.5, 0.2, 0.5]), ("box", [-2.0, -2.5, -1.0, 2.0, -1.5, 1.0])]
T0 = 0.5
# the world of tests/scene_setup.py (tools/fit_scene_sdf.py) as primitives: the pillar and the box
WORLD = [("cylinder", [3.0, 0.3, 0.4, -3.0, 3.0]), ("box", [5.0, -2.5, -3.0, 5.6, -0.8, 3.0])]
# the oracle scenario: K_ORACLE steps from 1.1 m in front of the pillar, flying at 1.5 m/s past it on either side
K_ORACLE = 12
X_START, V_START, Y_START = 1.5, 1.5, np.array([0.8, -0.3, 1.0])


@pytest.fixture(scope="module", autouse=True)
def _torch_first(gpu_ctx):
    """torch opens the device before the first controller of this module does, as in tests/test_gpu_rollout.py."""


def _wps():
    rng = np.random.default_rng(5)
    return (rng.uniform(-2, 2, (B, 2, 3)), np.stack([[yaw2quat(a) for a in row] for row in rng.uniform(-1, 1, (B, 2))]))


def _dyn_prims():
    return [Scene.moving(p, **kw) if kw is not None else p for p, kw in D.SPEC]


def _make(cfg, dynamic, predict=False, seed=21):
    """A controller (test_gpu_rollout's setup: latents, flag on, one goal) with a scene source: two scenes, of which
    instances 0 and 2 see the fixture (static or moving)."""
    n, x0 = _setup(cfg, B, seed)
    scene = Scene(n.ocp.ctx, [OTHER, _dyn_prims() if dynamic else R.SCENE], scene_of=SCENE_OF)
    n.set_sdf_scene(scene, predict=predict)
    return n, x0, scene


def _host_loop(n, scene, x0, steps, every, wps, t0, phase=0):
    """The loop a user writes around solve() with a scene source: the pose refreshed from the state every `every`-th
    step, the scene's clock, the references, the step, the plant."""
    ctx = n.ocp.ctx
    dt = float(n.ocp.dt[0])
    plant = _lib.plant_opts(n.cfg, dt=dt)
    dx = _lib.DeviceArray(ctx, (B, 10))
    xs, us, its, sts = [np.reshape(x0, (B, 10)).copy()], [], [], []
    for k in range(steps):
        n.set_x0(xs[-1])
        if (k + phase) % every == 0:
            ps = scene.pose(xs[-1], n.cfg)
            n.set_pose_device(ps["W_p_Bo"], ps["W_R_Bo"])
        n.set_scene_time(t0 + (phase + k) * dt)
        n.gen_refs_device("wps", wps=wps)
        n.solve()
        us.append(n.ocp.field("u0").numpy().reshape(B, 4))
        its.append(n.ocp.iters.copy())
        sts.append(n.ocp.status.copy())
        dx.upload(xs[-1])
        _lib.plant_step(ctx, plant, B, dx, n.ocp.field("u0"), dx)
        xs.append(dx.numpy())
    return np.stack(xs, 1), np.stack(us, 1), np.stack(sts, 1), np.stack(its, 1)


@pytest.mark.parametrize("dynamic,predict,every", [(False, False, 1), (False, False, 3), (True, True, 1), (True, False, 2)])
def test_rollout_with_scene_source_equals_host_driven_loop_bitwise(dynamic, predict, every):
    cfg = Config(mpc__N=10)
    wps = _wps()
    na, x0, sa = _make(cfg, dynamic, predict)
    nb, _, sb = _make(cfg, dynamic, predict)
    assert sa.is_dynamic == dynamic
    na.set_x0(x0)
    r = na.rollout(K, refs="wps", wps=wps, perceive_every=every, scene_t0=T0)
    x, u, status, iters = _host_loop(nb, sb, x0, K, every, wps, T0)
    np.testing.assert_array_equal(r.x, x)
    np.testing.assert_array_equal(r.u, u)
    np.testing.assert_array_equal(r.status, status)
    np.testing.assert_array_equal(r.iters, iters)
    pa, pb = na.ocp.download("p"), nb.ocp.download("p")
    np.testing.assert_array_equal(pa, pb)
    assert (r.iters > 0).all() and np.ptp(r.u[:, :, 0]) > 1e-3
    # the pose columns hold the last refresh: the camera pose of the state before step k_last
    k_last = (K - 1) // every * every
    ps = sb.pose(r.x[:, k_last], cfg)
    np.testing.assert_array_equal(pa[:, :, 1:4], np.repeat(ps["W_p_C"].numpy()[:, None], 11, 1))
    # the source reached the rows: h[2] is the reference's distance of the last linearisation point, not the network's
    dt = float(na.ocp.dt[0])
    h = na.ocp.download("h")
    t_last = T0 + (K - 1) * dt
    tau = np.concatenate([[0.0], np.cumsum(na.ocp.dt)]) if predict else None
    scenes = [OTHER, D.scene() if dynamic else R.SCENE]
    # the iterate the last step linearised about is x - dx (rti_apply added dx)
    xi = na.ocp.download("x") - na.ocp.download("dx")
    want = np.stack([SR.sdf_rows(scenes[s], xi[b], pa[b], na.model.max_df, t0=t_last, tau=tau)[0]
                     for b, s in enumerate(SCENE_OF)])
    ok = (r.status[:, -1] < 2)[:, None] & np.stack([SR.decided(scenes[s], xi[b], na.model.max_df, t0=t_last, tau=tau)
                                                     for b, s in enumerate(SCENE_OF)])
    print(f"\nlast step's h[2] against the reference on {ok.sum()} rows: {np.abs(h[..., 2] - want)[ok].max():.2e}; "
          f"{int((want < na.model.max_df).sum())} untruncated")
    # x - dx is the linearisation point up to one rounding of a coordinate (1e-15 m) and |grad| <= 1: the rows' bar
    assert ok.sum() >= 20 and np.abs(h[..., 2] - want)[ok].max() <= 1e-12
    # t and the clearance: the source scene, at t[j] for a moving one
    np.testing.assert_array_equal(r.t, T0 + np.arange(K + 1) * dt)
    dist = (lambda s, pts: D.distance(scenes[s], pts, r.t)) if dynamic else (lambda s, pts: R.distance(scenes[s], pts))
    want_c = np.stack([dist(s, r.x[b, :, :3]) if s == 1 else R.distance(OTHER, r.x[b, :, :3])
                       for b, s in enumerate(SCENE_OF)])
    assert r.clearance.shape == (B, K + 1) and np.abs(r.clearance - want_c).max() <= 1e-12
    for m in (na, nb):
        m.ocp.close()


def test_chunks_with_phase_are_the_uncut_rollout():
    """K one-step chunks with perceive_phase = k: the pose schedule and the scene's clock of the uncut rollout."""
    cfg = Config(mpc__N=10)
    wps = _wps()
    n, x0, _ = _make(cfg, dynamic=True, predict=True)
    n.set_x0(x0)
    xs, us, ts, cl = [np.reshape(x0, (B, 10))], [], [], []
    for k in range(K):
        r = n.rollout(1, refs="wps", wps=wps, perceive_every=2, perceive_phase=k, scene_t0=T0)
        xs.append(r.x[:, 1])
        us.append(r.u[:, 0])
        ts.append(r.t)
        cl.append(r.clearance)
    m, _, _ = _make(cfg, dynamic=True, predict=True)
    m.set_x0(x0)
    whole = m.rollout(K, refs="wps", wps=wps, perceive_every=2, scene_t0=T0)
    np.testing.assert_array_equal(whole.x, np.stack(xs, 1))
    np.testing.assert_array_equal(whole.u, np.stack(us, 1))
    np.testing.assert_array_equal(m.ocp.download("p"), n.ocp.download("p"))
    for k in range(K):
        np.testing.assert_array_equal(ts[k], whole.t[k:k + 2])
        np.testing.assert_array_equal(cl[k], whole.clearance[:, k:k + 2])
    n.ocp.close()
    m.ocp.close()


# ---- against the CPU oracle
def _start(n):
    """scene_setup's scenario moved up to the pillar: at X_START, flying at it with V_START, the goal beyond it."""
    x0 = S.setup(n, y0=Y_START)
    x0[:, 0] = X_START
    x0[:, 7] = V_START
    return x0


def oracle_loop(O, onet, n, cfg, prims, x0, steps, max_df):
    """scene_setup.oracle_loop with the scene source: before every step the camera pose of p from the plant state (as
    Nmpc.set_latent forms it), and column 2 of h / J_h from scene_sdf_ref.sdf_rows instead of the network, before the
    C IPM.  Returns the per-step diagnostics of scene_setup.oracle_loop, plus the plant states."""
    Bn, N, dt, shift = x0.shape[0], n.N, n.ocp.dt, int(cfg.mpc.shift)
    B_p_C, B_R_C = np.asarray(cfg.sensor.B_p_C, float).ravel(), np.asarray(cfg.sensor.B_R_C, float).reshape(3, 3)
    xs = np.repeat(x0[:, None], N + 1, axis=1)
    us = np.broadcast_to(n.model.u_hover, (Bn, N, 4)).copy()
    p = np.array(n.p, float).reshape(Bn, N + 1, -1)
    prob = {"yref": n.y, "W": n.W, "yN": n.yN, "WN": n.WN, "dt": dt}
    xo, hist = x0.copy(), []
    for _ in range(steps):
        for b in range(Bn):
            Rb = R.quat2rot(xo[b, 3:7])
            p[b, :, 1:4] = Rb @ B_p_C + xo[b, :3]
            p[b, :, 4:13] = (Rb @ B_R_C).reshape(9)
        if 0 < shift < N:
            xs[:, : N - shift] = xs[:, shift:N].copy()
            us[:, : N - shift] = us[:, shift:N].copy()
        xs[:, 0] = xo
        lin = O.linearize_batch(O.quad_model(cfg), onet, xs, us, p, dt, model=n.model)
        lin["h"][..., 2], lin["Jh"][..., 2] = SR.sdf_rows(prims, xs, p, max_df)
        r = O.qp_ipm_batch(lin, dict(prob, x=xs, u=us), xo, n.model, nthreads=4,
                           du_ws=np.zeros((Bn, N, 4)) if not hist else hist[-1]["du"])
        assert (r["status"] == 0).all()
        hist.append({"x0": xo.copy(), "h2min": lin["h"][..., 2].min(axis=1), "du": r["du"].copy(),
                     "sdf_slack": r["slack"][:, :, 2, 0].max(axis=1), "iters": r["iters"].copy()})
        xs, us = xs + r["dx"], us + r["du"]
        hist[-1]["u0"] = us[:, 0].copy()
        xo = S.plant(O, onet, cfg, xo, us[:, 0], dt[0])
    return hist, xo


def test_rollout_with_scene_source_matches_oracle_pipeline(oracle_lib):
    """Past the pillar of scene_setup's world with its exact distance: u_0 of every step of every instance within
    U0_ATOL of the CPU loop (oracle.linearize_batch, the SDF row from scene_sdf_ref, the C IPM, the oracle's integrator).
    Measured on the MI355X: see DESIGN §3.17."""
    O = oracle_lib
    cfg = Config(mpc__N=10)
    n = Nmpc(cfg, batch=B)
    x0 = _start(n)
    scene = Scene(n.ocp.ctx, WORLD)
    n.set_sdf_scene(scene)
    onet = O.Net(W.DEFAULT_SPEC, W.siren_weights(W.DEFAULT_SPEC, seed=0))
    hist, x_end = oracle_loop(O, onet, n, cfg, WORLD, x0, K_ORACLE, n.model.max_df)
    # on the CPU loop alone: the SDF row is active at some step and released at the last one, and nothing is hit
    bound = n.model.lh[n.model.h_cols.index(2)]
    active = np.array([(h["sdf_slack"] > 1e-6) | (h["h2min"] <= bound + 1e-6) for h in hist])  # [K, B]
    xo = np.stack([h["x0"] for h in hist] + [x_end], 1)
    clear = np.stack([R.distance(WORLD, xo[b, :, :3]) for b in range(B)])
    print(f"\nCPU loop: SDF row active at steps {[int(a.sum()) for a in active.T]} per instance, h2min per step "
          f"{np.round([h['h2min'].min() for h in hist], 3).tolist()}, min clearance {clear.min():.3f} m, final x {x_end[:, 0]}")
    assert active.any() and not active[-1].any()
    assert clear.min() > 0
    n.set_x0(x0)
    r = n.rollout(K_ORACLE)
    uo = np.stack([h["u0"] for h in hist], 1)
    d = np.abs(r.u - uo).max(axis=(0, 2))
    print(f"max |u0 - u0_oracle| per step {d}")
    assert (r.status == 0).all()
    assert d.max() <= U0_ATOL, d
    np.testing.assert_allclose(r.clearance, np.stack([R.distance(WORLD, r.x[b, :, :3]) for b in range(B)]), rtol=0, atol=1e-12)
    n.ocp.close()


def test_set_sdf_scene_none_restores_the_network():
    """test_gpu_rollout's scenario (hover references, shift 1) through the old signature: on a controller that never
    had a source, and on one that had one set, flew with it and dropped it -- the same bits; with the source, others."""
    cfg = Config(mpc__N=10, mpc__shift=1)
    n, x0 = _setup(cfg, B, 21)
    n.set_x0(x0)
    before = n.rollout(3, refs="hover")
    m, _ = _setup(cfg, B, 21)
    scene = Scene(m.ocp.ctx, R.SCENE)
    m.set_sdf_scene(scene)
    m.set_x0(x0)
    with_src = m.rollout(3, refs="hover")
    m.set_sdf_scene(None)
    # the controller as _setup leaves it: reset() marks every host region for upload (the source's rollout rewrote the
    # pose columns on the device) and the next set_x0 initialises the iterate again
    m.reset()
    m.p[...], m.y[...], m.W[...], m.yN[...], m.WN[...] = n.p, n.y, n.W, n.yN, n.WN
    m.set_x0(x0)
    after = m.rollout(3, refs="hover")
    for k in ("x", "u", "status", "iters"):
        np.testing.assert_array_equal(getattr(before, k), getattr(after, k))
    np.testing.assert_array_equal(n.ocp.download("p"), m.ocp.download("p"))
    assert before.clearance is None and after.clearance is None and with_src.clearance is not None
    assert (with_src.u != before.u).any()
    n.ocp.close()
    m.ocp.close()


def test_batch_split_over_parts_refuses_a_scene_source(monkeypatch):
    """An Ocp with more than one part (test_gpu_rollout's way to one on a single device: a capacity of two instances
    per device slot): set_sdf_scene is a ValueError with x0, the iterate and p of every part untouched, no part's solver
    has a source afterwards, and rollout() keeps its own refusal of a split batch."""
    from sdf_nmpc_amd import ocp as ocp_mod
    from sdf_nmpc_amd import shard
    from sdf_nmpc_amd.model import Quad
    cfg = Config(mpc__N=10)
    plan = shard.plan
    monkeypatch.setattr(shard, "plan", lambda total, capacity, n_dev: plan(total, 2, n_dev))
    o = ocp_mod.Ocp(Quad(cfg), batch=4, devices=[0, 0])
    assert len(o.parts) == 2
    m = Nmpc(cfg, batch=4, ocp=o)
    x0 = np.zeros((4, 10))
    x0[:, :3] = np.random.default_rng(2).uniform(-1, 1, (4, 3))
    x0[:, 3] = 1.0
    m.set_sdf_flag(1.0)
    m.set_latent(np.random.default_rng(3).normal(0, 1, (4, 128)), x0[:, :3], np.stack([np.eye(3)] * 4))
    r = Ref(cfg)
    r.p, r.q = np.array([0.5, -0.4, 0.3]), yaw2quat(0.4)
    r.use_weights(r.W_on)
    for k in range(m.N + 1):
        m.set_ref(r, k)
    m.set_x0(x0)
    m.solve()  # flush the host setters, so that the device fields are settled
    before = {k: o.download(k) for k in ("x", "u", "p", "x0")}
    scenes = [Scene(part.ctx, R.SCENE) for part in o.parts]  # on either part's context
    for sc in scenes:
        for kw in (dict(), dict(predict=True), dict(max_df=0.5)):
            with pytest.raises(ValueError, match="split"):
                m.set_sdf_scene(sc, **kw)
            for part in o.parts:
                part.ctx.synchronize()
            np.testing.assert_array_equal(m.x0, x0)
            for k, v in before.items():
                np.testing.assert_array_equal(o.download(k), v)
    with pytest.raises(ValueError, match="split"):
        m.set_sdf_scene(None)
    assert m._sdf_scene is None
    plant = _lib.plant_opts(cfg, dt=float(o.dt[0]))
    for part in o.parts:  # no part's solver took a source: the library refuses the source's rollout for it
        nb = part.hi - part.lo
        xl, ul = _lib.DeviceArray(part.ctx, (nb, 3, 10)), _lib.DeviceArray(part.ctx, (nb, 2, 4))
        with pytest.raises(_lib.SdfnmpcError, match="no scene source"):
            part.solver.rollout_scene_sdf(2, plant, xl, ul)
    with pytest.raises(ValueError, match="split"):  # and rollout() keeps its existing refusal
        m.rollout(2)
    for k, v in before.items():
        np.testing.assert_array_equal(o.download(k), v)
    m.set_x0(x0)
    m.solve()  # the controller still steps, with the network
    assert (o.status < 2).all() and np.isfinite(m.get_u()).all()
    for sc in scenes:
        sc.close()
    o.close()


def test_api_contract():
    """Every ValueError is raised with x0, the iterate and p untouched; the C refusals launch nothing."""
    cfg = Config(mpc__N=10)
    n, x0 = _setup(cfg, B, 21)
    ctx = n.ocp.ctx
    n.set_x0(x0)
    n.rollout(1)  # flush the host setters, so that the device fields are settled
    x0 = n.x0.copy()
    before = {k: n.ocp.download(k) for k in ("x", "u", "p", "x0")}

    def untouched():
        ctx.synchronize()
        np.testing.assert_array_equal(n.x0, x0)
        for k, v in before.items():
            np.testing.assert_array_equal(n.ocp.download(k), v)

    other_ctx = _lib.Context(ctx.device)
    elsewhere = Scene(other_ctx, R.SCENE)
    scene = Scene(ctx, R.SCENE)
    for bad in (elsewhere, Scene(ctx, [R.SCENE, OTHER], scene_of=[0, 1])):  # another context; scene_of for 2 of 3
        with pytest.raises(ValueError):
            n.set_sdf_scene(bad)
        untouched()
    for md in (0.0, -1.0, float("nan"), float("inf")):
        with pytest.raises(ValueError):
            n.set_sdf_scene(scene, max_df=md)
    with pytest.raises(ValueError):
        n.set_scene_time(float("nan"))
    m = Nmpc(Config(mpc__N=10, flags__enable_sdf=False), batch=B)  # a model whose flags read no SDF
    ms = Scene(m.ocp.ctx, R.SCENE)
    with pytest.raises(ValueError):
        m.set_sdf_scene(ms)
    with pytest.raises(_lib.SdfnmpcError, match="error -1"):  # and the library's own refusal of it
        m.ocp.parts[0].solver.set_sdf_scene(ms.h, None, 1.0)
    ms.close()
    m.ocp.close()
    untouched()
    # with a source: what excludes it, and the schedule / clock checks
    n.set_sdf_scene(scene)
    for kw in (dict(scene=scene, vae=object()), dict(vae=object()), dict(sensor=object()), dict(perceive_every=0),
               dict(perceive_phase=-1), dict(scene_t0=float("nan")), dict(scene_dt=-0.1), dict(scene_dt=float("inf"))):
        with pytest.raises(ValueError):
            n.rollout(2, refs="hover", **kw)
        untouched()
    # the library's refusals, reached by going around the method's checks: nothing is launched
    solver = n.ocp.parts[0].solver
    plant = _lib.plant_opts(cfg, dt=float(n.ocp.dt[0]))
    xl, ul = _lib.DeviceArray.from_numpy(ctx, np.full((B, 3, 10), -7.0)), _lib.DeviceArray(ctx, (B, 2, 4))
    ws = {k: _lib.DeviceArray.from_numpy(ctx, np.full((B, w), -7.0)) for k, w in (("W_p_Bo", 3), ("W_R_Bo", 9),
                                                                               ("W_p_C", 3), ("W_R_C", 9))}
    s = cfg.sensor

    def pose(every=1, **null):
        return _lib.PoseRefreshArgsC(every, (_lib.C.c_double * 3)(*[float(v) for v in np.asarray(s.B_p_C, float).ravel()]),
                                     (_lib.C.c_double * 9)(*[float(v) for v in np.asarray(s.B_R_C, float).ravel()]),
                                     *[None if k in null else ws[k].data_ptr() for k in ("W_p_Bo", "W_R_Bo", "W_p_C", "W_R_C")])

    def refused(code="error -1", steps=2, x_log=xl, **kw):
        with pytest.raises(_lib.SdfnmpcError, match=code):
            solver.rollout_scene_sdf(steps, plant, x_log, ul, **kw)
        untouched()
        np.testing.assert_array_equal(xl.numpy(), np.full((B, 3, 10), -7.0))
        for v in ws.values():
            assert (v.numpy() == -7.0).all()

    refused(pose=pose(every=0))
    refused(pose=pose(), phase=-1)
    refused(pose=pose(W_R_C=1))
    refused(pose=pose(W_p_Bo=1))
    for clock in (dict(t0=float("nan")), dict(dt=float("inf")), dict(dt=-0.1)):
        refused(pose=pose(), **clock)
    refused(pose=pose(), steps=0)        # what sdfnmpc_solver_rollout refuses
    refused(pose=pose(), x_log=None)
    n.set_sdf_scene(None)
    refused(pose=pose())                 # no source set on the solver
    with pytest.raises(_lib.SdfnmpcError, match="error -1"):
        solver.set_sdf_scene(elsewhere.h, None, 1.0)
    # pack_refs: the pose-only mode needs the pose
    with pytest.raises(_lib.SdfnmpcError, match="error -1"):
        _lib.pack_refs(ctx, _lib.ref_opts(cfg, -2), B, n.N, n.model.np, n.model.ny, {"p": n.ocp.field("p")})
    untouched()
    n.set_sdf_scene(scene)
    r = n.rollout(2, refs="hover")  # and it still runs afterwards
    assert r.clearance.shape == (B, 3) and r.t.shape == (3,)
    # the solver holds the scene's handle: closing the scene while it is the source returns to the network first
    scene.close()
    assert n._sdf_scene is None
    with pytest.raises(_lib.SdfnmpcError, match="no scene source"):
        solver.rollout_scene_sdf(2, plant, xl, ul)
    r = n.rollout(2, refs="hover")
    assert r.clearance is None and np.isfinite(r.u).all()
    elsewhere.close()
    other_ctx.close()
    n.ocp.close()
