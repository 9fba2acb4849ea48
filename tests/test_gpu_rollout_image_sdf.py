"""Closed-loop rollouts of a controller whose SDF is the distance field of its own camera image (Nmpc.set_sdf_image,
sdfnmpc_solver_rollout_image_sdf): bitwise against the host-driven loop render_from_state / sensor.apply / set_sdf_image /
set_pose_device / gen_refs_device / solve / plant_step (static and moving scenes, a sensor model, the unsigned field,
chunks), a static image against K solve calls, the way back to the network, the refusals, and the behaviour on the
pillar approach of tests/test_gpu_rollout_scene_sdf.py.  N = 10, B = 3, K <= 12, images 30 x 40."""
import numpy as np
import pytest

import scene_dyn_ref as D
import scene_ref as R
import scene_setup as S
from sdf_nmpc_amd import _lib
from sdf_nmpc_amd.config import Config
from sdf_nmpc_amd.controller import Nmpc
from sdf_nmpc_amd.reference import Ref, yaw2quat
from sdf_nmpc_amd.scene import Scene
from sdf_nmpc_amd.sensor import SensorModel
from test_gpu_rollout import _setup

pytestmark = [pytest.mark.gpu, pytest.mark.filterwarnings("ignore:no SDF weights"),
              pytest.mark.filterwarnings("ignore:QP reached")]

B, K = 3, 6
SHAPE = (30, 40)
SCENE_OF = np.array([1, 0, 1], np.int32)
OTHER = [("sphere", [1.5, 0.5, 0.2, 0.5]), ("box", [-2.0, -2.5, -1.0, 2.0, -1.5, 1.0])]
T0 = 0.5
WORLD = [("cylinder", [3.0, 0.3, 0.4, -3.0, 3.0]), ("box", [5.0, -2.5, -3.0, 5.6, -0.8, 3.0])]
K_APPROACH = 12
X_START, V_START, Y_START = 1.5, 1.5, np.array([0.8, -0.3, 1.0])


@pytest.fixture(scope="module", autouse=True)
def _torch_first(gpu_ctx):
    """torch opens the device before the first controller of this module does, as in tests/test_gpu_rollout.py."""


def _wps():
    rng = np.random.default_rng(5)
    return (rng.uniform(-2, 2, (B, 2, 3)), np.stack([[yaw2quat(a) for a in row] for row in rng.uniform(-1, 1, (B, 2))]))


def _dyn_prims():
    return [Scene.moving(p, **kw) if kw is not None else p for p, kw in D.SPEC]


def _make(cfg, dynamic=False, signed=True, seed=21):
    """A controller (test_gpu_rollout's setup: flag on, one goal) with an image source, two scenes of which instances 0
    and 2 see the fixture (static or moving); the source starts from the image at the start state."""
    n, x0 = _setup(cfg, B, seed)
    scene = Scene(n.ocp.ctx, [OTHER, _dyn_prims() if dynamic else R.SCENE], scene_of=SCENE_OF)
    n.set_sdf_image(scene.render_from_state(x0, cfg, SHAPE, normalized=True, t=T0), signed=signed)
    return n, x0, scene


def _sensor(cfg, ctx):
    return SensorModel(cfg, ctx, 7, noise_std=0.02, noise_std_quad=0.002, dropout=0.05)


def _host_loop(n, scene, x0, steps, every, wps, signed=True, sensor=None, t0=T0, dts=None, phase=0):
    """The loop a user writes around solve() with an image source: every `every`-th step a new normalised image from
    the state, degraded as frame phase + k, handed to the source, and its pose into p; the references, the step, the
    plant."""
    ctx = n.ocp.ctx
    dt = float(n.ocp.dt[0])
    dts = dt if dts is None else dts
    plant = _lib.plant_opts(n.cfg, dt=dt)
    dx = _lib.DeviceArray(ctx, (B, 10))
    xs, us, its, sts = [np.reshape(x0, (B, 10)).copy()], [], [], []
    for k in range(steps):
        n.set_x0(xs[-1])
        if (k + phase) % every == 0:
            img = scene.render_from_state(xs[-1], n.cfg, SHAPE, normalized=True, t=t0 + (phase + k) * dts)
            if sensor is not None:
                sensor.apply(img, phase + k, normalized=True)
            n.set_sdf_image(img, signed=signed)
            n.set_pose_device(img.pose["W_p_Bo"], img.pose["W_R_Bo"])
        n.gen_refs_device("wps", wps=wps)
        n.solve()
        us.append(n.ocp.field("u0").numpy().reshape(B, 4))
        its.append(n.ocp.iters.copy())
        sts.append(n.ocp.status.copy())
        dx.upload(xs[-1])
        _lib.plant_step(ctx, plant, B, dx, n.ocp.field("u0"), dx)
        xs.append(dx.numpy())
    return np.stack(xs, 1), np.stack(us, 1), np.stack(sts, 1), np.stack(its, 1)


@pytest.mark.parametrize("dynamic,every,signed,noisy", [(False, 1, True, False), (False, 3, True, False), (True, 2, True, False),
                                                        (False, 2, True, True), (False, 1, False, False)])
def test_rollout_with_image_source_equals_host_driven_loop_bitwise(dynamic, every, signed, noisy):
    cfg = Config(mpc__N=10)
    wps = _wps()
    na, x0, sa = _make(cfg, dynamic, signed)
    nb, _, sb = _make(cfg, dynamic, signed)
    assert sa.is_dynamic == dynamic
    sens = (lambda n: _sensor(cfg, n.ocp.ctx)) if noisy else (lambda n: None)
    dts = 0.2 if dynamic else None
    na.set_x0(x0)
    r = na.rollout(K, refs="wps", wps=wps, scene=sa, sensor=sens(na), perceive_every=every, scene_t0=T0, scene_dt=dts,
                   img_shape=SHAPE, keep_img=True)
    x, u, status, iters = _host_loop(nb, sb, x0, K, every, wps, signed, sens(nb), dts=dts)
    np.testing.assert_array_equal(r.x, x)
    np.testing.assert_array_equal(r.u, u)
    np.testing.assert_array_equal(r.status, status)
    np.testing.assert_array_equal(r.iters, iters)
    np.testing.assert_array_equal(na.ocp.download("p"), nb.ocp.download("p"))
    last = nb._sdf_image["images"].numpy()
    np.testing.assert_array_equal(r.img, last)  # the image the source last held
    np.testing.assert_array_equal(na._sdf_image["images"].numpy(), last)
    assert (r.iters > 0).all() and np.ptp(r.u[:, :, 0]) > 1e-3
    # keep_img is the sensor's output of the last render, bitwise
    k_last = (K - 1) // every * every
    dt = float(na.ocp.dt[0])
    want = sb.render_from_state(r.x[:, k_last], cfg, SHAPE, normalized=True, t=T0 + k_last * (dt if dts is None else dts))
    if noisy:
        exact = want.numpy()
        _sensor(cfg, nb.ocp.ctx).apply(want, k_last, normalized=True)
        assert (want.numpy() != exact).any()
    np.testing.assert_array_equal(r.img, want.numpy())
    # the image reached the rows, and the clearance is the scene's
    h = na.ocp.download("h")
    assert np.isfinite(h[..., 2]).all()
    assert r.clearance.shape == (B, K + 1) and np.isfinite(r.clearance).all()
    np.testing.assert_array_equal(r.t, T0 + np.arange(K + 1) * (dt if dts is None else dts))
    if not signed:
        np.testing.assert_array_equal(na._sdf_image["pooled"].numpy(), nb._sdf_image["pooled"].numpy())
        assert (h[..., 2] >= 0).all()
    for m in (na, nb):
        m.ocp.close()


def test_chunks_with_phase_are_the_uncut_rollout():
    """K one-step chunks with perceive_phase = k: the imaging schedule, the sensor's frames and the scene's clock of the
    uncut rollout."""
    cfg = Config(mpc__N=10)
    wps = _wps()
    n, x0, sn = _make(cfg, dynamic=True)
    n.set_x0(x0)
    kw = dict(refs="wps", wps=wps, perceive_every=2, scene_t0=T0, img_shape=SHAPE, keep_img=True)
    xs, us = [np.reshape(x0, (B, 10))], []
    for k in range(K):
        r = n.rollout(1, scene=sn, sensor=_sensor(cfg, n.ocp.ctx), perceive_phase=k, **kw)
        xs.append(r.x[:, 1])
        us.append(r.u[:, 0])
    m, _, sm = _make(cfg, dynamic=True)
    m.set_x0(x0)
    whole = m.rollout(K, scene=sm, sensor=_sensor(cfg, m.ocp.ctx), **kw)
    np.testing.assert_array_equal(whole.x, np.stack(xs, 1))
    np.testing.assert_array_equal(whole.u, np.stack(us, 1))
    np.testing.assert_array_equal(m.ocp.download("p"), n.ocp.download("p"))
    np.testing.assert_array_equal(whole.img, r.img)
    n.ocp.close()
    m.ocp.close()


def test_static_image_rollout_equals_solve_calls():
    """Without scene= the image and the pose stay as set: K steps of the rollout are K host solve calls; imgs= labelling
    still works beside the source."""
    cfg = Config(mpc__N=10)
    na, x0, sa = _make(cfg)
    nb, _, _ = _make(cfg)
    img = sa.render_from_state(x0, cfg, SHAPE, normalized=True).numpy()
    na.set_x0(x0)
    r = na.rollout(K, refs="hover", imgs=img)
    ctx = nb.ocp.ctx
    plant = _lib.plant_opts(cfg, dt=float(nb.ocp.dt[0]))
    dx = _lib.DeviceArray(ctx, (B, 10))
    xs, us = [x0.copy()], []
    for _ in range(K):
        nb.set_x0(xs[-1])
        nb.gen_refs_device("hover")
        nb.solve()
        us.append(nb.ocp.field("u0").numpy().reshape(B, 4))
        dx.upload(xs[-1])
        _lib.plant_step(ctx, plant, B, dx, nb.ocp.field("u0"), dx)
        xs.append(dx.numpy())
    np.testing.assert_array_equal(r.x, np.stack(xs, 1))
    np.testing.assert_array_equal(r.u, np.stack(us, 1))
    assert r.clearance is None and r.col.shape == (B, K + 1) and r.pts.shape == (B, K + 1, 3)
    for m in (na, nb):
        m.ocp.close()


def test_sources_replace_each_other_and_none_restores_the_network():
    """A controller that flew with a scene source, then an image source, then dropped it, gives the bits of one that
    never had a source; with the image source, others."""
    cfg = Config(mpc__N=10, mpc__shift=1)
    n, x0 = _setup(cfg, B, 21)
    n.set_x0(x0)
    before = n.rollout(3, refs="hover")
    m, _ = _setup(cfg, B, 21)
    scene = Scene(m.ocp.ctx, R.SCENE)
    m.set_sdf_scene(scene)
    m.set_x0(x0)
    with_scene = m.rollout(3, refs="hover")
    m.set_sdf_image(scene.render_from_state(x0, cfg, SHAPE, normalized=True))
    assert m._sdf_scene is None and m._sdf_image is not None and not scene._sdf_users
    m.reset()
    m.p[...], m.y[...], m.W[...], m.yN[...], m.WN[...] = n.p, n.y, n.W, n.yN, n.WN
    m.set_x0(x0)
    with_image = m.rollout(3, refs="hover")
    m.set_sdf_scene(scene)  # and back: the image source is gone
    assert m._sdf_image is None and m._sdf_scene is scene
    m.set_sdf_image(scene.render_from_state(x0, cfg, SHAPE, normalized=True), signed=False)
    m.set_sdf_image(None)
    assert m._sdf_image is None and m._sdf_scene is None
    m.reset()
    m.p[...], m.y[...], m.W[...], m.yN[...], m.WN[...] = n.p, n.y, n.W, n.yN, n.WN
    m.set_x0(x0)
    after = m.rollout(3, refs="hover")
    for k in ("x", "u", "status", "iters"):
        np.testing.assert_array_equal(getattr(before, k), getattr(after, k))
    np.testing.assert_array_equal(n.ocp.download("p"), m.ocp.download("p"))
    assert before.clearance is None and after.clearance is None and with_image.clearance is None
    assert (with_image.u != before.u).any() and (with_image.u != with_scene.u).any()
    scene.close()
    n.ocp.close()
    m.ocp.close()


def test_batch_split_over_parts_refuses_an_image_source(monkeypatch):
    """An Ocp with two parts on one device: set_sdf_image is a ValueError with x0, the iterate and p untouched."""
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
    m.solve()
    before = {k: o.download(k) for k in ("x", "u", "p", "x0")}
    img = np.full((4,) + SHAPE, 0.5, np.float32)
    for kw in (dict(), dict(signed=False), dict(max_df=0.5)):
        with pytest.raises(ValueError, match="split"):
            m.set_sdf_image(img, **kw)
    with pytest.raises(ValueError, match="split"):
        m.set_sdf_image(None)
    for part in o.parts:
        part.ctx.synchronize()
    np.testing.assert_array_equal(m.x0, x0)
    for k, v in before.items():
        np.testing.assert_array_equal(o.download(k), v)
    assert m._sdf_image is None
    plant = _lib.plant_opts(cfg, dt=float(o.dt[0]))
    for part in o.parts:  # no part's solver took a source
        nb = part.hi - part.lo
        xl, ul = _lib.DeviceArray(part.ctx, (nb, 3, 10)), _lib.DeviceArray(part.ctx, (nb, 2, 4))
        with pytest.raises(_lib.SdfnmpcError, match="no image source"):
            part.solver.rollout_image_sdf(2, plant, xl, ul)
    o.close()


def test_api_contract():
    """Every ValueError is raised with x0, the iterate and p untouched; the C refusals launch nothing."""
    cfg = Config(mpc__N=10)
    n, x0 = _setup(cfg, B, 21)
    ctx = n.ocp.ctx
    n.set_x0(x0)
    n.rollout(1)
    x0 = n.x0.copy()
    before = {k: n.ocp.download(k) for k in ("x", "u", "p", "x0")}

    def untouched():
        ctx.synchronize()
        np.testing.assert_array_equal(n.x0, x0)
        for k, v in before.items():
            np.testing.assert_array_equal(n.ocp.download(k), v)

    img = np.full((B,) + SHAPE, 0.5, np.float32)
    for bad in (dict(imgs=img[:2]), dict(imgs=np.full((B, 31, 40), 0.5, np.float32), signed=False),
                dict(imgs=np.full((B, 30, 41), 0.5, np.float32), signed=False), dict(imgs=img, max_df=0.0),
                dict(imgs=img, max_df=float("nan")), dict(imgs=img[:2], img_of=[0, 1, 2]), dict(imgs=img, img_of=[0, 1]),
                dict(imgs=img[0, 0])):
        with pytest.raises(ValueError):
            n.set_sdf_image(**bad)
        untouched()
    assert n._sdf_image is None
    m = Nmpc(Config(mpc__N=10, flags__enable_sdf=False), batch=B)  # a model whose flags read no SDF
    with pytest.raises(ValueError):
        m.set_sdf_image(img)
    o = _lib.img_sdf_opts(_lib.img_opts(5.0, 0.7, 0.5), _lib.DeviceArray.from_numpy(m.ocp.ctx, img), False,
                          pooled=_lib.DeviceArray(m.ocp.ctx, (B, 6, 8), np.float32))
    with pytest.raises(_lib.SdfnmpcError, match="error -1"):  # and the library's own refusal of it
        m.ocp.parts[0].solver.set_sdf_image(o)
    m.ocp.close()
    scene = Scene(ctx, R.SCENE)
    other_ctx = _lib.Context(ctx.device)
    elsewhere = Scene(other_ctx, R.SCENE)
    n.set_sdf_image(img[:2], img_of=[1, 0, 1])  # any number of images with a map
    with pytest.raises(ValueError):             # but re-imaging renders one per instance
        n.rollout(2, refs="hover", scene=scene, img_shape=SHAPE)
    untouched()
    n.set_sdf_image(img)
    for kw in (dict(vae=object()), dict(scene=scene, vae=object()), dict(sensor=object()), dict(scene=elsewhere),
               dict(scene=scene, img_shape=(30, 45)), dict(img_shape=(35, 40)), dict(scene=scene, imgs=img),
               dict(scene=scene, perceive_every=0), dict(scene=scene, perceive_phase=-1), dict(scene=scene, scene_t0=float("nan")),
               dict(scene=scene, scene_dt=-0.1), dict(scene=scene, sensor=_sensor(cfg, other_ctx))):
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
    held = n._sdf_image["images"].numpy()

    def perc(every=1, phase=0, h=SHAPE[0], w=SHAPE[1], scene_h=scene.h, **null):
        return _lib.PerceiveArgsC(scene_h, None, scene.img_opts(cfg), h, w, scene.scale(cfg, normalized=True),
                                  (_lib.C.c_double * 3)(*[float(v) for v in np.asarray(s.B_p_C, float).ravel()]),
                                  (_lib.C.c_double * 9)(*[float(v) for v in np.asarray(s.B_R_C, float).ravel()]), None,
                                  _lib.VaeOptsC(), every, phase, None, None, None,
                                  *[None if k in null else ws[k].data_ptr() for k in ("W_p_Bo", "W_R_Bo", "W_p_C", "W_R_C")])

    def refused(code="error -1", steps=2, x_log=xl, **kw):
        with pytest.raises(_lib.SdfnmpcError, match=code):
            solver.rollout_image_sdf(steps, plant, x_log, ul, **kw)
        untouched()
        np.testing.assert_array_equal(xl.numpy(), np.full((B, 3, 10), -7.0))
        np.testing.assert_array_equal(n._sdf_image["images"].numpy(), held)
        for v in ws.values():
            assert (v.numpy() == -7.0).all()

    refused(perceive=perc(every=0))
    refused(perceive=perc(phase=-1))
    refused(perceive=perc(h=35))          # the render size must equal the source's
    refused(perceive=perc(w=45))
    refused(perceive=perc(scene_h=None))
    refused(perceive=perc(scene_h=elsewhere.h))
    refused(perceive=perc(W_R_C=1))
    refused(sensor=_sensor(cfg, ctx).opts(B, *SHAPE, normalized=True))  # a sensor without re-imaging
    for clock in (dict(t0=float("nan")), dict(dt=float("inf")), dict(dt=-0.1)):
        refused(perceive=perc(), **clock)
    refused(perceive=perc(), steps=0)     # what sdfnmpc_solver_rollout refuses
    refused(perceive=perc(), x_log=None)
    n.set_sdf_scene(scene)                # a scene source is not an image source
    with pytest.raises(_lib.SdfnmpcError, match="no image source"):
        solver.rollout_image_sdf(2, plant, xl, ul, perceive=perc())
    n.set_sdf_image(None)
    with pytest.raises(_lib.SdfnmpcError, match="no image source"):
        solver.rollout_image_sdf(2, plant, xl, ul)
    untouched()
    n.set_sdf_image(img)
    r = n.rollout(2, refs="hover", scene=scene, img_shape=SHAPE)  # and it still runs afterwards
    assert r.clearance.shape == (B, 3) and r.t.shape == (3,) and r.img is None
    scene.close()                         # closing a scene that is no source changes nothing
    assert n._sdf_image is not None
    elsewhere.close()
    other_ctx.close()
    n.ocp.close()


# ---- behaviour
def _approach(n):
    x0 = S.setup(n, y0=Y_START)
    x0[:, 0] = X_START
    x0[:, 7] = V_START
    return x0


def test_image_source_keeps_clear_of_the_pillar():
    """test_gpu_rollout_scene_sdf.py's pillar approach (12 steps from 1.1 m at 1.5 m/s), on the image's own field and
    with the SDF flag off.  Measured on the MI355X: see DESIGN §3.18."""
    cfg = Config(mpc__N=10)
    res = {}
    for arm in ("image", "flag0"):
        n = Nmpc(cfg, batch=B)
        x0 = _approach(n)
        scene = Scene(n.ocp.ctx, WORLD)
        if arm == "flag0":
            n.set_sdf_flag(0.0)
        n.set_sdf_image(scene.render_from_state(x0, cfg, SHAPE, normalized=True))
        n.set_x0(x0)
        # one step at a time, to log h[2] and the QP's SDF slack of every step (chunks are the uncut rollout)
        clear, active = [], []
        bound = n.model.lh[n.model.h_cols.index(2)]
        for k in range(K_APPROACH):
            r = n.rollout(1, scene=scene, img_shape=SHAPE, perceive_phase=k)
            clear.append(r.clearance[:, 0])
            h2 = n.ocp.download("h")[..., 2]
            slack = n.ocp.download("slack").reshape(B, n.N + 1, 3, 2)[:, :, 2, 0]
            active.append((h2.min(axis=1) < bound + 1e-6) | (slack.max(axis=1) > 1e-6))
        clear.append(r.clearance[:, 1])
        res[arm] = (np.stack(clear, 1), np.array(active))
        scene.close()
        n.ocp.close()
    c_img, a_img = res["image"]
    c_off, a_off = res["flag0"]
    print(f"\nmin clearance per instance: image source {np.round(c_img.min(1), 3).tolist()}, flag 0 {np.round(c_off.min(1), 3).tolist()}; "
          f"overall {c_img.min():.3f} m against {c_off.min():.3f} m (exact source: 0.333 m); SDF row active at "
          f"{a_img.sum(0).tolist()} steps per instance")
    assert c_img.min() > 0
    assert a_img.any() and not a_off.any()
    assert c_off.min() < c_img.min()
