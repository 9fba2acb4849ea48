"""A scene that moves inside the device rollout (Nmpc.rollout(scene=, vae=, scene_t0=, scene_dt=),
sdfnmpc_solver_rollout_perceive_at): bitwise against the host-driven loop that renders with
render_from_state(..., t=scene_t0 + k * dt), the clock over a rollout cut into chunks, the clearance at the time of
every log row, and a static scene untouched by the clock.  The setup of tests/test_gpu_rollout_perceive.py: N = 10,
B = 3, K = 6, 18 x 32 images, two scenes of which one is dynamic, refs = 'wps'."""
import numpy as np
import pytest

import scene_dyn_ref as D
import scene_ref as R
from sdf_nmpc_amd import _lib
from sdf_nmpc_amd.config import Config
from sdf_nmpc_amd.scene import Scene
from sdf_nmpc_amd.vae import VaeWrapper
from test_gpu_rollout import _setup
from test_gpu_rollout_perceive import B, K, OTHER, SCENE_OF, SHAPE, _wps

pytestmark = [pytest.mark.gpu, pytest.mark.filterwarnings("ignore:no SDF weights"),
              pytest.mark.filterwarnings("ignore:QP reached")]

T0 = 0.5


@pytest.fixture(scope="module", autouse=True)
def _torch_first(gpu_ctx):
    """torch opens the device before the first controller of this module does, as in tests/test_gpu_rollout.py."""


def _dyn_prims():
    return [Scene.moving(p, **kw) if kw is not None else p for p, kw in D.SPEC]


def _make(cfg, seed=21, dynamic=True):
    """A controller, and a pair of scenes -- a static one and the moving fixture, which instances 0 and 2 see -- and an
    encoder on its context."""
    n, x0 = _setup(cfg, B, seed)
    ctx = n.ocp.ctx
    first = _dyn_prims() if dynamic else R.SCENE
    return n, x0, Scene(ctx, [OTHER, first], scene_of=SCENE_OF), VaeWrapper(cfg, batch=B, ctx=ctx)


def _host_loop(n, vae, scene, x0, steps, every, wps, t0):
    """The loop of tests/test_gpu_rollout_perceive.py with the scene's clock: the image before step k is rendered at
    t0 + k * dt."""
    ctx = n.ocp.ctx
    dt = float(n.ocp.dt[0])
    plant = _lib.plant_opts(n.cfg, dt=dt)
    dx = _lib.DeviceArray(ctx, (B, 10))
    xs, us, its, sts = [np.reshape(x0, (B, 10)).copy()], [], [], []
    for k in range(steps):
        n.set_x0(xs[-1])
        if k % every == 0:
            img = scene.render_from_state(xs[-1], n.cfg, SHAPE, normalized=False, t=t0 + k * dt)
            vae.set_img(img)
            vae.encode_to(n, img.pose["W_p_Bo"], img.pose["W_R_Bo"])
        n.gen_refs_device("wps", wps=wps)
        n.solve()
        us.append(n.ocp.field("u0").numpy().reshape(B, 4))
        its.append(n.ocp.iters.copy())
        sts.append(n.ocp.status.copy())
        dx.upload(xs[-1])
        _lib.plant_step(ctx, plant, B, dx, n.ocp.field("u0"), dx)
        xs.append(dx.numpy())
    return np.stack(xs, 1), np.stack(us, 1), np.stack(sts, 1), np.stack(its, 1)


@pytest.mark.parametrize("every", [1, 2])
def test_rollout_in_a_moving_scene_equals_host_driven_loop_bitwise(every):
    cfg = Config(mpc__N=10)
    wps = _wps()
    na, x0, sa, va = _make(cfg)
    nb, _, sb, vb = _make(cfg)
    assert sa.is_dynamic
    na.set_x0(x0)
    r = na.rollout(K, refs="wps", wps=wps, scene=sa, vae=va, perceive_every=every, img_shape=SHAPE, keep_img=True,
                   scene_t0=T0)
    x, u, status, iters = _host_loop(nb, vb, sb, x0, K, every, wps, T0)
    np.testing.assert_array_equal(r.x, x)
    np.testing.assert_array_equal(r.u, u)
    np.testing.assert_array_equal(r.status, status)
    np.testing.assert_array_equal(r.iters, iters)
    pa, pb = na.ocp.download("p"), nb.ocp.download("p")
    np.testing.assert_array_equal(pa, pb)
    assert np.abs(pa[:, :, 17:]).max() > 0 and np.ptp(r.u[:, :, 0]) > 1e-3
    # the last images: the last perceiving step's, of the scene at that step's time
    k_last = (K - 1) // every * every
    dt = float(na.ocp.dt[0])
    want = sb.render_from_state(r.x[:, k_last], cfg, SHAPE, normalized=False, t=T0 + k_last * dt).numpy()
    np.testing.assert_array_equal(r.img, want)
    stale = sb.render_from_state(r.x[:, k_last], cfg, SHAPE, normalized=False).numpy()
    assert (r.img != stale).any()  # the clock reached the kernel
    np.testing.assert_array_equal(va.latent64.numpy(), vb.latent64.numpy())
    for m in (na, nb):
        m.ocp.close()


def test_chunks_keep_the_clock():
    """Six one-step chunks with perceive_phase = k are the uncut rollout, bit for bit: x, p, t and the clearance."""
    cfg = Config(mpc__N=10)
    wps = _wps()
    n, x0, sc, vae = _make(cfg)
    n.set_x0(x0)
    xs, ts, cl = [np.reshape(x0, (B, 10))], [], []
    for k in range(K):
        r = n.rollout(1, refs="wps", wps=wps, scene=sc, vae=vae, perceive_every=2, img_shape=SHAPE, perceive_phase=k,
                      scene_t0=T0)
        xs.append(r.x[:, 1])
        ts.append(r.t)
        cl.append(r.clearance)
    m, _, sc2, vae2 = _make(cfg)
    m.set_x0(x0)
    whole = m.rollout(K, refs="wps", wps=wps, scene=sc2, vae=vae2, perceive_every=2, img_shape=SHAPE, scene_t0=T0)
    np.testing.assert_array_equal(whole.x, np.stack(xs, 1))
    np.testing.assert_array_equal(m.ocp.download("p"), n.ocp.download("p"))
    for k in range(K):
        np.testing.assert_array_equal(ts[k], whole.t[k:k + 2])
        np.testing.assert_array_equal(cl[k], whole.clearance[:, k:k + 2])
    n.ocp.close()
    m.ocp.close()


def test_clearance_is_measured_at_the_time_of_every_row():
    cfg = Config(mpc__N=10)
    n, x0, sc, vae = _make(cfg)
    n.set_x0(x0)
    dt = float(n.ocp.dt[0])
    r = n.rollout(K, refs="wps", wps=_wps(), scene=sc, vae=vae, perceive_every=3, img_shape=SHAPE, scene_t0=T0,
                  perceive_phase=2, scene_dt=0.3)
    assert r.t.shape == (K + 1,) and r.t.dtype == np.float64
    np.testing.assert_array_equal(r.t, np.array([T0 + (2 + j) * 0.3 for j in range(K + 1)]))
    assert r.clearance.shape == (B, K + 1) and r.clearance.dtype == np.float64
    pts = r.x[:, :, :3].reshape(-1, 3)
    p2s = np.repeat(SCENE_OF, K + 1)
    np.testing.assert_array_equal(r.clearance.ravel(), sc.distance(pts, p2s, t=np.tile(r.t, B)))
    scenes = [OTHER, D.scene()]
    want = np.stack([D.distance(scenes[s], r.x[b, :, :3], r.t) for b, s in enumerate(SCENE_OF)])
    print(f"\nclearance: max error {np.abs(r.clearance - want).max():.2e}")
    assert np.abs(r.clearance - want).max() <= 1e-12
    frozen = sc.distance(pts, p2s).reshape(B, K + 1)
    print(f"clearance at t[j] against the frozen scene: up to {np.abs(r.clearance - frozen).max():.3f} m apart")
    assert np.abs(r.clearance - frozen).max() > 0.1
    # the default period is the plant's
    n.set_x0(x0)
    r = n.rollout(2, refs="wps", wps=_wps(), scene=sc, vae=vae, img_shape=SHAPE, scene_t0=T0)
    np.testing.assert_array_equal(r.t, np.array([T0, T0 + dt, T0 + 2 * dt]))
    n.ocp.close()


def test_static_scene_ignores_the_clock():
    cfg = Config(mpc__N=10)
    wps = _wps()
    na, x0, sa, va = _make(cfg, dynamic=False)
    nb, _, sb, vb = _make(cfg, dynamic=False)
    assert not sa.is_dynamic
    na.set_x0(x0)
    nb.set_x0(x0)
    a = na.rollout(K, refs="wps", wps=wps, scene=sa, vae=va, perceive_every=2, img_shape=SHAPE, keep_img=True,
                   scene_t0=T0, scene_dt=0.2)
    b = nb.rollout(K, refs="wps", wps=wps, scene=sb, vae=vb, perceive_every=2, img_shape=SHAPE, keep_img=True)
    for k in ("x", "u", "status", "iters", "img", "clearance"):
        np.testing.assert_array_equal(getattr(a, k), getattr(b, k))
    np.testing.assert_array_equal(na.ocp.download("p"), nb.ocp.download("p"))
    np.testing.assert_array_equal(a.t, T0 + np.arange(K + 1) * 0.2)
    np.testing.assert_array_equal(b.t, np.arange(K + 1) * float(nb.ocp.dt[0]))
    na.ocp.close()
    nb.ocp.close()


def test_clock_api_contract():
    """Every new ValueError is raised before anything is uploaded or enqueued; so are the C entry point's refusals."""
    cfg = Config(mpc__N=10)
    n, x0, sc, vae = _make(cfg)
    n.set_x0(x0)
    n.rollout(1)  # flush the host setters, so that the device fields are settled
    x0 = n.x0.copy()
    before = {k: n.ocp.download(k) for k in ("x", "u", "p", "x0")}
    for kw in (dict(scene_t0=float("nan")), dict(scene_t0=float("inf")), dict(scene_dt=-0.1), dict(scene_dt=float("nan")),
               dict(scene_dt=float("inf"))):
        with pytest.raises(ValueError):
            n.rollout(2, refs="wps", wps=_wps(), scene=sc, vae=vae, img_shape=SHAPE, **kw)
        np.testing.assert_array_equal(n.x0, x0)
        for k, v in before.items():
            np.testing.assert_array_equal(n.ocp.download(k), v)
    # the library's own refusals, reached by going around the method's checks
    solver = n.ocp.parts[0].solver
    plant = _lib.plant_opts(cfg, dt=float(n.ocp.dt[0]))
    ctx = n.ocp.ctx
    xl, ul = _lib.DeviceArray.from_numpy(ctx, np.full((B, 3, 10), -7.0)), _lib.DeviceArray(ctx, (B, 2, 4))
    ws = {k: _lib.DeviceArray(ctx, (B, m)) for k, m in (("W_p_Bo", 3), ("W_R_Bo", 9), ("W_p_C", 3), ("W_R_C", 9))}
    img = _lib.DeviceArray(ctx, (B,) + SHAPE, np.float32)
    s = cfg.sensor
    perc = _lib.PerceiveArgsC(sc.h, _lib._ptr(sc._scene_of), sc.img_opts(cfg), SHAPE[0], SHAPE[1],
                              sc.scale(cfg, normalized=False),
                              (_lib.C.c_double * 3)(*[float(v) for v in np.asarray(s.B_p_C, float).ravel()]),
                              (_lib.C.c_double * 9)(*[float(v) for v in np.asarray(s.B_R_C, float).ravel()]),
                              vae.vae.h, _lib.VaeOptsC(B, SHAPE[0], SHAPE[1], 0, float(vae.opts.clip), None), 1, 0,
                              img.data_ptr(), vae.latent.data_ptr(), vae.latent64.data_ptr(),
                              *[ws[k].data_ptr() for k in ("W_p_Bo", "W_R_Bo", "W_p_C", "W_R_C")])
    for clock in ((float("nan"), 0.1), (0.0, float("inf")), (0.0, -0.1)):
        with pytest.raises(_lib.SdfnmpcError, match="error -1"):
            solver.rollout(2, plant, xl, ul, perceive=perc, scene_clock=clock)
        ctx.synchronize()
        np.testing.assert_array_equal(xl.numpy(), np.full((B, 3, 10), -7.0))
        for k, v in before.items():
            np.testing.assert_array_equal(n.ocp.download(k), v)
    r = n.rollout(2, scene=sc, vae=vae, img_shape=SHAPE, scene_t0=T0)  # and it still runs afterwards
    assert r.clearance.shape == (B, 3) and r.t.shape == (3,)
    n.ocp.close()
