"""The sensor model inside the device rollout (Nmpc.rollout(scene=, vae=, sensor=),
sdfnmpc_solver_rollout_perceive_sensor): bitwise against the host-driven loop that calls SensorModel.apply(img, frame =
phase + k) between Scene.render_from_state and VaeWrapper.set_img, the frame counter across chunks, the unchanged
rollout without a sensor, the effect of the degradation, and the API contract.  The setup of
tests/test_gpu_rollout_perceive.py: N = 10, B = 3, K = 6, 18 x 32 images, synthetic weights, refs = 'wps'."""
import numpy as np
import pytest

from sdf_nmpc_amd import _lib
from sdf_nmpc_amd.config import Config
from sdf_nmpc_amd.sensor import SensorModel
from test_gpu_rollout_perceive import B, K, SCENE_OF, SHAPE, _make, _wps

pytestmark = [pytest.mark.gpu, pytest.mark.filterwarnings("ignore:no SDF weights"),
              pytest.mark.filterwarnings("ignore:QP reached")]

SEED = 0x5E4502


@pytest.fixture(scope="module", autouse=True)
def _torch_first(gpu_ctx):
    """torch opens the device before the first controller of this module does, as in tests/test_gpu_rollout.py."""


def _sensor(cfg, ctx):
    """The reference's training augmentation with the outlier removal behind it, and no-return pixels."""
    return SensorModel.reference_augment(cfg, ctx, SEED, outlier_rm=True, min_range=0.1, miss_invalid=True)


def _host_loop(n, vae, scene, sensor, x0, steps, every, wps, phase=0):
    """tests/test_gpu_rollout_perceive.py's loop with the camera's imperfection: the image is degraded as frame
    phase + k before the encoder sees it.  Also returns the last degraded image."""
    ctx = n.ocp.ctx
    plant = _lib.plant_opts(n.cfg, dt=float(n.ocp.dt[0]))
    dx = _lib.DeviceArray(ctx, (B, 10))
    xs, us, its, sts, last = [np.reshape(x0, (B, 10)).copy()], [], [], [], None
    for k in range(steps):
        n.set_x0(xs[-1])
        if (k + phase) % every == 0:
            img = scene.render_from_state(xs[-1], n.cfg, SHAPE, normalized=False)
            sensor.apply(img, frame=phase + k, normalized=False)
            vae.set_img(img)
            vae.encode_to(n, img.pose["W_p_Bo"], img.pose["W_R_Bo"])
            last = img
        n.gen_refs_device("wps", wps=wps)
        n.solve()
        us.append(n.ocp.field("u0").numpy().reshape(B, 4))
        its.append(n.ocp.iters.copy())
        sts.append(n.ocp.status.copy())
        dx.upload(xs[-1])
        _lib.plant_step(ctx, plant, B, dx, n.ocp.field("u0"), dx)
        xs.append(dx.numpy())
    return np.stack(xs, 1), np.stack(us, 1), np.stack(sts, 1), np.stack(its, 1), last.numpy()


@pytest.mark.parametrize("every", [1, 2])
def test_rollout_with_sensor_equals_host_driven_loop_bitwise(every):
    cfg = Config(mpc__N=10)
    wps = _wps()
    na, x0, sa, va = _make(cfg)
    nb, _, sb, vb = _make(cfg)
    na.set_x0(x0)
    r = na.rollout(K, refs="wps", wps=wps, scene=sa, vae=va, perceive_every=every, img_shape=SHAPE, keep_img=True,
                   sensor=_sensor(cfg, na.ocp.ctx))
    x, u, status, iters, img = _host_loop(nb, vb, sb, _sensor(cfg, nb.ocp.ctx), x0, K, every, wps)
    np.testing.assert_array_equal(r.x, x)
    np.testing.assert_array_equal(r.u, u)
    np.testing.assert_array_equal(r.status, status)
    np.testing.assert_array_equal(r.iters, iters)
    np.testing.assert_array_equal(na.ocp.download("p"), nb.ocp.download("p"))
    assert r.img.shape == (B,) + SHAPE and r.img.dtype == np.float32
    np.testing.assert_array_equal(r.img.view(np.uint32), img.view(np.uint32))  # the degraded image the encoder saw
    assert (r.img == 0).any()
    np.testing.assert_array_equal(va.latent64.numpy(), vb.latent64.numpy())
    for m in (na, nb):
        m.ocp.close()


def test_frame_counter_runs_across_chunks():
    """Six one-step chunks with perceive_phase = the steps already taken are the uncut rollout, bit for bit: the
    sensor's frame is phase + k, not the step within the chunk."""
    cfg = Config(mpc__N=10)
    wps = _wps()
    n, x0, sc, vae = _make(cfg)
    sensor = _sensor(cfg, n.ocp.ctx)
    n.set_x0(x0)
    xs, us, imgs = [np.reshape(x0, (B, 10))], [], []
    for k in range(K):
        r = n.rollout(1, refs="wps", wps=wps, scene=sc, vae=vae, img_shape=SHAPE, perceive_phase=k, sensor=sensor,
                      keep_img=True)
        xs.append(r.x[:, 1])
        us.append(r.u[:, 0])
        imgs.append(r.img)
    m, _, sc2, vae2 = _make(cfg)
    m.set_x0(x0)
    whole = m.rollout(K, refs="wps", wps=wps, scene=sc2, vae=vae2, img_shape=SHAPE, sensor=_sensor(cfg, m.ocp.ctx),
                      keep_img=True)
    np.testing.assert_array_equal(whole.x, np.stack(xs, 1))
    np.testing.assert_array_equal(whole.u, np.stack(us, 1))
    np.testing.assert_array_equal(m.ocp.download("p"), n.ocp.download("p"))
    np.testing.assert_array_equal(whole.img.view(np.uint32), imgs[-1].view(np.uint32))
    assert not np.array_equal(imgs[0] == 0, imgs[1] == 0)  # another frame, other lost pixels
    n.ocp.close()
    m.ocp.close()


def _launches(ctx, *names):
    return [ctx.kernel_stats(k)[1] for k in names]


def test_rollout_without_sensor_is_unchanged_and_launches_no_sensor_kernel():
    cfg = Config(mpc__N=10)
    wps = _wps()
    na, x0, sa, va = _make(cfg)
    nb, _, sb, vb = _make(cfg)
    for m in (na, nb):
        m.set_x0(x0)
        m.ocp.ctx.enable_timing(True)
        m.ocp.ctx.reset_stats()
    r = na.rollout(K, refs="wps", wps=wps, scene=sa, vae=va, perceive_every=2, img_shape=SHAPE, keep_img=True, sensor=None)
    q = nb.rollout(K, refs="wps", wps=wps, scene=sb, vae=vb, perceive_every=2, img_shape=SHAPE, keep_img=True)
    for k in ("x", "u", "status", "iters", "clearance", "img"):
        np.testing.assert_array_equal(getattr(r, k), getattr(q, k))
    np.testing.assert_array_equal(na.ocp.download("p"), nb.ocp.download("p"))
    assert _launches(na.ocp.ctx, "scene_render", "sensor_degrade", "outlier_rm", "morph") == [K // 2, 0, 0, 0]
    # with the sensor: one degradation and one fused outlier removal per perceiving step, nothing else new
    na.ocp.ctx.reset_stats()
    na.rollout(K, refs="wps", wps=wps, scene=sa, vae=va, perceive_every=2, img_shape=SHAPE, sensor=_sensor(cfg, na.ocp.ctx))
    assert _launches(na.ocp.ctx, "scene_render", "sensor_degrade", "outlier_rm", "morph") == [K // 2] * 3 + [0]
    for m in (na, nb):
        m.ocp.ctx.enable_timing(False)
        m.ocp.close()


def test_degraded_rollout_differs_and_clearance_stays_exact():
    cfg = Config(mpc__N=10)
    wps = _wps()
    na, x0, sa, va = _make(cfg)
    nb, _, sb, vb = _make(cfg)
    na.set_x0(x0)
    nb.set_x0(x0)
    clean = na.rollout(K, refs="wps", wps=wps, scene=sa, vae=va, img_shape=SHAPE, keep_img=True)
    deg = nb.rollout(K, refs="wps", wps=wps, scene=sb, vae=vb, img_shape=SHAPE, keep_img=True,
                     sensor=_sensor(cfg, nb.ocp.ctx))
    assert (deg.img == 0).mean() > 0.03 and not (clean.img == 0).any()  # lost pixels; the exact image has none
    assert not np.array_equal(va.latent64.numpy(), vb.latent64.numpy())
    assert not np.array_equal(clean.x, deg.x)
    # the clearance is still measured against the scene itself, at the logged positions
    assert deg.clearance.shape == (B, K + 1)
    pts = deg.x[:, :, :3].reshape(-1, 3)
    np.testing.assert_array_equal(deg.clearance.ravel(), sb.distance(pts, np.repeat(SCENE_OF, K + 1)))
    na.ocp.close()
    nb.ocp.close()


def test_sensor_api_contract():
    """Every refusal comes before anything is uploaded or enqueued: the state, the iterate and p stay."""
    cfg = Config(mpc__N=10)
    n, x0, sc, vae = _make(cfg)
    n.set_x0(x0)
    n.rollout(1)  # flush the host setters, so that the device fields are settled
    x0 = n.x0.copy()
    before = {k: n.ocp.download(k) for k in ("x", "u", "p", "x0")}
    other_ctx = _lib.Context(0)
    sensor = _sensor(cfg, n.ocp.ctx)
    bad = [dict(sensor=sensor), dict(sensor=sensor, vae=vae), dict(scene=sc, vae=vae, sensor=_sensor(cfg, other_ctx)),
           dict(scene=sc, vae=vae, sensor=SensorModel(cfg, n.ocp.ctx, 1, stream_id=[0, 1]))]
    for kw in bad:
        with pytest.raises(ValueError):
            n.rollout(2, refs="wps", wps=_wps(), img_shape=SHAPE, **kw)
        np.testing.assert_array_equal(n.x0, x0)
        for k, v in before.items():
            np.testing.assert_array_equal(n.ocp.download(k), v)
    # the C entry point's own refusals launch nothing either: a sensor without perception, a missing scratch
    lib = _lib.load()
    o, _ = sensor.opts(B, *SHAPE, normalized=False)
    a = _lib.RolloutArgsC()
    assert lib.sdfnmpc_solver_rollout_perceive_sensor(n.ocp.parts[0].solver.h, _lib.C.byref(a), None, 0.0, 0.0,
                                                      _lib.C.byref(o), None) == -1
    assert b"sensor model needs perception" in lib.sdfnmpc_last_error()
    for k, v in before.items():
        np.testing.assert_array_equal(n.ocp.download(k), v)
    r = n.rollout(2, scene=sc, vae=vae, img_shape=SHAPE, sensor=sensor)  # and it still runs afterwards
    assert r.clearance.shape == (B, 3)
    n.ocp.close()
