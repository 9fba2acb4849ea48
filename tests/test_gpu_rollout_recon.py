"""A controller whose SDF is the distance field of the image its VAE latent retains (Nmpc.set_sdf_image(...,
reconstruct=vae), sdfnmpc_solver_rollout_image_recon): bitwise against reconstruct-then-set, against the host-driven
loop render_from_state / sensor.apply / reconstruct / set_sdf_image / set_pose_device / solve / plant_step (static
and moving scenes, perceive_every 1 and 2, signed and unsigned), chunks, and the refusals.  N = 10, B = 3, K = 6,
images 30 x 40: the scene, sensor and waypoints of tests/test_gpu_rollout_image_sdf.py."""
import types

import numpy as np
import pytest

import scene_ref as R
from sdf_nmpc_amd import _lib
from sdf_nmpc_amd import vae as V
from sdf_nmpc_amd.config import Config
from sdf_nmpc_amd.scene import Scene
from test_gpu_rollout import _setup
from test_gpu_rollout_image_sdf import B, K, OTHER, SCENE_OF, SHAPE, T0, _dyn_prims, _sensor, _wps

pytestmark = [pytest.mark.gpu, pytest.mark.filterwarnings("ignore:no SDF weights"),
              pytest.mark.filterwarnings("ignore:QP reached")]


@pytest.fixture(scope="module", autouse=True)
def _torch_first(gpu_ctx):
    """torch opens the device before the first controller of this module does, as in tests/test_gpu_rollout.py."""


@pytest.fixture(scope="module")
def weights():
    """Synthetic encoder and decoder parameters, generated once for every wrapper of the module."""
    es, ds = V.DEFAULT_ENCODER, V.DEFAULT_DECODER
    return (es, V.synthetic_encoder(es, 0)), (ds, V.synthetic_decoder(ds, 0))


def _vae(cfg, ctx, weights, decoder=True, batch=B):
    return V.VaeWrapper(cfg, weights=weights[0], batch=batch, ctx=ctx, decoder=weights[1] if decoder else None)


def _make(cfg, weights, dynamic=False, seed=21):
    n, x0 = _setup(cfg, B, seed)
    scene = Scene(n.ocp.ctx, [OTHER, _dyn_prims() if dynamic else R.SCENE], scene_of=SCENE_OF)
    return n, x0, scene, _vae(cfg, n.ocp.ctx, weights)


@pytest.mark.parametrize("signed", (True, False))
def test_reconstruct_keyword_equals_reconstruct_then_set(weights, signed):
    """set_sdf_image(imgs, reconstruct=vae); solve() gives bitwise the h, Jh and u0 of set_sdf_image(vae.reconstruct(
    imgs)) on a controller whose image options have is_depth off (the reconstruction is a range image)."""
    cfg = Config(mpc__N=10)
    assert cfg.sensor.is_depth
    na, x0, scene, va = _make(cfg, weights)
    imgs = scene.render_from_state(x0, cfg, SHAPE, normalized=True, t=T0).numpy()
    na.set_sdf_image(imgs, signed=signed, reconstruct=va)
    assert na._sdf_image["opts"].img.is_depth == 0
    np.testing.assert_array_equal(na._sdf_image["camera"].numpy(), imgs)
    rec = na._sdf_image["images"].numpy()
    assert rec.shape == imgs.shape and np.isfinite(rec).all() and rec.min() >= 0 and rec.max() <= 1 and (rec != imgs).any()
    nb, _ = _setup(Config(mpc__N=10, sensor__is_depth=False), B, 21)
    vb = _vae(cfg, nb.ocp.ctx, weights)  # the wrapper keeps the camera's is_depth: Depth2Range before the encoder
    nb.set_sdf_image(vb.reconstruct(imgs, normalized=True), signed=signed)
    np.testing.assert_array_equal(nb._sdf_image["images"].numpy(), rec)
    for n in (na, nb):
        n.set_x0(x0)
        n.solve()
    for k in ("h", "Jh", "u0"):
        np.testing.assert_array_equal(na.ocp.download(k), nb.ocp.download(k))
    assert np.isfinite(na.ocp.download("h")[..., 2]).all()
    scene.close()
    for n in (na, nb):
        n.ocp.close()


def _host_loop(n, scene, vae, x0, steps, every, wps, signed, sensor, dts=None, phase=0):
    ctx = n.ocp.ctx
    dt = float(n.ocp.dt[0])
    dts = dt if dts is None else dts
    plant = _lib.plant_opts(n.cfg, dt=dt)
    dx = _lib.DeviceArray(ctx, (B, 10))
    xs, us, its, sts = [np.reshape(x0, (B, 10)).copy()], [], [], []
    for k in range(steps):
        n.set_x0(xs[-1])
        if (k + phase) % every == 0:
            img = scene.render_from_state(xs[-1], n.cfg, SHAPE, normalized=True, t=T0 + (phase + k) * dts)
            sensor.apply(img, phase + k, normalized=True)
            n.set_sdf_image(img, signed=signed, reconstruct=vae)
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


@pytest.mark.parametrize("dynamic,every,signed", [(True, 2, True), (True, 1, False), (False, 1, True), (False, 2, False)])
def test_reconstructing_rollout_equals_host_driven_loop_bitwise(weights, dynamic, every, signed):
    cfg = Config(mpc__N=10)
    wps = _wps()
    dts = 0.2 if dynamic else None
    na, x0, sa, va = _make(cfg, weights, dynamic)
    nb, _, sb, vb = _make(cfg, weights, dynamic)
    for n, s, v in ((na, sa, va), (nb, sb, vb)):
        n.set_sdf_image(s.render_from_state(x0, cfg, SHAPE, normalized=True, t=T0), signed=signed, reconstruct=v)
    p_lat = np.reshape(np.array(na.p), (B, na.N + 1, -1))[..., 17:]  # the latents _setup gave the host setters
    assert np.abs(p_lat).max() > 0
    na.set_x0(x0)
    r = na.rollout(K, refs="wps", wps=wps, scene=sa, sensor=_sensor(cfg, na.ocp.ctx), perceive_every=every, scene_t0=T0,
                   scene_dt=dts, img_shape=SHAPE, keep_img=True)
    x, u, status, iters = _host_loop(nb, sb, vb, x0, K, every, wps, signed, _sensor(cfg, nb.ocp.ctx), dts=dts)
    np.testing.assert_array_equal(r.x, x)
    np.testing.assert_array_equal(r.u, u)
    np.testing.assert_array_equal(r.status, status)
    np.testing.assert_array_equal(r.iters, iters)
    np.testing.assert_array_equal(na.ocp.download("p"), nb.ocp.download("p"))
    np.testing.assert_array_equal(na.ocp.download("p")[..., 17:], p_lat)  # no network: the latent columns stay
    last = nb._sdf_image["images"].numpy()
    np.testing.assert_array_equal(r.img, last)  # keep_img: the reconstruction the source last held
    np.testing.assert_array_equal(na._sdf_image["camera"].numpy(), nb._sdf_image["camera"].numpy())
    np.testing.assert_array_equal(va.latent.numpy(), vb.latent.numpy())
    assert (r.img != na._sdf_image["camera"].numpy()).any() and r.img.min() >= 0 and r.img.max() <= 1
    assert (r.iters > 0).all() and np.isfinite(na.ocp.download("h")[..., 2]).all()
    assert r.clearance.shape == (B, K + 1) and np.isfinite(r.clearance).all()
    if not signed:
        np.testing.assert_array_equal(na._sdf_image["pooled"].numpy(), nb._sdf_image["pooled"].numpy())
    for m in (na, nb):
        m.ocp.close()


@pytest.mark.parametrize("signed", (True, False))
def test_two_chunks_with_phase_are_the_uncut_rollout(weights, signed):
    cfg = Config(mpc__N=10)
    wps = _wps()
    kw = dict(refs="wps", wps=wps, perceive_every=2, scene_t0=T0, img_shape=SHAPE, keep_img=True)
    runs = []
    for cuts in ((K,), (3, K - 3)):
        n, x0, s, v = _make(cfg, weights, dynamic=True)
        n.set_sdf_image(s.render_from_state(x0, cfg, SHAPE, normalized=True, t=T0), signed=signed, reconstruct=v)
        n.set_x0(x0)
        xs, us, done = [np.reshape(x0, (B, 1, 10))], [], 0
        for c in cuts:
            r = n.rollout(c, scene=s, sensor=_sensor(cfg, n.ocp.ctx), perceive_phase=done, **kw)
            xs.append(r.x[:, 1:])
            us.append(r.u)
            done += c
        runs.append((np.concatenate(xs, 1), np.concatenate(us, 1), n.ocp.download("p"), r.img))
        n.ocp.close()
    for a, b in zip(*runs):
        np.testing.assert_array_equal(a, b)


def test_refusals_leave_the_controller_untouched(weights):
    cfg = Config(mpc__N=10)
    n, x0, scene, vae = _make(cfg, weights)
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
    other_ctx = _lib.Context(ctx.device)
    for bad in (_vae(cfg, ctx, weights, decoder=False), _vae(cfg, other_ctx, weights), _vae(cfg, ctx, weights, batch=B + 1)):
        with pytest.raises(ValueError):
            n.set_sdf_image(img, reconstruct=bad)
        untouched()
    with pytest.raises(ValueError):
        n.set_sdf_image(img[:2], img_of=[0, 1, 0], reconstruct=vae)
    untouched()
    assert n._sdf_image is None
    n.set_sdf_image(img, reconstruct=vae)
    held, cam = n._sdf_image["images"].numpy(), n._sdf_image["camera"].numpy()
    for kw in (dict(vae=vae), dict(scene=scene, vae=vae), dict(scene=scene, img_shape=(30, 45)), dict(scene=scene, perceive_every=0)):
        with pytest.raises(ValueError):  # rollout(vae=...) with an image source stays the ValueError it is
            n.rollout(2, refs="hover", **kw)
        untouched()
    # the library's own refusals of the new entry, before its first launch
    solver = n.ocp.parts[0].solver
    plant = _lib.plant_opts(cfg, dt=float(n.ocp.dt[0]))
    xl, ul = _lib.DeviceArray.from_numpy(ctx, np.full((B, 3, 10), -7.0)), _lib.DeviceArray(ctx, (B, 2, 4))
    ws = {k: _lib.DeviceArray.from_numpy(ctx, np.full((B, w), -7.0)) for k, w in (("W_p_Bo", 3), ("W_R_Bo", 9),
                                                                               ("W_p_C", 3), ("W_R_C", 9))}
    s = cfg.sensor
    camera = n._sdf_image["camera"]

    def perc(h=SHAPE[0], vae_h=vae.vae.h, images=camera.data_ptr(), latent=vae.latent.data_ptr(), yz=vae.yz.data_ptr(), every=1):
        return _lib.PerceiveArgsC(scene.h, None, scene.img_opts(cfg), h, SHAPE[1], scene.scale(cfg, normalized=True),
                                  (_lib.C.c_double * 3)(*[float(v) for v in np.asarray(s.B_p_C, float).ravel()]),
                                  (_lib.C.c_double * 9)(*[float(v) for v in np.asarray(s.B_R_C, float).ravel()]), vae_h,
                                  _lib.VaeOptsC(B, h, SHAPE[1], 0, 1.0, yz), every, 0, images, latent, None,
                                  *[ws[k].data_ptr() for k in ("W_p_Bo", "W_R_Bo", "W_p_C", "W_R_C")])

    small = V.DecoderSpec(size_latent=64)
    dec64 = _lib.VaeDec(ctx, V.pack_decoder(small, V.synthetic_decoder(small, 0)))
    elsewhere = _lib.VaeDec(other_ctx, V.pack_decoder(*weights[1]))
    none = types.SimpleNamespace(h=None)
    for kw in (dict(perceive=perc(), dec=none), dict(perceive=None, dec=vae.dec), dict(perceive=perc(), dec=dec64),
               dict(perceive=perc(), dec=elsewhere), dict(perceive=perc(vae_h=None), dec=vae.dec),
               dict(perceive=perc(h=35), dec=vae.dec), dict(perceive=perc(images=None), dec=vae.dec),
               dict(perceive=perc(latent=None), dec=vae.dec), dict(perceive=perc(yz=None), dec=vae.dec),
               dict(perceive=perc(images=n._sdf_image["images"].data_ptr()), dec=vae.dec),
               dict(perceive=perc(every=0), dec=vae.dec), dict(perceive=perc(), dec=vae.dec, t0=float("nan")),
               dict(perceive=perc(), dec=vae.dec, steps=0)):
        steps = kw.pop("steps", 2)
        with pytest.raises(_lib.SdfnmpcError, match="error -1"):
            solver.rollout_image_sdf(steps, plant, xl, ul, **kw)
        untouched()
        np.testing.assert_array_equal(xl.numpy(), np.full((B, 3, 10), -7.0))
        np.testing.assert_array_equal(n._sdf_image["images"].numpy(), held)
        np.testing.assert_array_equal(camera.numpy(), cam)
        for v in ws.values():
            assert (v.numpy() == -7.0).all()
    r = n.rollout(2, refs="hover", scene=scene, img_shape=SHAPE, keep_img=True)  # and it still runs afterwards
    assert r.clearance.shape == (B, 3) and (r.img != held).any()
    dec64.close()
    elsewhere.close()
    scene.close()
    other_ctx.close()
    n.ocp.close()
