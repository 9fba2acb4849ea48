"""Perception inside the device rollout (Nmpc.rollout(scene=, vae=), sdfnmpc_solver_rollout_perceive): bitwise against
the host-driven loop built from the public pieces -- Scene.render_from_state, VaeWrapper.set_img / encode_to and the
host loop of tests/test_gpu_rollout.py -- the perception schedule, the clearance log, the unchanged behaviour without a
scene, and the API contract.  N = 10, B = 3, K = 6, synthetic VAE and SIREN weights, 18 x 32 images (the encoder's
resize runs), refs = 'wps'."""
import numpy as np
import pytest

import scene_ref as R
from sdf_nmpc_amd import _lib
from sdf_nmpc_amd.config import Config
from sdf_nmpc_amd.controller import Nmpc
from sdf_nmpc_amd.reference import yaw2quat
from sdf_nmpc_amd.scene import Scene
from sdf_nmpc_amd.vae import VaeWrapper
from test_gpu_rollout import _host_loop as _plain_host_loop
from test_gpu_rollout import _setup

pytestmark = [pytest.mark.gpu, pytest.mark.filterwarnings("ignore:no SDF weights"),
              pytest.mark.filterwarnings("ignore:QP reached")]

B, K, SHAPE = 3, 6, (18, 32)
SCENE_OF = [1, 0, 1]
OTHER = [("sphere", [2.0, 0.2, 0.0, 0.6]), ("box", [-10.0, -10.0, -1.6, 10.0, 10.0, -1.5])]


@pytest.fixture(scope="module", autouse=True)
def _torch_first(gpu_ctx):
    """torch opens the device before the first controller of this module does, as in tests/test_gpu_rollout.py."""


def _wps():
    rng = np.random.default_rng(5)
    return (rng.uniform(-2, 2, (B, 2, 3)), np.stack([[yaw2quat(a) for a in row] for row in rng.uniform(-1, 1, (B, 2))]))


def _make(cfg, seed=21):
    """A controller set up through the host setters, and a scene pair and an encoder on its context."""
    n, x0 = _setup(cfg, B, seed)
    ctx = n.ocp.ctx
    return n, x0, Scene(ctx, [R.SCENE, OTHER], scene_of=SCENE_OF), VaeWrapper(cfg, batch=B, ctx=ctx)


def _host_loop(n, vae, scene, x0, steps, every, wps, phase=0):
    """The loop a user writes: per step set_x0; every `every`-th step a new image of the scene from the current
    state, encoded and written into p with the body pose of that state; references; solve; plant."""
    ctx = n.ocp.ctx
    plant = _lib.plant_opts(n.cfg, dt=float(n.ocp.dt[0]))
    dx = _lib.DeviceArray(ctx, (B, 10))
    xs, us, its, sts = [np.reshape(x0, (B, 10)).copy()], [], [], []
    for k in range(steps):
        n.set_x0(xs[-1])
        if (k + phase) % every == 0:
            img = scene.render_from_state(xs[-1], n.cfg, SHAPE, normalized=False)
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


@pytest.mark.parametrize("every", [1, 2, 4])
def test_rollout_with_perception_equals_host_driven_loop_bitwise(every):
    cfg = Config(mpc__N=10)
    wps = _wps()
    na, x0, sa, va = _make(cfg)
    nb, _, sb, vb = _make(cfg)
    na.set_x0(x0)
    r = na.rollout(K, refs="wps", wps=wps, scene=sa, vae=va, perceive_every=every, img_shape=SHAPE, keep_img=True)
    x, u, status, iters = _host_loop(nb, vb, sb, x0, K, every, wps)
    np.testing.assert_array_equal(r.x, x)
    np.testing.assert_array_equal(r.u, u)
    np.testing.assert_array_equal(r.status, status)
    np.testing.assert_array_equal(r.iters, iters)
    pa, pb = na.ocp.download("p"), nb.ocp.download("p")
    np.testing.assert_array_equal(pa, pb)
    assert np.abs(pa[:, :, 17:]).max() > 0 and np.ptp(r.u[:, :, 0]) > 1e-3  # a latent arrived, the loop did something
    # the last images are those of the last perceiving step, from the state it saw
    k_last = (K - 1) // every * every
    want = sb.render_from_state(r.x[:, k_last], cfg, SHAPE, normalized=False).numpy()
    assert r.img.shape == (B,) + SHAPE and r.img.dtype == np.float32
    np.testing.assert_array_equal(r.img, want)
    np.testing.assert_array_equal(va.latent64.numpy(), vb.latent64.numpy())
    for m in (na, nb):
        m.ocp.close()


def test_latent_changes_exactly_at_the_perceiving_steps():
    """perceive_every = 2 over six one-step chunks (perceive_phase = the steps already taken): the latent and pose
    columns of p change at steps 0, 2 and 4 and at no other step; the chunks together are the uncut rollout."""
    cfg = Config(mpc__N=10)
    wps = _wps()
    n, x0, sc, vae = _make(cfg)
    n.set_x0(x0)
    p_prev = n.p.copy()  # what the host setters left: uploaded at the first flush
    changed, xs = [], [np.reshape(x0, (B, 10))]
    for k in range(K):
        r = n.rollout(1, refs="wps", wps=wps, scene=sc, vae=vae, perceive_every=2, img_shape=SHAPE, perceive_phase=k)
        p = n.ocp.download("p")
        changed.append(bool((p[:, :, 17:] != p_prev[:, :, 17:]).any()) or bool((p[:, :, 1:13] != p_prev[:, :, 1:13]).any()))
        if changed[-1]:  # every node of an instance carries the same latent and pose
            np.testing.assert_array_equal(p[:, :, 17:], np.broadcast_to(p[:, :1, 17:], p[:, :, 17:].shape))
            np.testing.assert_array_equal(p[:, 0, 17:], vae.latent64.numpy())
        p_prev = p
        xs.append(r.x[:, 1])
    assert changed == [True, False, True, False, True, False]
    m, _, sc2, vae2 = _make(cfg)
    m.set_x0(x0)
    whole = m.rollout(K, refs="wps", wps=wps, scene=sc2, vae=vae2, perceive_every=2, img_shape=SHAPE)
    np.testing.assert_array_equal(whole.x, np.stack(xs, 1))
    np.testing.assert_array_equal(m.ocp.download("p"), p_prev)
    n.ocp.close()
    m.ocp.close()


def test_clearance_is_the_exact_distance_of_the_logged_positions():
    cfg = Config(mpc__N=10)
    n, x0, sc, vae = _make(cfg)
    n.set_x0(x0)
    r = n.rollout(K, refs="wps", wps=_wps(), scene=sc, vae=vae, perceive_every=3, img_shape=SHAPE)
    assert r.clearance.shape == (B, K + 1) and r.clearance.dtype == np.float64 and r.img is None
    pts = r.x[:, :, :3].reshape(-1, 3)
    np.testing.assert_array_equal(r.clearance.ravel(), sc.distance(pts, np.repeat(SCENE_OF, K + 1)))
    want = np.stack([R.distance([R.SCENE, OTHER][s], r.x[b, :, :3]) for b, s in enumerate(SCENE_OF)])
    assert np.abs(r.clearance - want).max() <= 1e-12
    n.ocp.close()


def test_rollout_without_scene_is_unchanged():
    """The body of test_rollout_equals_host_driven_loop_bitwise (tests/test_gpu_rollout.py) at shift = 1, refs =
    'wps' with the call signature the method had before perception: the same results, bit for bit, and no
    perception fields."""
    cfg = Config(mpc__N=10, mpc__shift=1)
    Bn, Kn = 70, 3
    rng = np.random.default_rng(5)
    wps = (rng.uniform(-2, 2, (Bn, 2, 3)), np.stack([[yaw2quat(a) for a in row] for row in rng.uniform(-1, 1, (Bn, 2))]))
    na, x0 = _setup(cfg, Bn, 21)
    nb, _ = _setup(cfg, Bn, 21)
    na.set_x0(x0)
    r = na.rollout(Kn, refs="wps", wps=wps)
    x, u, status, iters = _plain_host_loop(nb, x0, Kn, "wps", wps)
    assert r.col is None and r.pts is None and r.clearance is None and r.img is None
    np.testing.assert_array_equal(r.u, u)
    np.testing.assert_array_equal(r.x, x)
    np.testing.assert_array_equal(r.iters, iters)
    np.testing.assert_array_equal(r.status, status)
    for a, b in zip(na.get_matrices(), nb.get_matrices()):
        np.testing.assert_array_equal(a, b)
    np.testing.assert_array_equal(na.ocp.download("p"), nb.ocp.download("p"))
    na.ocp.close()
    nb.ocp.close()


def test_perception_api_contract(monkeypatch):
    """Every ValueError is raised before anything is uploaded or enqueued: the state, the iterate and p stay."""
    cfg = Config(mpc__N=10)
    n, x0, sc, vae = _make(cfg)
    n.set_x0(x0)
    n.rollout(1)  # flush the host setters, so that the device fields are settled
    x0 = n.x0.copy()
    before = {k: n.ocp.download(k) for k in ("x", "u", "p", "x0")}
    other_ctx = _lib.Context(0)
    imgs = np.full((B,) + SHAPE, 0.5, np.float32)
    bad = [dict(scene=sc), dict(vae=vae), dict(scene=sc, vae=vae, imgs=imgs),
           dict(scene=sc, vae=VaeWrapper(cfg, batch=B, ctx=other_ctx)),
           dict(scene=Scene(other_ctx, R.SCENE), vae=vae),
           dict(scene=sc, vae=VaeWrapper(cfg, batch=B + 1, ctx=n.ocp.ctx)),
           dict(scene=Scene(n.ocp.ctx, R.SCENE, scene_of=[0, 0]), vae=vae),
           dict(scene=sc, vae=vae, perceive_every=0), dict(scene=sc, vae=vae, perceive_phase=-1)]
    for kw in bad:
        with pytest.raises(ValueError):
            n.rollout(2, refs="wps", wps=_wps(), img_shape=SHAPE, **kw)
        np.testing.assert_array_equal(n.x0, x0)
        for k, v in before.items():
            np.testing.assert_array_equal(n.ocp.download(k), v)
    # the C entry point's own refusals launch nothing either
    for kw in (dict(img_shape=(0, 32)), dict(img_shape=(18, 0))):
        with pytest.raises(_lib.SdfnmpcError, match="error -1"):
            n.rollout(2, scene=sc, vae=vae, **kw)
        for k, v in before.items():
            np.testing.assert_array_equal(n.ocp.download(k), v)
    r = n.rollout(2, scene=sc, vae=vae, img_shape=SHAPE)  # and it still runs afterwards
    assert r.clearance.shape == (B, 3)
    n.ocp.close()
    # a batch split over several parts is refused
    from sdf_nmpc_amd import ocp as ocp_mod
    from sdf_nmpc_amd import shard
    from sdf_nmpc_amd.model import Quad
    plan = shard.plan
    monkeypatch.setattr(shard, "plan", lambda total, capacity, n_dev: plan(total, 2, n_dev))
    o = ocp_mod.Ocp(Quad(cfg), batch=4, devices=[0, 0])
    assert len(o.parts) == 2
    m = Nmpc(cfg, batch=4, ocp=o)
    m.set_x0(np.tile(np.reshape(x0, (B, 10))[:1], (4, 1)))
    with pytest.raises(ValueError, match="split"):
        m.rollout(2, scene=Scene(o.ctx, R.SCENE), vae=VaeWrapper(cfg, batch=4, ctx=o.ctx))
    o.close()
