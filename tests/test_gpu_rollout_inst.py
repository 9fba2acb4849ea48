"""Rollouts in an instanced mesh scene (Scene.instanced, csrc/scene_inst.hip): a floor, a sphere that crosses the start
states, a yawing box and a sliding cylinder, as the image the encoder sees (perception inside the loop, with the scene's
clock) and as the SDF source (set_sdf_scene with and without predict) -- bitwise against the loops a user writes around
solve() on the host, in x, u, p, t and the clearance; a rollout cut into two chunks; and the swept clearance against a
direct call on the logged chords.  N = 10, B = 4, K = 6, 18 x 32 images.  The network weights are synthetic: no clearance
here says anything about the controller.

Every test here fails without the feature: there is no Scene.instanced."""
import numpy as np
import pytest

import mesh_inst_ref as I
from sdf_nmpc_amd import _lib
from sdf_nmpc_amd.config import Config
from sdf_nmpc_amd.reference import yaw2quat
from sdf_nmpc_amd.scene import Scene
from sdf_nmpc_amd.vae import VaeWrapper
from test_gpu_rollout import _setup

pytestmark = [pytest.mark.gpu, pytest.mark.filterwarnings("ignore:no SDF weights"),
              pytest.mark.filterwarnings("ignore:QP reached")]

B, K, SHAPE, T0, MAX_DF = 4, 6, (18, 32), 0.5, 3.0
# around the start states of test_gpu_rollout._setup (positions in [-1, 1]^3), parts of mesh_inst_ref.parts()
INSTANCES = [Scene.instance(2, (0.0, 0.0, -1.8)),
             Scene.instance(1, (0.6, -1.4, 0.1), v=(0.0, 1.2, 0.0)),
             Scene.instance(0, (2.0, 0.0, 0.0), rpy=(0.0, 0.1, 0.4), yaw_rate=0.5, v=(-0.4, 0.0, 0.0)),
             Scene.instance(3, (1.2, 1.2, -0.2), rpy=(0.2, 0.0, 0.0), amp=(0.0, 0.6, 0.0), omega=1.5, phase=0.2),
             Scene.instance(0, (-1.6, 0.4, 0.3), rpy=(0.3, 0.2, 0.1))]


@pytest.fixture(scope="module", autouse=True)
def _torch_first(gpu_ctx):
    """torch opens the device before the first controller of this module does, as in tests/test_gpu_rollout.py."""


def _wps():
    rng = np.random.default_rng(5)
    return (rng.uniform(-2, 2, (B, 2, 3)), np.stack([[yaw2quat(a) for a in row] for row in rng.uniform(-1, 1, (B, 2))]))


def _scene(ctx, **kw):
    return Scene.instanced(ctx, I.parts(), INSTANCES, closed=True, sdf_source=True, **kw)


def _make(cfg, seed=21):
    n, x0 = _setup(cfg, B, seed)
    ctx = n.ocp.ctx
    return n, x0, _scene(ctx), VaeWrapper(cfg, batch=B, ctx=ctx)


def _perceiving_host_loop(n, vae, scene, x0, steps, every, wps, t0):
    """tests/test_gpu_rollout_dyn.py's loop: the image before step k is rendered at t0 + k dt"""
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


def _source_host_loop(n, scene, x0, steps, every, wps, t0):
    """tests/test_gpu_rollout_scene_sdf.py's loop: the pose refreshed every `every`-th step, the scene's clock"""
    ctx = n.ocp.ctx
    dt = float(n.ocp.dt[0])
    plant = _lib.plant_opts(n.cfg, dt=dt)
    dx = _lib.DeviceArray(ctx, (B, 10))
    xs, us, its, sts = [np.reshape(x0, (B, 10)).copy()], [], [], []
    for k in range(steps):
        n.set_x0(xs[-1])
        if k % every == 0:
            ps = scene.pose(xs[-1], n.cfg)
            n.set_pose_device(ps["W_p_Bo"], ps["W_R_Bo"])
        n.set_scene_time(t0 + k * dt)
        n.gen_refs_device("wps", wps=wps)
        n.solve()
        us.append(n.ocp.field("u0").numpy().reshape(B, 4))
        its.append(n.ocp.iters.copy())
        sts.append(n.ocp.status.copy())
        dx.upload(xs[-1])
        _lib.plant_step(ctx, plant, B, dx, n.ocp.field("u0"), dx)
        xs.append(dx.numpy())
    return np.stack(xs, 1), np.stack(us, 1), np.stack(sts, 1), np.stack(its, 1)


def _check_log(r, scene, dt):
    """t, the clearance at the rows' own times, and swept=True's fields against a direct call on the log's chords"""
    np.testing.assert_array_equal(r.t, np.array([T0 + j * dt for j in range(K + 1)]))
    pts = r.x[:, :, :3].reshape(-1, 3)
    np.testing.assert_array_equal(r.clearance, scene.distance(pts, t=np.tile(r.t, B)).reshape(B, K + 1))
    assert (scene.distance(pts) != r.clearance.ravel()).any()  # the rows' times reached the kernel
    p0, p1 = r.x[:, :-1, :3].reshape(-1, 3), r.x[:, 1:, :3].reshape(-1, 3)
    s = scene.swept_distance(p0, p1, t0=np.tile(r.t[:-1], B), t1=np.tile(r.t[1:], B), eps=1e-3)
    np.testing.assert_array_equal(r.swept_clearance, s.dmin.reshape(B, K))
    np.testing.assert_array_equal(r.swept_gap, s.gap.reshape(B, K))
    np.testing.assert_array_equal(r.swept_s, s.s.reshape(B, K))
    assert (r.swept_clearance <= np.minimum(r.clearance[:, :-1], r.clearance[:, 1:])).all()


@pytest.mark.parametrize("every", [1, 2])
def test_perceiving_rollout_equals_host_driven_loop_bitwise(every):
    cfg = Config(mpc__N=10)
    wps = _wps()
    na, x0, sa, va = _make(cfg)
    nb, _, sb, vb = _make(cfg)
    assert sa.is_instanced and sa.is_dynamic and not sa.is_mesh
    dt = float(na.ocp.dt[0])
    na.set_x0(x0)
    r = na.rollout(K, refs="wps", wps=wps, scene=sa, vae=va, perceive_every=every, img_shape=SHAPE, keep_img=True,
                   scene_t0=T0, scene_dt=dt, swept=True)
    x, u, status, iters = _perceiving_host_loop(nb, vb, sb, x0, K, every, wps, T0)
    np.testing.assert_array_equal(r.x, x)
    np.testing.assert_array_equal(r.u, u)
    np.testing.assert_array_equal(r.status, status)
    np.testing.assert_array_equal(r.iters, iters)
    pa, pb = na.ocp.download("p"), nb.ocp.download("p")
    np.testing.assert_array_equal(pa, pb)
    assert np.abs(pa[:, :, 17:]).max() > 0 and np.ptp(r.u[:, :, 0]) > 1e-3
    np.testing.assert_array_equal(va.latent64.numpy(), vb.latent64.numpy())
    k_last = (K - 1) // every * every
    want = sb.render_from_state(r.x[:, k_last], cfg, SHAPE, normalized=False, t=T0 + k_last * dt).numpy()
    np.testing.assert_array_equal(r.img, want)
    stale = sb.render_from_state(r.x[:, k_last], cfg, SHAPE, normalized=False).numpy()
    assert (r.img != stale).any() and (r.img == stale).any()  # the clock reached the kernel; the floor stands
    _check_log(r, sa, dt)
    for m in (na, nb):
        m.ocp.close()


@pytest.mark.parametrize("predict", [True, False])
def test_scene_source_rollout_equals_host_driven_loop_bitwise(predict):
    cfg = Config(mpc__N=10)
    wps = _wps()
    out = []
    for _ in range(2):
        n, x0 = _setup(cfg, B, 21)
        scene = _scene(n.ocp.ctx)
        n.set_sdf_scene(scene, max_df=MAX_DF, predict=predict)
        out.append((n, scene))
    (na, sa), (nb, sb) = out
    na.set_x0(x0)
    r = na.rollout(K, refs="wps", wps=wps, perceive_every=2, scene_t0=T0, swept=True)
    x, u, status, iters = _source_host_loop(nb, sb, x0, K, 2, wps, T0)
    np.testing.assert_array_equal(r.x, x)
    np.testing.assert_array_equal(r.u, u)
    np.testing.assert_array_equal(r.status, status)
    np.testing.assert_array_equal(r.iters, iters)
    for k in ("p", "h", "Jh"):
        np.testing.assert_array_equal(na.ocp.download(k), nb.ocp.download(k))
    h = na.ocp.download("h")
    assert (r.iters > 0).all() and (h[..., 2] < h[..., 2].max()).any()  # the source reached the rows: not all truncated
    _check_log(r, sa, float(na.ocp.dt[0]))
    for m in (na, nb):
        m.ocp.close()


def test_predict_shows_the_nodes_the_instances_at_their_own_times():
    cfg = Config(mpc__N=10)
    wps = _wps()
    us = []
    for predict in (True, False):
        n, x0 = _setup(cfg, B, 21)
        n.set_sdf_scene(_scene(n.ocp.ctx), max_df=MAX_DF, predict=predict)
        n.set_x0(x0)
        us.append(n.rollout(K, refs="wps", wps=wps, perceive_every=2, scene_t0=T0).u)
        n.ocp.close()
    assert (us[0] != us[1]).any()


def test_two_chunks_are_the_uncut_rollout():
    """Steps 0..2 and 3..5 with perceive_phase = 3 for the second chunk: the perception schedule and the scene's clock
    of the uncut rollout, bit for bit in x, u, p, t and the clearance."""
    cfg = Config(mpc__N=10)
    wps = _wps()
    n, x0, sc, vae = _make(cfg)
    n.set_x0(x0)
    a = n.rollout(3, refs="wps", wps=wps, scene=sc, vae=vae, perceive_every=2, img_shape=SHAPE, scene_t0=T0)
    b = n.rollout(3, refs="wps", wps=wps, scene=sc, vae=vae, perceive_every=2, img_shape=SHAPE, scene_t0=T0,
                  perceive_phase=3)
    m, _, sc2, vae2 = _make(cfg)
    m.set_x0(x0)
    whole = m.rollout(K, refs="wps", wps=wps, scene=sc2, vae=vae2, perceive_every=2, img_shape=SHAPE, scene_t0=T0)
    np.testing.assert_array_equal(whole.x, np.concatenate([a.x, b.x[:, 1:]], 1))
    np.testing.assert_array_equal(whole.u, np.concatenate([a.u, b.u], 1))
    np.testing.assert_array_equal(m.ocp.download("p"), n.ocp.download("p"))
    np.testing.assert_array_equal(whole.t, np.concatenate([a.t, b.t[1:]]))
    np.testing.assert_array_equal(a.t[-1:], b.t[:1])
    np.testing.assert_array_equal(whole.clearance, np.concatenate([a.clearance, b.clearance[:, 1:]], 1))
    n.ocp.close()
    m.ocp.close()
