"""Rollouts in a mesh scene with movers (Scene.mesh(..., movers=), csrc/scene_mesh.hip's *_mesh_mixed kernels): a rough
tunnel around the start states with a sphere crossing it, as the image the encoder sees (perception inside the loop,
with the scene's clock) and as the SDF source (set_sdf_scene with predict) -- bitwise against the host-driven loops of
tests/test_gpu_rollout_dyn.py and tests/test_gpu_rollout_scene_sdf.py, the clearance against the two scenes that
kernels from before this feature answer, the swept clearance against a direct call on the log, a rollout cut into
chunks, and the brute-force hierarchy.  N = 10, B = 3, K = 6, 18 x 32 images.  The network weights are synthetic: no
clearance here says anything about the controller.

Every test here fails without the feature: Scene.mesh has no ``movers``."""
import numpy as np
import pytest

import scene_mixed_ref as M
from sdf_nmpc_amd.config import Config
from sdf_nmpc_amd.mesh import Mesh
from sdf_nmpc_amd.scene import Scene
from sdf_nmpc_amd.vae import VaeWrapper
from test_gpu_rollout import _setup
from test_gpu_rollout_dyn import _host_loop as _perceiving_host_loop
from test_gpu_rollout_perceive import B, K, SHAPE, _wps
from test_gpu_rollout_scene_sdf import _host_loop as _source_host_loop

pytestmark = [pytest.mark.gpu, pytest.mark.filterwarnings("ignore:no SDF weights"),
              pytest.mark.filterwarnings("ignore:QP reached")]

T0, MAX_DF = 0.5, 3.0
# around the start states of test_gpu_rollout._setup (positions in [-1, 1]^3): a tunnel of radius 2 along x, and a sphere
# that crosses it through the start states, with a slower box behind
TUNNEL = Mesh.tunnel([(-5, 0, 0), (-2, 0.3, 0.1), (1, -0.2, 0.2), (4, 0.2, -0.1), (7, 0, 0)], 2.0, segments=12, roughness=0.1,
                     seed=3)
MOVERS = [Scene.moving(Scene.sphere((0.6, -1.4, 0.1), 0.4), v=(0.0, 1.2, 0.0)),
          Scene.moving(Scene.box((1.8, -0.3, -0.4), (2.2, 0.3, 0.4)), rpy=(0.0, 0.1, 0.4), yaw_rate=0.5, v=(-0.4, 0.0, 0.0))]
FIELDS = ("x", "u", "status", "iters", "t", "clearance")


@pytest.fixture(scope="module", autouse=True)
def _torch_first(gpu_ctx):
    """torch opens the device before the first controller of this module does, as in tests/test_gpu_rollout.py."""


def _scene(ctx, **kw):
    return Scene.mesh(ctx, TUNNEL, sdf_source=True, movers=MOVERS, **kw)


def _make(cfg, seed=21, **kw):
    n, x0 = _setup(cfg, B, seed)
    ctx = n.ocp.ctx
    return n, x0, _scene(ctx, **kw), VaeWrapper(cfg, batch=B, ctx=ctx)


def _two_scenes_clearance(ctx, r):
    """min(M.distance, D.distance at Rollout.t) at every logged position: the scenes existing kernels answer"""
    Ms, Ds = Scene.mesh(ctx, TUNNEL), Scene(ctx, MOVERS)
    pts = r.x[:, :, :3].reshape(-1, 3)
    want = M.distance(Ms.distance(pts), Ds.distance(pts, t=np.tile(r.t, B))).reshape(B, -1)
    moved = (Ds.distance(pts) != Ds.distance(pts, t=np.tile(r.t, B))).any()
    from_both = (Ms.distance(pts) < Ds.distance(pts, t=np.tile(r.t, B))).any() and \
        (Ms.distance(pts) > Ds.distance(pts, t=np.tile(r.t, B))).any()
    Ms.close()
    Ds.close()
    return want, moved, from_both


def _check_swept(r, scene):
    """swept=True fills the three fields with what a direct call on the log's chords gives"""
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
    assert sa.is_dynamic and sa.is_mesh and not sa.is_indexed
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
    # the last images: the last perceiving step's, of the scene at that step's time -- the mover and the tunnel both in them
    k_last = (K - 1) // every * every
    want = sb.render_from_state(r.x[:, k_last], cfg, SHAPE, normalized=False, t=T0 + k_last * dt).numpy()
    np.testing.assert_array_equal(r.img, want)
    stale = sb.render_from_state(r.x[:, k_last], cfg, SHAPE, normalized=False).numpy()
    assert (r.img != stale).any() and (r.img == stale).any()  # the clock reached the kernel; the tunnel stands
    # t, the clearance and the swept clearance
    np.testing.assert_array_equal(r.t, np.array([T0 + j * dt for j in range(K + 1)]))
    want_c, moved, _ = _two_scenes_clearance(na.ocp.ctx, r)
    np.testing.assert_array_equal(r.clearance, want_c)
    assert moved and r.clearance.shape == (B, K + 1)
    _check_swept(r, sa)
    for m in (na, nb):
        m.ocp.close()


def test_scene_source_rollout_equals_host_driven_loop_bitwise():
    cfg = Config(mpc__N=10)
    wps = _wps()
    out = []
    for predict in (True, True, False):
        n, x0 = _setup(cfg, B, 21)
        scene = _scene(n.ocp.ctx)
        n.set_sdf_scene(scene, max_df=MAX_DF, predict=predict)
        out.append((n, scene))
    (na, sa), (nb, sb), (nc, _) = out
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
    dt = float(na.ocp.dt[0])
    np.testing.assert_array_equal(r.t, T0 + np.arange(K + 1) * dt)
    want_c, moved, from_both = _two_scenes_clearance(na.ocp.ctx, r)
    np.testing.assert_array_equal(r.clearance, want_c)
    assert moved and from_both  # the nearest thing is the tunnel at some rows and a mover at others
    _check_swept(r, sa)
    # the movers are seen at the node times: predict changes the controls
    nc.set_x0(x0)
    rc = nc.rollout(K, refs="wps", wps=wps, perceive_every=2, scene_t0=T0)
    assert (rc.u != r.u).any()
    for m in (na, nb, nc):
        m.ocp.close()


def test_predict_changes_no_bit_for_a_plain_mesh_scene():
    cfg = Config(mpc__N=10)
    wps = _wps()
    rs = []
    for predict in (True, False):
        n, x0 = _setup(cfg, B, 21)
        scene = Scene.mesh(n.ocp.ctx, TUNNEL, sdf_source=True, movers=[])
        assert scene.is_mesh and not scene.is_dynamic
        n.set_sdf_scene(scene, max_df=MAX_DF, predict=predict)
        n.set_x0(x0)
        rs.append(n.rollout(K, refs="wps", wps=wps, perceive_every=2, scene_t0=T0))
        n.ocp.close()
    for k in FIELDS:
        np.testing.assert_array_equal(getattr(rs[0], k), getattr(rs[1], k), err_msg=k)


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


def test_the_brute_force_hierarchy_changes_no_field():
    cfg = Config(mpc__N=10)
    wps = _wps()
    rs = []
    for leaf in (None, -1):
        n, x0, sc, vae = _make(cfg, leaf_size=leaf)
        n.set_x0(x0)
        rs.append(n.rollout(K, refs="wps", wps=wps, scene=sc, vae=vae, perceive_every=2, img_shape=SHAPE, keep_img=True,
                            scene_t0=T0, swept=True))
        n.set_sdf_scene(sc, max_df=MAX_DF, predict=True)
        n.set_x0(x0)
        rs.append(n.rollout(K, refs="wps", wps=wps, perceive_every=2, scene_t0=T0, swept=True))
        n.ocp.close()
    for a, b in ((rs[0], rs[2]), (rs[1], rs[3])):
        for k in FIELDS + ("swept_clearance", "swept_gap", "swept_s"):
            np.testing.assert_array_equal(getattr(a, k), getattr(b, k), err_msg=k)
    np.testing.assert_array_equal(rs[0].img, rs[2].img)
