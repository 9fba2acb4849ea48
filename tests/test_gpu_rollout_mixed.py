"""Rollouts in a mixed scene (Scene(..., grid=True, movers=), csrc/scene_grid.hip's *_mixed kernels): a forest of 16
cylinders behind a grid with three movers crossing it, as the image the encoder sees (perception inside the loop, with
the scene's clock) and as the SDF source (set_sdf_scene with predict) -- bitwise against the host-driven loops of
tests/test_gpu_rollout_dyn.py and tests/test_gpu_rollout_scene_sdf.py, the clearance against the two scenes that
existing kernels answer, and a rollout cut into chunks.  N = 10, B = 3, K = 6, 18 x 32 images."""
import numpy as np
import pytest

import scene_mixed_ref as M
from sdf_nmpc_amd.config import Config
from sdf_nmpc_amd.scene import Scene
from sdf_nmpc_amd.vae import VaeWrapper
from test_gpu_rollout import _setup
from test_gpu_rollout_dyn import _host_loop as _perceiving_host_loop
from test_gpu_rollout_perceive import B, K, SHAPE, _wps
from test_gpu_rollout_scene_sdf import _host_loop as _source_host_loop

pytestmark = [pytest.mark.gpu, pytest.mark.filterwarnings("ignore:no SDF weights"),
              pytest.mark.filterwarnings("ignore:QP reached")]

T0 = 0.5
# around the start states of test_gpu_rollout._setup (positions in [-1, 1]^3), which the forest keeps clear
STATICS = Scene.forest(16, (-4.0, -4.0, -2.0), (4.0, 4.0, 2.0), radius=(0.15, 0.4), seed=1, keep_clear=((0.0, 0.0), 1.8))
MOVERS = [Scene.moving(Scene.sphere((2.6, 0.4, 0.2), 0.4), v=(-0.6, 0.0, 0.0)),
          Scene.moving(Scene.box((-0.3, 2.0, -1.0), (0.3, 2.4, 1.0)), rpy=(0.0, 0.1, 0.4), yaw_rate=0.5, v=(0.0, -0.4, 0.0)),
          Scene.crowd(1, (-3.0, -3.0, -1.0), (3.0, 3.0, 1.0), seed=3)[0]]


@pytest.fixture(scope="module", autouse=True)
def _torch_first(gpu_ctx):
    """torch opens the device before the first controller of this module does, as in tests/test_gpu_rollout.py."""


def _mixed(ctx):
    return Scene(ctx, STATICS, grid=True, movers=MOVERS)


def _make(cfg, seed=21):
    n, x0 = _setup(cfg, B, seed)
    ctx = n.ocp.ctx
    return n, x0, _mixed(ctx), VaeWrapper(cfg, batch=B, ctx=ctx)


def _two_scenes_clearance(ctx, r):
    """min(G.distance, D.distance at Rollout.t) at every logged position: the scenes existing kernels answer"""
    G, D = Scene(ctx, STATICS, grid=True), Scene(ctx, MOVERS)
    pts = r.x[:, :, :3].reshape(-1, 3)
    want = M.distance(G.distance(pts), D.distance(pts, t=np.tile(r.t, B))).reshape(B, -1)
    moved = (D.distance(pts) != D.distance(pts, t=np.tile(r.t, B))).any()
    G.close()
    D.close()
    return want, moved


@pytest.mark.parametrize("every", [1, 2])
def test_perceiving_rollout_equals_host_driven_loop_bitwise(every):
    cfg = Config(mpc__N=10)
    wps = _wps()
    na, x0, sa, va = _make(cfg)
    nb, _, sb, vb = _make(cfg)
    assert sa.is_dynamic and sa.is_indexed
    dt = float(na.ocp.dt[0])
    na.set_x0(x0)
    r = na.rollout(K, refs="wps", wps=wps, scene=sa, vae=va, perceive_every=every, img_shape=SHAPE, keep_img=True,
                   scene_t0=T0, scene_dt=dt)
    x, u, status, iters = _perceiving_host_loop(nb, vb, sb, x0, K, every, wps, T0)
    np.testing.assert_array_equal(r.x, x)
    np.testing.assert_array_equal(r.u, u)
    np.testing.assert_array_equal(r.status, status)
    np.testing.assert_array_equal(r.iters, iters)
    pa, pb = na.ocp.download("p"), nb.ocp.download("p")
    np.testing.assert_array_equal(pa, pb)
    assert np.abs(pa[:, :, 17:]).max() > 0 and np.ptp(r.u[:, :, 0]) > 1e-3
    np.testing.assert_array_equal(va.latent64.numpy(), vb.latent64.numpy())
    # the last images: the last perceiving step's, of the scene at that step's time -- movers and forest both in them
    k_last = (K - 1) // every * every
    want = sb.render_from_state(r.x[:, k_last], cfg, SHAPE, normalized=False, t=T0 + k_last * dt).numpy()
    np.testing.assert_array_equal(r.img, want)
    stale = sb.render_from_state(r.x[:, k_last], cfg, SHAPE, normalized=False).numpy()
    assert (r.img != stale).any() and (r.img == stale).any()  # the clock reached the kernel; the forest stands
    # t and the clearance
    np.testing.assert_array_equal(r.t, np.array([T0 + j * dt for j in range(K + 1)]))
    want_c, moved = _two_scenes_clearance(na.ocp.ctx, r)
    np.testing.assert_array_equal(r.clearance, want_c)
    assert moved and r.clearance.shape == (B, K + 1)
    for m in (na, nb):
        m.ocp.close()


def test_scene_source_rollout_equals_host_driven_loop_bitwise():
    cfg = Config(mpc__N=10)
    wps = _wps()
    out = []
    for _ in range(2):
        n, x0 = _setup(cfg, B, 21)
        scene = _mixed(n.ocp.ctx)
        n.set_sdf_scene(scene, predict=True)
        out.append((n, scene))
    (na, sa), (nb, sb) = out
    na.set_x0(x0)
    r = na.rollout(K, refs="wps", wps=wps, perceive_every=2, scene_t0=T0)
    x, u, status, iters = _source_host_loop(nb, sb, x0, K, 2, wps, T0)
    np.testing.assert_array_equal(r.x, x)
    np.testing.assert_array_equal(r.u, u)
    np.testing.assert_array_equal(r.status, status)
    np.testing.assert_array_equal(r.iters, iters)
    for k in ("p", "h", "Jh"):
        np.testing.assert_array_equal(na.ocp.download(k), nb.ocp.download(k))
    h = na.ocp.download("h")
    assert (r.iters > 0).all() and (h[..., 2] < h[..., 2].max()).any()  # the source reached the rows: not all truncated
    # the rows of the last step are those of the two scenes, selected: movers at the node times (predict)
    dt = float(na.ocp.dt[0])
    np.testing.assert_array_equal(r.t, T0 + np.arange(K + 1) * dt)
    want_c, moved = _two_scenes_clearance(na.ocp.ctx, r)
    np.testing.assert_array_equal(r.clearance, want_c)
    assert moved
    for m in (na, nb):
        m.ocp.close()


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
