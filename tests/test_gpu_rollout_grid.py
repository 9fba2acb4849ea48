"""Rollouts in an indexed scene (Scene(..., grid=True), csrc/scene_grid.hip): a scene of 20 primitives gives, with
and without the grid, the same bits in every field of ``Rollout`` -- as the image the encoder sees (perception inside
the loop) and as the SDF source (set_sdf_scene) -- and a forest of 200 cylinders, which no plain scene holds, is held
against the brute-force kernels on chunks of 32 (tests/scene_grid_ref.py).  N = 10, B = 4, K = 3, 18 x 32 images."""
import numpy as np
import pytest

import scene_grid_ref as G
import scene_ref as R
from sdf_nmpc_amd.config import Config
from sdf_nmpc_amd.reference import yaw2quat
from sdf_nmpc_amd.scene import Scene
from sdf_nmpc_amd.vae import VaeWrapper
from test_gpu_rollout import _setup

pytestmark = [pytest.mark.gpu, pytest.mark.filterwarnings("ignore:no SDF weights"),
              pytest.mark.filterwarnings("ignore:QP reached")]

B, K, SHAPE = 4, 3, (18, 32)
# 20 primitives around the start states of test_gpu_rollout._setup (positions in [-1, 1]^3)
SMALL = Scene.forest(16, (-4.0, -4.0, -2.0), (4.0, 4.0, 2.0), radius=(0.15, 0.4), seed=1, keep_clear=((0.0, 0.0), 1.8)) + \
    list(R.SCENE)
FOREST = Scene.forest(200, (-9.0, -9.0, -2.0), (9.0, 9.0, 2.0), radius=(0.15, 0.4), seed=2, keep_clear=((0.0, 0.0), 2.2))


@pytest.fixture(scope="module", autouse=True)
def _torch_first(gpu_ctx):
    """torch opens the device before the first controller of this module does, as in tests/test_gpu_rollout.py."""


def _wps():
    rng = np.random.default_rng(5)
    return (rng.uniform(-2, 2, (B, 2, 3)), np.stack([[yaw2quat(a) for a in row] for row in rng.uniform(-1, 1, (B, 2))]))


def _fields_equal(a, b, fields):
    for f in fields:
        np.testing.assert_array_equal(getattr(a, f), getattr(b, f), err_msg=f)


def _perceiving(cfg, prims, grid):
    n, x0 = _setup(cfg, B, 21)
    scene = Scene(n.ocp.ctx, prims, grid=grid)
    vae = VaeWrapper(cfg, batch=B, ctx=n.ocp.ctx)
    n.set_x0(x0)
    r = n.rollout(K, refs="wps", wps=_wps(), scene=scene, vae=vae, perceive_every=1, img_shape=SHAPE, keep_img=True)
    return n, scene, r


def test_perceiving_rollout_equals_the_plain_scene_bitwise():
    assert len(SMALL) == 20
    cfg = Config(mpc__N=10)
    na, sa, ra = _perceiving(cfg, SMALL, True)
    nb, sb, rb = _perceiving(cfg, SMALL, False)
    assert sa.is_indexed and not sb.is_indexed
    _fields_equal(ra, rb, ("x", "u", "status", "iters", "img", "clearance"))
    np.testing.assert_array_equal(na.ocp.download("p"), nb.ocp.download("p"))
    assert ra.img.shape == (B,) + SHAPE and np.ptp(ra.img) > 0 and np.ptp(ra.u[:, :, 0]) > 1e-3
    assert np.isfinite(ra.clearance).all() and ra.clearance.shape == (B, K + 1)
    for m in (na, nb):
        m.ocp.close()


def test_scene_source_rollout_equals_the_plain_scene_bitwise():
    cfg = Config(mpc__N=10)
    out = []
    for grid in (True, False):
        n, x0 = _setup(cfg, B, 21)
        scene = Scene(n.ocp.ctx, SMALL, grid=grid)
        n.set_sdf_scene(scene)
        n.set_x0(x0)
        r = n.rollout(K, refs="wps", wps=_wps(), perceive_every=1)
        out.append((n, r, n.ocp.download("h"), n.ocp.download("Jh")))
    (na, ra, ha, Ja), (nb, rb, hb, Jb) = out
    _fields_equal(ra, rb, ("x", "u", "status", "iters", "clearance"))
    np.testing.assert_array_equal(ha, hb)
    np.testing.assert_array_equal(Ja, Jb)
    assert (ra.iters > 0).all() and (ha[..., 2] < ha[..., 2].max()).any()  # the source reached the rows: not all truncated
    for m in (na, nb):
        m.ocp.close()


def test_forest_of_200_against_the_chunked_brute_force():
    cfg = Config(mpc__N=10)
    n, scene, r = _perceiving(cfg, FOREST, True)
    ctx = n.ocp.ctx
    assert scene.is_indexed and (r.iters > 0).all()
    # the image the encoder last saw: the raw sensor image from the state before the last step
    ps = scene.pose(r.x[:, K - 1], cfg)
    want = G.chunked_render(ctx, FOREST, ps["W_p_C"], ps["W_R_C"], cfg, SHAPE, normalized=False)
    np.testing.assert_array_equal(r.img, want)
    raw_dmax = float(cfg.sensor.dmax) * Scene.scale(cfg, normalized=False)
    assert (want < raw_dmax).any()  # trees in sight
    np.testing.assert_array_equal(r.clearance, G.chunked_distance(ctx, FOREST, r.x[:, :, :3].reshape(-1, 3)).reshape(B, K + 1))
    assert np.isfinite(r.clearance).all() and r.clearance.max() < 5.0
    n.ocp.close()
