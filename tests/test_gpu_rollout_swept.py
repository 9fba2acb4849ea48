"""Swept clearance in the rollout log (Nmpc.rollout(swept=), controller._log_swept): entry k of swept_clearance /
swept_gap / swept_s covers log rows k -> k+1 of the plant between t[k] and t[k+1].  B = 2, N = 20, K = 6, in a static
scene of three primitives and in one with a mover that crosses the flight, with the scene perceived (scene=, vae=) and
with the scene as the controller's SDF source (set_sdf_scene)."""
import numpy as np
import pytest

import scene_dyn_ref as D
import scene_ref as R
import swept_ref as W
from sdf_nmpc_amd.config import Config
from sdf_nmpc_amd.scene import Scene
from sdf_nmpc_amd.vae import VaeWrapper
from test_gpu_rollout import _setup

pytestmark = [pytest.mark.gpu, pytest.mark.filterwarnings("ignore:no SDF weights"),
              pytest.mark.filterwarnings("ignore:QP reached")]

B, K, SHAPE, T0 = 2, 6, (18, 32), 0.25
STATIC = R.SCENE[:3]
# the start positions lie in [-1, 1]^3 (test_gpu_rollout._setup): a sphere that crosses that cube during the 0.45 s flown
CROSSING = [(R.SCENE[0], None), (R.SCENE[1], None), (("sphere", [-2.5, 0.1, 0.0, 0.4]), dict(v=(6.0, 0.0, 0.0)))]


@pytest.fixture(scope="module", autouse=True)
def _torch_first(gpu_ctx):
    """torch opens the device before the first controller of this module does, as in tests/test_gpu_rollout.py."""


def _make(cfg, moving, source):
    n, x0 = _setup(cfg, B, 21)
    ctx = n.ocp.ctx
    prims = [Scene.moving(p, **kw) if kw is not None else p for p, kw in CROSSING] if moving else STATIC
    scene = Scene(ctx, prims)
    kw = dict(scene_t0=T0)
    if source:
        n.set_sdf_scene(scene)
    else:
        kw.update(scene=scene, vae=VaeWrapper(cfg, batch=B, ctx=ctx), img_shape=SHAPE)
    n.set_x0(x0)
    return n, scene, kw


@pytest.mark.parametrize("source", [False, True])
@pytest.mark.parametrize("moving", [False, True])
def test_swept_clearance_of_the_log(moving, source):
    cfg = Config(mpc__N=20)
    na, sa, kwa = _make(cfg, moving, source)
    nb, sb, kwb = _make(cfg, moving, source)
    assert sa.is_dynamic == moving
    r = na.rollout(K, swept=True, **kwa)
    plain = nb.rollout(K, **kwb)
    # without swept nothing changes and nothing is computed
    assert plain.swept_clearance is None and plain.swept_gap is None and plain.swept_s is None
    for k in ("x", "u", "status", "clearance"):
        np.testing.assert_array_equal(getattr(r, k), getattr(plain, k))
    for a in (r.swept_clearance, r.swept_gap, r.swept_s):
        assert a.shape == (B, K) and a.dtype == np.float64
    # the same kernel on the same inputs: a direct call on the log, bit for bit
    p0, p1 = r.x[:, :-1, :3].reshape(-1, 3), r.x[:, 1:, :3].reshape(-1, 3)
    t0, t1 = np.tile(r.t[:-1], B), np.tile(r.t[1:], B)
    d = sa.swept_distance(p0, p1, t0=t0, t1=t1, eps=1e-3)
    np.testing.assert_array_equal(r.swept_clearance, d.dmin.reshape(B, K))
    np.testing.assert_array_equal(r.swept_gap, d.gap.reshape(B, K))
    np.testing.assert_array_equal(r.swept_s, d.s.reshape(B, K))
    # between the two rows' clearances: never above the smaller one, and D is L-Lipschitz in s, so not more than L / 2
    # below it
    V = W.speed_bound(D.scene(CROSSING)) if moving else 0.0
    assert abs(sa.speed_bound[0] - V) <= 1e-12 * V
    L = np.linalg.norm(r.x[:, 1:, :3] - r.x[:, :-1, :3], axis=2) + V * np.abs(np.diff(r.t))[None]
    ends = np.minimum(r.clearance[:, :-1], r.clearance[:, 1:])
    below = ends - r.swept_clearance
    print(f"\nmoving {moving}, source {source}: min(c[k], c[k+1]) - swept in [{below.min():.2e}, {below.max():.2e}], L / 2 <= "
          f"{L.max() / 2:.3f}, gap <= {r.swept_gap.max():.1e}, clearance {r.clearance.min():.3f}, swept "
          f"{r.swept_clearance.min():.3f}")
    assert (r.swept_clearance <= ends + 1e-9).all()
    assert (r.swept_clearance >= ends - L / 2 - 1e-9).all()
    assert (r.swept_gap <= 1e-3 + 1e-12).all() and ((r.swept_s >= 0) & (r.swept_s <= 1)).all()
    for m in (na, nb):
        m.ocp.close()


def test_swept_needs_a_scene():
    cfg = Config(mpc__N=20)
    n, x0 = _setup(cfg, B, 21)
    n.set_x0(x0)
    n.rollout(1)  # flush the host setters, so that the device fields are settled
    before = {k: n.ocp.download(k) for k in ("x", "u", "p", "x0")}
    with pytest.raises(ValueError, match="swept"):
        n.rollout(2, swept=True)  # no scene and no scene source: no clearance either
    for k, v in before.items():
        np.testing.assert_array_equal(n.ocp.download(k), v)
    scene = Scene(n.ocp.ctx, STATIC)
    n.set_sdf_scene(scene)
    for bad in (0.0, 1e-7, float("nan")):
        with pytest.raises(ValueError, match="swept"):
            n.rollout(2, swept=bad)
    n.set_sdf_scene(None)
    r = n.rollout(2)
    assert r.swept_clearance is None and r.clearance is None
    scene.close()
    n.ocp.close()


def test_swept_eps_reaches_the_kernel():
    cfg = Config(mpc__N=20)
    n, scene, kw = _make(cfg, True, True)
    r = n.rollout(K, swept=1e-5, **kw)
    assert (r.swept_gap <= 1e-5 + 1e-12).all()
    d = scene.swept_distance(r.x[:, :-1, :3].reshape(-1, 3), r.x[:, 1:, :3].reshape(-1, 3), t0=np.tile(r.t[:-1], B),
                             t1=np.tile(r.t[1:], B), eps=1e-5)
    np.testing.assert_array_equal(r.swept_clearance, d.dmin.reshape(B, K))
    n.ocp.close()
