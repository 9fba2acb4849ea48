"""Rollouts in a mesh scene (Scene.mesh, csrc/scene_mesh.hip): the perceiving rollout with the hierarchy gives the bits
of the same rollout without one (leaf_size = -1) in every field of ``Rollout`` -- states, inputs, status, the kept
images, the clearance of the log and the swept clearance between its rows -- and the same with a sensor model and a
vehicle model in the loop, which reach the mesh through the same dispatch.  N = 10, B = 2, K = 3, 18 x 32 images, one
scene per instance: the fixed scene as a mesh, and a cave around the start states."""
import numpy as np
import pytest

import mesh_ref as M
from sdf_nmpc_amd.config import Config
from sdf_nmpc_amd.mesh import Mesh
from sdf_nmpc_amd.reference import yaw2quat
from sdf_nmpc_amd.scene import Scene
from sdf_nmpc_amd.sensor import SensorModel
from sdf_nmpc_amd.vae import VaeWrapper
from sdf_nmpc_amd.vehicle import VehicleModel
from test_gpu_rollout import _setup

pytestmark = [pytest.mark.gpu, pytest.mark.filterwarnings("ignore:no SDF weights"),
              pytest.mark.filterwarnings("ignore:QP reached")]

B, K, SHAPE = 2, 3, (18, 32)
SCENE_OF = [0, 1]
# the start positions lie in [-1, 1]^3 (test_gpu_rollout._setup): the cave's axis passes through that cube
CAVE = Mesh.tunnel([(-4, -0.5, 0), (-1.5, 0.3, 0.2), (1, -0.2, -0.1), (3.5, 0.4, 0.1), (6, 0, 0)], 2.6, segments=14,
                   roughness=0.15, seed=5)
MESHES = [M.fixed_scene(), CAVE]
SENSOR_SEED = 0x5E4502                     # tests/test_gpu_rollout_sensor.py's model
BITES = dict(delay=2, gust_std=1.0, gust_tau=0.3, est_std_pos=0.05, est_std_vel=0.02, est_std_yaw=0.01)  # ..._vehicle.py's


@pytest.fixture(scope="module", autouse=True)
def _torch_first(gpu_ctx):
    """torch opens the device before the first controller of this module does, as in tests/test_gpu_rollout.py."""


def _wps():
    rng = np.random.default_rng(5)
    return (rng.uniform(-2, 2, (B, 2, 3)), np.stack([[yaw2quat(a) for a in row] for row in rng.uniform(-1, 1, (B, 2))]))


def _run(cfg, leaf, models):
    n, x0 = _setup(cfg, B, 21)
    ctx = n.ocp.ctx
    scene = Scene.mesh(ctx, MESHES, scene_of=SCENE_OF, leaf_size=leaf)
    assert scene.is_mesh and not scene.is_dynamic and not scene.is_indexed
    kw = {}
    if models:
        kw = dict(sensor=SensorModel.reference_augment(cfg, ctx, SENSOR_SEED, outlier_rm=True, min_range=0.1, miss_invalid=True),
                  vehicle=VehicleModel(cfg, ctx, B, seed=17, **BITES))
    n.set_x0(x0)
    r = n.rollout(K, refs="wps", wps=_wps(), scene=scene, vae=VaeWrapper(cfg, batch=B, ctx=ctx), perceive_every=1,
                  img_shape=SHAPE, keep_img=True, swept=True, **kw)
    return n, scene, r


@pytest.mark.parametrize("models", [False, True], ids=["plain", "sensor_and_vehicle"])
def test_rollout_with_the_hierarchy_equals_the_rollout_without_bitwise(models):
    cfg = Config(mpc__N=10)
    na, sa, ra = _run(cfg, None, models)
    nb, sb, rb = _run(cfg, -1, models)
    fields = ("x", "u", "status", "iters", "clearance", "swept_clearance", "swept_gap", "swept_s") + (("xhat",) if models else ())
    for f in fields:
        np.testing.assert_array_equal(getattr(ra, f), getattr(rb, f), err_msg=f)
    np.testing.assert_array_equal(ra.img.view(np.uint32), rb.img.view(np.uint32))
    np.testing.assert_array_equal(na.ocp.download("p"), nb.ocp.download("p"))
    raw_dmax = np.float32(float(cfg.sensor.dmax) * Scene.scale(cfg, normalized=False))
    assert ra.img.shape == (B,) + SHAPE and ra.img.dtype == np.float32
    assert all((ra.img[b] < raw_dmax).any() for b in range(B))          # both instances have their mesh in sight
    assert np.ptp(ra.u[:, :, 0]) > 1e-3 and (ra.iters > 0).all()
    # the logged clearance is the mesh's distance at the logged positions, and the swept one the same kernel on the chords
    p2s = np.repeat(SCENE_OF, K + 1)
    np.testing.assert_array_equal(ra.clearance, sa.distance(ra.x[:, :, :3].reshape(-1, 3), p2s).reshape(B, K + 1))
    d = sb.swept_distance(ra.x[:, :-1, :3].reshape(-1, 3), ra.x[:, 1:, :3].reshape(-1, 3), np.repeat(SCENE_OF, K), eps=1e-3)
    np.testing.assert_array_equal(ra.swept_clearance, d.dmin.reshape(B, K))
    assert np.isfinite(ra.clearance).all() and (ra.clearance >= 0).all() and ra.clearance.shape == (B, K + 1)
    assert (ra.clearance[1] > 1.0).all() and (ra.clearance[1] < 4.0).all()  # inside the cave, off its wall
    assert (ra.swept_clearance <= np.minimum(ra.clearance[:, :-1], ra.clearance[:, 1:]) + 1e-9).all()
    assert (ra.swept_gap <= 1e-3 + 1e-12).all()
    for m in (na, nb):
        m.ocp.close()
