"""The rigid-body vehicle inside the device rollouts (Nmpc.rollout(vehicle=model with a body)): bitwise against the
host-driven loop begin; [set_x0(estimate); gen_refs_device; solve; vehicle.step], the omega / rotor log rows, the
clearance of a scene-source rollout at the body's true positions, and the refusals.  B = 3, N = 10, K = 4."""
import math

import numpy as np
import pytest

import body_cases as BC
import scene_ref as R
from sdf_nmpc_amd import _lib
from sdf_nmpc_amd.config import Config
from sdf_nmpc_amd.scene import Scene
from sdf_nmpc_amd.vehicle import RigidBody, VehicleModel
from test_gpu_rollout import _setup
from test_gpu_rollout_vehicle import BITES, OTHER, SCENE_OF, _host_loop, _same, _wps

pytestmark = [pytest.mark.gpu, pytest.mark.filterwarnings("ignore:no SDF weights"),
              pytest.mark.filterwarnings("ignore:QP reached")]

B, K = 3, 4


@pytest.fixture(scope="module", autouse=True)
def _torch_first(gpu_ctx):
    """torch opens the device before the first controller of this module does, as in tests/test_gpu_rollout.py."""


def _plant(n, **kw):
    dt = float(n.ocp.dt[0])
    return _lib.plant_opts(n.cfg, dt=dt, substeps=math.ceil(dt / RigidBody(**BC.body_kw()).max_step()), **kw)


def _body_model(n, **kw):
    return VehicleModel(n.cfg, n.ocp.ctx, n.B, seed=17, body=RigidBody(**BC.body_kw()), **kw)


def test_rollout_equals_host_driven_loop_bitwise_and_logs_the_body():
    cfg = Config(mpc__N=10)
    wps = _wps(B)
    opts = dict(BITES, drag=(0.3, 0.2, 0.1), est_bias=[0.1, 0.0, -0.1, 0.0, 0.05, 0.0, 0.02])
    na, x0 = _setup(cfg, B, 21)
    nb, _ = _setup(cfg, B, 21)
    ma, mb = _body_model(na, **opts), _body_model(nb, **opts)
    na.ocp.ctx.enable_timing(True)
    na.set_x0(x0)
    r = na.rollout(K, refs="wps", wps=wps, plant=_plant(na), vehicle=ma)
    assert na.ocp.ctx.kernel_stats("plant_vehicle_body")[1] == K and na.ocp.ctx.kernel_stats("plant_vehicle")[1] == 0
    # the host loop, with the body's states read back around every call
    plant = _plant(nb)
    dx = _lib.DeviceArray.from_numpy(nb.ocp.ctx, np.reshape(x0, (B, 10)))
    nb.set_x0(np.reshape(x0, (B, 10)))
    mb.begin(dx, 0)
    om, ro, xs, xh, us = [mb.omega], [mb.rotor], [mb.x_true], [dx.numpy()], []
    for k in range(K):
        nb.set_x0(xh[-1])
        nb.gen_refs_device("wps", wps=wps)
        nb.solve()
        us.append(nb.ocp.field("u0").numpy().reshape(B, 4))
        mb.step(plant, nb.ocp.field("u0"), k, dx)
        xs.append(mb.x_true)
        xh.append(dx.numpy())
        om.append(mb.omega)
        ro.append(mb.rotor)
    assert r.omega.shape == (B, K + 1, 3) and r.rotor.shape == (B, K + 1, 4)
    np.testing.assert_array_equal(r.x, np.stack(xs, 1))
    np.testing.assert_array_equal(r.xhat, np.stack(xh, 1))
    np.testing.assert_array_equal(r.u, np.stack(us, 1))
    np.testing.assert_array_equal(r.omega, np.stack(om, 1))  # row 0 before the first step, row k + 1 after step k
    np.testing.assert_array_equal(r.rotor, np.stack(ro, 1))
    np.testing.assert_array_equal(r.omega[:, 0], 0.0)
    np.testing.assert_array_equal(r.rotor[:, 0], np.tile(ma.body.hover_speeds(), (B, 1)))
    np.testing.assert_array_equal(ma.omega, r.omega[:, -1])
    np.testing.assert_array_equal(ma.rotor, r.rotor[:, -1])
    np.testing.assert_array_equal(ma.x_true, r.x[:, -1])
    # the applied input is the command of two periods before, hover until then
    hover = np.array([9.81 / float(cfg.robot.limits.gamma), 0.0, 0.0, 0.0])
    np.testing.assert_array_equal(r.u_applied[:, :2], np.broadcast_to(hover, (B, 2, 4)))
    np.testing.assert_array_equal(r.u_applied[:, 2:], r.u[:, :-2])
    assert (r.iters > 0).all() and np.isfinite(r.x).all() and np.abs(r.omega[:, 1:]).max() > 1e-3
    for n in (na, nb):
        n.ocp.close()


def test_the_generic_host_loop_and_a_plain_vehicle_differ_from_the_body():
    """tests/test_gpu_rollout_vehicle.py's host loop, unchanged, drives a model with a body to the rollout's bits; a
    vehicle without a body has no omega / rotor and flies another path."""
    cfg = Config(mpc__N=10)
    wps = _wps(B)
    na, x0 = _setup(cfg, B, 21)
    nb, _ = _setup(cfg, B, 21)
    nc, _ = _setup(cfg, B, 21)
    na.set_x0(x0)
    r = na.rollout(K, refs="wps", wps=wps, plant=_plant(na), vehicle=_body_model(na, delay=1))
    _same(r, _host_loop(nb, _body_model(nb, delay=1), x0, K, wps, _plant(nb)))
    nc.set_x0(x0)
    plain = nc.rollout(K, refs="wps", wps=wps, plant=_plant(nc), vehicle=VehicleModel(cfg, nc.ocp.ctx, B, seed=17, delay=1))
    assert plain.omega is None and plain.rotor is None
    assert np.abs(plain.x[:, -1] - r.x[:, -1]).max() > 1e-3
    for n in (na, nb, nc):
        n.ocp.close()


def test_scene_source_clearance_is_taken_at_the_bodys_true_positions():
    cfg = Config(mpc__N=10)
    wps = _wps(B)
    n, x0 = _setup(cfg, B, 21)
    sc = Scene(n.ocp.ctx, [OTHER, R.SCENE], scene_of=np.array(SCENE_OF, np.int32))
    n.set_sdf_scene(sc)
    m = _body_model(n, est_bias=[0.3, -0.2, 0.1, 0, 0, 0, 0.0])
    n.set_x0(x0)
    r = n.rollout(K, refs="wps", wps=wps, perceive_every=2, plant=_plant(n), vehicle=m)
    assert r.omega is not None and np.abs(r.xhat[..., :3] - r.x[..., :3]).min() > 0.05
    np.testing.assert_array_equal(r.x[:, -1], m.x_true)
    pts = r.x[:, :, :3].reshape(-1, 3)
    np.testing.assert_array_equal(r.clearance.ravel(), sc.distance(pts, np.repeat(SCENE_OF, K + 1)))
    est = r.xhat[:, :, :3].reshape(-1, 3)
    assert np.abs(r.clearance.ravel() - sc.distance(est, np.repeat(SCENE_OF, K + 1))).max() > 1e-3
    n.ocp.close()


def test_rollout_refusals():
    """A plant step the inner loop does not admit (before anything is enqueued, and by the C entry point), and
    omega_log / rotor_log without a body."""
    cfg = Config(mpc__N=10)
    n, x0 = _setup(cfg, B, 21)
    n.set_x0(x0)
    n.rollout(1)
    before = {k: n.ocp.download(k) for k in ("x", "u", "p", "x0")}
    m = _body_model(n, delay=1)
    truth = m.x_true
    with pytest.raises(ValueError, match="substeps"):
        n.rollout(2, vehicle=m)  # the default plant: one substep of the control period
    solver, ctx = n.ocp.parts[0].solver, n.ocp.ctx
    logs = dict(x_log=_lib.DeviceArray(ctx, (B, 3, 10)), u_log=_lib.DeviceArray(ctx, (B, 2, 4)))
    ol, rl = _lib.DeviceArray(ctx, (B, 3, 3)), _lib.DeviceArray(ctx, (B, 3, 4))
    coarse = _lib.plant_opts(cfg, dt=float(n.ocp.dt[0]))
    plain = VehicleModel(cfg, ctx, B, delay=1)
    for plant, veh in ((coarse, (m.h, 0, None, None, ol, rl)), (_plant(n), (None, 0, None, None, ol, None)),
                       (_plant(n), (None, 0, None, None, None, rl)), (_plant(n), (plain.h, 0, None, None, ol, None)),
                       (_plant(n), (plain.h, 0, None, None, None, rl))):
        with pytest.raises(_lib.SdfnmpcError, match="error -1"):
            solver.rollout(2, plant, vehicle=veh, **logs)
    for k, v in before.items():
        np.testing.assert_array_equal(n.ocp.download(k), v)
    np.testing.assert_array_equal(m.x_true, truth)
    r = n.rollout(2, plant=_plant(n), vehicle=m)  # and it still runs afterwards
    assert np.isfinite(r.x).all() and (r.iters > 0).all() and r.rotor.shape == (B, 3, 4)
    n.ocp.close()
