"""The vehicle model inside the device rollouts (Nmpc.rollout(vehicle=), sdfnmpc_rollout_args.vehicle): bitwise against
the host-driven loops begin; [set_x0(estimate); perception; gen_refs_device; solve; vehicle.step] of all four rollout
loops, chunks against the uncut rollout, the everything-off model against rollout() without one, what the camera and
the controller see, and a model that bites."""
import numpy as np
import pytest

import scene_ref as R
from sdf_nmpc_amd import _lib
from sdf_nmpc_amd.config import Config
from sdf_nmpc_amd.reference import yaw2quat
from sdf_nmpc_amd.scene import Scene
from sdf_nmpc_amd.vae import VaeWrapper
from sdf_nmpc_amd.vehicle import VehicleModel
from test_gpu_rollout import _setup

pytestmark = [pytest.mark.gpu, pytest.mark.filterwarnings("ignore:no SDF weights"),
              pytest.mark.filterwarnings("ignore:QP reached")]

SHAPE = (18, 32)
SCENE_OF = [1, 0, 1]
OTHER = [("sphere", [2.0, 0.2, 0.0, 0.6]), ("box", [-10.0, -10.0, -1.6, 10.0, 10.0, -1.5])]
BITES = dict(delay=2, gust_std=1.0, gust_tau=0.3, est_std_pos=0.05, est_std_vel=0.02, est_std_yaw=0.01)


@pytest.fixture(scope="module", autouse=True)
def _torch_first(gpu_ctx):
    """torch opens the device before the first controller of this module does, as in tests/test_gpu_rollout.py."""


def _wps(B):
    rng = np.random.default_rng(5)
    return (rng.uniform(-2, 2, (B, 2, 3)), np.stack([[yaw2quat(a) for a in row] for row in rng.uniform(-1, 1, (B, 2))]))


def _host_loop(n, m, x0, steps, wps, plant=None, phase=0, perceive=None):
    """The loop a user writes around the model: begin, then per step the estimate as the measured state, perceive(k,
    x_true, x_hat), the references, the step, and the model's plant call under the device u0 the step left.  As the
    rollout, it starts from set_x0(true state): the first set_x0 initialises the iterate."""
    B, ctx = n.B, n.ocp.ctx
    plant = plant if plant is not None else _lib.plant_opts(n.cfg, dt=float(n.ocp.dt[0]))
    if n.x0 is None:
        n.set_x0(np.reshape(x0, (B, 10)))
    dx = _lib.DeviceArray.from_numpy(ctx, np.reshape(x0, (B, 10)))
    m.begin(dx, phase)
    xs, xh, us, its, sts = [m.x_true], [dx.numpy()], [], [], []
    for k in range(steps):
        n.set_x0(xh[-1])
        if perceive is not None:
            perceive(k, xs[-1], xh[-1])
        n.gen_refs_device("wps", wps=wps)
        n.solve()
        us.append(n.ocp.field("u0").numpy().reshape(B, 4))
        its.append(n.ocp.iters.copy())
        sts.append(n.ocp.status.copy())
        m.step(plant, n.ocp.field("u0"), phase + k, dx)
        xs.append(m.x_true)
        xh.append(dx.numpy())
    return dict(x=np.stack(xs, 1), xhat=np.stack(xh, 1), u=np.stack(us, 1), status=np.stack(sts, 1), iters=np.stack(its, 1))


def _same(r, want, keys=("x", "xhat", "u", "status", "iters")):
    for k in keys:
        np.testing.assert_array_equal(getattr(r, k), want[k] if isinstance(want, dict) else getattr(want, k), err_msg=k)


@pytest.mark.parametrize("kind", ["att", "att_tau"])
def test_rollout_equals_host_driven_loop_bitwise(kind):
    """B = 70: two blocks.  The plant's kind under the 'att' controller, two substeps, every term on."""
    cfg = Config(mpc__N=10)
    B, K = 70, 4
    wps = _wps(B)
    opts = dict(BITES, thrust_tau=0.05, drag=(0.3, 0.2, 0.1), est_bias=[0.1, 0.0, -0.1, 0.0, 0.05, 0.0, 0.02])
    plant = lambda n: _lib.plant_opts(cfg, model=kind, dt=float(n.ocp.dt[0]), substeps=2)
    na, x0 = _setup(cfg, B, 21)
    nb, _ = _setup(cfg, B, 21)
    ma, mb = (VehicleModel(cfg, n.ocp.ctx, B, seed=17, **opts) for n in (na, nb))
    na.set_x0(x0)
    r = na.rollout(K, refs="wps", wps=wps, plant=plant(na), vehicle=ma)
    want = _host_loop(nb, mb, x0, K, wps, plant(nb))
    assert r.xhat.shape == (B, K + 1, 10) and r.u_applied.shape == (B, K, 4)
    _same(r, want)
    np.testing.assert_array_equal(r.x[:, 0], x0)
    np.testing.assert_array_equal(na.x0, r.x[:, -1])  # the true final state
    np.testing.assert_array_equal(ma.x_true, r.x[:, -1])
    np.testing.assert_array_equal(na.ocp.field("x0").numpy().reshape(B, 10), r.xhat[:, -1])
    assert (r.iters > 0).all() and np.abs(r.xhat - r.x).max() > 1e-3
    for a, b in zip(na.get_matrices(), nb.get_matrices()):
        np.testing.assert_array_equal(a, b)
    for m in (na, nb):
        m.ocp.close()


def test_chunks_with_phase_are_the_uncut_rollout():
    """6 steps against 2 + 4 with perceive_phase carried, under d = 2, gusts and estimate noise: the ring, the gust and
    the thrust carry over in the model, and the second chunk's begin rewrites the estimate the first chunk's last
    plant call wrote."""
    cfg = Config(mpc__N=10)
    B = 70
    wps = _wps(B)
    na, x0 = _setup(cfg, B, 21)
    nb, _ = _setup(cfg, B, 21)
    ma, mb = (VehicleModel(cfg, n.ocp.ctx, B, seed=3, thrust_tau=0.05, **BITES) for n in (na, nb))
    na.set_x0(x0)
    whole = na.rollout(6, refs="wps", wps=wps, vehicle=ma, perceive_phase=5)
    nb.set_x0(x0)
    c1 = nb.rollout(2, refs="wps", wps=wps, vehicle=mb, perceive_phase=5)
    c2 = nb.rollout(4, refs="wps", wps=wps, vehicle=mb, perceive_phase=7)
    np.testing.assert_array_equal(c2.x[:, 0], c1.x[:, -1])
    np.testing.assert_array_equal(c2.xhat[:, 0], c1.xhat[:, -1])
    for k in ("x", "xhat"):
        np.testing.assert_array_equal(getattr(whole, k), np.concatenate([getattr(c1, k), getattr(c2, k)[:, 1:]], 1), err_msg=k)
    for k in ("u", "u_applied", "status", "iters"):
        np.testing.assert_array_equal(getattr(whole, k), np.concatenate([getattr(c1, k), getattr(c2, k)], 1), err_msg=k)
    for m in (na, nb):
        m.ocp.close()


def test_off_model_is_the_plain_rollout_and_no_vehicle_launches_no_new_kernel():
    cfg = Config(mpc__N=10, mpc__shift=1)
    B, K = 70, 3
    wps = _wps(B)
    na, x0 = _setup(cfg, B, 21)
    nb, _ = _setup(cfg, B, 21)
    for n in (na, nb):
        n.ocp.ctx.enable_timing(True)
    off = VehicleModel(cfg, nb.ocp.ctx, B, seed=9)
    assert off.neutral
    nb.ocp.ctx.reset_stats()
    na.set_x0(x0)
    nb.set_x0(x0)
    ra = na.rollout(K, refs="wps", wps=wps)
    rb = nb.rollout(K, refs="wps", wps=wps, vehicle=off)
    assert ra.xhat is None and ra.u_applied is None
    _same(rb, ra, ("x", "u", "status", "iters"))
    np.testing.assert_array_equal(rb.xhat, rb.x)
    np.testing.assert_array_equal(rb.u_applied, rb.u)
    np.testing.assert_array_equal(off.x_true, rb.x[:, -1])
    np.testing.assert_array_equal(na.ocp.download("p"), nb.ocp.download("p"))
    for ctx in (na.ocp.ctx, nb.ocp.ctx):
        assert ctx.kernel_stats("plant")[1] == K
        for name in ("plant_vehicle", "vehicle_begin", "vehicle_reset"):
            assert ctx.kernel_stats(name)[1] == 0, name
    for m in (na, nb):
        m.ocp.close()


def _make_perceive(cfg, B=3, seed=21):
    n, x0 = _setup(cfg, B, seed)
    ctx = n.ocp.ctx
    return n, x0, Scene(ctx, [R.SCENE, OTHER], scene_of=SCENE_OF), VaeWrapper(cfg, batch=B, ctx=ctx)


@pytest.mark.parametrize("axis", [0, 2])
def test_perceiving_rollout_sees_from_the_true_state_and_believes_the_estimate(axis):
    """The setup of tests/test_gpu_rollout_perceive.py under a constant estimate bias of 0.5 m in x, no noise -- and
    the same in z."""
    cfg = Config(mpc__N=10)
    B, K, every = 3, 6, 2
    wps = _wps(B)
    bias = [0.0] * 7
    bias[axis] = 0.5
    na, x0, sa, va = _make_perceive(cfg)
    nb, _, sb, vb = _make_perceive(cfg)
    ma = VehicleModel(cfg, na.ocp.ctx, B, est_bias=bias)
    na.set_x0(x0)
    r = na.rollout(K, refs="wps", wps=wps, scene=sa, vae=va, perceive_every=every, img_shape=SHAPE, keep_img=True,
                   vehicle=ma)
    other = [i for i in range(10) if i != axis]
    np.testing.assert_allclose(r.xhat[..., axis] - r.x[..., axis], 0.5, atol=1e-12)
    np.testing.assert_array_equal(r.xhat[..., other], r.x[..., other])
    # the camera saw from where the vehicle was
    k_last = (K - 1) // every * every
    want = sb.render_from_state(r.x[:, k_last], cfg, SHAPE, normalized=False).numpy()
    np.testing.assert_array_equal(r.img, want)
    # and the estimate's view is another one (already at the start state, where instances 0 and 2 have obstacles in view)
    seen = lambda x: sb.render_from_state(x, cfg, SHAPE, normalized=False).numpy()
    assert np.ptp(seen(r.x[:, 0])) > 0 and (seen(r.xhat[:, 0]) != seen(r.x[:, 0])).any()
    # the controller was told the pose of its estimate
    pa = na.ocp.download("p")
    ps = sb.pose(r.xhat[:, k_last], cfg)
    nb.set_x0(x0)
    nb.rollout(1)  # settle nb's device fields, then the pose columns alone
    nb.set_pose_device(ps["W_p_Bo"], ps["W_R_Bo"])
    np.testing.assert_array_equal(pa[:, :, 1:13], nb.ocp.download("p")[:, :, 1:13])
    pt = sb.pose(r.x[:, k_last], cfg)
    assert np.abs(ps["W_p_Bo"].numpy() - pt["W_p_Bo"].numpy()).max() > 0.4
    # the clearance is the true vehicle's
    pts = r.x[:, :, :3].reshape(-1, 3)
    np.testing.assert_array_equal(r.clearance.ravel(), sa.distance(pts, np.repeat(SCENE_OF, K + 1)))
    # and the whole run is the host loop's
    nc, _, sc, vc = _make_perceive(cfg)

    def perceive(k, x_true, x_hat):
        if k % every == 0:
            img = sc.render_from_state(x_true, cfg, SHAPE, normalized=False)
            est = sc.pose(x_hat, cfg)
            vc.set_img(img)
            vc.encode_to(nc, est["W_p_Bo"], est["W_R_Bo"])

    want = _host_loop(nc, VehicleModel(cfg, nc.ocp.ctx, B, est_bias=bias), x0, K, wps, perceive=perceive)
    _same(r, want)
    np.testing.assert_array_equal(pa, nc.ocp.download("p"))
    for m in (na, nb, nc):
        m.ocp.close()


def test_scene_source_rollout_equals_host_driven_loop_bitwise():
    """The pose refresh reads the estimate: the controller believes it."""
    cfg = Config(mpc__N=10)
    B, K, every = 3, 6, 2
    wps = _wps(B)
    opts = dict(BITES, est_bias=[0.2, -0.1, 0, 0, 0, 0, 0.05])
    ns = []
    for _ in range(2):
        n, x0 = _setup(cfg, B, 21)
        sc = Scene(n.ocp.ctx, [OTHER, R.SCENE], scene_of=np.array(SCENE_OF, np.int32))
        n.set_sdf_scene(sc)
        ns.append((n, sc, VehicleModel(cfg, n.ocp.ctx, B, seed=4, **opts)))
    (na, sa, ma), (nb, sb, mb) = ns
    na.set_x0(x0)
    r = na.rollout(K, refs="wps", wps=wps, perceive_every=every, vehicle=ma)

    def perceive(k, x_true, x_hat):
        if k % every == 0:
            ps = sb.pose(x_hat, cfg)
            nb.set_pose_device(ps["W_p_Bo"], ps["W_R_Bo"])

    want = _host_loop(nb, mb, x0, K, wps, perceive=perceive)
    _same(r, want)
    np.testing.assert_array_equal(na.ocp.download("p"), nb.ocp.download("p"))
    pts = r.x[:, :, :3].reshape(-1, 3)
    np.testing.assert_array_equal(r.clearance.ravel(), sa.distance(pts, np.repeat(SCENE_OF, K + 1)))
    for m in (na, nb):
        m.ocp.close()


def test_image_source_rollout_equals_host_driven_loop_bitwise():
    """The image is rendered from the true state, its pose in p is the estimate's."""
    cfg = Config(mpc__N=10)
    B, K, every, shape = 3, 6, 2, (30, 40)
    wps = _wps(B)
    opts = dict(BITES, est_bias=[0.2, -0.1, 0, 0, 0, 0, 0.05])
    ns = []
    for _ in range(2):
        n, x0 = _setup(cfg, B, 21)
        sc = Scene(n.ocp.ctx, [OTHER, R.SCENE], scene_of=np.array(SCENE_OF, np.int32))
        n.set_sdf_image(sc.render_from_state(x0, cfg, shape, normalized=True))
        ns.append((n, sc, VehicleModel(cfg, n.ocp.ctx, B, seed=4, **opts)))
    (na, sa, ma), (nb, sb, mb) = ns
    na.set_x0(x0)
    r = na.rollout(K, refs="wps", wps=wps, scene=sa, perceive_every=every, img_shape=shape, keep_img=True, vehicle=ma)

    def perceive(k, x_true, x_hat):
        if k % every == 0:
            nb.set_sdf_image(sb.render_from_state(x_true, cfg, shape, normalized=True))
            ps = sb.pose(x_hat, cfg)
            nb.set_pose_device(ps["W_p_Bo"], ps["W_R_Bo"])

    want = _host_loop(nb, mb, x0, K, wps, perceive=perceive)
    _same(r, want)
    np.testing.assert_array_equal(na.ocp.download("p"), nb.ocp.download("p"))
    np.testing.assert_array_equal(r.img, nb._sdf_image["images"].numpy())
    k_last = (K - 1) // every * every
    np.testing.assert_array_equal(r.img, sb.render_from_state(r.x[:, k_last], cfg, shape, normalized=True).numpy())
    for m in (na, nb):
        m.ocp.close()


def test_a_model_that_bites():
    """gust_std = 1, delay = 2, est_std_pos = 0.05 over B = 130, K = 8: the true path leaves the perfect run's, the
    estimate's error has the configured standard deviations (1170 samples per axis: the sample standard deviation of a
    normal is within 3 / sqrt(2 n) = 6 % of sigma at three sigma, the bar is 25 %), and the applied input is the
    command of two periods before, hover until then."""
    cfg = Config(mpc__N=10)
    B, K = 130, 8
    wps = _wps(B)
    na, x0 = _setup(cfg, B, 21)
    nb, _ = _setup(cfg, B, 21)
    m = VehicleModel(cfg, na.ocp.ctx, B, seed=12, gust_std=1.0, delay=2, est_std_pos=0.05)
    na.set_x0(x0)
    nb.set_x0(x0)
    r = na.rollout(K, refs="wps", wps=wps, vehicle=m)
    perfect = nb.rollout(K, refs="wps", wps=wps)
    d = np.abs(r.x[:, -1, :3] - perfect.x[:, -1, :3]).max(-1)
    print(f"\nfinal position against the perfect run: median {np.median(d):.3f} m, max {d.max():.3f} m")
    assert np.median(d) > 1e-2
    err = r.xhat - r.x
    sd = err[..., :3].reshape(-1, 3).std(0)
    print(f"std of the position estimate's error per axis: {sd} (configured 0.05)")
    assert (np.abs(sd / 0.05 - 1.0) <= 0.25).all()
    assert np.abs(err[..., :3].mean()) <= 0.01
    np.testing.assert_array_equal(err[..., 3:], 0.0)  # no velocity or yaw error was configured
    np.testing.assert_array_equal(r.u_applied[:, 2:], r.u[:, :-2])
    hover = np.array([9.81 / float(cfg.robot.limits.gamma), 0.0, 0.0, 0.0])
    np.testing.assert_array_equal(r.u_applied[:, :2], np.broadcast_to(hover, (B, 2, 4)))
    for n in (na, nb):
        n.ocp.close()


def test_rollout_refusals():
    """A model of another context or batch size, a negative first frame; the C entry point: xhat_log / uapp_log
    without a vehicle, and a frame counter that would overflow."""
    import ctypes as C
    cfg = Config(mpc__N=10)
    B = 3
    n, x0 = _setup(cfg, B, 21)
    n.set_x0(x0)
    n.rollout(1)
    x0 = n.x0.copy()
    before = {k: n.ocp.download(k) for k in ("x", "u", "p", "x0")}
    other = _lib.Context(0)
    m = VehicleModel(cfg, n.ocp.ctx, B, delay=1)
    for kw in (dict(vehicle=VehicleModel(cfg, other, B, delay=1)), dict(vehicle=VehicleModel(cfg, n.ocp.ctx, B + 1, delay=1)),
               dict(vehicle=m, perceive_phase=-1)):
        with pytest.raises(ValueError):
            n.rollout(2, **kw)
        for k, v in before.items():
            np.testing.assert_array_equal(n.ocp.download(k), v)
    solver, ctx = n.ocp.parts[0].solver, n.ocp.ctx
    K = 2
    logs = dict(x_log=_lib.DeviceArray(ctx, (B, K + 1, 10)), u_log=_lib.DeviceArray(ctx, (B, K, 4)))
    xh, ua = _lib.DeviceArray(ctx, (B, K + 1, 10)), _lib.DeviceArray(ctx, (B, K, 4))
    plant = _lib.plant_opts(cfg, dt=float(n.ocp.dt[0]))
    wrong = VehicleModel(cfg, ctx, B + 1, delay=1)
    foreign = VehicleModel(cfg, other, B, delay=1)
    for veh in ((None, 0, xh, None), (None, 0, None, ua), (wrong.h, 0, None, None), (foreign.h, 0, None, None),
                (m.h, -1, None, None), (m.h, 2**31 - 2, None, None)):
        with pytest.raises(_lib.SdfnmpcError, match="error -1"):
            solver.rollout(K, plant, vehicle=veh, **logs)
        for k, v in before.items():
            np.testing.assert_array_equal(n.ocp.download(k), v)
    r = n.rollout(2, vehicle=m)  # and it still runs afterwards
    assert (r.status == 0).all()
    n.ocp.close()
    other.close()
