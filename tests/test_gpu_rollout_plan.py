"""The launch sequence of the device rollouts, which the bitwise tests of tests/test_gpu_rollout*.py see only through
its results: per flavour (plain, latent, scene source, image source, reconstruction; with and without a vehicle) the
number of launches of every stage's kernel, as the loop's definition gives it -- before step k with
(k + phase) % every == 0 the flavour's stages once each, and per step one reference pack (when asked for), one RTI
step and one plant call; the scene time the scene-source loop leaves in the solver; and the refusals the entry points
share, per entry point.  N = 10, B = 2, K = 5, every = 2, phase = 1: the perceiving steps are k = 1 and 3."""
import ctypes as C

import numpy as np
import pytest

import scene_dyn_ref as D
import scene_ref as R
from sdf_nmpc_amd import _lib
from sdf_nmpc_amd import vae as V
from sdf_nmpc_amd.config import Config
from sdf_nmpc_amd.scene import Scene
from sdf_nmpc_amd.sensor import SensorModel
from sdf_nmpc_amd.vehicle import VehicleModel
from test_gpu_rollout import _setup

pytestmark = [pytest.mark.gpu, pytest.mark.filterwarnings("ignore:no SDF weights"),
              pytest.mark.filterwarnings("ignore:QP reached")]

B, K, EVERY, PHASE = 2, 5, 2, 1
N_P = sum((k + PHASE) % EVERY == 0 for k in range(K))  # 2: k = 1 and 3
SHAPE = (30, 40)
T0 = 0.5
SCHEDULE = dict(perceive_every=EVERY, perceive_phase=PHASE)
STAGES = ("scene_pose", "scene_render", "sensor_degrade", "vae_pre", "minpool5", "ref_pack", "scene_sdf_rows",
          "img_sdf_rows", "plant", "plant_vehicle", "rti_apply")


@pytest.fixture(scope="module", autouse=True)
def _torch_first(gpu_ctx):
    """torch opens the device before the first controller of this module does, as in tests/test_gpu_rollout.py."""


@pytest.fixture(scope="module")
def weights():
    """Synthetic encoder and decoder parameters, generated once for every wrapper of the module."""
    es, ds = V.DEFAULT_ENCODER, V.DEFAULT_DECODER
    return (es, V.synthetic_encoder(es, 0)), (ds, V.synthetic_decoder(ds, 0))


def _vae(cfg, ctx, weights, decoder=False):
    return V.VaeWrapper(cfg, weights=weights[0], batch=B, ctx=ctx, decoder=weights[1] if decoder else None)


def _sensor(cfg, ctx):
    return SensorModel(cfg, ctx, 7, noise_std=0.02, noise_std_quad=0.002, dropout=0.05)


def _counted(n, want, **kw):
    """n.rollout(K, **kw) from the current state with the launch counters running: every stage named in STAGES was
    launched want[stage] times, 0 when want does not name it."""
    ctx = n.ocp.ctx
    ctx.synchronize()
    ctx.enable_timing(True)
    ctx.reset_stats()
    r = n.rollout(K, **kw)
    got = {name: ctx.kernel_stats(name)[1] for name in STAGES}
    ctx.enable_timing(False)
    print(f"\nlaunches: {got}")
    assert got == {name: want.get(name, 0) for name in STAGES}
    assert (r.iters > 0).all()
    return r


def _vehicle(cfg, ctx, on):
    """A model that is not neutral (one period of input delay), or none."""
    return VehicleModel(cfg, ctx, B, delay=1) if on else None


def test_plain_rollout_launches_the_step_and_the_plant():
    cfg = Config(mpc__N=10)
    n, x0 = _setup(cfg, B, 21)
    n.set_x0(x0)
    _counted(n, dict(plant=K, rti_apply=K))
    _counted(n, dict(plant=K, rti_apply=K, ref_pack=K), refs="hover")
    n.ocp.close()


@pytest.mark.parametrize("vehicle", [False, True])
def test_latent_rollout_launch_counts(weights, vehicle):
    """Pose, render, sensor, encode and the latent's pack on the two perceiving steps; under a vehicle the pose is a
    pair of launches (the camera from the true state, the body from the estimate) and the plant call is the model's."""
    cfg = Config(mpc__N=10)
    n, x0 = _setup(cfg, B, 21)
    ctx = n.ocp.ctx
    scene, vae, veh = Scene(ctx, R.SCENE), _vae(cfg, ctx, weights), _vehicle(cfg, ctx, vehicle)
    n.set_x0(x0)
    want = dict(scene_pose=N_P, scene_render=N_P, sensor_degrade=N_P, vae_pre=N_P, ref_pack=N_P, plant=K, rti_apply=K)
    if vehicle:
        want.update(scene_pose=2 * N_P, plant=0, plant_vehicle=K)
    _counted(n, want, scene=scene, vae=vae, sensor=_sensor(cfg, ctx), img_shape=SHAPE, vehicle=veh, **SCHEDULE)
    scene.close()
    n.ocp.close()


@pytest.mark.parametrize("vehicle", [False, True])
def test_scene_source_rollout_launch_counts(vehicle):
    """The pose refresh is one launch from the estimate also under a vehicle; nothing is rendered or encoded."""
    cfg = Config(mpc__N=10)
    n, x0 = _setup(cfg, B, 21)
    ctx = n.ocp.ctx
    scene, veh = Scene(ctx, R.SCENE), _vehicle(cfg, ctx, vehicle)
    n.set_sdf_scene(scene)
    n.set_x0(x0)
    want = dict(scene_pose=N_P, ref_pack=N_P, scene_sdf_rows=K, rti_apply=K, **{"plant_vehicle" if vehicle else "plant": K})
    _counted(n, want, vehicle=veh, **SCHEDULE)
    scene.close()
    n.ocp.close()


@pytest.mark.parametrize("recon", [False, True])
def test_image_source_rollout_launch_counts(weights, recon):
    """The unsigned image source: pose, render, pool and the pose's pack on the two perceiving steps; the
    reconstructing source encodes (and decodes) there too."""
    cfg = Config(mpc__N=10)
    n, x0 = _setup(cfg, B, 21)
    ctx = n.ocp.ctx
    scene = Scene(ctx, R.SCENE)
    img = scene.render_from_state(x0, cfg, SHAPE, normalized=True)
    n.set_sdf_image(img, signed=False, reconstruct=_vae(cfg, ctx, weights, decoder=True) if recon else None)
    n.set_x0(x0)
    want = dict(scene_pose=N_P, scene_render=N_P, minpool5=N_P, ref_pack=N_P, img_sdf_rows=K, plant=K, rti_apply=K)
    if recon:
        want.update(vae_pre=N_P)
    _counted(n, want, scene=scene, img_shape=SHAPE, **SCHEDULE)
    scene.close()
    n.ocp.close()


def test_scene_source_rollout_leaves_the_last_steps_time_in_the_solver():
    """After the rollout a solve() sees the moving scene at scene_t0 + (phase + K - 1) dt: the same bits as after
    setting that time by hand, and others than one second later (max_df = 5 m keeps the scene inside the truncation)."""
    cfg = Config(mpc__N=10)
    out = []
    for later in (None, 0.0, 1.0):
        n, x0 = _setup(cfg, B, 21)
        scene = Scene(n.ocp.ctx, [Scene.moving(p, **kw) if kw is not None else p for p, kw in D.SPEC])
        assert scene.is_dynamic
        n.set_sdf_scene(scene, max_df=5.0)
        n.set_x0(x0)
        n.rollout(K, scene_t0=T0, **SCHEDULE)
        if later is not None:
            n.set_scene_time(T0 + (PHASE + K - 1) * float(n.ocp.dt[0]) + later)
        n.solve()
        out.append({k: n.ocp.download(k) for k in ("h", "Jh", "u0")})
        scene.close()
        n.ocp.close()
    for k in ("h", "Jh", "u0"):
        np.testing.assert_array_equal(out[0][k], out[1][k], err_msg=k)
    assert (out[0]["h"][..., 2] != out[2]["h"][..., 2]).any()


CLOCK = "the scene clock needs a finite t0 and a finite dt >= 0"
SCHED = "perceive needs every >= 1 and phase >= 0"
STEPS = "steps must be >= 1"
FRAMES = "the sensor's frame counter (phase + steps) overflows"
ENTRY_POINTS = ("rollout", "perceive", "perceive_at", "perceive_sensor", "scene_sdf", "image_sdf", "image_recon")
# (entry point, what is wrong with the call, the message): everything else about the call is right
REFUSALS = ([(e, dict(dt=-1.0), CLOCK) for e in ("perceive_at", "scene_sdf", "image_sdf", "image_recon")]
            + [(e, dict(every=0), SCHED) for e in ("perceive_sensor", "image_sdf", "image_recon")]
            + [(e, dict(steps=0), STEPS) for e in ENTRY_POINTS]
            + [(e, dict(phase=2**31 - 2, steps=5, sensor=True), FRAMES) for e in ("perceive_sensor", "image_sdf", "image_recon")])


def test_refusals_per_entry_point(weights):
    """Each entry point refuses a call that is wrong in one way with -1 and the message it has always had, before
    anything is launched or uploaded: x0, the iterate and p are untouched."""
    cfg = Config(mpc__N=10)
    lib = _lib.load()
    n, x0 = _setup(cfg, B, 21)
    ctx, solver = n.ocp.ctx, n.ocp.parts[0].solver
    scene = Scene(ctx, R.SCENE)
    enc, rec = _vae(cfg, ctx, weights), _vae(cfg, ctx, weights, decoder=True)
    n.set_sdf_image(scene.render_from_state(x0, cfg, SHAPE, normalized=True), signed=False, reconstruct=rec)
    n.set_x0(x0)
    n.rollout(1)  # flush the host setters, so that the device fields are settled
    before = {k: n.ocp.download(k) for k in ("x0", "x", "u", "p")}
    plant = _lib.plant_opts(cfg, dt=float(n.ocp.dt[0])).c(ctx, B)
    logs = _lib.DeviceArray(ctx, (B, 6, 10)), _lib.DeviceArray(ctx, (B, 5, 4))
    ws = [_lib.DeviceArray(ctx, (B, w)) for w in (3, 9, 3, 9)]
    cam = _lib.DeviceArray(ctx, (B,) + SHAPE, np.float32)
    s = cfg.sensor
    ext = ((C.c_double * 3)(*[float(v) for v in np.asarray(s.B_p_C, float).ravel()]),
           (C.c_double * 9)(*[float(v) for v in np.asarray(s.B_R_C, float).ravel()]))
    sensors = {norm: _sensor(cfg, ctx).opts(B, *SHAPE, normalized=norm) for norm in (False, True)}

    def perc(v, normalized, clip, images, every, phase):
        vo = _lib.VaeOptsC() if v is None else _lib.VaeOptsC(B, *SHAPE, 0, clip, _lib._ptr(v.yz) if v.depth2range else None)
        return _lib.PerceiveArgsC(scene.h, None, scene.img_opts(cfg), *SHAPE, scene.scale(cfg, normalized=normalized), *ext,
                                  None if v is None else v.vae.h, vo, every, phase, _lib._ptr(images),
                                  None if v is None else v.latent.data_ptr(), None if v is None else v.latent64.data_ptr(),
                                  *[w.data_ptr() for w in ws])

    def call(entry, steps=2, dt=0.0, every=1, phase=0, sensor=False):
        a = _lib.RolloutArgsC(steps, 0, None, None, None, None, None, 0, plant, logs[0].data_ptr(), logs[1].data_ptr(),
                              None, None, None, None, 0, None, None)
        sn = lambda norm: (C.byref(sensors[norm][0]), _lib._ptr(sensors[norm][1])) if sensor else (None, None)
        if entry == "rollout":
            return lib.sdfnmpc_solver_rollout(solver.h, C.byref(a))
        if entry == "perceive":
            return lib.sdfnmpc_solver_rollout_perceive(solver.h, C.byref(a), None)
        if entry == "perceive_at":
            return lib.sdfnmpc_solver_rollout_perceive_at(solver.h, C.byref(a), None, 0.0, dt)
        if entry == "perceive_sensor":
            pc = perc(enc, False, float(enc.opts.clip), cam, every, phase)
            return lib.sdfnmpc_solver_rollout_perceive_sensor(solver.h, C.byref(a), C.byref(pc), 0.0, dt, *sn(False))
        if entry == "scene_sdf":
            pose = _lib.PoseRefreshArgsC(every, *ext, *[w.data_ptr() for w in ws])
            return lib.sdfnmpc_solver_rollout_scene_sdf(solver.h, C.byref(a), C.byref(pose), phase, 0.0, dt)
        if entry == "image_sdf":
            pc = perc(None, True, 1.0, None, every, phase)
            return lib.sdfnmpc_solver_rollout_image_sdf(solver.h, C.byref(a), C.byref(pc), 0.0, dt, *sn(True))
        pc = perc(rec, True, 1.0, cam, every, phase)
        return lib.sdfnmpc_solver_rollout_image_recon(solver.h, C.byref(a), C.byref(pc), 0.0, dt, *sn(True), rec.dec.h)

    def check(entry, wrong, message):
        assert call(entry, **wrong) == -1, (entry, wrong)
        assert message in lib.sdfnmpc_last_error().decode(), (entry, wrong)
        ctx.synchronize()
        for k, v in before.items():
            np.testing.assert_array_equal(n.ocp.download(k), v, err_msg=f"{entry} {wrong}: {k}")

    for entry, wrong, message in REFUSALS:
        if entry != "scene_sdf":
            check(entry, wrong, message)
    solver.set_sdf_scene(scene.h, None, 1.0)  # the scene-source loop needs a scene source
    for entry, wrong, message in REFUSALS:
        if entry == "scene_sdf":
            check(entry, wrong, message)
    n.set_sdf_scene(None)
    scene.close()
    n.ocp.close()
