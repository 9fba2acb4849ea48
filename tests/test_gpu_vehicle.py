"""The vehicle kernel (csrc/vehicle.hip, sdfnmpc_plant_step_vehicle) against the CPU truth tests/vehicle_ref.py: both
model kinds, partial waves / blocks, substeps, every term alone and all together, frames 0 / 3 / 11 with delays 0 / 1
/ 3; the everything-off model against sdfnmpc_plant_step bit for bit; and the entry points' refusals.

Not bitwise: the device's fp64 log, cos, sincos and exp differ from numpy's by ulps (the normals, the gust's phi, the
yaw error), and the kernel's f_expl keeps plant.hip's operation order.  Measured on an MI355X: see MEASURED_ERR."""
import ctypes as C

import numpy as np
import pytest

import plant_ref
import vehicle_ref
from sdf_nmpc_amd import _lib
from sdf_nmpc_amd.vehicle import VehicleModel
from tolerances import lin_close

pytestmark = pytest.mark.gpu

DT = 0.075
KINDS = ("att", "att_tau")
FRAMES = (0, 3, 11)
MEASURED_ERR = 1.56e-15  # max |got - ref| / scale over every case of test_step_matches_reference (printed per case)

BIAS = np.array([0.5, -0.2, 0.1, 0.05, 0.0, -0.03, 0.2])
# every term alone, then all together under each delay
TERMS = {
    "delay1": dict(delay=1),
    "delay3": dict(delay=3),
    "lag": dict(thrust_tau=0.05),
    "drag": dict(drag=(0.3, 0.2, 0.1)),
    "gust_white": dict(gust_std=1.0),
    "gust_ou": dict(gust_std=0.8, gust_tau=0.4),
    "est_noise": dict(est_std_pos=0.05, est_std_vel=0.1, est_std_yaw=0.02),
    "est_bias": dict(est_bias=BIAS),
    "all_d0": dict(delay=0, thrust_tau=0.05, drag=(0.3, 0.2, 0.1), gust_std=0.8, gust_tau=0.4, est_std_pos=0.05,
                   est_std_vel=0.1, est_std_yaw=0.02, est_bias=BIAS),
    "all_d1": dict(delay=1, thrust_tau=0.05, drag=(0.3, 0.2, 0.1), gust_std=0.8, gust_tau=0.4, est_std_pos=0.05,
                   est_std_vel=0.1, est_std_yaw=0.02, est_bias=BIAS),
    "all_d3": dict(delay=3, thrust_tau=0.05, drag=(0.3, 0.2, 0.1), gust_std=0.8, gust_tau=0.4, est_std_pos=0.05,
                   est_std_vel=0.1, est_std_yaw=0.02, est_bias=BIAS),
}


def _run(gpu_ctx, cfg, kind, B, substeps, opts, mismatch, seed):
    """begin at frame 0, then one plant call at each of FRAMES: (device, reference) pairs of (x_true, estimate) after
    begin and after every call."""
    rng = np.random.default_rng(2000 + 10 * B + substeps)
    x, _ = plant_ref.states(rng, B)
    us = [plant_ref.states(rng, B)[1] for _ in FRAMES]
    acc = rng.uniform(-2, 2, (B, 3)) if mismatch else None
    gs = rng.uniform(0.8, 1.2, B) if mismatch else None
    stream = None if B == 1 else (np.arange(B)[::-1] * 3 + 1).astype(np.int32)  # not the identity
    plant = _lib.plant_opts(cfg, model=kind, dt=DT, substeps=substeps, acc_dist=acc, gamma_scale=gs)
    m = VehicleModel(cfg, gpu_ctx, B, seed=seed, stream_id=stream, **opts)
    r = vehicle_ref.Vehicle(cfg, B, seed=seed, stream_id=stream, **opts)
    dx = _lib.DeviceArray.from_numpy(gpu_ctx, x)
    m.begin(dx, FRAMES[0])
    pairs = [((m.x_true, dx.numpy()), (x, r.begin(x, FRAMES[0])))]
    for f, u in zip(FRAMES, us):
        du = _lib.DeviceArray.from_numpy(gpu_ctx, u)
        m.step(plant, du, f, dx)
        est = r.step(kind, u, f, DT, substeps, acc, gs)
        pairs.append(((m.x_true, dx.numpy()), (r.x_true.copy(), est)))
        np.testing.assert_array_equal(du.numpy(), u)
    m.close()
    return pairs


@pytest.mark.parametrize("substeps", [1, 4])
@pytest.mark.parametrize("B", [1, 37, 130])  # a partial wave, a partial block, three blocks
@pytest.mark.parametrize("kind", KINDS)
def test_step_matches_reference(gpu_ctx, cfg, kind, B, substeps):
    worst = 0.0
    for name, opts in TERMS.items():
        for mismatch in ((False, True) if name.startswith("all") else (False,)):
            pairs = _run(gpu_ctx, cfg, kind, B, substeps, opts, mismatch, seed=0x5eed0000beef + B)
            for i, (got, want) in enumerate(pairs):
                for g, w, what in zip(got, want, ("x_true", "estimate")):
                    assert np.isfinite(g).all()
                    err = np.abs(g - w).max() / max(1.0, float(np.abs(w).max()))
                    worst = max(worst, err)
                    assert lin_close(g, w), (name, mismatch, i, what, err)
            if name == "est_bias":  # begin and every call add the bias
                for got, _ in pairs:
                    np.testing.assert_allclose(got[1][:, :3] - got[0][:, :3], np.tile(BIAS[:3], (B, 1)), atol=1e-12)
    print(f"\n{kind} B={B} substeps={substeps}: max |got - ref| / scale over {len(TERMS)} models = {worst:.2e}")


@pytest.mark.parametrize("kind", KINDS)
def test_every_term_changes_the_result(gpu_ctx, cfg, kind):
    """Each term alone moves the true state or the estimate away from the plain plant's by far more than the bar."""
    B = 37
    base = _run(gpu_ctx, cfg, kind, B, 1, {}, False, seed=3)[-1][0]
    for name, opts in TERMS.items():
        got = _run(gpu_ctx, cfg, kind, B, 1, opts, False, seed=3)[-1][0]
        d = max(np.abs(got[0] - base[0]).max(), np.abs(got[1] - base[1]).max())
        assert d > 1e-4, (name, d)


@pytest.mark.parametrize("substeps", [1, 4])
@pytest.mark.parametrize("B", [1, 37, 130])
@pytest.mark.parametrize("kind", KINDS)
def test_everything_off_is_plant_step_bitwise(cfg, kind, B, substeps):
    ctx = _lib.Context(0)  # its own context: the timing switch and the statistics are per context
    rng = np.random.default_rng(77 + B)
    x, u = plant_ref.states(rng, B)
    acc, gs = rng.uniform(-2, 2, (B, 3)), rng.uniform(0.8, 1.2, B)
    plant = _lib.plant_opts(cfg, model=kind, dt=DT, substeps=substeps, acc_dist=acc, gamma_scale=gs)
    du = _lib.DeviceArray.from_numpy(ctx, u)
    want = _lib.DeviceArray(ctx, (B, 10))
    _lib.plant_step(ctx, plant, B, _lib.DeviceArray.from_numpy(ctx, x), du, want)
    ctx.enable_timing(True)
    m = VehicleModel(cfg, ctx, B, seed=5)
    assert m.neutral
    dx = _lib.DeviceArray.from_numpy(ctx, x)
    m.begin(dx, 4)
    np.testing.assert_array_equal(dx.numpy(), x)
    np.testing.assert_array_equal(m.x_true, x)
    m.step(plant, du, 4, dx)
    np.testing.assert_array_equal(m.x_true, want.numpy())
    np.testing.assert_array_equal(dx.numpy(), want.numpy())
    assert ctx.kernel_stats("plant")[1] == 1
    assert ctx.kernel_stats("plant_vehicle")[1] == 0 and ctx.kernel_stats("vehicle_begin")[1] == 0
    # and a model that is not neutral is timed under its own name
    m2 = VehicleModel(cfg, ctx, B, seed=5, delay=1)
    m2.begin(dx, 0)
    m2.step(plant, du, 0, dx)
    assert ctx.kernel_stats("plant_vehicle")[1] == 1 and ctx.kernel_stats("plant")[1] == 1
    m.close()
    m2.close()
    ctx.close()


def test_reset_restores_the_hidden_states(gpu_ctx, cfg):
    """Two runs of the same frames from the same state with a reset between give the same bits; without the reset
    the ring, the thrust and the gust carry over and the second run differs."""
    B = 37
    opts = dict(delay=2, thrust_tau=0.05, gust_std=0.8, gust_tau=0.4)
    x, u = plant_ref.states(np.random.default_rng(8), B)
    plant = _lib.plant_opts(cfg, dt=DT)
    m = VehicleModel(cfg, gpu_ctx, B, seed=1, **opts)
    du = _lib.DeviceArray.from_numpy(gpu_ctx, u)
    runs = []
    for reset in (False, True, False):
        if reset:
            m.reset()
        dx = _lib.DeviceArray.from_numpy(gpu_ctx, x)
        m.begin(dx, 0)
        for f in range(3):
            m.step(plant, du, f, dx)
        runs.append(m.x_true)
    np.testing.assert_array_equal(runs[0], runs[1])
    assert np.abs(runs[2] - runs[1]).max() > 1e-6
    m.close()


def _opts(**kw):
    base = dict(seed=0, d=0, tau_m=0.0, drag=(C.c_double * 3)(0, 0, 0), gust_std=0.0, gust_tau=0.0, est_std_p=0.0,
                est_std_v=0.0, est_std_yaw=0.0, est_bias=None, stream_id=None, g=9.81, gamma=20.0)
    if "drag" in kw:
        kw["drag"] = (C.c_double * 3)(*kw["drag"])
    base.update(kw)
    return _lib.VehicleOptsC(**base)


@pytest.mark.parametrize("bad", [dict(d=-1), dict(d=9), dict(tau_m=-0.1), dict(tau_m=float("nan")),
                                 dict(tau_m=float("inf")), dict(drag=(0.1, -0.1, 0.0)), dict(drag=(0.0, 0.0, float("nan"))),
                                 dict(gust_std=-1.0), dict(gust_std=float("inf")), dict(gust_tau=-0.5),
                                 dict(gust_tau=float("nan")), dict(est_std_p=-0.01), dict(est_std_v=float("nan")),
                                 dict(est_std_yaw=-1.0), dict(g=0.0), dict(gamma=float("nan"))])
def test_create_refusals(gpu_ctx, bad):
    lib = _lib.load()
    h = C.c_void_p()
    o = _opts(**bad)
    assert lib.sdfnmpc_vehicle_create(gpu_ctx.h, C.byref(o), 4, C.byref(h)) == -1
    assert lib.sdfnmpc_last_error() and not h.value


def test_create_and_step_argument_refusals(gpu_ctx, cfg):
    """NULL arguments, B < 0, a vehicle of another context or batch size, a bad frame: SDFNMPC_E_ARG, nothing is
    launched and the estimate buffer is untouched.  B = 0 is a no-op."""
    lib = _lib.load()
    h = C.c_void_p()
    o = _opts(d=2)
    assert lib.sdfnmpc_vehicle_create(None, C.byref(o), 4, C.byref(h)) == -1
    assert lib.sdfnmpc_vehicle_create(gpu_ctx.h, None, 4, C.byref(h)) == -1
    assert lib.sdfnmpc_vehicle_create(gpu_ctx.h, C.byref(o), 4, None) == -1
    assert lib.sdfnmpc_vehicle_create(gpu_ctx.h, C.byref(o), -1, C.byref(h)) == -1
    assert lib.sdfnmpc_vehicle_reset(None) == -1

    B = 5
    x, u = plant_ref.states(np.random.default_rng(3), B)
    m = VehicleModel(cfg, gpu_ctx, B, delay=2, est_std_pos=0.1)
    dx, du = _lib.DeviceArray.from_numpy(gpu_ctx, x), _lib.DeviceArray.from_numpy(gpu_ctx, u)
    m.begin(dx, 0)
    truth = m.x_true
    sentinel = np.full((B, 10), -7.25)
    dout = _lib.DeviceArray.from_numpy(gpu_ctx, sentinel)
    other = _lib.Context(0)
    po = _lib.plant_opts(cfg, dt=DT).c(gpu_ctx, B)
    bad_po = _lib.plant_opts(cfg, dt=DT, substeps=0).c(gpu_ctx, B)
    good = [gpu_ctx.h, C.byref(po), m.h, B, du.ptr, 0, dout.ptr]
    cases = {"null_ctx": (0, None), "null_opts": (1, None), "null_vehicle": (2, None), "other_batch": (3, B - 1),
             "null_u": (4, None), "frame_neg": (5, -1), "frame_max": (5, 2**31 - 1), "null_out": (6, None),
             "other_ctx": (0, other.h), "plant_opts": (1, C.byref(bad_po))}
    for what, (pos, val) in cases.items():
        args = list(good)
        args[pos] = val
        assert lib.sdfnmpc_plant_step_vehicle(*args) == -1, what
        assert lib.sdfnmpc_last_error()
    assert lib.sdfnmpc_vehicle_begin(other.h, m.h, dx.ptr, 0) == -1
    assert lib.sdfnmpc_vehicle_begin(gpu_ctx.h, m.h, dx.ptr, -1) == -1
    assert lib.sdfnmpc_vehicle_begin(gpu_ctx.h, m.h, None, 0) == -1
    assert lib.sdfnmpc_vehicle_begin(gpu_ctx.h, None, dx.ptr, 0) == -1
    gpu_ctx.synchronize()
    np.testing.assert_array_equal(dout.numpy(), sentinel)
    np.testing.assert_array_equal(m.x_true, truth)
    assert lib.sdfnmpc_plant_step_vehicle(*good) == 0  # and it still runs
    assert np.abs(m.x_true - truth).max() > 0
    m.close()
    other.close()
    # B = 0: created, begun and stepped without a launch
    m0 = VehicleModel(cfg, gpu_ctx, 0, delay=2)
    m0.begin(None, 0)
    m0.step(_lib.plant_opts(cfg, dt=DT), None, 0, None)
    assert m0.x_true.shape == (0, 10)
    m0.close()
