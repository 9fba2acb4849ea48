"""The rigid-body vehicle kernel (csrc/vehicle_body.hip, sdfnmpc_vehicle_set_body) against the CPU truth
tests/rigid_body_ref.py on the cases of tests/body_cases.py: one call and six calls at B = 3 (less than a wave), 64 (a
full block) and 65 (one lane into a second block); repeatability, cut call sequences, reset, the return to the plain
vehicle bit for bit; and every refusal.

Not bitwise against numpy: the device's atan2, sincos, sqrt and reciprocal square root differ from numpy's by ulps and
the kernel multiplies by 1 / m and 1 / J where the restatement divides.  The bar is tolerances.lin_close, 1e-9 of the
array's scale; every comparison prints its error (pytest -s).  Measured on an MI355X: at most 2.1e-15 over the one-call
cases."""
import ctypes as C

import numpy as np
import pytest

import body_cases as BC
import plant_ref
import rigid_body_ref as RB
from sdf_nmpc_amd import _lib
from sdf_nmpc_amd.vehicle import RigidBody, VehicleModel
from tolerances import lin_close

pytestmark = pytest.mark.gpu


def _err(g, w):
    return float(np.abs(np.asarray(g) - w).max()) / max(1.0, float(np.abs(w).max()))


def _model(cfg, ctx, B, tau_mot=RB.LOOP["tau_mot"], **kw):
    return VehicleModel(cfg, ctx, B, body=RigidBody(**BC.body_kw(tau_mot)), **kw)


@pytest.mark.parametrize("substeps", BC.SUBSTEPS)
@pytest.mark.parametrize("B", BC.BATCHES)
def test_one_call_matches_reference(gpu_ctx, cfg, B, substeps):
    worst = 0.0
    for name, *_ in BC.ONE_CALL:
        i, want = BC.one_call_inputs(B, substeps, name), BC.one_call_ref(B, substeps, name)
        assert (i["x"][:, 3] < 0).any()
        m = _model(cfg, gpu_ctx, B, i["tau_mot"], drag=i["drag"])
        dx = _lib.DeviceArray.from_numpy(gpu_ctx, i["x"])
        m.begin(dx, 0)
        m.set_body_state(i["omega"], i["rotor"])
        plant = _lib.plant_opts(cfg, dt=i["dt"], substeps=substeps, acc_dist=i["acc"], gamma_scale=i["gs"])
        m.step(plant, _lib.DeviceArray.from_numpy(gpu_ctx, i["u"]), 0, dx)
        got = dict(x=m.x_true, omega=m.omega, rotor=m.rotor, est=dx.numpy())
        m.close()
        for k, g in got.items():
            assert np.isfinite(g).all(), (name, k)
            worst = max(worst, _err(g, want[k]))
            assert lin_close(g, want[k]), (name, k, _err(g, want[k]))
        np.testing.assert_array_equal(got["est"], got["x"])  # no estimate error configured: a copy
    print(f"\nB={B} substeps={substeps}: max |got - ref| / scale over {len(BC.ONE_CALL)} cases = {worst:.2e}")


def _gpu_seq(cfg, ctx, B, cuts=(BC.SEQ_CALLS,)):
    """The six calls of body_cases.seq_inputs, in chunks of `cuts` calls (the model is not touched between chunks)."""
    i = BC.seq_inputs(B)
    m = _model(cfg, ctx, B, stream_id=i["stream"], **BC.SEQ)
    dx = _lib.DeviceArray.from_numpy(ctx, i["x"])
    m.begin(dx, 0)
    m.set_body_state(i["omega"], i["rotor"])
    est0 = dx.numpy()
    plant = _lib.plant_opts(cfg, dt=BC.SEQ_DT, substeps=BC.SEQ_SUBSTEPS)
    rows, f = [], 0
    for n in cuts:
        for _ in range(n):
            m.step(plant, _lib.DeviceArray.from_numpy(ctx, i["us"][f]), f, dx)
            rows.append(dict(x=m.x_true, est=dx.numpy(), omega=m.omega, rotor=m.rotor))
            f += 1
    assert f == BC.SEQ_CALLS
    m.close()
    return est0, rows


@pytest.mark.parametrize("B", BC.BATCHES)
def test_six_calls_match_reference(gpu_ctx, cfg, B):
    """Delay 2, gust and estimate noise on.  The single-call bar suffices over the sequence: measured on an MI355X the
    worst error is 1.4e-15 of the scale (B = 65), beside 8.9e-16 by which the restatement itself moves when its start
    state and commands move by one ulp.  The applied input is not an output of a single call (a rollout logs it:
    tests/test_gpu_rollout_body.py); here the restatement's is pinned to the delayed commands, and the truth that
    follows from it is compared."""
    est0, rows = _gpu_seq(cfg, gpu_ctx, B)
    want0, want, _ = BC.seq_ref(B)
    assert lin_close(est0, want0)
    hover = np.array([RB.G / float(cfg.robot.limits.gamma), 0.0, 0.0, 0.0])
    worst = 0.0
    for f, (g, w) in enumerate(zip(rows, want)):
        np.testing.assert_array_equal(w["u_app"], np.tile(hover, (B, 1)) if f < 2 else BC.seq_inputs(B)["us"][f - 2])
        for k in ("x", "est", "omega", "rotor"):
            worst = max(worst, _err(g[k], w[k]))
            assert lin_close(g[k], w[k]), (f, k, _err(g[k], w[k]))
    print(f"\nB={B}: six calls, max |got - ref| / scale = {worst:.2e}")


def test_u_applied_is_the_delayed_command(gpu_ctx, cfg):
    """What the body applied shows in the truth: with delay 2 the first two calls fly the hover input whatever is
    commanded, so two models given different commands agree bit for bit until the third call."""
    B = 3
    i = BC.seq_inputs(B)
    out = []
    for us in (i["us"], i["us"][::-1]):
        m = _model(cfg, gpu_ctx, B, delay=2)
        dx = _lib.DeviceArray.from_numpy(gpu_ctx, i["x"])
        m.begin(dx, 0)
        plant = _lib.plant_opts(cfg, dt=BC.SEQ_DT, substeps=BC.SEQ_SUBSTEPS)
        xs = []
        for f in range(3):
            m.step(plant, _lib.DeviceArray.from_numpy(gpu_ctx, us[f]), f, dx)
            xs.append(m.x_true)
        out.append(xs)
        m.close()
    np.testing.assert_array_equal(out[0][0], out[1][0])
    np.testing.assert_array_equal(out[0][1], out[1][1])
    assert np.abs(out[0][2] - out[1][2]).max() > 1e-6


def test_repeatable_cut_and_reset(gpu_ctx, cfg):
    B = 65
    a0, a = _gpu_seq(cfg, gpu_ctx, B)
    b0, b = _gpu_seq(cfg, gpu_ctx, B)
    c0, c = _gpu_seq(cfg, gpu_ctx, B, cuts=(3, 3))
    np.testing.assert_array_equal(a0, b0)
    for ra, rb, rc in zip(a, b, c):
        for k in ra:
            np.testing.assert_array_equal(ra[k], rb[k], err_msg=k)  # the same seed twice: the same bits
            np.testing.assert_array_equal(ra[k], rc[k], err_msg=k)  # cut 3 + 3 without a reset: the uncut bits
    # reset: hover rotors, no body rate; and a second run after it repeats the first
    body = RigidBody(**BC.body_kw())
    m = VehicleModel(cfg, gpu_ctx, B, body=body, delay=1)
    np.testing.assert_array_equal(m.omega, 0.0)
    np.testing.assert_array_equal(m.rotor, np.tile(body.hover_speeds(), (B, 1)))
    x, u = plant_ref.states(np.random.default_rng(4), B)
    plant = _lib.plant_opts(cfg, dt=BC.SEQ_DT, substeps=BC.SEQ_SUBSTEPS)
    du = _lib.DeviceArray.from_numpy(gpu_ctx, u)
    runs = []
    for _ in range(2):
        dx = _lib.DeviceArray.from_numpy(gpu_ctx, x)
        m.begin(dx, 0)
        for f in range(2):
            m.step(plant, du, f, dx)
        runs.append((m.x_true, m.omega, m.rotor))
        assert np.abs(m.omega).max() > 1e-3 and np.abs(m.rotor - body.hover_speeds()).max() > 1e-3
        m.reset()
        np.testing.assert_array_equal(m.omega, 0.0)
        np.testing.assert_array_equal(m.rotor, np.tile(body.hover_speeds(), (B, 1)))
    for g, w in zip(runs[1], runs[0]):
        np.testing.assert_array_equal(g, w)
    m.close()


@pytest.mark.parametrize("kind", ["att", "att_tau"])
def test_without_a_body_it_is_the_plain_vehicle_bitwise(cfg, kind):
    """set_body(None) returns the plain vehicle's kernel and bits; with a body the plant's kind changes nothing."""
    ctx = _lib.Context(0)
    ctx.enable_timing(True)
    B = 65
    opts = dict(seed=9, delay=1, drag=(0.3, 0.2, 0.1), gust_std=0.5, gust_tau=0.3, est_std_pos=0.05)
    x, u = plant_ref.states(np.random.default_rng(11), B)
    plant = _lib.plant_opts(cfg, model=kind, dt=0.075, substeps=4)
    du = _lib.DeviceArray.from_numpy(ctx, u)

    def fly(m):
        dx = _lib.DeviceArray.from_numpy(ctx, x)
        m.begin(dx, 2)
        for f in (2, 3):
            m.step(plant, du, f, dx)
        return m.x_true, dx.numpy()

    plain = VehicleModel(cfg, ctx, B, **opts)
    want = fly(plain)
    assert ctx.kernel_stats("plant_vehicle")[1] == 2 and ctx.kernel_stats("plant_vehicle_body")[1] == 0
    m = VehicleModel(cfg, ctx, B, body=RigidBody(**BC.body_kw()), **opts)
    assert not m.neutral
    with_body = fly(m)
    assert ctx.kernel_stats("plant_vehicle")[1] == 2 and ctx.kernel_stats("plant_vehicle_body")[1] == 2
    assert np.abs(with_body[0] - want[0]).max() > 1e-4
    if kind == "att_tau":  # the kind only supplies the limits
        m2 = VehicleModel(cfg, ctx, B, body=RigidBody(**BC.body_kw()), **opts)
        dx = _lib.DeviceArray.from_numpy(ctx, x)
        m2.begin(dx, 2)
        for f in (2, 3):
            m2.step(_lib.plant_opts(cfg, model="att", dt=0.075, substeps=4), du, f, dx)
        np.testing.assert_array_equal(m2.x_true, with_body[0])
        m2.close()
    m.set_body(None)
    m.reset()
    got = fly(m)
    assert ctx.kernel_stats("plant_vehicle")[1] == 4
    np.testing.assert_array_equal(got[0], want[0])
    np.testing.assert_array_equal(got[1], want[1])
    with pytest.raises(ValueError):
        m.omega
    # an everything-off vehicle with a body is not neutral, and without it is the plant again
    off = VehicleModel(cfg, ctx, B, body=RigidBody(**BC.body_kw()))
    assert not off.neutral
    off.set_body(None)
    assert off.neutral
    for v in (plain, m, off):
        v.close()
    ctx.close()


def _body_c(**kw):
    o = RigidBody(**BC.body_kw()).c()
    for k, v in kw.items():
        if k in ("inertia", "k_rate"):
            v = (C.c_double * 3)(*v)
        setattr(o, k, v)
    return o


NAN, INF = float("nan"), float("inf")
BAD_BODY = [dict(mass=0.0), dict(mass=-1.0), dict(mass=NAN), dict(mass=INF), dict(inertia=(0.017, 0.0, 0.028)),
            dict(inertia=(0.017, 0.018, NAN)), dict(inertia=(-0.017, 0.018, 0.028)), dict(wp_max=0.0), dict(wp_max=INF),
            dict(wp_max=NAN), dict(tau_att=0.0), dict(tau_att=-0.1), dict(tau_att=NAN), dict(tau_att=INF),
            dict(k_rate=(20.0, 0.0, 8.0)), dict(k_rate=(20.0, 20.0, -8.0)), dict(k_rate=(NAN, 20.0, 8.0)),
            dict(k_rate=(20.0, INF, 8.0)), dict(wp_idle=0.0), dict(wp_idle=-1.0), dict(wp_idle=25.0), dict(wp_idle=30.0),
            dict(wp_idle=NAN), dict(tau_mot=-0.01), dict(tau_mot=NAN), dict(tau_mot=INF)]


def test_refusals(cfg):
    """Every refusal returns SDFNMPC_E_ARG, launches nothing, and leaves the vehicle and the outputs as they were."""
    ctx = _lib.Context(0)
    ctx.enable_timing(True)
    lib = _lib.load()
    B = 5
    x, u = plant_ref.states(np.random.default_rng(3), B)
    du = _lib.DeviceArray.from_numpy(ctx, u)
    sentinel = np.full((B, 10), -7.25)
    dout = _lib.DeviceArray.from_numpy(ctx, sentinel)
    m = VehicleModel(cfg, ctx, B, delay=1)
    m.begin(_lib.DeviceArray.from_numpy(ctx, x), 0)
    ctx.synchronize()
    names = ("plant", "plant_vehicle", "plant_vehicle_body", "vehicle_body_reset", "vehicle_reset", "vehicle_begin")
    launched = lambda: [ctx.kernel_stats(n)[1] for n in names]
    before = launched()
    for bad in BAD_BODY:
        o = _body_c(**bad)
        assert lib.sdfnmpc_vehicle_set_body(m.h, C.byref(o)) == -1, bad
        assert lib.sdfnmpc_last_error()
        assert lib.sdfnmpc_vehicle_body_state(m.h, None, None) == -1, bad  # still without a body
    assert lib.sdfnmpc_vehicle_set_body(None, C.byref(_body_c())) == -1
    # a body beside a thrust lag
    lagged = VehicleModel(cfg, ctx, B, thrust_tau=0.05)
    before_lag = launched()
    assert lib.sdfnmpc_vehicle_set_body(lagged.h, C.byref(_body_c())) == -1
    assert "thrust lag" in lib.sdfnmpc_last_error().decode()
    with pytest.raises(_lib.SdfnmpcError):
        VehicleModel(cfg, ctx, B, thrust_tau=0.05, body=RigidBody(**BC.body_kw()))
    assert launched()[:4] == before_lag[:4]
    assert launched()[:4] == before[:4]
    # a step the inner loop does not admit: (dt / substeps) max(1 / tau_mot, k_rate, 2 / tau_att) > 1
    m.set_body(RigidBody(**BC.body_kw()))
    truth, om, ro = m.x_true, m.omega, m.rotor
    for dt, sub, tau_mot in ((0.075, 1, 0.02), (0.075, 3, 0.02), (0.0201, 1, 0.02), (0.075, 1, 0.0), (0.051, 1, 0.0)):
        m.set_body(RigidBody(**BC.body_kw(tau_mot)))
        before = launched()
        po = _lib.plant_opts(cfg, dt=dt, substeps=sub).c(ctx, B)
        assert lib.sdfnmpc_plant_step_vehicle(ctx.h, C.byref(po), m.h, B, du.ptr, 0, dout.ptr) == -1, (dt, sub, tau_mot)
        assert "substeps" in lib.sdfnmpc_last_error().decode()
        assert launched() == before
    ctx.synchronize()
    np.testing.assert_array_equal(dout.numpy(), sentinel)
    np.testing.assert_array_equal(m.x_true, truth)
    np.testing.assert_array_equal(m.omega, om)
    np.testing.assert_array_equal(m.rotor, ro)
    # k_rate and tau_att bind too
    for kw in (dict(k_rate=(20.0, 60.0, 8.0)), dict(tau_att=0.03)):
        m.set_body(RigidBody(**dict(BC.body_kw(), **kw)))
        po = _lib.plant_opts(cfg, dt=0.02, substeps=1).c(ctx, B)
        assert lib.sdfnmpc_plant_step_vehicle(ctx.h, C.byref(po), m.h, B, du.ptr, 0, dout.ptr) == -1, kw
    np.testing.assert_array_equal(dout.numpy(), sentinel)
    # and at the limit it runs
    m.set_body(RigidBody(**BC.body_kw()))
    po = _lib.plant_opts(cfg, dt=0.02, substeps=1).c(ctx, B)
    assert lib.sdfnmpc_plant_step_vehicle(ctx.h, C.byref(po), m.h, B, du.ptr, 0, dout.ptr) == 0
    assert np.abs(dout.numpy() - sentinel).min() > 0 and np.isfinite(m.x_true).all()
    # the Python layer says the same before anything is enqueued
    with pytest.raises(ValueError, match="substeps"):
        m.check_plant(_lib.plant_opts(cfg, dt=0.075, substeps=1))
    m.check_plant(_lib.plant_opts(cfg, dt=0.075, substeps=4))
    # B = 0: a body without a launch
    m0 = VehicleModel(cfg, ctx, 0, body=RigidBody(**BC.body_kw()))
    m0.step(_lib.plant_opts(cfg, dt=0.02), None, 0, None)
    assert m0.omega.shape == (0, 3) and m0.rotor.shape == (0, 4)
    for v in (m, lagged, m0):
        v.close()
    ctx.close()
