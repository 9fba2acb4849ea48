"""The plant kernel (csrc/plant.hip, sdfnmpc_plant_step) against the CPU truth tests/plant_ref.py: both model
kinds, partial waves / blocks, substeps, the two mismatch terms, in place and out of place; the perfect-model pin
against the preparation phase's own x_{k+1}; and the entry point's refusals."""
import numpy as np
import pytest

import plant_ref
from sdf_nmpc_amd import _lib
from sdf_nmpc_amd.config import Config
from tolerances import lin_close

pytestmark = pytest.mark.gpu

DT = 0.075  # mpc.T / mpc.N of the default config
KINDS = ("att", "att_tau")


_REF = {}


def _case(cfg, kind, B, substeps, mismatch):
    """Inputs and the CPU reference, computed once per case and shared by the in-place / out-of-place runs."""
    key = (kind, B, substeps, mismatch)
    if key not in _REF:
        rng = np.random.default_rng(1000 + 10 * B + substeps)
        x, u = plant_ref.states(rng, B)
        acc = rng.uniform(-2, 2, (B, 3)) if mismatch else None
        gs = rng.uniform(0.8, 1.2, B) if mismatch else None
        want = plant_ref.step(cfg, kind, x, u, DT, substeps, acc, gs)
        for a in (x, u, want):
            a.setflags(write=False)
        _REF[key] = (x, u, acc, gs, want)
    return _REF[key]


@pytest.mark.parametrize("inplace", [False, True])
@pytest.mark.parametrize("mismatch", [False, True])
@pytest.mark.parametrize("substeps", [1, 4])
@pytest.mark.parametrize("B", [1, 37, 130])  # a partial wave, a partial block, three blocks
@pytest.mark.parametrize("kind", KINDS)
def test_plant_step_matches_reference(gpu_ctx, cfg, kind, B, substeps, mismatch, inplace):
    x, u, acc, gs, want = _case(cfg, kind, B, substeps, mismatch)
    opts = _lib.plant_opts(cfg, model=kind, dt=DT, substeps=substeps, acc_dist=acc, gamma_scale=gs)
    dx = _lib.DeviceArray.from_numpy(gpu_ctx, x)
    du = _lib.DeviceArray.from_numpy(gpu_ctx, u)
    dout = dx if inplace else _lib.DeviceArray.from_numpy(gpu_ctx, np.full((B, 10), np.nan))
    _lib.plant_step(gpu_ctx, opts, B, dx, du, dout)
    got = dout.numpy()
    scale = max(1.0, float(np.abs(want).max()))
    print(f"\n{kind} B={B} substeps={substeps} mismatch={mismatch} inplace={inplace}: "
          f"max |got - ref| / scale = {np.abs(got - want).max() / scale:.2e}")
    assert np.isfinite(got).all()
    assert lin_close(got, want)
    if not inplace:
        np.testing.assert_array_equal(dx.numpy(), x)  # the input is left alone
    np.testing.assert_array_equal(du.numpy(), u)
    if mismatch:  # the terms are really applied: the same call without them differs
        assert not lin_close(plant_ref.step(cfg, kind, x, u, DT, substeps), want)


@pytest.mark.parametrize("kind", KINDS)
def test_perfect_model_plant_equals_preparation_phase(gpu_ctx, kind):
    """substeps = 1, no mismatch, the controller's kind: plant_step(x_k, u_k, dt_k) is the x_{k+1} that the
    preparation phase (linearize_kernel, dual numbers, eight lanes per node) computes from the same rows, to
    1e-13 -- the same tableau and accumulation order; the compiler's contractions may differ."""
    cfg = Config(mpc__model=kind)
    B, N, np_ = 37, 3, 17
    dt = np.array([0.01, 0.05, DT])
    rng = np.random.default_rng(77)
    x, u = plant_ref.states(rng, B * (N + 1))
    x, u = x.reshape(B, N + 1, 10), u.reshape(B, N + 1, 4)[:, :N].copy()
    p = np.zeros((B, N + 1, np_))
    p[..., 4:13] = np.eye(3).ravel()
    p[..., 13] = 1.0
    bufs = {k: _lib.DeviceArray.from_numpy(gpu_ctx, v) for k, v in dict(x=x, u=u, p=p, dt=dt).items()}
    for k, s in dict(xn=(B, N, 10), AB=(B, N, 14, 10), y=(B, N, 11), Jy=(B, N, 14, 11), yN=(B, 4), JyN=(B, 10, 4),
                     h=(B, N + 1, 3), Jh=(B, N + 1, 10, 3)).items():
        bufs[k] = _lib.DeviceArray(gpu_ctx, s)
    _lib.linearize(gpu_ctx, None, _lib.quad_model(cfg), B, N, np_, bufs, no_sdf=True)
    xn = bufs["xn"].numpy()
    for k in range(N):
        out = _lib.DeviceArray.from_numpy(gpu_ctx, np.full((B, 10), np.nan))
        _lib.plant_step(gpu_ctx, _lib.plant_opts(cfg, dt=dt[k]), B, _lib.DeviceArray.from_numpy(gpu_ctx, x[:, k]),
                        _lib.DeviceArray.from_numpy(gpu_ctx, u[:, k]), out)
        got = out.numpy()
        print(f"\n{kind} node {k}: max |plant - xn| = {np.abs(got - xn[:, k]).max():.2e}")
        assert lin_close(got, xn[:, k], rtol=1e-13)


def _bad(cfg, **kw):
    o = _lib.plant_opts(cfg, model=kw.pop("model", "att"), dt=kw.pop("dt", DT), substeps=kw.pop("substeps", 1))
    for k, v in kw.items():
        setattr(o, k, v)
    return o


@pytest.mark.parametrize("what,code", [("substeps0", -1), ("substeps65", -1), ("dt0", -1), ("dtneg", -1), ("dtnan", -1),
                                       ("tau_roll0", -1), ("tau_pitchneg", -1), ("kind2", -4), ("kindneg", -4),
                                       ("null_x", -1), ("null_u", -1), ("null_out", -1), ("null_opts", -1),
                                       ("null_ctx", -1), ("Bneg", -1)])
def test_plant_step_refusals(gpu_ctx, cfg, what, code):
    """SDFNMPC_E_ARG (-1) / SDFNMPC_E_UNSUPPORTED (-4) with a message, and the output buffer untouched."""
    import ctypes as C
    B = 5
    x, u = plant_ref.states(np.random.default_rng(3), B)
    dx, du = _lib.DeviceArray.from_numpy(gpu_ctx, x), _lib.DeviceArray.from_numpy(gpu_ctx, u)
    sentinel = np.full((B, 10), -7.25)
    dout = _lib.DeviceArray.from_numpy(gpu_ctx, sentinel)
    opts = {"substeps0": _bad(cfg, substeps=0), "substeps65": _bad(cfg, substeps=65), "dt0": _bad(cfg, dt=0.0),
            "dtneg": _bad(cfg, dt=-0.01), "dtnan": _bad(cfg, dt=float("nan")),
            "tau_roll0": _bad(cfg, model="att_tau", tau_roll=0.0),
            "tau_pitchneg": _bad(cfg, model="att_tau", tau_pitch=-0.1), "kind2": _bad(cfg, kind=2),
            "kindneg": _bad(cfg, kind=-1)}.get(what, _bad(cfg))
    o = opts.c(gpu_ctx, B)
    args = [gpu_ctx.h, C.byref(o), B, dx.ptr, du.ptr, dout.ptr]
    pos = {"null_ctx": 0, "null_opts": 1, "null_x": 3, "null_u": 4, "null_out": 5}
    if what in pos:
        args[pos[what]] = None
    if what == "Bneg":
        args[2] = -1
    lib = _lib.load()
    rc = lib.sdfnmpc_plant_step(*args)
    assert rc == code, (what, rc)
    assert lib.sdfnmpc_last_error()
    gpu_ctx.synchronize()
    np.testing.assert_array_equal(dout.numpy(), sentinel)
    if what.startswith("tau"):  # the lags' constants are the 'att_tau' plant's only: 'att' ignores them
        o.kind = 0
        assert lib.sdfnmpc_plant_step(gpu_ctx.h, C.byref(o), B, dx.ptr, du.ptr, dout.ptr) == 0
        assert lin_close(dout.numpy(), plant_ref.step(cfg, "att", x, u, DT))


def test_plant_step_empty_batch_and_limits(gpu_ctx, cfg):
    """B = 0 is a no-op; substeps = 64, the largest accepted, runs and agrees with the reference."""
    x, u = plant_ref.states(np.random.default_rng(4), 3)
    dx, du = _lib.DeviceArray.from_numpy(gpu_ctx, x), _lib.DeviceArray.from_numpy(gpu_ctx, u)
    _lib.plant_step(gpu_ctx, _lib.plant_opts(cfg, dt=DT), 0, dx, du, dx)
    np.testing.assert_array_equal(dx.numpy(), x)
    out = _lib.DeviceArray(gpu_ctx, (3, 10))
    _lib.plant_step(gpu_ctx, _lib.plant_opts(cfg, model="att_tau", dt=DT, substeps=64), 3, dx, du, out)
    assert lin_close(out.numpy(), plant_ref.step(cfg, "att_tau", x, u, DT, 64))


def test_plant_registered_for_kernel_stats(cfg):
    ctx = _lib.Context(0)  # its own context: the timing switch and the statistics are per context
    x, u = plant_ref.states(np.random.default_rng(5), 8)
    dx, du = _lib.DeviceArray.from_numpy(ctx, x), _lib.DeviceArray.from_numpy(ctx, u)
    ctx.enable_timing(True)
    for _ in range(3):
        _lib.plant_step(ctx, _lib.plant_opts(cfg, dt=DT), 8, dx, du, dx)
    ms, n = ctx.kernel_stats("plant")
    assert n == 3 and ms > 0.0
    dx.close()
    du.close()
    ctx.close()
