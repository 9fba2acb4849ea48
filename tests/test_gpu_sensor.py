"""csrc/sensor.hip through sdf_nmpc_amd.sensor.SensorModel and sdfnmpc_sensor_apply against the numpy oracle
tests/sensor_ref.py: the integer decisions (already invalid, miss, dropout, boxes) bitwise, the streams and the frame
counter, the noise value within the tolerance tests/sensor_ref.py derives, the noise statistics within five standard
errors, the identity, the outlier removal behind it, and the refusals."""
import ctypes as C

import numpy as np
import pytest

import preproc_ref as PR
import sensor_ref as SR
from sdf_nmpc_amd import _lib
from sdf_nmpc_amd.sensor import SensorModel
from test_sensor_ref import STAT_SEED, STAT_SHAPE, noise_statistics

pytestmark = pytest.mark.gpu

STREAMS = [5, 0, 5]
BOXES = dict(p_box=0.8, n_min=1, n_max=3, scale=(0.02, 0.06), ratio=(0.2, 5.0))
SEED = 0xC0FFEE1234567


def _image(H, W, seed=2):
    """[3][H][W] in [0.3, 0.9] with instances 0 and 2 identical, a few pixels at vmax = 1 and a few already 0."""
    rng = np.random.default_rng(seed)
    a = rng.uniform(0.3, 0.9, (3, H, W)).astype(np.float32)
    a[:, 1, 2:5] = 1.0
    a[:, 3, 1] = 0.0
    a[2] = a[0]
    return a


def _model(cfg, ctx, seed=SEED, streams=STREAMS, **kw):
    args = dict(noise_std=0.01, dropout=0.1, boxes=BOXES, miss_invalid=True, frames=5, stream_id=streams)
    args.update(kw)
    return SensorModel(cfg, ctx, seed, **args)


def _oracle(model, img, frame):
    B, H, W = img.shape
    st = np.arange(B) if model.stream_id is None else model.stream_id
    return SR.degrade(img, model.seed, frame, st, a=np.float32(model.noise_std), b=np.float32(model.noise_std_quad),
                      vmax=1.0, p_thresh=model.p_thresh, miss_invalid=model.miss_invalid, table=model.table(B, H, W))


@pytest.mark.parametrize("H,W", [(7, 13), (18, 32)])
def test_zero_mask_equals_the_oracle_bitwise(cfg, gpu_ctx, H, W):
    img = _image(H, W)
    m = _model(cfg, gpu_ctx)
    frame = 7  # reads the box table's entry 7 % 5
    got = m.apply(img, frame, normalized=True)
    ref, zero, _ = _oracle(m, img, frame)
    assert got.dtype == np.float32 and np.array_equal(got == 0, zero)
    assert zero[:, 1, 2:5].all() and zero[:, 3, 1].all()  # the misses and the pixels that were invalid already
    n_drop = (SR.words(SEED, frame, STREAMS, H, W)[2] < np.uint32(m.p_thresh)).sum()
    assert 0 < n_drop < 0.25 * 3 * H * W and SR.box_mask(m.table(3, H, W), frame, 3, H, W).any()
    # the surviving pixels carry the oracle's noise: sigma Z_TOL and the rounding of the fp32 sum
    assert np.abs(got - ref).max() <= 0.01 * SR.Z_TOL + 2.0**-23
    assert (got[~zero] != img[~zero]).mean() > 0.9
    # instances 0 and 2 share a stream and an input: the same bits; instance 1 does not
    assert np.array_equal(got[0].view(np.uint32), got[2].view(np.uint32))
    assert not np.array_equal(got[0] == 0, got[1] == 0)
    # another frame or seed: another mask (and the oracle follows)
    for other, fr in ((m, frame + 1), (_model(cfg, gpu_ctx, seed=SEED + 1), frame)):
        g2 = other.apply(img, fr, normalized=True)
        assert not np.array_equal(g2 == 0, zero)
        assert np.array_equal(g2 == 0, _oracle(other, img, fr)[1])
    # instance 1 alone, as a batch of one, reproduces its slice: nothing depends on the place in the batch
    one = _model(cfg, gpu_ctx, streams=[0]).apply(img[1:2], frame, normalized=True)
    assert np.array_equal(one.view(np.uint32), got[1:2].view(np.uint32))
    # without stream_id the stream is the instance's index
    nat = _model(cfg, gpu_ctx, streams=None)
    assert np.array_equal(nat.apply(img, frame, normalized=True) == 0, _oracle(nat, img, frame)[1])


def _raw_opts(**kw):
    o = _lib.SensorOptsC()
    o.seed, o.a, o.b, o.vmax, o.p_thresh = STAT_SEED, 0.125, 0.0, 100.0, 0
    for k, v in kw.items():
        setattr(o, k, v)
    return o


def _z_of(ctx, shape, frame):
    dev = _lib.DeviceArray.from_numpy(ctx, np.ones(shape, np.float32))
    _lib.sensor_apply(ctx, _raw_opts(), frame, dev)
    return (dev.numpy().astype(np.float64) - 1.0) / 0.125


@pytest.mark.parametrize("shape", [(3, 7, 13), STAT_SHAPE])
def test_noise_value_against_the_float64_oracle(gpu_ctx, shape):
    z = _z_of(gpu_ctx, shape, 3)
    _, _, z_ref = SR.degrade(np.ones(shape), STAT_SEED, 3, a=0.125, vmax=100.0)
    err = np.abs(z - z_ref).max()
    print(f"max |z_dev - z_ref| at {shape}: {err:.3e} (Z_TOL {SR.Z_TOL})")
    assert SR.Z_TOL < SR.Z_TOL_MAX  # the condition on the tolerance itself
    assert err <= SR.Z_TOL


def test_noise_statistics_within_five_standard_errors(gpu_ctx):
    z = _z_of(gpu_ctx, STAT_SHAPE, 3)
    mean, var, b_mean, b_var = noise_statistics(z)
    print(f"n = {z.size}: |mean| {mean:.4f} (bound {b_mean:.4f}), |var - 1| {var:.4f} (bound {b_var:.4f})")
    assert mean <= b_mean and var <= b_var


def test_quadratic_noise_and_raw_units(cfg, gpu_ctx):
    img = _image(18, 32)
    m = SensorModel(cfg, gpu_ctx, SEED, noise_std=0.01, noise_std_quad=0.03)
    got = m.apply(img, 2, normalized=True)
    v = img.astype(np.float64)
    ref, zero, z = SR.degrade(img, SEED, 2, a=np.float32(0.01), b=np.float32(0.03), vmax=1.0)
    assert np.array_equal(got == 0, zero)
    assert np.abs(got - ref).max() <= (0.01 + 0.03) * SR.Z_TOL + 2.0**-22  # sigma <= a + b at v <= 1; fp32 sums
    far, near = (v > 0.8) & ~zero & (v < 1), (v < 0.4) & ~zero
    assert np.std((got - v)[far]) > 1.5 * np.std((got - v)[near])  # the noise grows with range
    # the same model on the raw image (vmax = dmax 1000 / mm_resolution): the same decisions, the same values
    s = m.vmax(False)
    raw = m.apply((img * np.float32(s)).astype(np.float32), 2, normalized=False)
    assert np.array_equal(raw == 0, zero)
    np.testing.assert_allclose(raw / s, ref, rtol=0, atol=0.04 * SR.Z_TOL + 2.0**-21)


def test_identity_and_invalid_pixels_stay(cfg, gpu_ctx):
    img = _image(7, 13)
    clean = SensorModel(cfg, gpu_ctx, SEED).apply(img, 0, normalized=True)
    assert np.array_equal(clean.view(np.uint32), img.view(np.uint32))  # nothing switched on: bitwise unchanged
    noisy = SensorModel(cfg, gpu_ctx, SEED, noise_std=0.05, noise_std_quad=0.05).apply(img, 0, normalized=True)
    assert (noisy[img == 0] == 0).all() and (noisy[img != 0] != img[img != 0]).mean() > 0.9
    assert noisy.min() >= 0.0 and noisy.max() <= 1.0  # clamped to [0, vmax]
    dev = _lib.DeviceArray.from_numpy(gpu_ctx, img)  # a device array is degraded in place
    assert SensorModel(cfg, gpu_ctx, SEED, noise_std=0.05, noise_std_quad=0.05).apply(dev, 0, normalized=True) is dev
    assert np.array_equal(dev.numpy().view(np.uint32), noisy.view(np.uint32))


def test_outlier_removal_behind_the_degradation(cfg, gpu_ctx):
    img = _image(18, 32)
    kw = dict(noise_std=0.02, dropout=0.2, miss_invalid=True, boxes=BOXES)
    plain = SensorModel(cfg, gpu_ctx, SEED, **kw).apply(img, 4, normalized=True)
    got = SensorModel(cfg, gpu_ctx, SEED, outlier_rm=True, min_range=0.35, **kw).apply(img, 4, normalized=True)
    want = PR.remove_close_outliers(plain, 3, 0.35)
    assert np.array_equal(got.view(np.uint32), want.view(np.uint32)) and not np.array_equal(got, plain)


def test_refusals_launch_nothing(gpu_ctx):
    lib = _lib.load()
    B, H, W = 2, 5, 6
    img = _lib.DeviceArray.from_numpy(gpu_ctx, np.full((B, H, W), 0.5, np.float32))
    scratch = _lib.DeviceArray(gpu_ctx, (B, H, W), np.float32)
    tab = _lib.DeviceArray.from_numpy(gpu_ctx, np.zeros((1, B, 2, 4), np.int16))
    call = lambda o, frame=0, im=img.data_ptr(), b=B, h=H, w=W, sc=None, ctx=gpu_ctx.h: lib.sdfnmpc_sensor_apply(
        ctx, None if o is None else C.byref(o), frame, im, b, h, w, sc)
    nan, inf = float("nan"), float("inf")
    bad = [dict(a=-0.1), dict(a=nan), dict(b=-1.0), dict(b=inf), dict(vmax=0.0), dict(vmax=-1.0), dict(vmax=inf),
           dict(boxes=tab.data_ptr(), n_frames=0, max_boxes=2), dict(boxes=tab.data_ptr(), n_frames=1, max_boxes=9),
           dict(boxes=tab.data_ptr(), n_frames=1, max_boxes=-1), dict(outlier_rm=1, min_range=0.1),
           dict(outlier_rm=1, min_range=nan)]
    for kw in bad:
        assert call(_raw_opts(**kw), sc=scratch.data_ptr() if "min_range" in kw and kw["min_range"] != 0.1 else None) == -1, kw
    o = _raw_opts()
    assert call(None) == -1 and call(o, ctx=None) == -1 and call(o, im=None) == -1 and call(o, frame=-1) == -1
    assert call(o, b=-1) == -1 and call(o, h=0) == -1 and call(o, w=0) == -1
    assert (img.numpy() == 0.5).all()
    assert call(o, im=None, b=0) == 0  # B == 0: a no-op
    assert call(_raw_opts(boxes=tab.data_ptr(), n_frames=1, max_boxes=2, outlier_rm=1, min_range=0.1), sc=scratch.data_ptr()) == 0
    assert (img.numpy() != 0.5).any()
    with pytest.raises(ValueError):
        SensorModel(None, gpu_ctx, 1, dropout=1.0)
    with pytest.raises(ValueError):
        SensorModel(None, gpu_ctx, 1, noise_std=-1.0)
