"""The VAE encoder's CPU checkers at image shapes other than 270 x 480 (tests/vae_shape_cases.py): the fp64 C oracle
(oracle/vae.c) against a plain torch restatement (tests/vae_enc_ref.py) and against the reference's own ``Encoder``
(tests/golden/vae_shapes_golden.npz, made by tests/golden/make_vae_shapes_golden.py), and the conditions on the inputs
under which the GPU bar of tests/test_gpu_vae_shapes.py can see a wrong border column.

Measured (fp64 oracle against the fp64 restatement, of the latent's scale): at most 5.2e-15 over the seven cases and the
``batchnorm=False`` one.  The restatement in fp32 against fp64: latent at most 4.4e-7, pooled features at most 4.7e-7
of max |feature| (tests/tolerances.py quotes both).  A flipped border row or column moves the oracle's latent by
5.2e-3 of its scale or more, a flipped corner pixel by 1.2e-4 or more."""
import os

import numpy as np
import pytest
import torch

import vae_enc_ref as R
import vae_shape_cases as SC
from tolerances import VAE_LATENT_RTOL, vae_latent_err

ORACLE_VS_RESTATEMENT = 1e-12  # fp64 summation order; 10^7 below the GPU bar


@pytest.fixture(scope="module")
def vsg():
    return np.load(os.path.join(os.path.dirname(__file__), "golden", "vae_shapes_golden.npz"))


@pytest.fixture(scope="module")
def base(oracle_lib):
    """Per case key: spec, params, flat, the three normalised images and the oracle's latents of them (computed once)."""
    out = {}
    for H, W, L, _ in SC.CASES:
        spec = SC.spec_of(H, W, L)
        params, flat = SC.weights_of(spec)
        pre = SC.normalised(SC.images(SC.GOLDEN_B, H, W))
        pre.setflags(write=False)
        lat = oracle_lib.vae_encode(pre, flat, L=L)
        lat.setflags(write=False)
        out[SC.case_key(H, W, L)] = (spec, params, flat, pre, lat)
    return out


def _worst(lat, ref):
    return max(vae_latent_err(lat[b], ref[b]) for b in range(len(ref)))


@pytest.mark.parametrize("case", SC.CASES, ids=SC.CASE_IDS)
def test_map_sizes(case):
    H, W, L, maps = case
    assert SC.spec_of(H, W, L).maps() == maps


@pytest.mark.parametrize("case", SC.CASES, ids=SC.CASE_IDS)
def test_oracle_vs_restatement(case, base):
    H, W, L, _ = case
    spec, params, _, pre, lat = base[SC.case_key(H, W, L)]
    ref = R.encode_ref(spec, params, pre)
    assert ref.shape == (SC.GOLDEN_B, L) and ref.dtype == np.float64
    err = _worst(lat, ref)
    print(f"{SC.case_key(H, W, L)}: oracle vs restatement {err:.2e}")
    assert err <= ORACLE_VS_RESTATEMENT


def test_oracle_vs_restatement_without_batchnorm(oracle_lib):
    """``batchnorm=False``: the convolutions carry biases and there is no BatchNorm to fold."""
    H, W, L = 36, 50, 128
    spec = SC.spec_of(H, W, L, batchnorm=False)
    params, flat = SC.weights_of(spec)
    assert not any("running_mean" in k for k in params)
    pre = SC.normalised(SC.images(SC.GOLDEN_B, H, W))
    lat = oracle_lib.vae_encode(pre, flat, L=L, bn=False)
    err = _worst(lat, R.encode_ref(spec, params, pre))
    print(f"36x50 batchnorm=False: oracle vs restatement {err:.2e}")
    assert err <= ORACLE_VS_RESTATEMENT


@pytest.mark.parametrize("case", SC.CASES, ids=SC.CASE_IDS)
def test_oracle_vs_reference_golden(case, base, vsg):
    """The margins of test_vae.test_oracle_encoder_vs_reference, per image."""
    H, W, L, _ = case
    key = SC.case_key(H, W, L)
    lat = base[key][4]
    l64, l32 = vsg[key + "/latent64"], vsg[key + "/latent"]
    assert l64.shape == (SC.GOLDEN_B, L) and l64.dtype == np.float64 and l32.dtype == np.float32
    e64, e32 = _worst(lat, l64), _worst(lat, l32)
    print(f"{key}: oracle vs reference fp64 {e64:.2e}, vs reference fp32 {e32:.2e}")
    assert e64 <= 0.1 * VAE_LATENT_RTOL
    assert e32 <= VAE_LATENT_RTOL


@pytest.mark.parametrize("case", [c for c in SC.CASES if c[2] >= 32], ids=[i for i, c in zip(SC.CASE_IDS, SC.CASES) if c[2] >= 32])
def test_bar_sees_the_border(case, base, oracle_lib):
    """Conditions on the inputs, checked on the oracle alone: a flipped border row or column moves the latent by at
    least 100 bars, a flipped corner pixel by at least 5 (two images; the smaller move of the two counts)."""
    H, W, L, _ = case
    _, _, flat, pre, lat = base[SC.case_key(H, W, L)]
    pre, lat = pre[:2], lat[:2]

    def moved(where):
        p = oracle_lib.vae_encode(SC.perturbed(pre, where), flat, L=L)
        return min(np.abs(p[b] - lat[b]).max() / np.abs(lat[b]).max() for b in range(2))

    for where in SC.BORDERS:
        d = moved(where)
        print(f"{SC.case_key(H, W, L)} {where}: {d:.2e}")
        assert d >= 100 * VAE_LATENT_RTOL, where
    for where in SC.CORNERS:
        d = moved(where)
        print(f"{SC.case_key(H, W, L)} {where}: {d:.2e}")
        assert d >= 5 * VAE_LATENT_RTOL, where


@pytest.mark.parametrize("case", SC.CASES, ids=SC.CASE_IDS)
def test_fp32_gap_of_the_restatement(case, base):
    """For the record (tests/tolerances.py): plain fp32 evaluation against fp64, of the latent and of the pooled
    features (relative to max |feature| of the image, the scale of tests/test_gpu_vae_shapes.py's elementwise check)."""
    H, W, L, _ = case
    spec, params, _, pre, _ = base[SC.case_key(H, W, L)]
    l64, l32 = R.encode_ref(spec, params, pre), R.encode_ref(spec, params, pre, torch.float32)
    assert l32.dtype == np.float32
    f64, f32 = R.features_ref(spec, params, pre), R.features_ref(spec, params, pre, torch.float32)
    assert f64.shape == (SC.GOLDEN_B, 2048)
    gl = _worst(l32, l64)
    gf = max(np.abs(f32[b].astype(np.float64) - f64[b]).max() / np.abs(f64[b]).max() for b in range(SC.GOLDEN_B))
    print(f"{SC.case_key(H, W, L)}: fp32 vs fp64 latent {gl:.2e}, features {gf:.2e}")
    assert gl <= 0.1 * VAE_LATENT_RTOL
    assert gf <= 0.1 * VAE_LATENT_RTOL


def test_nan_in_the_last_pixel_stays_in_its_image(oracle_lib, base):
    spec, params, flat, pre, lat = base[SC.case_key(36, 50, 128)]
    p = np.array(pre)
    p[1, -1, -1] = np.nan
    got = oracle_lib.vae_encode(p, flat, L=128)
    assert np.isnan(got[1]).any()
    assert np.array_equal(got[0], lat[0]) and np.array_equal(got[2], lat[2])
    ref = R.encode_ref(spec, params, p)
    assert np.isnan(ref[1]).any() and np.isfinite(ref[0]).all() and np.isfinite(ref[2]).all()
