"""The VAE decoder's host side without a GPU: the numpy fp64 decoder (tests/vae_dec_ref.py) against the reference's
own ``Decoder`` (tests/golden/vae_dec_golden.npz), the fold-and-pack round trip of the `.vaed` blob, the state_dict
conversion, and the refusals."""
import os

import numpy as np
import pytest

import vae_dec_ref as R
from sdf_nmpc_amd import vae as V


@pytest.fixture(scope="module")
def dg():
    return np.load(os.path.join(os.path.dirname(__file__), "golden", "vae_dec_golden.npz"))


@pytest.fixture(scope="module")
def synth_params():
    return {bn: V.synthetic_decoder(V.DecoderSpec(batchnorm=bn), 0) for bn in (True, False)}


@pytest.mark.parametrize("bn", (True, False))
def test_numpy_decoder_vs_reference_golden(dg, synth_params, bn):
    """Both are fp64; only the summation order differs."""
    s = f"_bn{int(bn)}"
    lg = R.block_maps(synth_params[bn], dg["z"])
    assert lg.shape == (3, 128, 240)
    np.testing.assert_allclose(lg[:, ::3, ::3], dg["logits_s3" + s], rtol=1e-10, atol=1e-10 * np.abs(lg).max())
    np.testing.assert_allclose(lg[:, -1, :], dg["logits_lastrow" + s], rtol=1e-10, atol=1e-10 * np.abs(lg).max())
    np.testing.assert_allclose(lg[:, :, -1], dg["logits_lastcol" + s], rtol=1e-10, atol=1e-10 * np.abs(lg).max())
    np.testing.assert_allclose(R.sigmoid(R.bilinear(lg[:1], (270, 480)))[0, ::3, ::3], dg["img270_s3" + s], rtol=1e-10)
    np.testing.assert_allclose(R.sigmoid(R.bilinear(lg, (54, 96))), dg["img54" + s], rtol=1e-10)


def test_golden_file_is_small(dg):
    path = os.path.join(os.path.dirname(__file__), "golden", "vae_dec_golden.npz")
    assert os.path.getsize(path) < 1 << 20
    assert dg["z"].shape == (3, 128) and all(dg[k].dtype == np.float64 for k in dg.files)


def test_spec_and_synthetic_weights():
    spec = V.DEFAULT_DECODER
    shapes = spec.param_shapes()
    assert sum(int(np.prod(s)) for _, s in shapes) == 10456481 + 0  # 10.45 M parameters
    assert spec.n_flops() == 2 * 1794048000
    p = V.synthetic_decoder(spec, 0)
    assert list(p) == [n for n, _ in shapes] and all(p[n].shape == s and p[n].dtype == np.float32 for n, s in shapes)
    assert all(np.array_equal(p[n], v) for n, v in V.synthetic_decoder(spec, 0).items())  # deterministic
    assert not np.array_equal(p["layers.resnet.4.layers.0.weight"], V.synthetic_decoder(spec, 1)["layers.resnet.4.layers.0.weight"])
    w = p["layers.resnet.4.layers.0.weight"]  # [Cin][Cout][3][3], U(+-sqrt(6 / (Cin 9)))
    assert w.shape == (512, 256, 3, 3) and np.abs(w).max() <= np.sqrt(6 / (512 * 9)) and np.abs(w).max() > 0.99 * np.sqrt(6 / (512 * 9))
    v = p["layers.resnet.4.layers.1.running_var"]
    assert v.min() >= 0.5 and v.max() <= 1.5 and v.std() > 0.1  # non-trivial statistics
    # without batchnorm the convolutions carry biases, and the shortcut keeps its BatchNorm (resnet.py:98-101)
    names = [n for n, _ in V.DecoderSpec(batchnorm=False).param_shapes()]
    assert "layers.resnet.4.layers.0.bias" in names and "layers.resnet.4.shortcut.0.bias" in names
    assert "layers.resnet.4.shortcut.1.running_var" in names and "layers.resnet.4.layers.1.weight" not in names
    # the encoder's stream is another one
    assert not np.array_equal(V.synthetic_encoder(V.DEFAULT_ENCODER, 0)["layers.resnet.0.bias"][:8],
                              p["layers.resnet.0.bias"][:8])


@pytest.mark.parametrize("bn", (True, False))
def test_fold_and_pack_round_trip(synth_params, bn):
    """The blob holds the folded layers in launch order; evaluating the FOLDED layers as plain biased transposed
    convolutions reproduces the unfolded decoder (BatchNorm on the output-channel axis of [Cin][Cout][k][k])."""
    spec, params = V.DecoderSpec(batchnorm=bn), synth_params[bn]
    blob = V.pack_decoder(spec, params)
    assert blob[:8] == b"SDFNVAED"
    L, got_bn, layers = V.unpack_decoder(blob)
    assert (L, got_bn) == (128, bn)
    want = V.decoder_layers(spec, params)
    assert [n for n, _, _ in layers] == [n for n, _, _ in want] == ["head"] + [f"d{i}{k}" for i in range(4) for k in "asb"] + ["tail"]
    for (n, w, b), (_, w2, b2) in zip(layers, want):
        assert w.dtype == np.float32 and np.array_equal(w, w2) and np.array_equal(b, b2), n
    # the folded layers, in fp64, on one latent
    f64 = {n: (w, b) for n, w, b in V.decoder_layers(spec, params, dtype=np.float64)}
    z = np.linspace(-1.5, 1.5, 128)[None]
    x = R.elu(z @ f64["head"][0] + f64["head"][1]).reshape(1, 8, 15, 512).transpose(0, 3, 1, 2)
    for i in range(4):
        wt = lambda k: f64[f"d{i}{k}"][0].transpose(2, 3, 0, 1)  # noqa: E731  [k][k][Cin][Cout] -> torch's layout
        y = np.maximum(R.conv_transpose(x, wt("a"), f64[f"d{i}a"][1], 2, 1, 1), 0.0)
        y = R.conv_transpose(y, wt("b"), f64[f"d{i}b"][1], 1, 1, 0)
        x = np.maximum(y + R.conv_transpose(x, wt("s"), f64[f"d{i}s"][1], 2, 0, 1), 0.0)
    tw = f64["tail"][0][:, :, :, None].transpose(2, 3, 0, 1)
    lg = R.conv_transpose(x, tw, f64["tail"][1], 1, 2, 0)[:, 0]
    ref = R.block_maps(params, z)
    np.testing.assert_allclose(lg, ref, rtol=0, atol=1e-12 * np.abs(ref).max())


def test_decoder_from_state_dict_accepts_a_whole_vae(synth_params):
    enc = V.synthetic_encoder(V.DEFAULT_ENCODER, 0)
    for bn in (True, False):
        dec = synth_params[bn]
        sd = {"encoder." + k: v for k, v in enc.items()}
        sd.update({"decoder." + k: v for k, v in dec.items()})
        sd["decoder.layers.resnet.4.shortcut.1.num_batches_tracked"] = np.array(7)
        spec, params = V.decoder_from_state_dict(sd)
        assert spec == V.DecoderSpec(size_latent=128, batchnorm=bn)
        assert list(params) == [n for n, _ in spec.param_shapes()]
        assert all(np.array_equal(params[k], dec[k]) for k in dec)
        spec2, params2 = V.decoder_from_state_dict(dec)  # a bare Decoder's keys
        assert spec2 == spec and all(np.array_equal(params2[k], dec[k]) for k in dec)
    # the encoder's converter keeps its return value on the same whole-Vae key set
    espec, eparams = V.from_state_dict(sd)
    assert espec == V.EncoderSpec(size_latent=128, batchnorm=True) and all(np.array_equal(eparams[k], enc[k]) for k in enc)
    s64 = V.DecoderSpec(size_latent=64)
    assert V.decoder_from_state_dict(V.synthetic_decoder(s64, 3))[0] == s64


def test_refusals(synth_params):
    dec = synth_params[True]
    with pytest.raises(ValueError):  # no decoder among the keys
        V.decoder_from_state_dict({"encoder." + k: v for k, v in V.synthetic_encoder(V.DEFAULT_ENCODER, 0).items()})
    bad = dict(dec)
    bad["layers.resnet.5.layers.0.weight"] = bad["layers.resnet.5.layers.0.weight"][:, :-1]
    with pytest.raises(ValueError):
        V.decoder_from_state_dict(bad)
    with pytest.raises(ValueError):
        V.pack_decoder(V.DEFAULT_DECODER, bad)
    missing = {k: v for k, v in dec.items() if k != "layers.resnet.8.bias"}
    with pytest.raises(ValueError):
        V.decoder_from_state_dict(missing)
    with pytest.raises(ValueError):
        V.pack_decoder(V.DecoderSpec(nb_chan=2), dec)
    with pytest.raises(ValueError):  # batchnorm parameters under a spec without batchnorm
        V.pack_decoder(V.DecoderSpec(batchnorm=False), dec)
    blob = V.pack_decoder(V.DEFAULT_DECODER, dec)
    for broken in (blob[:10], blob[:-4], b"SDFNVAEW" + blob[8:]):
        with pytest.raises(ValueError):
            V.unpack_decoder(broken)
