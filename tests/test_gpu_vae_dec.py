"""VAE decoder on the GPU (csrc/vae_dec.hip) through the C ABI and ``VaeWrapper``: against the reference's own
``Decoder`` outputs (tests/golden/vae_dec_golden.npz) and the numpy fp64 restatement tests/vae_dec_ref.py, at the
north-star fp32 bars of tests/vae_dec_tolerances.py."""
import ctypes as C
import os

import numpy as np
import pytest

import vae_dec_ref as R
from sdf_nmpc_amd import _lib, synth
from sdf_nmpc_amd import vae as V
from sdf_nmpc_amd.weights import prng_uniform
from vae_dec_tolerances import VAE_DEC_IMG_ATOL, VAE_DEC_LOGIT_RTOL

pytestmark = pytest.mark.gpu

SIZES = ((270, 480), (54, 96), (128, 240), (7, 9))  # the sensor's, downsampling, identity, an odd size
CONFIGS = ((128, True), (128, False), (64, True), (64, False))  # (size_latent, batchnorm)


@pytest.fixture(scope="module")
def dg():
    return np.load(os.path.join(os.path.dirname(__file__), "golden", "vae_dec_golden.npz"))


@pytest.fixture(scope="module")
def decs(gpu_ctx):
    """Per (L, batchnorm): the parameters, the device decoder, five latents and their fp64 logits, computed once."""
    out = {}
    for L, bn in CONFIGS:
        spec = V.DecoderSpec(size_latent=L, batchnorm=bn)
        params = V.synthetic_decoder(spec, 0)
        z = np.stack([4.0 * prng_uniform(977 + L, b, L) - 2.0 for b in range(5)]).astype(np.float32)
        out[(L, bn)] = dict(spec=spec, params=params, dec=_lib.VaeDec(gpu_ctx, V.pack_decoder(spec, params)), z=z,
                            logits=R.block_maps(params, z.astype(np.float64)))
    yield out
    for d in out.values():
        d["dec"].close()


def _decode(ctx, dec, z, size, want_logits=True):
    z = np.ascontiguousarray(z, dtype=np.float32)
    B = z.shape[0]
    dz = _lib.DeviceArray.from_numpy(ctx, z)
    img = _lib.DeviceArray(ctx, (B,) + tuple(size), np.float32)
    lg = _lib.DeviceArray(ctx, (B, 128, 240), np.float32) if want_logits else None
    _lib.vae_decode(ctx, dec, dz, img, lg)
    ctx.synchronize()
    return img.numpy(), (lg.numpy() if want_logits else None)


def test_decoder_vs_reference_golden(gpu_ctx, decs, dg):
    """The golden latents against the reference's own fp64 Decoder (stride-3 samples and far edges of the large maps)."""
    for bn in (True, False):
        s, dec = f"_bn{int(bn)}", decs[(128, bn)]["dec"]
        img, lg = _decode(gpu_ctx, dec, dg["z"], (270, 480))
        scale = max(np.abs(dg["logits_s3" + s]).max(), np.abs(dg["logits_lastrow" + s]).max())
        e_lg = max(np.abs(lg[:, ::3, ::3] - dg["logits_s3" + s]).max(), np.abs(lg[:, -1, :] - dg["logits_lastrow" + s]).max(),
                   np.abs(lg[:, :, -1] - dg["logits_lastcol" + s]).max()) / scale
        e_270 = np.abs(img[0, ::3, ::3] - dg["img270_s3" + s]).max()
        img54, _ = _decode(gpu_ctx, dec, dg["z"], (54, 96), want_logits=False)
        e_54 = np.abs(img54 - dg["img54" + s]).max()
        print(f"batchnorm={bn}: logits {e_lg:.2e} of max|logit|, image (270, 480) {e_270:.2e}, (54, 96) {e_54:.2e}")
        assert e_lg <= VAE_DEC_LOGIT_RTOL, (bn, e_lg)
        assert e_270 <= VAE_DEC_IMG_ATOL and e_54 <= VAE_DEC_IMG_ATOL, (bn, e_270, e_54)


@pytest.mark.parametrize("B", (1, 3, 5))
@pytest.mark.parametrize("L,bn", CONFIGS)
def test_shapes_vs_numpy(gpu_ctx, decs, L, bn, B):
    """B = 3, 5: image boundaries fall inside M tiles at the 16 x 30 map (480 cells an image, 256 a tile); 5 crosses
    the head's grouping of four images.  Every output size: the sensor's, downsampling, identity, odd."""
    d = decs[(L, bn)]
    ref = d["logits"][:B]
    for size in SIZES:
        img, lg = _decode(gpu_ctx, d["dec"], d["z"][:B], size)
        e_lg = np.abs(lg - ref).max() / np.abs(ref).max()
        e_img = np.abs(img - R.sigmoid(R.bilinear(ref, size))).max()
        print(f"L={L} batchnorm={bn} B={B} {size}: logits {e_lg:.2e}, image {e_img:.2e}")
        assert e_lg <= VAE_DEC_LOGIT_RTOL, (size, e_lg)
        assert e_img <= VAE_DEC_IMG_ATOL, (size, e_img)
        assert img.min() >= 0.0 and img.max() <= 1.0


def test_map_edges(gpu_ctx, decs):
    """The last row and column of every map, by name: there the odd-phase taps of the stride-2 layers fall outside
    the input (its zero padding at the bottom and right), the shortcut's last row and column are shift-only
    phases, and the 3x3 / 5x5 taps leave the map.  The last row of the map with h rows covers the logits' last
    128 / h rows (plus the two rows the later layers' taps reach back): each band is checked on its own, as is
    the first row and column."""
    d = decs[(128, True)]
    ref = d["logits"][:3]
    _, lg = _decode(gpu_ctx, d["dec"], d["z"][:3], (128, 240))
    scale = np.abs(ref).max()
    for h in (8, 16, 32, 64, 128):
        n = 128 // h + (2 if h < 128 else 0)
        e_row = np.abs(lg[:, -n:, :] - ref[:, -n:, :]).max() / scale
        e_col = np.abs(lg[:, :, -n:] - ref[:, :, -n:]).max() / scale
        assert e_row <= VAE_DEC_LOGIT_RTOL, f"last row of the {h} x {h * 15 // 8} map: {e_row:.2e}"
        assert e_col <= VAE_DEC_LOGIT_RTOL, f"last column of the {h} x {h * 15 // 8} map: {e_col:.2e}"
    assert np.abs(lg[:, 0] - ref[:, 0]).max() / scale <= VAE_DEC_LOGIT_RTOL, "first row"
    assert np.abs(lg[:, :, 0] - ref[:, :, 0]).max() / scale <= VAE_DEC_LOGIT_RTOL, "first column"
    # the corner pixel sees every one of them at once
    assert abs(lg[:, -1, -1] - ref[:, -1, -1]).max() / scale <= VAE_DEC_LOGIT_RTOL, "bottom-right corner"


def test_batch_invariance_determinism_nan(gpu_ctx, decs):
    d = decs[(128, True)]
    z = d["z"]
    img5, lg5 = _decode(gpu_ctx, d["dec"], z, (54, 96))
    again, lg_again = _decode(gpu_ctx, d["dec"], z, (54, 96))
    assert np.array_equal(img5, again) and np.array_equal(lg5, lg_again), "a second call differs"
    for b in range(5):
        img1, lg1 = _decode(gpu_ctx, d["dec"], z[b:b + 1], (54, 96))
        assert np.array_equal(lg1[0], lg5[b]) and np.array_equal(img1[0], img5[b]), f"image {b} depends on its batch"
    zn = z.copy()
    zn[2, 17] = np.nan
    imgn, lgn = _decode(gpu_ctx, d["dec"], zn, (54, 96))
    assert not np.isfinite(imgn[2]).any() and not np.isfinite(lgn[2]).any(), "a NaN latent must poison its image"
    for b in (0, 1, 3, 4):
        assert np.array_equal(imgn[b], img5[b]) and np.array_equal(lgn[b], lg5[b]), f"the NaN of image 2 reached image {b}"


def test_kernel_stats_names(gpu_ctx, decs):
    d = decs[(128, True)]
    gpu_ctx.enable_timing(True)
    gpu_ctx.reset_stats()
    try:
        _decode(gpu_ctx, d["dec"], d["z"][:2], (54, 96))
        names = ["vae_dec_head", "vae_dec_tail", "vae_dec_resize"] + [f"vae_dec_{k}{c}" for k in ("up", "sc", "conv")
                                                                       for c in (256, 128, 64, 32)]
        for n in names:
            ms, cnt = gpu_ctx.kernel_stats(n)
            assert cnt == 1 and ms > 0.0, n
    finally:
        gpu_ctx.enable_timing(False)
        gpu_ctx.reset_stats()


def test_wrapper(gpu_ctx, cfg):
    """``decode`` after ``set_latent`` and after ``encode`` (the latent on the device), ``decode_to`` and
    ``reconstruct`` bitwise the same, ValueError without a decoder."""
    B = 2
    vae = V.VaeWrapper(cfg, batch=B, ctx=gpu_ctx, decoder=True)
    L = vae.spec.size_latent
    params = V.synthetic_decoder(vae.dec_spec, 0)
    z = np.stack([2.0 * prng_uniform(31, b, L) - 1.0 for b in range(B)]).astype(np.float32)
    vae.set_latent(z)
    img = vae.decode()
    assert img.shape == (B,) + tuple(cfg.sensor.shape_imgs[-2:]) and img.dtype == np.float32
    assert np.abs(img - R.decode(params, z.astype(np.float64), img.shape[1:])).max() <= VAE_DEC_IMG_ATOL
    small = vae.decode((54, 96))
    assert small.shape == (B, 54, 96)
    out = _lib.DeviceArray(gpu_ctx, (B, 54, 96), np.float32)
    assert np.array_equal(vae.decode_to(out).numpy(), small)
    # after encode(): the latent decoded is the one on the device
    raw = synth.depth_images(B, 270, 480, seed=5)
    vae.set_img(raw)
    lat = vae.encode()
    after = vae.decode((54, 96))
    assert np.abs(after - R.decode(params, lat.astype(np.float64), (54, 96))).max() <= VAE_DEC_IMG_ATOL
    rec = vae.reconstruct(raw)
    assert rec.shape == (B, 270, 480)
    assert np.array_equal(rec.numpy(), vae.decode((270, 480)))
    assert np.array_equal(vae.latent.numpy(), lat)
    with pytest.raises(ValueError):
        vae.decode_to(_lib.DeviceArray(gpu_ctx, (B + 1, 54, 96), np.float32))
    plain = V.VaeWrapper(cfg, batch=1, ctx=gpu_ctx)
    assert plain.dec is None
    with pytest.raises(ValueError):
        plain.decode()
    with pytest.raises(ValueError):
        plain.reconstruct(raw[:1])
    one = V.VaeWrapper(cfg, batch=1, ctx=gpu_ctx, decoder=(vae.dec_spec, params))
    one.set_latent(z[0])
    assert one.decode((54, 96)).shape == (54, 96)
    assert np.array_equal(one.decode((54, 96)), small[0])
    # one device output is kept, whatever sizes are swept; close() frees the handles and may be repeated
    for size in ((7, 9), (12, 20), (54, 96)):
        one.decode(size)
        assert list(one._dec_out) == [size]
    for w in (one, plain, vae):
        w.close()
        w.close()
        assert w.vae.h is None and not w._dec_out and (w.dec is None or w.dec.h is None)


def test_c_refusals_launch_nothing(gpu_ctx, decs):
    d = decs[(128, True)]
    lib = _lib.load()
    dz = _lib.DeviceArray.from_numpy(gpu_ctx, d["z"][:2])
    sentinel = np.full((2, 7, 9), -3.0, np.float32)
    img = _lib.DeviceArray.from_numpy(gpu_ctx, sentinel)
    ctx, dec, E_ARG = gpu_ctx.h, d["dec"].h, -1
    calls = [(None, dec, 2, dz.data_ptr(), 7, 9, img.data_ptr(), None), (ctx, None, 2, dz.data_ptr(), 7, 9, img.data_ptr(), None),
             (ctx, dec, 2, None, 7, 9, img.data_ptr(), None), (ctx, dec, 2, dz.data_ptr(), 7, 9, None, None),
             (ctx, dec, -1, dz.data_ptr(), 7, 9, img.data_ptr(), None), (ctx, dec, 2, dz.data_ptr(), 0, 9, img.data_ptr(), None),
             (ctx, dec, 2, dz.data_ptr(), 7, 0, img.data_ptr(), None)]
    gpu_ctx.enable_timing(True)
    gpu_ctx.reset_stats()
    try:
        for c in calls:
            assert lib.sdfnmpc_vae_decode(*c) == E_ARG, c
        assert lib.sdfnmpc_vae_decode(ctx, dec, 0, None, 7, 9, None, None) == 0  # B == 0: a no-op
        other = _lib.Context(gpu_ctx.device)  # the workspace ties the decoder to the context it was loaded on
        assert lib.sdfnmpc_vae_decode(other.h, dec, 2, dz.data_ptr(), 7, 9, img.data_ptr(), None) == E_ARG
        assert other.kernel_stats("vae_dec_head")[1] == 0
        other.close()
        gpu_ctx.synchronize()
        assert gpu_ctx.kernel_stats("vae_dec_head")[1] == 0, "a refused call launched a kernel"
    finally:
        gpu_ctx.enable_timing(False)
        gpu_ctx.reset_stats()
    assert np.array_equal(img.numpy(), sentinel)
    assert lib.sdfnmpc_vae_dec_size_latent(dec) == 128 and lib.sdfnmpc_vae_dec_size_latent(None) == -1
    h = C.c_void_p()
    blob = V.pack_decoder(d["spec"], d["params"])
    assert lib.sdfnmpc_vae_dec_load(ctx, blob[:100], 100, C.byref(h)) != 0 and not h.value  # truncated
    enc = V.pack(V.DEFAULT_ENCODER, V.synthetic_encoder(V.DEFAULT_ENCODER, 0))
    assert lib.sdfnmpc_vae_dec_load(ctx, enc, len(enc), C.byref(h)) != 0 and not h.value  # the encoder's magic
