"""The VAE encoder on the GPU (csrc/vae_enc.hip, sdfnmpc_vae_load / sdfnmpc_vae_encode) at image shapes and latent sizes
other than 270 x 480 and 128 (tests/vae_shape_cases.py says what each shape reaches), against the fp64 C oracle
(oracle/vae.c) and the plain restatement (tests/vae_enc_ref.py), both pinned to the reference's own ``Encoder`` at these
shapes by tests/test_vae_enc_ref.py.  Small maps make an edge visible: at 36 x 50 a wrong border column is a quarter of
the last map, and that test shows a flipped border row or column to move the latent by 500 bars or more.

One encoder is loaded per case (45 MB of weights each) and shared by the tests; all are freed with the module."""
import copy
import re
import struct
import types

import numpy as np
import pytest

import vae_enc_ref as R
import vae_shape_cases as SC
from sdf_nmpc_amd import _lib, synth
from sdf_nmpc_amd import vae as V
from tolerances import VAE_LATENT_RTOL, vae_latent_err

pytestmark = pytest.mark.gpu

E_FORMAT, E_UNSUPPORTED = -3, -4  # SDFNMPC_E_FORMAT, SDFNMPC_E_UNSUPPORTED (include/sdfnmpc.h)


def _views(spec, flat):
    """The parameter dict as views of the flat vector (one copy of the 11 M weights per case on the host)."""
    out, off = {}, 0
    for name, shape in spec.param_shapes():
        n = int(np.prod(shape))
        out[name] = flat[off:off + n].reshape(shape)
        off += n
    return out


def _load(gpu_ctx, cfg, H, W, L, edit=None):
    spec = SC.spec_of(H, W, L)
    params, flat = SC.weights_of(spec)
    params = _views(spec, flat)
    if edit is not None:
        edit(params)  # in place: flat follows
    vae = _lib.Vae(gpu_ctx, V.pack(spec, params))
    assert vae.size_latent == L
    yz = V.depth2range_table((H, W), cfg.sensor.hfov, cfg.sensor.vfov)
    return types.SimpleNamespace(spec=spec, params=params, flat=flat, vae=vae, yz=yz, H=H, W=W, L=L)


@pytest.fixture(scope="module")
def encoders(gpu_ctx, cfg):
    """(H, W, L) -> the loaded encoder of that case, made on first use."""
    cache = {}

    def get(H, W, L):
        if (H, W, L) not in cache:
            cache[(H, W, L)] = _load(gpu_ctx, cfg, H, W, L)
        return cache[(H, W, L)]

    yield get
    for e in cache.values():
        e.vae.close()


def _encode(gpu_ctx, cfg, e, imgs, clip=SC.CLIP, yz=True):
    """(latent fp32 [B, L], latent64 [B, L]) of raw images [B, Hi, Wi] (float32 or uint16)."""
    import torch
    t = torch.from_numpy(np.ascontiguousarray(imgs)).cuda()
    yzt = torch.from_numpy(e.yz).cuda()
    B = imgs.shape[0]
    lat = torch.full((B, e.L), np.nan, dtype=torch.float32, device="cuda")
    lat64 = torch.full((B, e.L), np.nan, dtype=torch.float64, device="cuda")
    torch.cuda.synchronize()
    _lib.vae_encode(gpu_ctx, e.vae, _lib.vae_opts(cfg, clip), t, yzt, lat, lat64, depth2range=yz)
    torch.cuda.synchronize()
    return lat.cpu().numpy(), lat64.cpu().numpy()


def _oracle(oracle_lib, e, imgs, clip=SC.CLIP, yz=True, return_pre=False):
    pre = np.stack([oracle_lib.vae_preprocess(im, (e.H, e.W), clip, e.yz if yz else None) for im in imgs])
    lat = oracle_lib.vae_encode(pre, e.flat, L=e.L)
    return (lat, pre) if return_pre else lat


def _assert_bar(lat, ref, what):
    errs = [vae_latent_err(lat[b], ref[b]) for b in range(len(ref))]
    print(f"{what}: max error {max(errs):.2e} of the latent's scale (bar {VAE_LATENT_RTOL:.0e})")
    assert np.isfinite(lat).all(), what
    assert max(errs) <= VAE_LATENT_RTOL, (what, int(np.argmax(errs)), max(errs))


# (a) ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", SC.CASES, ids=SC.CASE_IDS)
def test_parity_per_case(case, gpu_ctx, cfg, oracle_lib, encoders):
    """B = 5: a ragged group of 4 images in the head; M crosses a 128-row tile inside an image at the larger shapes."""
    H, W, L, _ = case
    e = encoders(H, W, L)
    imgs = SC.images(5, H, W)
    lat, lat64 = _encode(gpu_ctx, cfg, e, imgs)
    _assert_bar(lat, _oracle(oracle_lib, e, imgs), f"{SC.case_key(H, W, L)} B=5")
    assert np.array_equal(lat64, lat.astype(np.float64))


# (b) ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("H,W,L,B", [(8, 8, 128, 130), (9, 11, 32, 70)], ids=["8x8_B130", "9x11_B70"])
def test_many_images_in_one_tile(H, W, L, B, gpu_ctx, cfg, oracle_lib, encoders):
    """(8, 8) at B = 130: every convolution has M = 130 rows of 130 different images, one full tile and one of 2 rows;
    (9, 11) at B = 70: M = 280 in the first block, 70 after."""
    e = encoders(H, W, L)
    imgs = SC.images(B, H, W)
    lat, lat64 = _encode(gpu_ctx, cfg, e, imgs)
    _assert_bar(lat, _oracle(oracle_lib, e, imgs), f"{SC.case_key(H, W, L)} B={B}")
    assert np.array_equal(lat64, lat.astype(np.float64))


# (c) ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("H,W", [(36, 50), (8, 8)], ids=["36x50", "8x8"])
def test_last_map_elementwise(H, W, gpu_ctx, cfg, oracle_lib):
    """size_latent = 2048 with the mean Linear the identity: the last maps are 2 x 2 and 1 x 1, every adaptive-pool bin
    is one pixel, so the "latent" is the last ResBlock's output itself, element by element -- an error in one channel
    or one output pixel is not averaged away by a 2048-long dot product.  Also vae_linear_kernel at 64 output groups.
    The bar: VAE_LATENT_RTOL of max |feature| of the image; the restatement's own fp32 evaluation is within 4.7e-7 of
    that scale (tests/tolerances.py), so the bar has 20x of headroom over plain fp32."""
    def identity_head(p):
        p["layers.mean.weight"][...] = np.eye(2048, dtype=np.float32)
        p["layers.mean.bias"][...] = 0.0

    e = _load(gpu_ctx, cfg, H, W, 2048, edit=identity_head)
    try:
        imgs = SC.images(5, H, W)
        lat, _ = _encode(gpu_ctx, cfg, e, imgs)
    finally:
        e.vae.close()
    pre = np.stack([oracle_lib.vae_preprocess(im, (H, W), SC.CLIP, e.yz) for im in imgs])
    feat = R.features_ref(e.spec, e.params, pre)
    assert feat.shape == lat.shape == (5, 2048)
    assert (np.abs(feat) > 0).mean() > 0.2  # a live map, not one the ReLU has emptied
    worst = 0.0
    for b in range(5):
        scale = np.abs(feat[b]).max()
        d = np.abs(lat[b].astype(np.float64) - feat[b]).max() / scale
        worst = max(worst, d)
    print(f"{H}x{W} L=2048 identity head: max elementwise error {worst:.2e} of max |feature|")
    assert np.isfinite(lat).all()
    assert worst <= VAE_LATENT_RTOL


# (d) ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("H,W,L", [(36, 50, 128), (61, 135, 128)], ids=["36x50", "61x135"])
def test_edges_follow_the_oracle(H, W, L, gpu_ctx, cfg, oracle_lib, encoders):
    """Two normalised images and their four border-row / border-column flips in one batch (clip 1, no Depth2Range: the
    encoder sees exactly these pixels).  Each latent meets the bar against its own oracle latent, and the GPU's move
    from the base latent agrees with the oracle's move (>= 440 bars, tests/test_vae_enc_ref.py) to two bars."""
    e = encoders(H, W, L)
    base = SC.normalised(SC.images(2, H, W))
    batch = np.concatenate([base] + [SC.perturbed(base, w) for w in SC.BORDERS])
    lat, _ = _encode(gpu_ctx, cfg, e, batch, clip=1.0, yz=False)
    ref, pre = _oracle(oracle_lib, e, batch, clip=1.0, yz=False, return_pre=True)
    assert np.array_equal(pre, batch)
    _assert_bar(lat, ref, f"{H}x{W} borders")
    for k, where in enumerate(SC.BORDERS):
        for b in range(2):
            i = 2 * (k + 1) + b
            scale = np.abs(ref[b]).max()
            d_gpu = lat[i].astype(np.float64) - lat[b].astype(np.float64)
            d_ref = ref[i] - ref[b]
            assert np.abs(d_ref).max() >= 100 * VAE_LATENT_RTOL * scale, (where, b)
            assert np.abs(d_gpu - d_ref).max() <= 2 * VAE_LATENT_RTOL * scale, (where, b)


# (e) ------------------------------------------------------------------------------------------------------------
def test_batch_independence_and_repeatability(gpu_ctx, cfg, encoders):
    e = encoders(23, 77, 40)
    imgs = SC.images(9, 23, 77)
    a, _ = _encode(gpu_ctx, cfg, e, imgs)
    b, _ = _encode(gpu_ctx, cfg, e, imgs)
    assert np.isfinite(a).all() and np.array_equal(a, b)
    for i in (0, 4, 8):
        s, _ = _encode(gpu_ctx, cfg, e, imgs[i:i + 1])
        assert np.array_equal(s[0], a[i]), i


# (f) ------------------------------------------------------------------------------------------------------------
def test_nan_at_the_far_corner(gpu_ctx, cfg, oracle_lib, encoders):
    """Pixel (35, 49) sits in the stem's last pool window, the one that also holds the -inf padding column (Wc = 25):
    the NaN-sticky maximum must let the NaN win over -inf.  As in the reference and the oracle, the NaN reaches every
    output of its image and no other image."""
    e = encoders(36, 50, 128)
    imgs = SC.images(3, 36, 50)
    clean, _ = _encode(gpu_ctx, cfg, e, imgs)
    bad = imgs.copy()
    bad[1, 35, 49] = np.nan
    lat, _ = _encode(gpu_ctx, cfg, e, bad)
    ref = _oracle(oracle_lib, e, bad)
    assert np.isnan(ref[1]).all() and np.isfinite(ref[[0, 2]]).all()
    assert np.isnan(lat[1]).all()
    assert np.array_equal(lat[0], clean[0]) and np.array_equal(lat[2], clean[2])


# (g) ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("yz", [True, False], ids=["depth2range", "no_depth2range"])
def test_resize_and_uint16_into_a_small_encoder(yz, gpu_ctx, cfg, oracle_lib, encoders):
    e = encoders(36, 50, 128)
    up = synth.depth_images(2, 18, 32, seed=SC.IMAGE_SEED)              # float32 metres, upsampled
    mm = synth.depth_images(2, 61, 135, seed=SC.IMAGE_SEED, kind="mm")  # uint16 millimetres, downsampled
    assert up.dtype == np.float32 and mm.dtype == np.uint16
    for name, imgs, clip in (("float32 18x32", up, SC.CLIP), ("uint16 61x135", mm, 5000.0)):
        lat, _ = _encode(gpu_ctx, cfg, e, imgs, clip=clip, yz=yz)
        _assert_bar(lat, _oracle(oracle_lib, e, imgs, clip=clip, yz=yz), f"{name} -> 36x50 yz={yz}")


# (h) ------------------------------------------------------------------------------------------------------------
def test_wrapper_at_a_non_default_config(gpu_ctx, cfg, oracle_lib):
    """VaeWrapper builds its spec from cfg.sensor.shape_imgs and cfg.nn.size_latent.  (The config's nn.vae_seed takes
    precedence over the ``seed`` argument, so both are set.)"""
    cfg2 = copy.deepcopy(cfg)
    cfg2.sensor.shape_imgs = [1, 36, 50]
    cfg2.nn.size_latent = 40
    cfg2.nn.vae_seed = SC.WEIGHT_SEED
    assert tuple(cfg.sensor.shape_imgs) == (1, 270, 480) and cfg.nn.size_latent == 128  # the copy is a copy
    imgs = SC.images(3, 36, 50)
    w = V.VaeWrapper(cfg2, batch=3, ctx=gpu_ctx, seed=SC.WEIGHT_SEED, decoder=True)
    try:
        assert w.spec == SC.spec_of(36, 50, 40)
        w.set_img(imgs)
        got = w.encode()
        rec = w.decode()
    finally:
        w.close()
    e = _load(gpu_ctx, cfg2, 36, 50, 40)
    try:
        lat, _ = _encode(gpu_ctx, cfg2, e, imgs, clip=V.clip_scale(cfg2))
    finally:
        e.vae.close()
    assert got.shape == (3, 40) and np.array_equal(got, lat)
    _assert_bar(lat, _oracle(oracle_lib, e, imgs, clip=V.clip_scale(cfg2)), "wrapper 36x50 L=40")
    assert rec.shape == (3, 36, 50) and rec.dtype == np.float32
    assert np.isfinite(rec).all() and rec.min() >= 0.0 and rec.max() <= 1.0


# (i) ------------------------------------------------------------------------------------------------------------
def _patched(blob, **fields):
    names = ("magic", "version", "nb_chan", "L", "H", "W", "n_convs", "n_floats", "reserved")
    h = dict(zip(names, V._HDR.unpack_from(blob)))
    h.update(fields)
    return V._HDR.pack(*[h[n] for n in names]) + blob[V._HDR.size:]


def test_loader_refusals(gpu_ctx, cfg, oracle_lib, encoders):
    """Every malformed or unsupported blob is refused with its code before anything is uploaded or launched, and the
    context is left usable: a valid load and encode after each refusal gives the latents of the first one, bit for bit."""
    e = encoders(8, 8, 128)
    blob = V.pack(e.spec, e.params)
    assert V._HDR.size == 40 and struct.calcsize("<8s8I") == 40
    n_floats = V._HDR.unpack_from(blob)[7]
    assert len(blob) == 40 + 4 * n_floats and V._HDR.unpack_from(blob)[6] == 13
    imgs = SC.images(5, 8, 8)
    want, _ = _encode(gpu_ctx, cfg, e, imgs)
    _assert_bar(want, _oracle(oracle_lib, e, imgs), "8x8 before the refusals")
    bad = [
        ("wrong magic", _patched(blob, magic=b"SDFNVAEX"), E_FORMAT),
        ("version 2", _patched(blob, version=2), E_FORMAT),
        ("cut inside the header", blob[:20], E_FORMAT),
        ("cut inside the body", blob[:40 + 4 * (n_floats // 2)], E_FORMAT),
        ("H = 7", _patched(blob, H=7), E_UNSUPPORTED),
        ("W = 7", _patched(blob, W=7), E_UNSUPPORTED),
        ("L = 0", _patched(blob, L=0), E_UNSUPPORTED),
        ("L = 4097", _patched(blob, L=4097), E_UNSUPPORTED),
        ("n_convs = 12", _patched(blob, n_convs=12), E_UNSUPPORTED),
        # the size agrees with the header, the header's count not with the layer list
        ("n_floats + 1", _patched(blob, n_floats=n_floats + 1) + b"\0\0\0\0", E_FORMAT),
    ]
    for what, b, code in bad:
        with pytest.raises(_lib.SdfnmpcError) as ei:
            _lib.Vae(gpu_ctx, b)
        m = re.match(r"sdfnmpc error (-?\d+): (.+)", str(ei.value))
        assert m and int(m.group(1)) == code and "vaew" in m.group(2), (what, str(ei.value))
        again = types.SimpleNamespace(**{**vars(e), "vae": _lib.Vae(gpu_ctx, blob)})
        try:
            got, _ = _encode(gpu_ctx, cfg, again, imgs)
        finally:
            again.vae.close()
        assert np.array_equal(got, want), what
