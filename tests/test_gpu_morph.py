"""csrc/morph.hip through sdf_nmpc_amd.preprocessing: bitwise against the reference's modules (the goldens) and against
the numpy restatement tests/preproc_ref.py on shapes that cross the kernel's tile seams, the border value, the
untouched input, the fused outlier removal against its three-launch composition, the kinds of input, the refusals."""
import ctypes as C

import numpy as np
import pytest

import preproc_ref as PR
from sdf_nmpc_amd import _lib
from sdf_nmpc_amd import preprocessing as P
from test_preproc_ref import golden_cases, run_case, same_bits

pytestmark = pytest.mark.gpu

T = _lib.MORPH_TILE
ELEMENTS = {"ones3": np.ones((3, 3), np.uint8), "asym": PR.ASYM, "disc3": PR.disc(3), "disc10": PR.disc(10)}
# B = 3 small odd images; one pixel beyond the tile and beyond twice the tile (halo seams, a partial last tile); one
# pixel; an image smaller than every element but the 3 x 3
SHAPES = [(3, 7, 13), (1, T + 1, T + 1), (2, 2 * T + 1, 2 * T + 1), (1, 1, 1), (2, 3, 2)]


def _image(shape, seed):
    """Values in [0.1, 1] with about a quarter of the pixels 0, in patches and alone."""
    rng = np.random.default_rng(seed)
    a = rng.uniform(0.1, 1.0, shape).astype(np.float32)
    a[rng.uniform(size=shape) < 0.15] = 0.0
    H, W = shape[-2:]
    for im in a.reshape(-1, H, W) if H > 4 else ():
        y, x = rng.integers(0, H), rng.integers(0, W)
        im[y:y + 4, x:x + 5] = 0.0
    return a


@pytest.mark.parametrize("name", golden_cases()[1])
def test_equals_the_reference_bitwise(gpu_ctx, name):
    G, _ = golden_cases()
    got = run_case(G, name, lambda a, k, iz: P.Dilate(k, iz, ctx=gpu_ctx)(a), lambda a, k, iz: P.Erode(k, iz, ctx=gpu_ctx)(a),
                   lambda a, ks, mr: P.RemoveCloseOutliers(ks, mr, ctx=gpu_ctx)(a))
    assert same_bits(got, G[f"{name}/out"])
    op = name.split("-")[0]
    if op in ("open", "close"):  # the composed modules, too
        cls = P.Open if op == "open" else P.Close
        assert same_bits(cls(G[f"{name}/kernel_erode"], G[f"{name}/kernel_dilate"], ctx=gpu_ctx)(G[f"{name}/img"]),
                         G[f"{name}/out"])


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_equals_the_restatement_bitwise_across_tile_seams(gpu_ctx, shape):
    img = _image(shape, 7)
    dev = _lib.DeviceArray.from_numpy(gpu_ctx, img)
    for ename, k in ELEMENTS.items():
        for iz in (False, True):
            got_d, got_e = P.Dilate(k, iz, ctx=gpu_ctx)(dev).numpy(), P.Erode(k, iz, ctx=gpu_ctx)(dev).numpy()
            assert same_bits(got_d, PR.dilate(img, k, iz)), (ename, iz, "dilate")
            assert same_bits(got_e, PR.erode(img, k, iz)), (ename, iz, "erode")
    assert same_bits(dev.numpy(), img)  # ignore_zeros calls included: the input is as it was
    for ks in (3, 5, 2):  # the fused launch, and the general path at an odd and an even size
        got = P.RemoveCloseOutliers(ks, 0.3, ctx=gpu_ctx)(dev).numpy()
        assert same_bits(got, PR.remove_close_outliers(img, ks, 0.3)), ks
    assert same_bits(P.Open(PR.ASYM, PR.disc(3), ctx=gpu_ctx)(img), PR.open_(img, PR.ASYM, PR.disc(3)))
    assert same_bits(P.Close(PR.ASYM, PR.disc(3), ctx=gpu_ctx)(img), PR.close(img, PR.ASYM, PR.disc(3)))


def test_border_value_where_every_included_tap_is_padding(gpu_ctx):
    one = np.ones((T + 3, T + 3), np.float32)
    e = P.Erode(PR.ASYM, ctx=gpu_ctx)(one)
    assert e[0, -1] == 2.0 and (np.delete(e.ravel(), T + 2) == 1.0).all()
    assert P.Erode(PR.ASYM, True, ctx=gpu_ctx)(one)[0, -1] == 0.0
    d = P.Dilate(np.array([[1, 0, 0]]), ctx=gpu_ctx)(np.full((2, 4), 0.5, np.float32))
    assert (d[:, :3] == 0.5).all() and (d[:, 3] == -1.5).all()  # the excluded taps' bias, as the reference's module


def test_fused_outlier_removal_equals_the_three_launch_composition(gpu_ctx):
    """outlier_rm_kernel against threshold; Erode(ones 3 x 3); Dilate(ones 3 x 3); restore, on an image with short
    values, isolated pixels and zero patches, over several tiles and a batch."""
    img = _image((3, 2 * T + 5, 3 * T + 2), 11)
    img[0, 5, 7] = 0.05
    img[1, :, 20] = 0.0
    ones = np.ones((3, 3))
    for min_range in (0.1, 0.35):
        t = np.where(img < np.float32(min_range), np.float32(0), img)
        m = P.Dilate(ones, ctx=gpu_ctx)(P.Erode(ones, ctx=gpu_ctx)(t))
        want = np.where(m > 0, t, m)
        got = P.RemoveCloseOutliers(3, min_range, ctx=gpu_ctx)(img)
        assert same_bits(got, want)
        assert (got == 0).sum() > (img == 0).sum()  # something was removed
    gpu_ctx.enable_timing(True)
    gpu_ctx.reset_stats()
    P.RemoveCloseOutliers(3, 0.1, ctx=gpu_ctx)(img)
    assert gpu_ctx.kernel_stats("outlier_rm")[1] == 1 and gpu_ctx.kernel_stats("morph")[1] == 0  # one fused launch
    P.RemoveCloseOutliers(5, 0.1, ctx=gpu_ctx)(img)
    assert gpu_ctx.kernel_stats("outlier_rm")[1] == 1 and gpu_ctx.kernel_stats("morph")[1] == 2
    gpu_ctx.enable_timing(False)


def test_kinds_of_input_come_back_as_they_came(gpu_ctx):
    import torch
    img = _image((2, 9, 11), 3)
    want = PR.erode(img, PR.disc(1))
    er = P.Erode(PR.disc(1), ctx=gpu_ctx)
    assert same_bits(er(img[0]), want[0]) and same_bits(er(img[:, None]), want[:, None])  # [H, W], [B, 1, H, W]
    t = er(torch.from_numpy(img))
    assert isinstance(t, torch.Tensor) and not t.is_cuda and same_bits(t.numpy(), want)
    src = torch.from_numpy(img).cuda()
    c = er(src)
    assert isinstance(c, torch.Tensor) and c.is_cuda and c.shape == src.shape and same_bits(c.cpu().numpy(), want)
    assert same_bits(src.cpu().numpy(), img)
    d = er(_lib.DeviceArray.from_numpy(gpu_ctx, img[:, None]))
    assert isinstance(d, _lib.DeviceArray) and d.shape == (2, 1, 9, 11) and same_bits(d.numpy(), want[:, None])
    er_t = P.Erode(torch.from_numpy(PR.disc(1)), ctx=gpu_ctx)  # the element may be a tensor, as in the reference
    assert same_bits(er_t(img), want)
    with pytest.raises(ValueError):
        er(np.zeros((2, 2, 9, 11), np.float32))
    with pytest.raises(ValueError):
        P.Dilate()


def test_refusals_launch_nothing(gpu_ctx):
    lib = _lib.load()
    B, H, W = 2, 5, 6
    src = _lib.DeviceArray.from_numpy(gpu_ctx, np.full((B, H, W), 0.5, np.float32))
    out = _lib.DeviceArray.from_numpy(gpu_ctx, np.full((B, H, W), 7.0, np.float32))
    ones = np.ones((21, 21), np.uint8)
    kp, s, o = ones.ctypes.data, src.data_ptr(), out.data_ptr()
    zeros = np.zeros((3, 3), np.uint8)
    bad_morph = [(None, 0, kp, 3, 3, 0, s, B, H, W, o), (gpu_ctx.h, 2, kp, 3, 3, 0, s, B, H, W, o),
                 (gpu_ctx.h, -1, kp, 3, 3, 0, s, B, H, W, o), (gpu_ctx.h, 0, None, 3, 3, 0, s, B, H, W, o),
                 (gpu_ctx.h, 0, kp, 22, 3, 0, s, B, H, W, o), (gpu_ctx.h, 1, kp, 3, 0, 0, s, B, H, W, o),
                 (gpu_ctx.h, 1, zeros.ctypes.data, 3, 3, 0, s, B, H, W, o), (gpu_ctx.h, 0, kp, 3, 3, 0, s, -1, H, W, o),
                 (gpu_ctx.h, 0, kp, 3, 3, 0, s, B, 0, W, o), (gpu_ctx.h, 0, kp, 3, 3, 0, s, B, H, 0, o),
                 (gpu_ctx.h, 0, kp, 3, 3, 0, None, B, H, W, o), (gpu_ctx.h, 0, kp, 3, 3, 0, s, B, H, W, None),
                 (gpu_ctx.h, 0, kp, 3, 3, 1, s, B, H, W, s)]
    for a in bad_morph:
        assert lib.sdfnmpc_morph(*a) == -1, a
    bad_rm = [(None, 3, 0.1, s, B, H, W, o), (gpu_ctx.h, 0, 0.1, s, B, H, W, o), (gpu_ctx.h, 22, 0.1, s, B, H, W, o),
              (gpu_ctx.h, 3, float("nan"), s, B, H, W, o), (gpu_ctx.h, 5, float("inf"), s, B, H, W, o),
              (gpu_ctx.h, 3, 0.1, s, -1, H, W, o), (gpu_ctx.h, 3, 0.1, s, B, 0, W, o), (gpu_ctx.h, 3, 0.1, None, B, H, W, o),
              (gpu_ctx.h, 3, 0.1, s, B, H, W, None), (gpu_ctx.h, 3, 0.1, s, B, H, W, s)]
    for a in bad_rm:
        assert lib.sdfnmpc_outlier_rm(*a) == -1, a
    assert (out.numpy() == 7.0).all() and (src.numpy() == 0.5).all()
    assert lib.sdfnmpc_morph(gpu_ctx.h, 0, kp, 3, 3, 0, None, 0, H, W, None) == 0  # B == 0: a no-op
    assert lib.sdfnmpc_outlier_rm(gpu_ctx.h, 3, C.c_float(0.1), None, 0, H, W, None) == 0
    with pytest.raises(_lib.SdfnmpcError, match="no 1"):
        P.Erode(np.zeros((3, 3)), ctx=gpu_ctx)(np.ones((4, 4), np.float32))
