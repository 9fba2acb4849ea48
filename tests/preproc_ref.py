"""numpy restatement of the morphology csrc/morph.hip computes (include/sdfnmpc.h, sdfnmpc_morph / sdfnmpc_outlier_rm),
written from its stated semantics: pad by the element's origin (k // 2) on the top / left and k - origin - 1 on the
bottom / right with the border value -2 (dilate) / +2 (erode); the erosion is the minimum over the element's k_h x k_w
taps of the padded image plus a bias, 0 where the element is 1 and +2 where it is 0; the dilation the maximum with the
bias 0 / -2 of the *flipped* element on the same padding; with ignore_zeros zeros count as the border value and a
result equal to it becomes 0.  Inputs are never modified.
tests/test_preproc_ref.py pins it bitwise to the reference's modules through tests/golden/preproc_golden.npz."""
import numpy as np


def _scan(img, kernel, dilate, ignore_zeros):
    a = np.array(img, dtype=np.float32)  # a copy
    k = np.asarray(kernel) != 0
    if k.ndim != 2 or not k.any():
        raise ValueError("the structuring element needs a 1")
    (kh, kw), border = k.shape, np.float32(-2.0 if dilate else 2.0)
    oh, ow = kh // 2, kw // 2
    if ignore_zeros:
        a[a == 0] = border
    pad = np.pad(a, [(0, 0)] * (a.ndim - 2) + [(oh, kh - oh - 1), (ow, kw - ow - 1)], constant_values=border)
    H, W = a.shape[-2:]
    inc = k[::-1, ::-1] if dilate else k
    taps = [pad[..., i:i + H, j:j + W] + (np.float32(0) if inc[i, j] else border) for i in range(kh) for j in range(kw)]
    out = (np.maximum if dilate else np.minimum).reduce(taps)
    if ignore_zeros:
        out[out == border] = 0
    return out


def dilate(img, kernel=np.ones((3, 3)), ignore_zeros=False):
    return _scan(img, kernel, True, ignore_zeros)


def erode(img, kernel=np.ones((3, 3)), ignore_zeros=False):
    return _scan(img, kernel, False, ignore_zeros)


def open_(img, kernel_erode=np.ones((3, 3)), kernel_dilate=np.ones((3, 3))):
    return dilate(erode(img, kernel_erode), kernel_dilate)


def close(img, kernel_erode=np.ones((3, 3)), kernel_dilate=np.ones((3, 3))):
    return erode(dilate(img, kernel_dilate), kernel_erode)


def remove_close_outliers(img, kernel_size=3, min_range=0.1):
    a = np.asarray(img, dtype=np.float32)
    t = np.where(a < np.float32(min_range), np.float32(0), a)
    k = np.ones((kernel_size, kernel_size))
    m = open_(t, k, k)
    return np.where(m > 0, t, m)


def disc(radius):
    """The (2 r + 1)^2 disc element: 1 where i^2 + j^2 <= r^2 from the centre."""
    r = np.arange(-radius, radius + 1)
    return (r[:, None] ** 2 + r[None, :] ** 2 <= radius * radius).astype(np.uint8)


ASYM = np.array([[1, 1, 0], [0, 1, 0], [0, 0, 0], [0, 0, 1]], np.uint8)  # even-sized and asymmetric: exposes the flip
