"""The reference's image morphology (utils/preprocessing.py:100-259) on the device: ``Dilate``, ``Erode``, ``Open``,
``Close`` and ``RemoveCloseOutliers`` with the reference's constructor arguments (``ctx`` instead of ``device``),
computed by csrc/morph.hip through sdfnmpc_morph / sdfnmpc_outlier_rm.

The modules are callable on a numpy array, a torch tensor or a ``_lib.DeviceArray`` of shape [H, W], [B, H, W] or
[B, 1, H, W] (float32, normalised by dmax as the reference's modules assume) and return the same kind and shape.  A
``DeviceArray`` result is asynchronous on the context stream; numpy and torch results are complete on return.  Unlike
the reference's modules, none of them modifies its input.

The semantics are the reference's as written, not a textbook's: the padding follows the element's origin (k // 2)
with border value -2 / +2, and ``Dilate`` scans the *flipped* element over the unflipped padding (include/sdfnmpc.h).
``ToDevice``, ``Reshape``, ``ClipDistance`` and ``Depth2Range`` are part of the encoder's first kernel (vae.py).
"""
from __future__ import annotations

import numpy as np

from . import _lib


def _element(kernel):
    k = np.asarray(kernel.cpu().numpy() if hasattr(kernel, "cpu") else kernel)
    if k.ndim != 2:
        raise ValueError(f"the structuring element must be 2-d, got shape {k.shape}")
    return np.ascontiguousarray(k != 0, dtype=np.uint8)


class _Images:
    """An input image batch on the device as float32 [B][H][W], and how to hand a result back as the input's kind."""

    def __init__(self, ctx, img):
        self.ctx = ctx
        self.shape = tuple(int(v) for v in img.shape)
        s = self.shape
        if len(s) == 4 and s[1] != 1:
            raise ValueError(f"a 4-d image batch must be [B, 1, H, W], got {s}")
        if len(s) not in (2, 3, 4):
            raise ValueError(f"images must be [H, W], [B, H, W] or [B, 1, H, W], got {s}")
        self.s3 = (1,) * (len(s) == 2) + (s[0],) * (len(s) > 2) + s[-2:]
        self.torch = type(img).__module__.split(".")[0] == "torch"
        self.like = img
        if isinstance(img, (_lib.DeviceArray, _lib.FieldView)):
            if np.dtype(img.dtype) != np.float32:
                raise TypeError(f"device images must be float32, got {img.dtype}")
            self.kind, self.dev = "device", _lib.FieldView(img.data_ptr(), self.s3, np.float32, ctx)
        elif self.torch and img.is_cuda:
            import torch
            if img.dtype != torch.float32 or not img.is_contiguous():
                raise TypeError("a device tensor must be contiguous float32")
            self.kind, self.dev = "cuda", _lib.FieldView(_lib.sync_producer(img).data_ptr(), self.s3, np.float32, ctx)
        else:
            a = img.detach().numpy() if self.torch else np.asarray(img)
            self.kind, self.dev = "host", _lib.DeviceArray.from_numpy(ctx, a.reshape(self.s3), dtype=np.float32)

    def new(self):
        """A float32 [B][H][W] device array for a result (for a device tensor: a new tensor's memory)."""
        if self.kind == "cuda":
            import torch
            t = torch.empty_like(self.like)
            _lib.sync_producer(t)
            v = _lib.FieldView(t.data_ptr(), self.s3, np.float32, self.ctx)
            v._tensor = t
            return v
        return _lib.DeviceArray(self.ctx, self.s3, np.float32)

    def give(self, out):
        if self.kind == "device":
            out.shape = self.shape  # the same memory under the caller's shape
            out._inputs = self.like
            return out
        if self.kind == "cuda":
            self.ctx.synchronize()
            return out._tensor
        a = out.numpy().reshape(self.shape)
        if self.torch:
            import torch
            return torch.from_numpy(a)
        return a


class _Morph:
    op = None

    def __init__(self, kernel=np.ones((3, 3)), ignore_zeros=False, ctx=None):
        if ctx is None:
            raise ValueError(f"{type(self).__name__} needs ctx, a _lib.Context (the morphology runs on the device)")
        self.ctx, self.kernel, self.ignore_zeros = ctx, _element(kernel), bool(ignore_zeros)

    def _run(self, src, dst):
        _lib.morph(self.ctx, _lib.MORPH_OPS[self.op], self.kernel, self.ignore_zeros, src, dst)

    def __call__(self, img):
        im = _Images(self.ctx, img)
        out = im.new()
        self._run(im.dev, out)
        return im.give(out)


class Dilate(_Morph):
    """preprocessing.py:100-148.  kernel: the structuring element (0s and 1s, at most 21 x 21)."""
    op = "dilate"


class Erode(_Morph):
    """preprocessing.py:152-199."""
    op = "erode"


class _Pair:
    first = second = None

    def __init__(self, kernel_erode=np.ones((3, 3)), kernel_dilate=np.ones((3, 3)), ctx=None):
        self.ctx = ctx
        self.erode, self.dilate = Erode(kernel_erode, False, ctx), Dilate(kernel_dilate, False, ctx)

    def __call__(self, img):
        im = _Images(self.ctx, img)
        mid, out = _lib.DeviceArray(self.ctx, im.s3, np.float32), im.new()
        getattr(self, self.first)._run(im.dev, mid)
        getattr(self, self.second)._run(mid, out)
        out._mid = mid  # the intermediate of an asynchronous pair stays alive with its result
        return im.give(out)


class Open(_Pair):
    """preprocessing.py:203-218: dilate(erode(img))."""
    first, second = "erode", "dilate"


class Close(_Pair):
    """preprocessing.py:222-237: erode(dilate(img))."""
    first, second = "dilate", "erode"


class RemoveCloseOutliers:
    """preprocessing.py:241-259: values below min_range become 0, the image is opened with a kernel_size x kernel_size
    element, and the thresholded value returns where the opening is > 0.  kernel_size 3 is one fused kernel."""

    def __init__(self, kernel_size=3, min_range=0.1, ctx=None):
        if ctx is None:
            raise ValueError("RemoveCloseOutliers needs ctx, a _lib.Context")
        self.ctx, self.kernel_size, self.min_range = ctx, int(kernel_size), float(min_range)

    def __call__(self, img):
        im = _Images(self.ctx, img)
        out = im.new()
        _lib.outlier_rm(self.ctx, self.kernel_size, self.min_range, im.dev, out)
        return im.give(out)
