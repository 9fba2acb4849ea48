"""Collision check of points against depth or range images (the reference's utils/collision_checker.py:
ColChecker), on the HIP kernel of csrc/df_truth.hip through the C ABI (sdfnmpc_colcheck).

Same constructor, method, defaults and conventions as the reference; the Warp kernel it launched is restated
as written in the library.  Inputs are numpy arrays or torch tensors; the labels come back as a torch bool
tensor on the checker's device.  There is no CPU path: without a gfx950 device the first check raises.
"""
from __future__ import annotations

import numpy as np


def as_image_batch(imgs):
    """[B, H, W] or [H, W] -> torch tensor [B, H, W] (collision_checker.py:100-102)."""
    import torch
    if not torch.is_tensor(imgs):
        imgs = torch.from_numpy(np.asarray(imgs))
    if imgs.ndim == 2:
        imgs = imgs.unsqueeze(0)
    if imgs.ndim != 3:
        raise AssertionError('input image must have size [B, H, W] or [H, W]')
    return imgs


class _DeviceSide:
    """The context a checker launches on (created at first use, on torch's current stream of the device, so the
    launches are ordered with the caller's torch work) and the conversion of the inputs to device tensors."""

    def __init__(self, device=None):
        from . import _lib
        self._ctx = device if isinstance(device, _lib.Context) else None
        self._device_arg = None if self._ctx is not None else device

    @property
    def ctx(self):
        if self._ctx is None:
            import torch
            from . import _lib
            d = self._device_arg
            idx = 0 if d is None else d if isinstance(d, int) else (torch.device(d).index or 0)
            self._ctx = _lib.Context(idx, stream=torch.cuda.current_stream(idx).cuda_stream)
        return self._ctx

    @property
    def device(self):
        import torch
        return torch.device("cuda", self.ctx.device)

    def inputs(self, imgs, points, p_to_i):
        import torch
        dev = self.device
        imgs = as_image_batch(imgs).to(dev, torch.float32).contiguous()
        if not torch.is_tensor(points):
            points = torch.from_numpy(np.asarray(points))
        points = points.to(dev, torch.float32).reshape(-1, 3).contiguous()
        if p_to_i is not None:  # None: the default ordering, point j -> image j / (n / B), formed by the kernel
            if not torch.is_tensor(p_to_i):
                p_to_i = torch.from_numpy(np.asarray(p_to_i))
            p_to_i = p_to_i.to(dev, torch.int32).reshape(-1).contiguous()
            if p_to_i.shape[0] != points.shape[0]:
                raise ValueError("p_to_i needs one entry per point")
        return imgs, points, p_to_i

    def launch(self, fn, *outputs):
        """Run fn(ctx) once torch's current stream has produced the inputs and allocated the outputs, and wait
        for it, so that torch may read the outputs on any stream of its own."""
        from . import _lib
        _lib.sync_producer(outputs[0])
        fn(self.ctx)
        self.ctx.synchronize()


class ColChecker:
    """Parallelized collision checker in depth or range images.
    outside             -- 'col', 'free', or 'extrapolate'
    device              -- None (cuda:0), a device index / string / torch.device, or an sdf_nmpc_amd Context
    """

    def __init__(self, dmax, hfov, vfov, safe_ball_size, is_depth=False, is_spherical=False, outside='free',
                 device=None):
        assert outside in ['free', 'col', 'extrapolate']
        self.dmax = dmax
        self.hfov = hfov
        self.vfov = vfov
        self.safe_ball_size = safe_ball_size
        self.is_depth = is_depth
        self.is_spherical = is_spherical
        self.outside = 0 if outside == 'free' else 1 if outside == 'col' else 2
        self._dev = device if isinstance(device, _DeviceSide) else _DeviceSide(device)

    @property
    def device(self):
        return self._dev.device

    def check_image_points(self, imgs, points, p_to_i=None):
        """Collision labels (torch bool [n]) of points [n, 3] in the images.
        Size of image array: [B, H, W] or [H, W].
        Images are assumed normalized wrt dmax.
        Points are unormalized Cartesian coordinates.
        p_to_i is an array mapping each point to the index of the corresponding image (its entries must lie
        in [0, B): they are not checked). If set to None, default ordering is assumed.
        """
        import torch
        from . import _lib
        imgs, points, p_to_i = self._dev.inputs(imgs, points, p_to_i)
        out = torch.zeros(points.shape[0], dtype=torch.uint8, device=imgs.device)
        opts = _lib.img_opts(self.dmax, self.hfov, self.vfov, self.is_depth, self.is_spherical)
        self._dev.launch(lambda ctx: _lib.colcheck(ctx, opts, self.outside, self.safe_ball_size, imgs, points, p_to_i,
                                                   out), out)
        return out.bool()
