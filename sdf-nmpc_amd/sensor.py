"""A reproducible model of an imperfect depth camera (csrc/sensor.hip, sdfnmpc_sensor_apply): no-return pixels,
range noise, dropped pixels and erased boxes, with 0 the invalid value -- the reference's training augmentation
(utils/data.py:11-108) as a function of (seed, stream, frame, pixel), optionally followed by the reference's
``RemoveCloseOutliers``.  ``SensorModel.apply`` degrades a device image in place; ``Nmpc.rollout(scene=, vae=,
sensor=)`` runs the same stage between the renderer and the encoder inside the device loop.

Units: ``noise_std``, ``noise_std_quad`` and ``min_range`` are in dmax-normalised units, as the reference's
``std_range = 0.02`` and ``min_range = 0.1`` are (an image in [0, 1]; multiply metres by 1 / sensor.dmax): the noise
standard deviation of a pixel of normalised value v is ``noise_std + noise_std_quad * v**2``.  ``apply`` converts them
to the units of the image it is given (normalised, or the raw sensor image of 1000 / mm_resolution per metre).

The erased boxes do not depend on the image, so they are drawn here with numpy, not on the device: ``box_table``
follows torchvision's ``RandomErasing`` as data.py:70,103-106 configures it.
"""
from __future__ import annotations

import math

import numpy as np

from . import _lib


def box_table(seed, streams, n_frames, H, W, p_box=0.3, n_min=1, n_max=4, scale=(0.02, 0.06), ratio=(0.2, 5.0),
              max_boxes=None):
    """int16 [n_frames][B][max_boxes][4] of (y0, x0, h, w), h == 0: none.  Entry (f, b) is drawn from
    numpy.random.default_rng([seed, f, streams[b]]) alone, so it does not depend on the batch around it: with
    probability p_box, n in [n_min, n_max] boxes, each of area H W uniform(scale) and aspect exp(uniform(log ratio)),
    h = round(sqrt(area aspect)), w = round(sqrt(area / aspect)), placed uniformly where it fits (0 < h < H and 0 < w <
    W, as RandomErasing asks); a box that does not fit after 10 draws is skipped."""
    streams = np.asarray(streams, dtype=np.int64).ravel()
    max_boxes = int(n_max if max_boxes is None else max_boxes)
    if not (0 <= n_min <= n_max <= max_boxes <= _lib.SENSOR_MAX_BOXES):
        raise ValueError(f"boxes: 0 <= n_min <= n_max <= max_boxes <= {_lib.SENSOR_MAX_BOXES}")
    if not (0.0 <= p_box <= 1.0 and 0.0 < scale[0] <= scale[1] and 0.0 < ratio[0] <= ratio[1]):
        raise ValueError("boxes: p_box in [0, 1], 0 < scale[0] <= scale[1], 0 < ratio[0] <= ratio[1]")
    if H > 32767 or W > 32767:
        raise ValueError("boxes: the table's entries are int16")
    tab = np.zeros((int(n_frames), streams.size, max_boxes, 4), np.int16)
    lr = (math.log(ratio[0]), math.log(ratio[1]))
    for f in range(int(n_frames)):
        for b, st in enumerate(streams):
            rng = np.random.default_rng([int(seed) & (2**64 - 1), f, int(st) & 0xffffffff])
            if not rng.random() < p_box:
                continue
            slot = 0
            for _ in range(int(rng.integers(n_min, n_max + 1))):
                for _try in range(10):
                    area = H * W * rng.uniform(scale[0], scale[1])
                    aspect = math.exp(rng.uniform(lr[0], lr[1]))
                    h, w = int(round(math.sqrt(area * aspect))), int(round(math.sqrt(area / aspect)))
                    if not (0 < h < H and 0 < w < W):
                        continue
                    tab[f, b, slot] = (rng.integers(0, H - h + 1), rng.integers(0, W - w + 1), h, w)
                    slot += 1
                    break
    return tab


class SensorModel:
    """The degradation of one camera per instance.  cfg: the config (sensor.dmax, sensor.mm_resolution); ctx: the
    context the images live on; seed: the 64-bit key of every random decision.

    noise_std, noise_std_quad: the range noise a + b v^2 (normalised units, see the module text); dropout: the
    probability that a pixel is lost; boxes: None, or a dict of ``box_table``'s keywords (p_box, n_min, n_max, scale,
    ratio); miss_invalid: a pixel at or beyond dmax reads 0, as a real depth camera reports no return; outlier_rm,
    min_range: ``RemoveCloseOutliers(3, min_range)`` after the degradation; frames: the period of the box table (the
    boxes of frame f are those of f % frames); stream_id: one int per instance, the camera's identity in the random
    streams (None: the instance's index) -- two instances with the same stream_id see the same noise."""

    def __init__(self, cfg, ctx, seed, noise_std=0.0, noise_std_quad=0.0, dropout=0.0, boxes=None, miss_invalid=False,
                 outlier_rm=False, min_range=0.1, frames=64, stream_id=None):
        if not (math.isfinite(noise_std) and noise_std >= 0 and math.isfinite(noise_std_quad) and noise_std_quad >= 0):
            raise ValueError("noise_std and noise_std_quad must be finite and not negative")
        if not 0.0 <= dropout < 1.0:
            raise ValueError(f"dropout {dropout}: a probability in [0, 1)")
        if int(frames) < 1:
            raise ValueError("frames must be at least 1")
        self.cfg, self.ctx, self.seed = cfg, ctx, int(seed) & (2**64 - 1)
        self.noise_std, self.noise_std_quad, self.dropout = float(noise_std), float(noise_std_quad), float(dropout)
        self.boxes = None if boxes is None else dict(boxes)
        self.miss_invalid, self.outlier_rm, self.min_range = bool(miss_invalid), bool(outlier_rm), float(min_range)
        self.frames = int(frames)
        self.stream_id = None if stream_id is None else np.ascontiguousarray(stream_id, dtype=np.int32).ravel()
        self.p_thresh = min(int(math.floor(self.dropout * 2.0**32)), 2**32 - 1)
        self._dev = {}

    @classmethod
    def reference_augment(cls, cfg, ctx, seed, **kw):
        """The reference's training augmentation (data.py:39-48): std_range 0.02, 3-10 % erased pixels (here their
        midpoint), and with probability 0.3 one to four boxes of area fraction 0.02-0.06 and aspect 0.2-5."""
        args = dict(noise_std=0.02, dropout=0.065,
                    boxes=dict(p_box=0.3, n_min=1, n_max=4, scale=(0.02, 0.06), ratio=(0.2, 5.0)))
        args.update(kw)
        return cls(cfg, ctx, seed, **args)

    def vmax(self, normalized) -> float:
        """The image's value at dmax: 1 for a normalised image, dmax * 1000 / mm_resolution for a raw one -- the fp32
        product the renderer writes for a pixel without a hit (csrc/scene.hip), so that miss_invalid finds it."""
        s = self.cfg.sensor
        return 1.0 if normalized else float(np.float32(s.dmax) * np.float32(1000.0 / float(s.mm_resolution)))

    def table(self, B, H, W):
        """The host box table for a batch of B images of H x W (None without boxes)."""
        if self.boxes is None:
            return None
        streams = np.arange(B) if self.stream_id is None else self.stream_id
        return box_table(self.seed, streams, self.frames, H, W, **self.boxes)

    def opts(self, B, H, W, normalized):
        """(SensorOptsC, scratch) for a batch of B images of H x W; the device arrays they name are cached here."""
        if self.stream_id is not None and self.stream_id.size != B:
            raise ValueError(f"stream_id names {self.stream_id.size} instances, the call has {B}")
        key = (int(B), int(H), int(W))
        if key not in self._dev:
            tab = self.table(B, H, W)
            self._dev[key] = dict(
                boxes=None if tab is None else _lib.DeviceArray.from_numpy(self.ctx, tab),
                stream=None if self.stream_id is None else _lib.DeviceArray.from_numpy(self.ctx, self.stream_id),
                scratch=_lib.DeviceArray(self.ctx, key, np.float32) if self.outlier_rm else None)
        d, s = self._dev[key], self.vmax(normalized)
        tab = d["boxes"]
        o = _lib.SensorOptsC(self.seed, self.noise_std * s, self.noise_std_quad / s, s, self.p_thresh,
                             int(self.miss_invalid), int(self.outlier_rm), self.min_range * s, _lib._ptr(tab),
                             self.frames, 0 if tab is None else int(tab.shape[2]), _lib._ptr(d["stream"]))
        return o, d["scratch"]

    def apply(self, img, frame, normalized=False):
        """Degrade img [B, H, W] float32 as frame number ``frame`` (>= 0).  A device array (DeviceArray, or a torch
        tensor on the context's device) is changed in place, asynchronously on the context stream, and returned; a
        numpy array is copied, and the degraded copy returned.  normalized: the image's units (False: the raw sensor
        image ``Scene.render(normalized=False)`` gives and ``VaeWrapper.set_img`` expects)."""
        host = not hasattr(img, "data_ptr")
        dev = _lib.DeviceArray.from_numpy(self.ctx, np.asarray(img), dtype=np.float32) if host else _lib.sync_producer(img)
        if len(dev.shape) != 3 or np.dtype(str(dev.dtype).replace("torch.", "")) != np.float32:
            raise ValueError(f"images must be float32 [B, H, W], got {dev.dtype} {tuple(dev.shape)}")
        o, scratch = self.opts(*(int(v) for v in dev.shape), normalized)
        _lib.sensor_apply(self.ctx, o, int(frame), dev, scratch)
        return dev.numpy() if host else img
