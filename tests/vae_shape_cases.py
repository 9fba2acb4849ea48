"""TEST INFRASTRUCTURE: the image shapes and latent sizes the VAE encoder is tested at besides 270 x 480
(tests/test_vae_enc_ref.py on the CPU, tests/test_gpu_vae_shapes.py on the device, tests/golden/make_vae_shapes_golden.py).

Each case: (H, W, L, maps) with ``maps`` what ``EncoderSpec.maps()`` must give -- the stem convolution, the maxpool, then
the four block outputs.  What each reaches in csrc/vae_enc.hip (ST_PY x ST_PX = 7 x 8 pooled stem tiles, HD_OUT = 32
outputs per linear workgroup, 128-row GEMM tiles; maps 1..3 are stored in parity-phase column order, vae_col):

  (8, 8, 128)     the loader's minimum; 3x3 convolutions on 2x2 and 1x1 maps (only the centre tap inside); every head
                  bin on the one pixel
  (9, 11, 32)     odd input; a phased map of width 3
  (36, 50, 128)   Wc = 25 odd: the pool's right-hand padding column; Hc = 18 even: no bottom padding; two stem tiles in
                  x, the second with 5 of 8 columns; phased widths 13 and 7
  (23, 77, 40)    three x tiles, the last with 4 of 8; phased width 5; the head on a 1 x 3 map; L no multiple of 32
  (61, 135, 128)  phased widths 17 and 9; five x tiles, the last with 2 of 8
  (64, 96, 1)     everything even; L = 1
  (90, 30, 200)   tall; exactly one x tile; the head's map 1 wide, so its bins overlap; L = 200: 7 output groups
"""
import numpy as np

WEIGHT_SEED = 3   # V.synthetic_encoder(spec, WEIGHT_SEED)
IMAGE_SEED = 5    # synth.depth_images(B, H, W, seed=IMAGE_SEED)
CLIP = 5.0        # metres: ClipDistance of the float32 images
GOLDEN_B = 3      # images per case in tests/golden/vae_shapes_golden.npz

CASES = [
    (8, 8, 128, [(4, 4), (2, 2), (1, 1), (1, 1), (1, 1), (1, 1)]),
    (9, 11, 32, [(5, 6), (3, 3), (2, 2), (1, 1), (1, 1), (1, 1)]),
    (36, 50, 128, [(18, 25), (9, 13), (5, 7), (3, 4), (2, 2), (2, 2)]),
    (23, 77, 40, [(12, 39), (6, 20), (3, 10), (2, 5), (1, 3), (1, 3)]),
    (61, 135, 128, [(31, 68), (16, 34), (8, 17), (4, 9), (2, 5), (2, 5)]),
    (64, 96, 1, [(32, 48), (16, 24), (8, 12), (4, 6), (2, 3), (2, 3)]),
    (90, 30, 200, [(45, 15), (23, 8), (12, 4), (6, 2), (3, 1), (3, 1)]),
]
CASE_IDS = [f"{h}x{w}_L{l}" for h, w, l, _ in CASES]


def case_key(H, W, L):
    return f"{H}x{W}_L{L}"


def spec_of(H, W, L, batchnorm=True):
    from sdf_nmpc_amd import vae as V
    return V.EncoderSpec(size_latent=L, shape=(H, W), batchnorm=batchnorm)


def weights_of(spec):
    """(params, flat): the synthetic parameters of a spec and their concatenation in state_dict order (the oracle's)."""
    from sdf_nmpc_amd import vae as V
    params = V.synthetic_encoder(spec, WEIGHT_SEED)
    return params, flat_of(spec, params)


def flat_of(spec, params):
    return np.concatenate([params[n].ravel() for n, _ in spec.param_shapes()])


def images(B, H, W):
    """Raw float32 depth images in metres."""
    from sdf_nmpc_amd import synth
    return synth.depth_images(B, H, W, seed=IMAGE_SEED)


def normalised(imgs):
    """Depth / 5 m clipped to [0, 1], float32: preprocessed pixels without the Depth2Range table."""
    return np.clip(np.asarray(imgs, np.float32) / np.float32(CLIP), 0.0, 1.0).astype(np.float32)


def flip(x):
    """The +-0.25 perturbation of normalised pixels that stays in [0, 1]: x - 0.25 where x > 0.5, else x + 0.25."""
    x = np.asarray(x, np.float32)
    return np.where(x > 0.5, x - np.float32(0.25), x + np.float32(0.25)).astype(np.float32)


BORDERS = ("row0", "rowN", "col0", "colN")
CORNERS = ("c00", "c0N", "cN0", "cNN")


def perturbed(pre, where):
    """A copy of normalised images [B, H, W] with one border row / column, or one corner pixel, flipped."""
    out = np.array(pre, np.float32, copy=True)
    sl = {"row0": (slice(None), 0, slice(None)), "rowN": (slice(None), -1, slice(None)),
          "col0": (slice(None), slice(None), 0), "colN": (slice(None), slice(None), -1),
          "c00": (slice(None), 0, 0), "c0N": (slice(None), 0, -1), "cN0": (slice(None), -1, 0),
          "cNN": (slice(None), -1, -1)}[where]
    out[sl] = flip(out[sl])
    return out
