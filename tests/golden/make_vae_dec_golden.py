"""Regenerates tests/golden/vae_dec_golden.npz: the reference's own VAE decoder on synthetic weights.

    python tests/golden/make_vae_dec_golden.py <path of the reference checkout>

For ``batchnorm`` True and False, the reference's ``Decoder`` (sdf_nmpc/network/vae.py:63-90) in eval mode and
fp64 is loaded with ``sdf_nmpc_amd.vae.synthetic_decoder(DecoderSpec(batchnorm=...), seed 0)`` and run on three
latents (L = 128, U(-2, 2) from the counter-based PRNG).  Written, arrays only, suffix ``_bn1`` / ``_bn0``:

  z ...................... [3, 128] the latents (shared)
  logits_s3 .............. [3, 43, 80]  the pre-upsample logits [3, 128, 240] at rows / columns 0, 3, 6, ...
  logits_lastrow/_lastcol  [3, 240] / [3, 128]  their last row and last column
  img270_s3 .............. [90, 160] the image of latent 0 at (270, 480), rows / columns 0, 3, 6, ...
  img54 .................. [3, 54, 96] the images at (54, 96)

The dense fp64 arrays would take 3.8 MB; a committed file may hold 1 MiB, so the two large maps are sampled with
stride 3 (both parities of both axes, every 2 x 2 output phase of the stride-2 layers) plus the far edges.  No
weights are stored: the 10.45 M parameters come from the PRNG.  The script also prints the reference's own
fp32-against-fp64 gap (tests/vae_dec_tolerances.py quotes it).
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)

from sdf_nmpc_amd import vae as V  # noqa: E402
from sdf_nmpc_amd.weights import prng_uniform  # noqa: E402


def latents():
    return np.stack([4.0 * prng_uniform(4242, b, 128) - 2.0 for b in range(3)])


def main(ref_root):
    import torch

    sys.path.insert(0, ref_root)
    from sdf_nmpc.network.vae import Decoder

    z = latents()
    out = {"z": z}
    for bn in (True, False):
        spec = V.DecoderSpec(batchnorm=bn)
        params = V.synthetic_decoder(spec, 0)
        res = {}
        for dt in (torch.float64, torch.float32):
            for size in ((270, 480), (54, 96)):
                dec = Decoder(1, 128, size, batchnorm=bn).to(dt).eval()
                sd = dec.state_dict()
                for k in sd:
                    if not k.endswith("num_batches_tracked"):
                        assert tuple(sd[k].shape) == tuple(params[k].shape), k
                        sd[k] = torch.from_numpy(params[k]).to(dt)
                assert set(params) == {k for k in sd if not k.endswith("num_batches_tracked")}
                dec.load_state_dict(sd)
                with torch.no_grad():
                    zt = torch.from_numpy(z).to(dt)
                    res[(dt, size)] = dec(zt)[:, 0].double().numpy()
                    if size == (270, 480):
                        res[(dt, "logits")] = dec.layers["resnet"][:9](zt)[:, 0].double().numpy()
        lg, i270, i54 = res[(torch.float64, "logits")], res[(torch.float64, (270, 480))], res[(torch.float64, (54, 96))]
        assert lg.shape == (3, 128, 240) and i270.shape == (3, 270, 480) and i54.shape == (3, 54, 96)
        gl = np.abs(res[(torch.float32, "logits")] - lg).max() / np.abs(lg).max()
        gi = np.abs(res[(torch.float32, (270, 480))] - i270).max()
        print(f"batchnorm={bn}: max|logit| {np.abs(lg).max():.4f}, image range [{i270.min():.3f}, {i270.max():.3f}]; "
              f"reference fp32 vs fp64: logits {gl:.2e} of max|logit|, image (270, 480) {gi:.2e} absolute")
        s = f"_bn{int(bn)}"
        out.update({"logits_s3" + s: lg[:, ::3, ::3], "logits_lastrow" + s: lg[:, -1, :], "logits_lastcol" + s: lg[:, :, -1],
                    "img270_s3" + s: i270[0, ::3, ::3], "img54" + s: i54})
    path = os.path.join(HERE, "vae_dec_golden.npz")
    np.savez(path, **out)
    print(path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main(sys.argv[1])
