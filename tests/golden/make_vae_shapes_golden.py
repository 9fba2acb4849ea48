"""Regenerates tests/golden/vae_shapes_golden.npz: the reference's own VAE encoder at the image shapes and latent sizes
of tests/vae_shape_cases.py, on synthetic weights.

    python tests/golden/make_vae_shapes_golden.py <path of the reference checkout>

For every case (H, W, L) the reference's ``Encoder`` (sdf_nmpc/network/vae.py:6-46) in eval mode is loaded with
``sdf_nmpc_amd.vae.synthetic_encoder(EncoderSpec(size_latent=L, shape=(H, W)), 3)`` and run on three images,
``synth.depth_images(3, H, W, seed=5) / 5`` clipped to [0, 1] (vae_shape_cases.normalised).  Written, arrays only, per
case key ``<H>x<W>_L<L>``:

  <key>/latent64 .. [3, L] float64  the Encoder in fp64
  <key>/latent .... [3, L] float32  the reference's own fp32 run

No weights and no images are stored: both come from the counter-based PRNG.  The script prints the reference's own
fp32-against-fp64 gap per case (tests/tolerances.py quotes the largest).
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import vae_shape_cases as SC  # noqa: E402


def main(ref_root):
    import torch

    sys.path.insert(0, ref_root)
    from sdf_nmpc.network.vae import Encoder

    out = {}
    for H, W, L, _ in SC.CASES:
        spec = SC.spec_of(H, W, L)
        params, _ = SC.weights_of(spec)
        pre = SC.normalised(SC.images(SC.GOLDEN_B, H, W))
        res = {}
        for dt in (torch.float64, torch.float32):
            enc = Encoder(1, L, batchnorm=True).to(dt).eval()
            sd = enc.state_dict()
            for k in sd:
                if not k.endswith("num_batches_tracked"):
                    assert tuple(sd[k].shape) == tuple(params[k].shape), k
                    sd[k] = torch.from_numpy(params[k]).to(dt)
            assert set(params) == {k for k in sd if not k.endswith("num_batches_tracked")}
            enc.load_state_dict(sd)
            with torch.no_grad():
                res[dt] = enc(torch.from_numpy(pre).to(dt)[:, None]).numpy()
        l64, l32 = res[torch.float64], res[torch.float32]
        assert l64.shape == (SC.GOLDEN_B, L) and l64.dtype == np.float64 and l32.dtype == np.float32
        gap = max(np.abs(l32[b].astype(np.float64) - l64[b]).max() / np.abs(l64[b]).max() for b in range(SC.GOLDEN_B))
        key = SC.case_key(H, W, L)
        print(f"{key}: max|latent| {np.abs(l64).max():.4f}, reference fp32 vs fp64 {gap:.2e} of the latent's scale")
        out[key + "/latent64"] = l64
        out[key + "/latent"] = l32
    path = os.path.join(HERE, "vae_shapes_golden.npz")
    np.savez(path, **out)
    print(path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main(sys.argv[1])
