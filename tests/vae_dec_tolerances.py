"""Tolerances of the VAE decoder tests (fp32 network, csrc/vae_dec.hip), beside tests/tolerances.py.

The reference's own fp32 torch decoder differs from its fp64 evaluation, on the golden latents
(tests/golden/make_vae_dec_golden.py prints it), by 9.0e-7 (batchnorm) / 9.3e-7 (none) x max|logit| on the
pre-upsample logits and by 2.5e-6 / 1.4e-6 absolute on the image at (270, 480): under a third of either bar.  The GPU
kernels (fp32-exact split products, BatchNorm folded, another summation order) are held to the north-star fp32 bar of
tests/tolerances.py against the fp64 values: 1e-5 relative to max|logit| on the logits, 1e-5 absolute on the image (the
sigmoid's slope is <= 1/4 and the resize a convex combination).
"""
VAE_DEC_LOGIT_RTOL = 1e-5
VAE_DEC_IMG_ATOL = 1e-5
