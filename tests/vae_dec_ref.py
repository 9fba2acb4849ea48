"""numpy fp64 restatement of the reference's VAE decoder (sdf_nmpc/network/vae.py:63-90, resnet.py:59-111) in eval
mode, written from the layer definitions: every layer as torch defines it, on the UNFOLDED parameters of
``sdf_nmpc_amd.vae.DecoderSpec.param_shapes`` (the BatchNorms applied as such), so that it checks the host's
folding and tap tables as well as the kernels.  tests/golden/vae_dec_golden.npz pins it to the reference's own
``Decoder`` (tests/test_vae_dec_ref.py).
"""
import numpy as np

BN_EPS = 1e-5
BLOCKS = (512, 256, 128, 64)


def conv_transpose(x, w, b, stride, pad, out_pad):
    """torch.nn.ConvTranspose2d: x [B, Cin, H, W], w [Cin, Cout, k, k] -> [B, Cout, Ho, Wo],
    out[co, s iy - pad + ky, s ix - pad + kx] += x[ci, iy, ix] w[ci, co, ky, kx]."""
    B, _, H, W = x.shape
    k = w.shape[2]
    Ho, Wo = (H - 1) * stride - 2 * pad + k + out_pad, (W - 1) * stride - 2 * pad + k + out_pad
    out = np.zeros((B, w.shape[1], Ho, Wo))
    for ky in range(k):
        for kx in range(k):
            c = np.einsum("bchw,cd->bdhw", x, w[:, :, ky, kx], optimize=True)
            iy = np.arange(H)
            ix = np.arange(W)
            oy, ox = stride * iy - pad + ky, stride * ix - pad + kx
            my, mx = (oy >= 0) & (oy < Ho), (ox >= 0) & (ox < Wo)
            out[:, :, oy[my][:, None], ox[mx][None, :]] += c[:, :, iy[my][:, None], ix[mx][None, :]]
    if b is not None:
        out += b[None, :, None, None]
    return out


def batchnorm(x, p, prefix):
    g, beta, m, v = (p[prefix + s].astype(np.float64) for s in (".weight", ".bias", ".running_mean", ".running_var"))
    return (x - m[None, :, None, None]) / np.sqrt(v[None, :, None, None] + BN_EPS) * g[None, :, None, None] + \
        beta[None, :, None, None]


def elu(x):
    return np.where(x > 0, x, np.expm1(np.minimum(x, 0)))


def bilinear(x, size):
    """torch Upsample(size, mode='bilinear', align_corners=False) of x [B, H, W]."""
    H, W = x.shape[-2:]
    h, w = size
    if (h, w) == (H, W):
        return x.copy()

    def axis(n_in, n_out):
        src = np.maximum((n_in / n_out) * (np.arange(n_out) + 0.5) - 0.5, 0.0)
        i0 = np.minimum(np.floor(src).astype(int), n_in - 1)
        i1 = np.minimum(i0 + 1, n_in - 1)
        return i0, i1, src - i0

    y0, y1, ly = axis(H, h)
    x0, x1, lx = axis(W, w)
    ly, lx = ly[None, :, None], lx[None, None, :]
    top = x[:, y0][:, :, x0] * (1 - lx) + x[:, y0][:, :, x1] * lx
    bot = x[:, y1][:, :, x0] * (1 - lx) + x[:, y1][:, :, x1] * lx
    return top * (1 - ly) + bot * ly


def sigmoid(x):
    return 1.0 / (1.0 + np.exp(-x))


def block_maps(params, z, return_maps=False):
    """Pre-upsample logits [B, 128, 240] of latents z [B, L] (fp64); with return_maps also every block's output."""
    p = {k: np.asarray(v, dtype=np.float64) for k, v in params.items()}

    def deconv(x, prefix, stride, pad, out_pad):
        return conv_transpose(x, p[prefix + ".weight"], p.get(prefix + ".bias"), stride, pad, out_pad)

    def norm(x, prefix):
        return batchnorm(x, p, prefix) if (prefix + ".running_mean") in p else x

    z = np.atleast_2d(np.asarray(z, dtype=np.float64))
    x = elu(z @ p["layers.resnet.0.weight"].T + p["layers.resnet.0.bias"]).reshape(z.shape[0], 512, 8, 15)
    maps = [x]
    for i in range(len(BLOCKS)):
        q = f"layers.resnet.{4 + i}"
        y = np.maximum(norm(deconv(x, q + ".layers.0", 2, 1, 1), q + ".layers.1"), 0.0)
        y = norm(deconv(y, q + ".layers.3", 1, 1, 0), q + ".layers.4")
        s = norm(deconv(x, q + ".shortcut.0", 2, 0, 1), q + ".shortcut.1")
        x = np.maximum(y + s, 0.0)
        maps.append(x)
    logits = deconv(x, "layers.resnet.8", 1, 2, 0)[:, 0]
    return (logits, maps) if return_maps else logits


def decode(params, z, size):
    """The decoder's image [B, h, w] of latents z [B, L] at ``size``, fp64."""
    return sigmoid(bilinear(block_maps(params, z), size))
