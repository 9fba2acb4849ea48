"""Plain torch restatement of the reference's VAE encoder (sdf_nmpc/network/vae.py:6-46, resnet.py:5-56) in eval mode,
written from the layer definitions with torch's functional operations on the CPU: every layer as torch defines it, on
the UNFOLDED parameters of ``sdf_nmpc_amd.vae.EncoderSpec.param_shapes`` (each BatchNorm applied as such, from its
running statistics), so that it checks the host's folding (``vae._fold``) as well as the kernels and the C oracle
(oracle/vae.c).  Dropout and Dropout2d are identities in eval mode.  tests/golden/vae_shapes_golden.npz pins it to the
reference's own ``Encoder`` (tests/test_vae_enc_ref.py).  The counterpart of tests/vae_dec_ref.py.
"""
import numpy as np
import torch
import torch.nn.functional as F

BN_EPS = 1e-5
BLOCKS = ((64, 2), (128, 2), (256, 2), (512, 1))  # (size_in, stride) of the four ResBlocks


def _tensors(params, dtype):
    return {k: torch.from_numpy(np.ascontiguousarray(v)).to(dtype) for k, v in params.items()}


def _conv(p, x, prefix, stride, pad):
    return F.conv2d(x, p[prefix + ".weight"], p.get(prefix + ".bias"), stride=stride, padding=pad)


def _norm(p, x, prefix):
    if (prefix + ".running_mean") not in p:  # batchnorm=False: an Identity
        return x
    return F.batch_norm(x, p[prefix + ".running_mean"], p[prefix + ".running_var"], p[prefix + ".weight"],
                        p[prefix + ".bias"], training=False, eps=BN_EPS)


def last_map(spec, params, pre, dtype=torch.float64):
    """The last ResBlock's output [B, 512, h, w] (a torch tensor) on preprocessed images ``pre`` [B, H, W]."""
    p = _tensors(params, dtype)
    x = torch.from_numpy(np.array(pre, dtype=np.float32)).to(dtype)  # a copy: the caller's array may be read-only
    if x.ndim == 2:
        x = x[None]
    assert tuple(x.shape[-2:]) == tuple(spec.shape), (x.shape, spec.shape)
    x = x[:, None]  # one channel
    with torch.no_grad():
        x = F.elu(_conv(p, x, "layers.resnet.0", 2, 3))
        x = F.max_pool2d(x, kernel_size=3, stride=2, padding=1)
        for i, (cin, s) in enumerate(BLOCKS):
            q = f"layers.resnet.{3 + i}"
            assert x.shape[1] == cin
            y = F.relu(_norm(p, _conv(p, x, q + ".layers.0", s, 1), q + ".layers.1"))
            y = _norm(p, _conv(p, y, q + ".layers.3", 1, 1), q + ".layers.4")
            sc = x if s == 1 else _norm(p, _conv(p, x, q + ".shortcut.0", s, 0), q + ".shortcut.1")
            x = F.relu(y + sc)
    return x


def features_ref(spec, params, pre, dtype=torch.float64):
    """AdaptiveAvgPool2d((2, 2)) + Flatten of the last map: [B, 2048] (numpy, feature c * 4 + i * 2 + j), before the
    mean Linear."""
    x = last_map(spec, params, pre, dtype)
    with torch.no_grad():
        return F.adaptive_avg_pool2d(x, (2, 2)).flatten(1).numpy()


def encode_ref(spec, params, pre, dtype=torch.float64):
    """Encoder.forward: the latent means [B, L] (numpy, in ``dtype``) of preprocessed images ``pre`` [B, H, W]."""
    p = _tensors({k: params[k] for k in ("layers.mean.weight", "layers.mean.bias")}, dtype)
    f = torch.from_numpy(features_ref(spec, params, pre, dtype))
    with torch.no_grad():
        return (f @ p["layers.mean.weight"].T + p["layers.mean.bias"]).numpy()
