"""In-loop VAE encoder: depth image -> latent, on the device, for config C5.

Host-side plumbing: architecture spec, deterministic synthetic weights, BatchNorm folding into the
packed `.vaew` layout that ``csrc/vae_enc.hip`` consumes through the C ABI (``include/sdfnmpc.h``),
the Depth2Range table, and ``VaeWrapper`` -- the mirror of the reference's ``sdf_nmpc/vae.py``
``VaeWrapper`` (set_img / set_latent / encode / decode) whose encode and decode run on the GPU.  The decoder
(``DecoderSpec``, ``synthetic_decoder``, ``pack_decoder``: a `.vaed` blob of its own for ``csrc/vae_dec.hip``) is
optional (``VaeWrapper(..., decoder=)``).

Reference anchors (``/root/reference``):
  * encoder architecture ........ ``sdf_nmpc/network/vae.py:6-46`` (``Encoder``; ``forward`` = mean head)
  * residual block .............. ``sdf_nmpc/network/resnet.py:5-56`` (``ResBlock``, non-bottleneck)
  * preprocessing ............... ``sdf_nmpc/vae.py:15-24`` -> ``utils/preprocessing.py``
                                  ``ToDevice`` :263-276, ``Reshape`` :99-112, ``ClipDistance`` :84-96,
                                  ``Depth2Range`` :5-30
  * wrapper API ................. ``sdf_nmpc/vae.py:7-50``

Inference semantics (``model.eval()``): Dropout / Dropout2d are identities and BatchNorm uses its
running statistics, so every BatchNorm folds into the preceding convolution:
``w' = w * g / sqrt(v + eps)``, ``b' = (b - m) * g / sqrt(v + eps) + beta`` (fp64, rounded once to fp32).

The real ``vae.pt`` is a git-LFS pointer in the reference checkout, so tests use weights from the
counter-based PRNG of ``weights.py`` (``synthetic_encoder``); ``from_state_dict`` / ``from_torchscript``
convert a real checkpoint offline.
"""
from __future__ import annotations

import dataclasses
import struct
from typing import Dict, List, Tuple

import numpy as np

from .weights import prng_uniform

MAGIC = b"SDFNVAEW"
VERSION = 1
BN_EPS = 1e-5  # torch.nn.BatchNorm2d default (resnet.py:32-37)
_HDR = struct.Struct("<8s8I")  # magic, version, nb_chan, size_latent, H, W, n_convs, n_floats, reserved


@dataclasses.dataclass(frozen=True)
class EncoderSpec:
    """``Encoder(nb_chan, size_latent, batchnorm)`` (vae.py:11) on ``shape_imgs`` (default.yaml sensor)."""
    nb_chan: int = 1
    size_latent: int = 128
    shape: Tuple[int, int] = (270, 480)
    batchnorm: bool = True
    widths: Tuple[int, ...] = (64, 128, 256, 512)  # ResBlock inputs (vae.py:22-25), strides 2,2,2,1

    def blocks(self):
        """(size_in, stride) of the four ResBlocks."""
        return [(64, 2), (128, 2), (256, 2), (512, 1)]

    def maps(self):
        """Spatial sizes: stem conv, maxpool, then each block output."""
        H, W = self.shape
        conv = lambda n, k, s, p: (n + 2 * p - k) // s + 1  # noqa: E731
        h, w = conv(H, 7, 2, 3), conv(W, 7, 2, 3)
        out = [(h, w)]
        h, w = conv(h, 3, 2, 1), conv(w, 3, 2, 1)
        out.append((h, w))
        for _, s in self.blocks():
            h, w = conv(h, 3, s, 1), conv(w, 3, s, 1)
            out.append((h, w))
        return out

    def param_shapes(self) -> List[Tuple[str, Tuple[int, ...]]]:
        """``Encoder.state_dict()`` names and shapes in order (num_batches_tracked omitted)."""
        bn = self.batchnorm
        out = [("layers.resnet.0.weight", (64, self.nb_chan, 7, 7)), ("layers.resnet.0.bias", (64,))]

        def conv(prefix, cin, cout, k):
            out.append((prefix + ".weight", (cout, cin, k, k)))
            if not bn:
                out.append((prefix + ".bias", (cout,)))

        def norm(prefix, c):
            if bn:
                out.extend([(prefix + s, (c,)) for s in (".weight", ".bias", ".running_mean", ".running_var")])

        for i, (cin, s) in enumerate(self.blocks()):
            p = f"layers.resnet.{3 + i}"
            cout = cin * s
            conv(p + ".layers.0", cin, cout, 3)
            norm(p + ".layers.1", cout)
            conv(p + ".layers.3", cout, cout, 3)
            norm(p + ".layers.4", cout)
            if s != 1:
                conv(p + ".shortcut.0", cin, cout, 1)
                norm(p + ".shortcut.1", cout)
        F = 512 * 2 * 2
        out += [("layers.mean.weight", (self.size_latent, F)), ("layers.mean.bias", (self.size_latent,)),
                ("layers.logvar.weight", (self.size_latent, F)), ("layers.logvar.bias", (self.size_latent,))]
        return out

    def n_flops(self) -> int:
        """Algorithmic FLOPs of one encode (2 x MAC of every conv / linear, mean head only)."""
        (h0, w0), (hp, wp), *blk = self.maps()
        mac = h0 * w0 * 64 * 49 * self.nb_chan
        h, w = hp, wp
        for (cin, s), (ho, wo) in zip(self.blocks(), blk):
            cout = cin * s
            mac += ho * wo * cout * 9 * cin + ho * wo * cout * 9 * cout
            if s != 1:
                mac += ho * wo * cout * cin
            h, w = ho, wo
        mac += 2048 * self.size_latent
        return 2 * mac


DEFAULT_ENCODER = EncoderSpec()


def synthetic_encoder(spec: EncoderSpec = DEFAULT_ENCODER, seed: int = 0) -> Dict[str, np.ndarray]:
    """Deterministic encoder parameters (stream t = position in ``param_shapes``).

    Conv weights He-uniform U(+-sqrt(6/fan_in)) so activations stay O(1) through the ReLU stack, biases
    U(+-1/sqrt(fan_in)) (torch's default bias init), BatchNorm gamma U(0.5,1.5), beta U(-0.2,0.2),
    running_mean U(-0.2,0.2), running_var U(0.5,1.5) so the folding is exercised, linear weights
    U(+-1/sqrt(fan_in)).  Values are rounded once from double to fp32.
    """
    out = {}
    for t, (name, shape) in enumerate(spec.param_shapes()):
        n = int(np.prod(shape))
        u = prng_uniform(seed + 1000, t, n)
        kind = name.rsplit(".", 1)[1]
        is_bn = ("layers.resnet." in name and len(shape) == 1 and not name.endswith(".0.bias")
                 and spec.batchnorm)
        if is_bn:
            lo, hi = {"weight": (0.5, 1.5), "bias": (-0.2, 0.2), "running_mean": (-0.2, 0.2),
                      "running_var": (0.5, 1.5)}[kind]
            v = lo + (hi - lo) * u
        elif len(shape) == 4:
            fan_in = int(np.prod(shape[1:]))
            v = (2.0 * u - 1.0) * np.sqrt(6.0 / fan_in)
        else:  # linear weight / any bias
            fan_in = shape[1] if len(shape) == 2 else _fan_in_of_bias(spec, name)
            v = (2.0 * u - 1.0) / np.sqrt(fan_in)
        out[name] = v.astype(np.float32).reshape(shape)
    return out


def _fan_in_of_bias(spec, name):
    shapes = dict(spec.param_shapes())
    w = shapes[name[: -len("bias")] + "weight"]
    return int(np.prod(w[1:]))


# ---------------------------------------------------------------------------------------------
# folding + packing: the device layout
# ---------------------------------------------------------------------------------------------
def _fold(params, conv, norm, bn):
    """(w [Cout][KH][KW][Cin] fp32, b [Cout] fp32) of conv (+ BatchNorm), folded in fp64."""
    w = params[conv + ".weight"].astype(np.float64)
    b = params[conv + ".bias"].astype(np.float64) if (conv + ".bias") in params else np.zeros(w.shape[0])
    if bn:
        g, beta = params[norm + ".weight"].astype(np.float64), params[norm + ".bias"].astype(np.float64)
        m, v = params[norm + ".running_mean"].astype(np.float64), params[norm + ".running_var"].astype(np.float64)
        sc = g / np.sqrt(v + BN_EPS)
        w = w * sc[:, None, None, None]
        b = (b - m) * sc + beta
    return (np.ascontiguousarray(w.transpose(0, 2, 3, 1)).astype(np.float32), b.astype(np.float32))


def device_layers(spec: EncoderSpec, params: Dict[str, np.ndarray]):
    """The packed conv list in launch order: stem, then per block (conv_a, [shortcut], conv_b), head.

    Each entry is (name, w, b); w is [Cout][KH][KW][Cin] (K contiguous per output channel, the GEMM's
    B-operand layout), the head is the mean Linear as a [L][2048] matrix.
    """
    bn = spec.batchnorm
    layers = [("stem",) + _fold(params, "layers.resnet.0", None, False)]
    for i, (cin, s) in enumerate(spec.blocks()):
        p = f"layers.resnet.{3 + i}"
        layers.append((f"b{i}a",) + _fold(params, p + ".layers.0", p + ".layers.1", bn))
        if s != 1:
            layers.append((f"b{i}s",) + _fold(params, p + ".shortcut.0", p + ".shortcut.1", bn))
        layers.append((f"b{i}b",) + _fold(params, p + ".layers.3", p + ".layers.4", bn))
    layers.append(("head", params["layers.mean.weight"].astype(np.float32),
                   params["layers.mean.bias"].astype(np.float32)))
    return layers


def pack(spec: EncoderSpec, params: Dict[str, np.ndarray]) -> bytes:
    """Serialise to the `.vaew` layout read by ``sdfnmpc_vae_load`` (include/sdfnmpc.h)."""
    if spec.nb_chan != 1 or tuple(spec.widths) != (64, 128, 256, 512):
        raise ValueError("only the reference encoder (1 channel, widths 64..512) is built")
    body = []
    for _, w, b in device_layers(spec, params):
        body += [np.ascontiguousarray(w, dtype="<f4").tobytes(), np.ascontiguousarray(b, dtype="<f4").tobytes()]
    blob = b"".join(body)
    hdr = _HDR.pack(MAGIC, VERSION, spec.nb_chan, spec.size_latent, spec.shape[0], spec.shape[1],
                    len(body) // 2, len(blob) // 4, 0)
    return hdr + blob


def save(path: str, spec: EncoderSpec, params: Dict[str, np.ndarray]) -> None:
    with open(path, "wb") as f:
        f.write(pack(spec, params))


def from_state_dict(sd, spec: EncoderSpec = None) -> Tuple[EncoderSpec, Dict[str, np.ndarray]]:
    """An ``Encoder`` (or whole ``Vae``: keys under ``encoder.``) state_dict -> (spec, params)."""
    sd = {k: (v.detach().cpu().numpy() if hasattr(v, "detach") else np.asarray(v)) for k, v in sd.items()}
    if any(k.startswith("encoder.") for k in sd):
        sd = {k[len("encoder."):]: v for k, v in sd.items() if k.startswith("encoder.")}
    L = sd["layers.mean.weight"].shape[0]
    bn = "layers.resnet.3.layers.1.running_mean" in sd
    spec = spec or EncoderSpec(size_latent=L, batchnorm=bn)
    params = {}
    for name, shape in spec.param_shapes():
        a = np.asarray(sd[name], dtype=np.float32)
        if a.shape != shape:
            raise ValueError(f"{name}: shape {a.shape} != {shape}")
        params[name] = a
    return spec, params


def from_torchscript(path: str, shape=(270, 480)) -> Tuple[EncoderSpec, Dict[str, np.ndarray]]:
    """Convert a VAE TorchScript archive of YOUR OWN (what ``sdf_nmpc/vae.py:11`` loads) offline."""
    import torch  # offline only

    m = torch.jit.load(path, map_location="cpu")
    sd = m.state_dict()
    spec, params = from_state_dict(sd)
    return dataclasses.replace(spec, shape=tuple(shape)), params


# ---------------------------------------------------------------------------------------------
# decoder (network/vae.py:63-90, resnet.py:59-111): spec, synthetic weights, folding, the `.vaed` blob
# ---------------------------------------------------------------------------------------------
MAGIC_DEC = b"SDFNVAED"
VERSION_DEC = 1
_HDR_DEC = struct.Struct("<8s4I")  # magic, version, size_latent, batchnorm, n_floats
DEC_MAP = (512, 8, 15)              # Unflatten(1, (512, 8, 15)) (vae.py:77)
DEC_BLOCKS = (512, 256, 128, 64)    # ResBlockDeconv inputs (vae.py:79-82), each stride 2, output_padding 1
DEC_LOGITS = (128, 240)             # the map before the Upsample


@dataclasses.dataclass(frozen=True)
class DecoderSpec:
    """``Decoder(nb_chan, size_latent, shape_imgs, batchnorm)`` (vae.py:65); ``shape`` is the Upsample's size."""
    nb_chan: int = 1
    size_latent: int = 128
    shape: Tuple[int, int] = (270, 480)
    batchnorm: bool = True

    def param_kinds(self) -> List[Tuple[str, Tuple[int, ...], str]]:
        """``Decoder.state_dict()`` names, shapes and what each is ('linear', 'deconv', 'bias', 'bn'), in order
        (num_batches_tracked omitted).  The shortcut's BatchNorm is there even without ``batchnorm``
        (resnet.py:98-101); the convolutions then carry biases as well."""
        bn = self.batchnorm
        F = int(np.prod(DEC_MAP))
        out = [("layers.resnet.0.weight", (F, self.size_latent), "linear"), ("layers.resnet.0.bias", (F,), "bias")]

        def deconv(prefix, cin, cout, k):
            out.append((prefix + ".weight", (cin, cout, k, k), "deconv"))
            if not bn:
                out.append((prefix + ".bias", (cout,), "bias"))

        def norm(prefix, c):
            out.extend([(prefix + s, (c,), "bn") for s in (".weight", ".bias", ".running_mean", ".running_var")])

        for i, cin in enumerate(DEC_BLOCKS):
            p, cout = f"layers.resnet.{4 + i}", cin // 2
            deconv(p + ".layers.0", cin, cout, 3)
            if bn:
                norm(p + ".layers.1", cout)
            deconv(p + ".layers.3", cout, cout, 3)
            if bn:
                norm(p + ".layers.4", cout)
            deconv(p + ".shortcut.0", cin, cout, 1)
            norm(p + ".shortcut.1", cout)
        out += [("layers.resnet.8.weight", (DEC_BLOCKS[-1] // 2, self.nb_chan, 5, 5), "deconv"),
                ("layers.resnet.8.bias", (self.nb_chan,), "bias")]
        return out

    def param_shapes(self) -> List[Tuple[str, Tuple[int, ...]]]:
        return [(n, s) for n, s, _ in self.param_kinds()]

    def n_flops(self) -> int:
        """Algorithmic FLOPs of one decode (2 x MAC of the linear layer and every transposed convolution)."""
        c, h, w = DEC_MAP
        mac = c * h * w * self.size_latent
        for cin in DEC_BLOCKS:
            cout = cin // 2
            mac += h * w * cin * cout * 9 + h * w * cin * cout  # every input pixel meets each tap once
            h, w = 2 * h, 2 * w
            mac += h * w * cout * cout * 9
        mac += h * w * (DEC_BLOCKS[-1] // 2) * 25 * self.nb_chan
        return 2 * mac


DEFAULT_DECODER = DecoderSpec()


def synthetic_decoder(spec: DecoderSpec = DEFAULT_DECODER, seed: int = 0) -> Dict[str, np.ndarray]:
    """Deterministic decoder parameters, the scheme of ``synthetic_encoder`` on a stream base of its own (stream
    t = position in ``param_shapes``): transposed-convolution weights [Cin][Cout][k][k] U(+-sqrt(6 / (Cin k k))),
    the linear weight and every bias U(+-1/sqrt(fan_in)), BatchNorm gamma U(0.5,1.5), beta U(-0.2,0.2),
    running_mean U(-0.2,0.2), running_var U(0.5,1.5).  Values are rounded once from double to fp32."""
    kinds = spec.param_kinds()
    shapes = {n: s for n, s, _ in kinds}
    out = {}
    for t, (name, shape, kind) in enumerate(kinds):
        u = prng_uniform(seed + 2000, t, int(np.prod(shape)))
        if kind == "bn":
            lo, hi = {"weight": (0.5, 1.5), "bias": (-0.2, 0.2), "running_mean": (-0.2, 0.2),
                      "running_var": (0.5, 1.5)}[name.rsplit(".", 1)[1]]
            v = lo + (hi - lo) * u
        elif kind == "deconv":
            v = (2.0 * u - 1.0) * np.sqrt(6.0 / (shape[0] * shape[2] * shape[3]))
        else:  # the linear weight, any bias
            w = shapes[name[: -len("bias")] + "weight"] if kind == "bias" else shape
            fan_in = w[1] if len(w) == 2 else w[0] * w[2] * w[3]
            v = (2.0 * u - 1.0) / np.sqrt(fan_in)
        out[name] = v.astype(np.float32).reshape(shape)
    return out


def _fold_deconv(params, conv, norm):
    """(w [k][k][Cin][Cout] fp64, b [Cout] fp64) of a transposed convolution (+ BatchNorm when its statistics are in
    ``params``): the scale applies to the OUTPUT-channel axis of the transposed weight [Cin][Cout][k][k]."""
    w = params[conv + ".weight"].astype(np.float64)
    b = params[conv + ".bias"].astype(np.float64) if (conv + ".bias") in params else np.zeros(w.shape[1])
    if norm is not None and (norm + ".running_mean") in params:
        g, beta = params[norm + ".weight"].astype(np.float64), params[norm + ".bias"].astype(np.float64)
        m, v = params[norm + ".running_mean"].astype(np.float64), params[norm + ".running_var"].astype(np.float64)
        sc = g / np.sqrt(v + BN_EPS)
        w = w * sc[None, :, None, None]
        b = (b - m) * sc + beta
    return np.ascontiguousarray(w.transpose(2, 3, 0, 1)), b


def decoder_layers(spec: DecoderSpec, params: Dict[str, np.ndarray], dtype=np.float32):
    """The folded layer list in launch order, (name, w, b) each: ``head`` (w [L][F], b [F], the features in the
    map's NHWC order (y, x, c)), per block ``d{i}a`` (stride-2 3x3), ``d{i}s`` (shortcut), ``d{i}b`` (stride-1 3x3)
    with w [k][k][Cin][Cout] in the transposed convolution's own tap indices, and ``tail`` (w [5][5][32], b [1]).
    Folded in fp64 and rounded once to ``dtype``."""
    c, h, w_ = DEC_MAP
    L = spec.size_latent
    hw = params["layers.resnet.0.weight"].astype(np.float64).reshape(c, h, w_, L).transpose(1, 2, 0, 3).reshape(-1, L)
    hb = params["layers.resnet.0.bias"].astype(np.float64).reshape(c, h, w_).transpose(1, 2, 0).reshape(-1)
    layers = [("head", np.ascontiguousarray(hw.T), hb)]
    for i in range(len(DEC_BLOCKS)):
        p = f"layers.resnet.{4 + i}"
        layers.append((f"d{i}a",) + _fold_deconv(params, p + ".layers.0", p + ".layers.1"))
        layers.append((f"d{i}s",) + _fold_deconv(params, p + ".shortcut.0", p + ".shortcut.1"))
        layers.append((f"d{i}b",) + _fold_deconv(params, p + ".layers.3", p + ".layers.4"))
    tw, tb = _fold_deconv(params, "layers.resnet.8", None)
    layers.append(("tail", np.ascontiguousarray(tw[:, :, :, 0]), tb))
    return [(n, w.astype(dtype), b.astype(dtype)) for n, w, b in layers]


def pack_decoder(spec: DecoderSpec, params: Dict[str, np.ndarray]) -> bytes:
    """Serialise to the `.vaed` layout read by ``sdfnmpc_vae_dec_load`` (include/sdfnmpc.h)."""
    if spec.nb_chan != 1:
        raise ValueError("only the reference decoder (1 channel) is built")
    for name, shape in spec.param_shapes():
        if name not in params or tuple(params[name].shape) != tuple(shape):
            raise ValueError(f"{name}: expected shape {shape}")
    body = []
    for _, w, b in decoder_layers(spec, params):
        body += [np.ascontiguousarray(w, dtype="<f4").tobytes(), np.ascontiguousarray(b, dtype="<f4").tobytes()]
    blob = b"".join(body)
    return _HDR_DEC.pack(MAGIC_DEC, VERSION_DEC, spec.size_latent, int(spec.batchnorm), len(blob) // 4) + blob


def unpack_decoder(blob: bytes):
    """(size_latent, batchnorm, [(name, w, b)]) of a `.vaed` blob: the inverse of ``pack_decoder``'s layout."""
    if len(blob) < _HDR_DEC.size:
        raise ValueError("vaed: truncated header")
    magic, ver, L, bn, n = _HDR_DEC.unpack_from(blob)
    if magic != MAGIC_DEC or ver != VERSION_DEC:
        raise ValueError("not a version-1 .vaed blob")
    if len(blob) != _HDR_DEC.size + 4 * n:
        raise ValueError("vaed: size mismatch")
    a = np.frombuffer(blob, "<f4", offset=_HDR_DEC.size)
    F = int(np.prod(DEC_MAP))
    shapes = [("head", (L, F), F)]
    for i, cin in enumerate(DEC_BLOCKS):
        co = cin // 2
        shapes += [(f"d{i}a", (3, 3, cin, co), co), (f"d{i}s", (1, 1, cin, co), co), (f"d{i}b", (3, 3, co, co), co)]
    shapes.append(("tail", (5, 5, DEC_BLOCKS[-1] // 2), 1))
    if sum(int(np.prod(s)) + nb for _, s, nb in shapes) != n:
        raise ValueError("vaed: parameter count does not match the reference decoder")
    out, off = [], 0
    for name, s, nb in shapes:
        k = int(np.prod(s))
        out.append((name, a[off:off + k].reshape(s), a[off + k:off + k + nb]))
        off += k + nb
    return L, bool(bn), out


def decoder_from_state_dict(sd, spec: DecoderSpec = None) -> Tuple[DecoderSpec, Dict[str, np.ndarray]]:
    """A ``Decoder`` (or whole ``Vae``: keys under ``decoder.``) state_dict -> (spec, params)."""
    sd = {k: (v.detach().cpu().numpy() if hasattr(v, "detach") else np.asarray(v)) for k, v in sd.items()}
    if any(k.startswith("decoder.") for k in sd):
        sd = {k[len("decoder."):]: v for k, v in sd.items() if k.startswith("decoder.")}
    if "layers.resnet.0.weight" not in sd or np.ndim(sd["layers.resnet.0.weight"]) != 2:
        raise ValueError("no decoder in this state_dict (layers.resnet.0.weight [F, L] is missing)")
    L = sd["layers.resnet.0.weight"].shape[1]
    bn = "layers.resnet.4.layers.1.running_mean" in sd
    spec = spec or DecoderSpec(size_latent=L, batchnorm=bn)
    params = {}
    for name, shape in spec.param_shapes():
        if name not in sd:
            raise ValueError(f"{name}: missing")
        a = np.asarray(sd[name], dtype=np.float32)
        if a.shape != shape:
            raise ValueError(f"{name}: shape {a.shape} != {shape}")
        params[name] = a
    return spec, params


def decoder_from_torchscript(path: str, shape=(270, 480)) -> Tuple[DecoderSpec, Dict[str, np.ndarray]]:
    """The decoder of a VAE TorchScript archive of YOUR OWN (what ``sdf_nmpc/vae.py:11`` loads), offline."""
    import torch  # offline only

    m = torch.jit.load(path, map_location="cpu")
    spec, params = decoder_from_state_dict(m.state_dict())
    return dataclasses.replace(spec, shape=tuple(shape)), params


# ---------------------------------------------------------------------------------------------
# preprocessing constants (utils/preprocessing.py)
# ---------------------------------------------------------------------------------------------
def depth2range_table(shape, hfov, vfov) -> np.ndarray:
    """``Depth2Range.yz_sqrt`` (preprocessing.py:16-27) in fp32 with correctly rounded operations.

    torch's scalar ``tan`` is correctly rounded (numpy's fp32 ``tan`` is not, so it is taken in fp64 and
    rounded once); torch's vectorised fp32 ``sqrt`` is within 1 ulp of the correctly rounded one used here
    (tests/test_vae.py pins the table and the preprocessed pixels to the golden file at that bar).
    """
    H, W = int(shape[-2]), int(shape[-1])
    u, v = np.meshgrid(np.arange(W, dtype=np.float32), np.arange(H, dtype=np.float32), indexing="xy")
    th = np.float32(np.tan(np.float64(np.float32(hfov))))
    tv = np.float32(np.tan(np.float64(np.float32(vfov))))
    a = th * (np.float32(1) - np.float32(2) * u / np.float32(W))
    b = tv * (np.float32(1) - np.float32(2) * v / np.float32(H))
    return np.sqrt(np.float32(1) + a * a + b * b).astype(np.float32)


def clip_scale(cfg) -> float:
    """``ClipDistance.dmax`` (preprocessing.py:91): dmax / mm_resolution * 1000."""
    return cfg.sensor.dmax / cfg.sensor.mm_resolution * 1000


class VaeWrapper:
    """Mirror of the reference's ``VaeWrapper`` (sdf_nmpc/vae.py:7-50) over a batch of B images.

    ``set_img(img)`` takes one raw image [H, W] (B = 1, as the reference) or a batch [B, H, W] (numpy
    float32 / uint16, or a device array -- ``_lib.DeviceArray`` or a torch tensor, used in place);
    ``encode()`` runs preprocessing + the encoder on the GPU and returns the latent means [L] / [B, L] as
    numpy.  ``encode_to(nmpc)`` writes them straight into an ``Nmpc``'s device parameters (set_latent on
    the device, no host round trip).  No tensor library is needed.

    ``decoder``: None (nothing is allocated; ``decode`` raises ValueError), True (synthetic weights from the
    seed), ``(DecoderSpec, params)`` or the path of a TorchScript VAE.  ``decode(shape=None)`` is the reference's
    method: the image of ``self.latent`` -- after ``encode()`` the latent on the device, no host round trip -- as
    numpy [H, W] (B = 1) or [B, H, W], by default at ``cfg.sensor.shape_imgs[-2:]``: a normalised RANGE image in
    [0, 1] whatever ``sensor.is_depth`` says.  ``decode_to(dev_img)`` decodes into a device array [B, H, W] float32
    without a download; ``reconstruct(imgs)`` is ``set_img``, encode, decode on the device.
    """

    def __init__(self, cfg, weights=None, batch: int = 1, device: int = 0, ctx=None, seed: int = 0, decoder=None):
        from . import _lib

        self.cfg = cfg
        self.B = int(batch)
        self._own_ctx = ctx is None
        self.ctx = ctx if ctx is not None else _lib.Context(device)
        spec = EncoderSpec(size_latent=int(cfg.nn.size_latent), shape=tuple(cfg.sensor.shape_imgs[-2:]))
        if weights is None:
            weights = cfg.nn.get("vae_weights")
            seed = int(cfg.nn.get("vae_seed", seed))
        if weights is None:
            params = synthetic_encoder(spec, seed)
        elif isinstance(weights, str):
            spec, params = from_torchscript(weights, spec.shape)
        else:
            spec, params = weights
        self.spec = spec
        self.vae = _lib.Vae(self.ctx, pack(spec, params), self.B)
        yz = depth2range_table(spec.shape, cfg.sensor.hfov, cfg.sensor.vfov)
        self.yz = _lib.DeviceArray.from_numpy(self.ctx, yz)
        self.opts = _lib.vae_opts(cfg, clip_scale(cfg) if not cfg.sensor.get("is_normalized", False) else 1.0)
        self.depth2range = bool(cfg.sensor.get("is_depth", True))
        self.img = None
        self.latent = _lib.DeviceArray.from_numpy(self.ctx, np.zeros((self.B, spec.size_latent), np.float32))
        self.latent64 = _lib.DeviceArray.from_numpy(self.ctx, np.zeros((self.B, spec.size_latent), np.float64))
        self.dec = self.dec_spec = None
        if decoder is not None and decoder is not False:
            if decoder is True:
                dspec = DecoderSpec(size_latent=spec.size_latent, shape=spec.shape)
                dparams = synthetic_decoder(dspec, seed)
            elif isinstance(decoder, str):
                dspec, dparams = decoder_from_torchscript(decoder, spec.shape)
            else:
                dspec, dparams = decoder
            if dspec.size_latent != spec.size_latent:
                raise ValueError(f"the decoder's latent size {dspec.size_latent} is not the encoder's {spec.size_latent}")
            self.dec_spec = dspec
            self.dec = _lib.VaeDec(self.ctx, pack_decoder(dspec, dparams))
        self._dec_out = {}

    def set_img(self, img):
        from . import _lib

        if hasattr(img, "data_ptr"):  # already on the device: [B][H][W] float32 / uint16, used in place
            if tuple(img.shape)[0] != self.B or len(img.shape) != 3:
                raise ValueError(f"expected a device array [{self.B}, H, W], got {tuple(img.shape)}")
            self.img = _lib.sync_producer(img)  # a torch tensor may still be in flight on torch's stream
            return
        a = np.asarray(img)
        if a.dtype != np.uint16:
            a = a.astype(np.float32)
        if a.ndim == 2:
            a = a[None]
        if a.shape[0] != self.B:
            raise ValueError(f"expected {self.B} images, got {a.shape[0]}")
        if self.img is None or not isinstance(self.img, _lib.DeviceArray) or self.img.shape != a.shape or \
                self.img.dtype != a.dtype:
            self.img = _lib.DeviceArray(self.ctx, a.shape, a.dtype)
        self.img.upload(a)

    def set_latent(self, latent):
        self.latent.upload(np.reshape(np.asarray(latent, dtype=np.float32), (self.B, -1)))

    def encode(self):
        self._run()
        out = self.latent.numpy()
        return out[0] if self.B == 1 else out

    def _run(self):
        if self.img is None:
            raise ValueError("set_img before encode")
        from . import _lib
        _lib.vae_encode(self.ctx, self.vae, self.opts, self.img, self.yz, self.latent, self.latent64,
                        depth2range=self.depth2range)

    def _need_decoder(self):
        if self.dec is None:
            raise ValueError("this VaeWrapper has no decoder (VaeWrapper(..., decoder=True | (spec, params) | path))")

    def decode_to(self, dev_img, logits=None):
        """Decode ``self.latent`` into dev_img, a device array [B, H, W] float32 (the output size is its own); no
        download.  logits: optional device [B, 128, 240] float32, the map before the resize and the sigmoid."""
        from . import _lib

        self._need_decoder()
        shape = tuple(int(v) for v in dev_img.shape)
        if len(shape) != 3 or shape[0] != self.B or np.dtype(str(dev_img.dtype).replace("torch.", "")) != np.float32:
            raise ValueError(f"expected a device array [{self.B}, H, W] float32, got {shape} {dev_img.dtype}")
        _lib.vae_decode(self.ctx, self.dec, self.latent, dev_img, logits)
        return dev_img

    def decode(self, shape=None):
        """The reference's ``decode`` (sdf_nmpc/vae.py:42-45): the reconstruction of ``self.latent`` as numpy."""
        from . import _lib

        self._need_decoder()
        h, w = (int(v) for v in (shape if shape is not None else self.cfg.sensor.shape_imgs[-2:]))
        out = self._dec_out.get((h, w))
        if out is None:  # one device output is kept: the last size asked for
            for old in self._dec_out.values():
                old.close()
            self._dec_out = {(h, w): _lib.DeviceArray(self.ctx, (self.B, h, w), np.float32)}
            out = self._dec_out[(h, w)]
        img = self.decode_to(out).numpy()
        return img[0] if self.B == 1 else img

    def reconstruct(self, imgs, normalized=None, out=None):
        """``set_img(imgs)``, encode, decode on the device: the image the latent retains, a device array [B, H, W]
        float32 of the input's own size (``out``, or a new one).  normalized: True for images already divided by
        sensor.dmax (clip = 1), False for raw sensor images (clip = dmax / mm_resolution * 1000), None as the
        config says (sensor.is_normalized)."""
        from . import _lib

        self._need_decoder()
        self.set_img(imgs)
        shape = tuple(int(v) for v in self.img.shape)
        if out is None:
            out = _lib.DeviceArray(self.ctx, shape, np.float32)
        elif tuple(int(v) for v in out.shape) != shape:
            raise ValueError(f"out {tuple(out.shape)} is not the images' {shape}")
        clip = self.opts.clip
        if normalized is not None:
            self.opts.clip = 1.0 if normalized else float(clip_scale(self.cfg))
        try:
            self._run()
        finally:
            self.opts.clip = clip
        return self.decode_to(out)

    def close(self):
        """Free the encoder, the decoder and the decode output on the device (idempotent; the wrapper's context, when
        it made one, goes with the wrapper)."""
        for old in self._dec_out.values():
            old.close()
        self._dec_out = {}
        self.vae.close()
        if self.dec is not None:
            self.dec.close()

    def encode_to(self, nmpc, W_p_Bo, W_R_Bo, flag=None):
        """encode + ``nmpc.set_latent_device`` with the fp64 latents (no host round trip).  The encoder and
        the controller's parts may use other streams: set_latent_device drains the encoder's stream before
        any part on another context reads latent64 in place (controller._producer_done)."""
        self._run()
        nmpc.set_latent_device(self.latent64, W_p_Bo, W_R_Bo, flag)
