"""Time the VAE decoder (csrc/vae_dec.hip) at batch B beside the encoder of the same run: ms per 512 images between
HIP events, TFLOP/s, and the per-kernel split (``vae_dec*`` of sdfnmpc_ctx_kernel_stats, from a second, timed pass).

    python tools/vae_dec_bench.py [B=512] [out_h=270] [out_w=480]
"""
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from sdf_nmpc_amd import _lib, synth  # noqa: E402
from sdf_nmpc_amd import vae as V  # noqa: E402
from sdf_nmpc_amd.config import Config  # noqa: E402

DEC_KERNELS = ["vae_dec_head"] + [f"vae_dec_{k}{c}" for c in (256, 128, 64, 32) for k in ("up", "sc", "conv")] + \
    ["vae_dec_tail", "vae_dec_resize"]


def _events(fn, steps):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(steps):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / steps


def main(B=512, out_h=270, out_w=480, steps=5):
    if os.environ.get("SDFNMPC_LIB"):  # a diagnostic build (tools/build_variant.sh)
        _lib.LIB_PATH = os.environ["SDFNMPC_LIB"]
    cfg = Config()
    ctx = _lib.Context(0, stream=torch.cuda.current_stream().cuda_stream)
    es, ds = V.DEFAULT_ENCODER, V.DEFAULT_DECODER
    enc = _lib.Vae(ctx, V.pack(es, V.synthetic_encoder(es, 0)))
    dec = _lib.VaeDec(ctx, V.pack_decoder(ds, V.synthetic_decoder(ds, 0)))
    imgs = torch.from_numpy(synth.depth_images(8, 270, 480, seed=1)).cuda().repeat((B + 7) // 8, 1, 1)[:B].contiguous()
    yz = torch.from_numpy(V.depth2range_table((270, 480), cfg.sensor.hfov, cfg.sensor.vfov)).cuda()
    lat = torch.empty(B, 128, device="cuda")
    out = torch.empty(B, out_h, out_w, device="cuda")
    opts = _lib.vae_opts(cfg, 5.0)
    encode = lambda: _lib.vae_encode(ctx, enc, opts, imgs, yz, lat)  # noqa: E731
    decode = lambda: _lib.vae_decode(ctx, dec, lat, out)             # noqa: E731
    for _ in range(2):
        encode()
        decode()
    torch.cuda.synchronize()
    t_enc, t_dec = _events(encode, steps), _events(decode, steps)
    img = out.cpu().numpy()
    assert np.isfinite(img).all() and img.min() >= 0 and img.max() <= 1
    s = 512.0 / B
    print(f"B={B}, output {out_h} x {out_w} (HIP events, {steps} calls each)")
    print(f"  encode {t_enc:8.3f} ms = {t_enc * s:8.3f} ms per 512 images  {es.n_flops() * B / t_enc / 1e9:7.1f} TFLOP/s")
    print(f"  decode {t_dec:8.3f} ms = {t_dec * s:8.3f} ms per 512 images  {ds.n_flops() * B / t_dec / 1e9:7.1f} TFLOP/s"
          f"   decode / encode = {t_dec / t_enc:.2f} (FLOPs: {ds.n_flops() / es.n_flops():.2f})")
    ctx.enable_timing(True)
    ctx.reset_stats()
    for _ in range(steps):
        decode()
    torch.cuda.synchronize()
    total = 0.0
    for k in DEC_KERNELS:
        ms, n = ctx.kernel_stats(k)
        total += ms / steps
        print(f"  {k:16s} {ms / steps * s:8.3f} ms per 512 images ({n // steps} launches a decode)")
    print(f"  {'sum':16s} {total * s:8.3f} ms per 512 images")
    ctx.enable_timing(False)


if __name__ == "__main__":
    main(*[int(v) for v in sys.argv[1:4]])
