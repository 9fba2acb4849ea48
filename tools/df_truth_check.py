#!/usr/bin/env python3
"""Score a NeuralDF against the geometry its latent was conditioned on (the reference's
scripts/neural_nets/df_test.py): sample points in the frustum of a batch of images, compute the distance field
the images themselves imply (sdf_nmpc_amd.df_computer.DfComputer, HIP kernels) and the network's prediction
(Net.eval_host), and print mean and max |df - truth| and the share of sign disagreements.

  images   --images imgs.npy ([B, H, W] raw metres) or synth.depth_images(--batch, seed --seed)
  latents  --vae-weights enc.pt runs the VAE encoder on the images; otherwise --latent lat.npy ([B, L])
  network  --sdf-weights net.sdfw, or the SIREN initialisation of --net-seed

Exit codes: 0 done (the figures are a report, not a verdict), 1 a runtime failure, 2 bad arguments, 124 the
time limit (--time-limit seconds, default 120) ran out.
"""
import argparse
import os
import signal
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def frustum_points(n_img, per_img, dmax, hfov, vfov, rng):
    """Uniform in depth and in the tangent plane, inside the field of view (camera frame, x forward)."""
    x = rng.uniform(0.05 * dmax, dmax, (n_img, per_img))
    y = x * np.tan(hfov) * rng.uniform(-1, 1, x.shape)
    z = x * np.tan(vfov) * rng.uniform(-1, 1, x.shape)
    return np.stack([x, y, z], -1).reshape(-1, 3).astype(np.float32)


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--images")
    ap.add_argument("--batch", type=int, default=2)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--vae-weights")
    ap.add_argument("--latent")
    ap.add_argument("--sdf-weights")
    ap.add_argument("--net-seed", type=int, default=0)
    ap.add_argument("--points", type=int, default=1500, help="points per image (df_test.py's batch)")
    ap.add_argument("--unsigned", action="store_true", help="compare against the unsigned field")
    ap.add_argument("--device", type=int, default=0)
    ap.add_argument("--time-limit", type=int, default=120)
    args = ap.parse_args(argv)  # exits 2 on bad arguments
    if not args.vae_weights and not args.latent:
        ap.error("give --vae-weights (the encoder is run) or --latent (one row per image)")
    if args.points < 1 or args.batch < 1:
        ap.error("--points and --batch must be positive")

    def on_alarm(*_):
        print("df_truth_check: time limit reached", file=sys.stderr)
        os._exit(124)
    signal.signal(signal.SIGALRM, on_alarm)
    signal.alarm(max(1, args.time_limit))

    import torch  # noqa: F401 -- before the library is loaded, so that both use the HIP runtime torch brings
    from sdf_nmpc_amd import _lib, synth
    from sdf_nmpc_amd.config import Config
    from sdf_nmpc_amd.df_computer import DfComputer
    from sdf_nmpc_amd.vae import VaeWrapper

    cfg = Config()
    s = cfg.sensor
    raw = np.load(args.images).astype(np.float32) if args.images else synth.depth_images(
        args.batch, *s.shape_imgs[-2:], seed=args.seed)
    if raw.ndim == 2:
        raw = raw[None]
    if raw.ndim != 3:
        ap.error("--images must hold [B, H, W] or [H, W]")
    B = raw.shape[0]
    ctx = _lib.Context(args.device)
    if args.vae_weights:
        vae = VaeWrapper(cfg, weights=args.vae_weights, batch=B, ctx=ctx)
        vae.set_img(raw)
        latent = np.reshape(vae.encode(), (B, -1)).astype(np.float64)
    else:
        latent = np.load(args.latent).astype(np.float64).reshape(-1, int(cfg.nn.size_latent))
        if latent.shape[0] != B:
            ap.error(f"--latent holds {latent.shape[0]} rows for {B} images")
    net = _lib.Net.from_file(ctx, args.sdf_weights) if args.sdf_weights else _lib.Net.siren(ctx, args.net_seed)

    imgs = np.minimum(raw, np.float32(s.dmax)) / np.float32(s.dmax)  # normalised, as the classes expect
    pts = frustum_points(B, args.points, s.dmax, s.hfov, s.vfov, np.random.default_rng(args.seed))
    dfc = DfComputer(not args.unsigned, s.dmax, s.hfov, s.vfov, net.max_df, s.is_depth, s.is_spherical, device=ctx)
    truth, _ = dfc.get_df(imgs, pts)  # default ordering: args.points consecutive points per image
    truth = truth.cpu().numpy().astype(np.float64)
    inp = np.concatenate([pts.astype(np.float64), np.repeat(latent, args.points, axis=0)], axis=1)
    df, _ = net.eval_host(inp, want_grad=False)
    err = np.abs(df - truth)
    sign = np.mean((df < 0) != (truth < 0))
    print(f"images {B} x {raw.shape[1]}x{raw.shape[2]}, {args.points} points each, "
          f"{'unsigned' if args.unsigned else 'signed'} truth")
    print(f"mean |df - truth| = {err.mean():.6f}  max = {err.max():.6f}  sign disagreements = {sign:.4%}")
    signal.alarm(0)
    return 0


if __name__ == "__main__":
    try:
        sys.exit(main())
    except SystemExit:
        raise
    except Exception as e:  # noqa: BLE001 -- report and exit 1
        print(f"df_truth_check: {type(e).__name__}: {e}", file=sys.stderr)
        sys.exit(1)
