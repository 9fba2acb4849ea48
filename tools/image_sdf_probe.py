"""Network, labels or truth?  The forest rollout of tools/scene_sdf_probe.py flown on one controller configuration with
three sources of the SDF row: the network (the SIREN initialisation unless weights are given; a new image of the scene
before every step, encoded), the distance field of the camera image itself (Nmpc.set_sdf_image, csrc/df_truth.hip -- the
network's training target: signed and unsigned, with an exact camera and through a SensorModel), and the exact distance
of the scene (Nmpc.set_sdf_scene).  Every imaging arm re-images before every `--every`-th step.  Prints, per arm, ms per
control step (the arms alternate inside every repetition; best of --reps after a warm-up; the clearance launch after
the loop included) and the distribution of the minimum clearance over the batch; img_sdf_rows per launch inside a timed
rollout next to sdf_hoist + sdf_mlp; and img_sdf_rows alone from HIP events, 20 launches after 5, signed and unsigned,
at the iterate and image the rollout left, with the share of rows that scan the whole voxel grid (no voxel within 1 m
counts: h[2] = max_df with the flag on).

    timeout 900 python tools/image_sdf_probe.py --B 256 --N 40
    timeout 900 python tools/image_sdf_probe.py --B 1024 --N 40 --K 10 --reps 1
    timeout 900 python tools/image_sdf_probe.py --reconstruct --B 1024 --N 40 --K 10 --reps 1

--reconstruct flies the rung between the camera image and the network instead: the field of the image the VAE's latent
retains (Nmpc.set_sdf_image(..., reconstruct=vae), sdfnmpc_solver_rollout_image_recon), signed and unsigned, beside the
network, the camera image and the exact scene, and prints the reconstructing rollout's ms per step beside the
host-driven loop of the same pieces (render_from_state, set_sdf_image(reconstruct=), set_pose_device, gen_refs_device,
solve, plant_step) from the same run.  A clearance lost with the reconstruction is the bottleneck's; one lost only below
it is the NeuralDF's.  WITH SYNTHETIC VAE WEIGHTS THE RECONSTRUCTION IS NOISE in about [0.27, 0.77] dmax, so the
recon arms' clearance numbers mean nothing until a trained checkpoint is converted (vae.from_torchscript /
decoder_from_torchscript); the timings do not depend on the weights.
Prints a summary and a JSON line.  Diagnostic, not a test."""
import argparse
import json
import os
import sys
import time
import warnings

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
from sdf_nmpc_amd import _lib
from sdf_nmpc_amd.config import Config
from sdf_nmpc_amd.scene import Scene
from sdf_nmpc_amd.sensor import SensorModel
from sdf_nmpc_amd.vae import VaeWrapper
from perceive_probe import forest
from rollout_probe import controller

Q = (0, 5, 25, 50, 75, 95, 100)
ARMS = ("net", "img_signed", "img_unsigned", "img_signed_sensor", "img_unsigned_sensor", "exact")
RECON_ARMS = ("net", "img_signed", "recon_signed", "recon_unsigned", "exact")
KERNELS = ("sdf_hoist", "sdf_mlp", "img_sdf_rows", "scene_sdf_rows", "scene_render", "sensor", "minpool5", "linearize",
           "rti_qp_pack", "rti_qp")


def fly(cfg, a, arm, timed=False, keep=False):
    """One rollout of an arm on a fresh controller: (Rollout, ms per step, kernel stats of a timed run, rows probe)."""
    n, x0, wps = controller(cfg, a.B, 1)
    ctx = n.ocp.ctx
    scene = Scene(ctx, forest(16))
    shape = tuple(int(v) for v in a.shape)
    kw, vae = {}, None
    if arm == "net":
        vae = VaeWrapper(cfg, batch=a.B, ctx=ctx)
        kw = dict(scene=scene, vae=vae, perceive_every=a.every, img_shape=shape)
    elif arm == "exact":
        n.set_sdf_scene(scene)
    elif arm.startswith("recon"):
        vae = VaeWrapper(cfg, batch=a.B, ctx=ctx, decoder=True)
        n.set_sdf_image(scene.render_from_state(x0, cfg, shape, normalized=True), signed="unsigned" not in arm,
                        reconstruct=vae)
        kw = dict(scene=scene, perceive_every=a.every, img_shape=shape)
    else:
        n.set_sdf_image(scene.render_from_state(x0, cfg, shape, normalized=True), signed="unsigned" not in arm)
        kw = dict(scene=scene, perceive_every=a.every, img_shape=shape)
        if arm.endswith("sensor"):
            kw["sensor"] = SensorModel.reference_augment(cfg, ctx, 7)
    n.set_x0(x0)
    stats, rows = {}, {}
    if timed:
        ctx.reset_stats()
        ctx.enable_timing(True)
    ctx.synchronize()
    t0 = time.perf_counter()
    r = n.rollout(a.K, refs="wps", wps=wps, **kw)
    ms = (time.perf_counter() - t0) / a.K * 1e3
    if timed:
        for k in KERNELS:
            t, c = ctx.kernel_stats(k)
            stats[k] = (t / max(c, 1) * 1e3, c)
        ctx.enable_timing(False)
        ctx.reset_stats()
    if keep:  # img_sdf_rows alone, at the iterate, the parameters and the image the rollout left
        solver, src = n.ocp.parts[0].solver, n._sdf_image
        f = {k: solver.field(k) for k in ("x", "p", "h", "Jh")}
        fn = lambda: _lib.img_sdf_rows(ctx, src["opts"], a.B, a.N, n.model.np, f["x"], f["p"], f["h"], f["Jh"])
        for _ in range(5):
            fn()
        ctx.synchronize()
        ctx.reset_stats()
        ctx.enable_timing(True)
        for _ in range(20):
            fn()
        t, c = ctx.kernel_stats("img_sdf_rows")
        ctx.enable_timing(False)
        ctx.reset_stats()
        h2, flag = f["h"].numpy()[..., 2], f["p"].numpy()[..., 0]
        rows = {"us": t / c * 1e3, "full_scan_share": float((h2[flag != 0] == n.model.max_df).mean()),
                "rows": a.B * (a.N + 1)}
    if vae is not None:
        vae.vae.close()
        if vae.dec is not None:
            vae.dec.close()
    scene.close()
    n.ocp.close()
    return r, ms, stats, rows


def host_loop_recon(cfg, a, signed=True):
    """The loop a user writes around solve() with a reconstructing source, on a fresh controller: ms per step."""
    n, x0, wps = controller(cfg, a.B, 1)
    ctx = n.ocp.ctx
    scene = Scene(ctx, forest(16))
    shape = tuple(int(v) for v in a.shape)
    vae = VaeWrapper(cfg, batch=a.B, ctx=ctx, decoder=True)
    plant = _lib.plant_opts(cfg, dt=float(n.ocp.dt[0]))
    x = np.reshape(x0, (a.B, 10)).copy()
    dx = _lib.DeviceArray(ctx, (a.B, 10))
    ctx.synchronize()
    t0 = time.perf_counter()
    for k in range(a.K):
        n.set_x0(x if a.B > 1 else x[0])
        if k % a.every == 0:
            img = scene.render_from_state(x, cfg, shape, normalized=True)
            n.set_sdf_image(img, signed=signed, reconstruct=vae)
            n.set_pose_device(img.pose["W_p_Bo"], img.pose["W_R_Bo"])
        n.gen_refs_device("wps", wps=wps)
        n.solve()
        dx.upload(x)
        _lib.plant_step(ctx, plant, a.B, dx, n.ocp.field("u0"), dx)
        x = dx.numpy()
    ms = (time.perf_counter() - t0) / a.K * 1e3
    vae.vae.close()
    vae.dec.close()
    scene.close()
    n.ocp.close()
    return ms


def main_reconstruct(cfg, a):
    res = {"B": a.B, "N": a.N, "K": a.K, "every": a.every, "shape": list(a.shape), "reconstruct": True}
    ms = {k: [] for k in RECON_ARMS + ("recon_signed_host_loop",)}
    runs = {}
    for rep in range(a.reps + 1):  # repetition 0 warms up; the arms alternate inside every repetition
        for arm in RECON_ARMS:
            r, t, _, _ = fly(cfg, a, arm)
            runs[arm] = r
            if rep:
                ms[arm].append(t)
        t = host_loop_recon(cfg, a)
        if rep:
            ms["recon_signed_host_loop"].append(t)
    print(f"B={a.B} N={a.N} K={a.K} images {a.shape[0]} x {a.shape[1]}: ms per control step (best of {a.reps}), min clearance "
          f"over the batch at percentiles {Q}")
    for arm in RECON_ARMS:
        mc = runs[arm].clearance.min(axis=1)
        res[f"{arm}_ms_per_step"] = min(ms[arm])
        res[f"{arm}_min_clearance_percentiles"] = dict(zip(map(str, Q), np.percentile(mc, Q).round(4).tolist()))
        res[f"{arm}_collided"] = int((mc < 0).sum())
        print(f"  {arm:22s} {res[f'{arm}_ms_per_step']:.3f} ms/step  clearance "
              f"{list(res[f'{arm}_min_clearance_percentiles'].values())}  collided {res[f'{arm}_collided']}")
    res["recon_signed_host_loop_ms_per_step"] = min(ms["recon_signed_host_loop"])
    print(f"reconstructing rollout {res['recon_signed_ms_per_step']:.3f} ms/step against the host-driven loop of the same "
          f"pieces {res['recon_signed_host_loop_ms_per_step']:.3f} ms/step")
    print("NOTE: synthetic VAE weights reconstruct noise in about [0.27, 0.77] dmax: the recon arms' clearance numbers mean "
          "nothing until a trained checkpoint is converted; the timings hold")
    print(json.dumps(res))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--B", type=int, default=256)
    ap.add_argument("--N", type=int, default=40)
    ap.add_argument("--K", type=int, default=30)
    ap.add_argument("--every", type=int, default=1)
    ap.add_argument("--reps", type=int, default=2)
    ap.add_argument("--shape", type=int, nargs=2, default=(270, 480), help="image size (multiples of 5)")
    ap.add_argument("--reconstruct", action="store_true", help="the rung of the VAE's reconstruction (see above)")
    a = ap.parse_args()
    warnings.simplefilter("ignore")
    cfg = Config(mpc__N=a.N)
    if a.reconstruct:
        return main_reconstruct(cfg, a)
    res = {"B": a.B, "N": a.N, "K": a.K, "every": a.every, "shape": list(a.shape)}
    ms = {k: [] for k in ARMS}
    runs = {}
    for rep in range(a.reps + 1):  # repetition 0 warms up; the arms alternate inside every repetition
        for arm in ARMS:
            r, t, _, _ = fly(cfg, a, arm)
            runs[arm] = r
            if rep:
                ms[arm].append(t)
    for arm in ARMS:
        mc = runs[arm].clearance.min(axis=1)
        res[f"{arm}_ms_per_step"] = min(ms[arm])
        res[f"{arm}_min_clearance_percentiles"] = dict(zip(map(str, Q), np.percentile(mc, Q).round(4).tolist()))
        res[f"{arm}_collided"] = int((mc < 0).sum())
        res[f"{arm}_qp_iters_mean"] = float(runs[arm].iters.mean())
    for arm in ("net", "img_signed", "img_unsigned"):  # the kernels of the step, per launch, from one timed rollout each
        _, _, st, rows = fly(cfg, a, arm, timed=True, keep=arm != "net")
        for k, (us, cnt) in st.items():
            if cnt:
                res[f"{arm}_{k}_us"] = us
        for k, v in rows.items():
            res[f"{arm}_alone_{k}"] = v
    print(f"B={a.B} N={a.N} K={a.K} images {a.shape[0]} x {a.shape[1]}: ms per control step (best of {a.reps}), min clearance "
          f"over the batch at percentiles {Q}")
    for arm in ARMS:
        print(f"  {arm:22s} {res[f'{arm}_ms_per_step']:.3f} ms/step  clearance "
              f"{list(res[f'{arm}_min_clearance_percentiles'].values())}  collided {res[f'{arm}_collided']}  "
              f"QP iterations {res[f'{arm}_qp_iters_mean']:.1f}")
    net = res.get("net_sdf_hoist_us", 0.0) + res.get("net_sdf_mlp_us", 0.0)
    print(f"per launch in a timed rollout: sdf_hoist + sdf_mlp {net:.1f} us; img_sdf_rows signed "
          f"{res.get('img_signed_img_sdf_rows_us', float('nan')):.1f} us, unsigned {res.get('img_unsigned_img_sdf_rows_us', float('nan')):.1f} us")
    for arm in ("img_signed", "img_unsigned"):
        print(f"img_sdf_rows alone ({arm[4:]}) over {res[f'{arm}_alone_rows']} rows: {res[f'{arm}_alone_us']:.1f} us; "
              f"{res[f'{arm}_alone_full_scan_share']:.1%} of the flagged rows at max_df")
    print(json.dumps(res))
    if res.get("img_signed_img_sdf_rows_us", 0.0) > net:
        print("NOTE: the signed scan took longer than the network's two kernels in this run")


if __name__ == "__main__":
    main()
