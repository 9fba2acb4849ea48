"""What does the controller's distance constraint know of the world?  The B = 256 forest rollout of
tools/perceive_probe.py flown two ways on one controller configuration: with the network as the SDF (the SIREN
initialisation unless weights are given: a new image of the scene before every step, encoded, as perceive_probe runs
it) and with the exact signed distance of the same scene (Nmpc.set_sdf_scene, csrc/scene_sdf.hip) -- on the static
forest, and on the moving one with `predict` off (every node sees the scene of the step's time) and on (node k sees it
at its own time).  Prints the distribution of the minimum clearance over the batch for each arm, ms per control step
(the arms alternate inside every repetition; best of --reps after a warm-up; every arm's time includes the one
clearance launch and its download after the loop), the step without perception both ways
(the network's sdf_hoist + sdf_mlp against scene_sdf_rows in the same preparation phase), and the kernels' own times
from HIP events: scene_sdf_rows at 16 primitives over B (N+1) rows, 20 launches after 5, static / dynamic / dynamic
with per-node times, next to sdf_hoist + sdf_mlp per step from a timed rollout of the same run.

    timeout 600 python tools/scene_sdf_probe.py --B 256 --N 40
    timeout 600 python tools/scene_sdf_probe.py --B 1024 --N 40 --K 20
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
from sdf_nmpc_amd.vae import VaeWrapper
from perceive_probe import forest, moving_forest
from rollout_probe import controller

Q = (0, 5, 25, 50, 75, 95, 100)


def fly(cfg, a, arm, timed=False):
    """One rollout of an arm on a fresh controller: (Rollout, ms per step, kernel stats of a timed run)."""
    n, x0, wps = controller(cfg, a.B, 1)
    ctx = n.ocp.ctx
    moving = arm.startswith("moving")
    scene = Scene(ctx, (moving_forest if moving else forest)(16))
    kw, vae = {}, None
    if arm.endswith("net"):        # the network sees the scene through the camera and the encoder
        vae = VaeWrapper(cfg, batch=a.B, ctx=ctx)
        kw = dict(scene=scene, vae=vae, perceive_every=a.every)
    elif arm.endswith("blind"):    # the network without perception: the step alone (its clearance is measured below, after the loop)
        pass
    else:
        n.set_sdf_scene(scene, predict=arm.endswith("predict"))
    n.set_x0(x0)
    stats = {}
    if timed:
        ctx.reset_stats()
        ctx.enable_timing(True)
    ctx.synchronize()
    t0 = time.perf_counter()
    r = n.rollout(a.K, refs="wps", wps=wps, **kw)
    if r.clearance is None:  # inside the timed span, where rollout() measures it for the other arms
        t = np.arange(a.K + 1) * float(n.ocp.dt[0])
        pts = np.ascontiguousarray(r.x[:, :, :3]).reshape(-1, 3)
        r.clearance = scene.distance(pts, t=np.tile(t, max(n.B, 1)) if moving else None).reshape(-1, a.K + 1)
    ms = (time.perf_counter() - t0) / a.K * 1e3
    if timed:
        for k in ("sdf_hoist", "sdf_mlp", "scene_sdf_rows", "linearize", "rti_qp_pack", "rti_qp"):
            t, c = ctx.kernel_stats(k)
            stats[k] = (t / max(c, 1) * 1e3, c)
        ctx.enable_timing(False)
    if vae is not None:
        vae.vae.close()
    n.ocp.close()
    return r, ms, stats


def rows_kernel_times(cfg, a, res):
    """HIP events around scene_sdf_rows alone: B (N+1) rows against 16 primitives."""
    ctx = _lib.Context(0)
    B, N = a.B, a.N
    rng = np.random.default_rng(0)
    x = np.zeros((B, N + 1, 10))
    x[..., :3] = rng.uniform([-1, -4, -1.5], [8, 4, 2], (B, N + 1, 3))
    p = np.ones((B, N + 1, 17))
    d = {k: _lib.DeviceArray.from_numpy(ctx, v) for k, v in dict(x=x, p=p, h=np.zeros((B, N + 1, 3)),
                                                                   Jh=np.zeros((B, N + 1, 10, 3))).items()}
    tau = _lib.DeviceArray.from_numpy(ctx, np.arange(N + 1) * float(cfg.mpc.T) / N)
    for name, prims, t in (("static", forest(16), None), ("dynamic", moving_forest(16), None),
                           ("dynamic_tau", moving_forest(16), tau)):
        scene = Scene(ctx, prims)
        fn = lambda: _lib.scene_sdf_rows(ctx, scene.h, B, N, 17, d["x"], d["p"], d["h"], d["Jh"], 1.0, t0=1.3, tau=t)
        for _ in range(5):
            fn()
        ctx.synchronize()
        ctx.reset_stats()
        ctx.enable_timing(True)
        for _ in range(20):
            fn()
        ms, cnt = ctx.kernel_stats("scene_sdf_rows")
        ctx.enable_timing(False)
        ctx.reset_stats()
        res[f"scene_sdf_rows_{name}_us"] = ms / cnt * 1e3
        res[f"untruncated_share_{name}"] = float((d["h"].numpy()[..., 2] < 1.0).mean())
        scene.close()
    res["rows"] = B * (N + 1)
    ctx.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--B", type=int, default=256)
    ap.add_argument("--N", type=int, default=40)
    ap.add_argument("--K", type=int, default=50)
    ap.add_argument("--every", type=int, default=1)
    ap.add_argument("--reps", type=int, default=2)
    a = ap.parse_args()
    warnings.simplefilter("ignore")
    cfg = Config(mpc__N=a.N)
    res = {"B": a.B, "N": a.N, "K": a.K, "every": a.every}
    arms = ("static_net", "static_exact", "static_blind", "moving_net", "moving_exact", "moving_exact_predict")
    ms = {k: [] for k in arms}
    runs = {}
    for rep in range(a.reps + 1):  # repetition 0 warms up; the arms alternate inside every repetition
        for arm in arms:
            r, t, _ = fly(cfg, a, arm)
            runs[arm] = r
            if rep:
                ms[arm].append(t)
    for arm in arms:
        mc = runs[arm].clearance.min(axis=1)
        res[f"{arm}_ms_per_step"] = min(ms[arm])
        res[f"{arm}_ms_all"] = [round(t, 3) for t in ms[arm]]
        res[f"{arm}_min_clearance_percentiles"] = dict(zip(map(str, Q), np.percentile(mc, Q).round(4).tolist()))
        res[f"{arm}_collided"] = int((mc < 0).sum())
        res[f"{arm}_qp_iters_mean"] = float(runs[arm].iters.mean())
    for arm in ("static_blind", "static_exact"):  # the kernels of the step, per launch, from one timed rollout each
        _, _, st = fly(cfg, a, arm, timed=True)
        for k, (us, cnt) in st.items():
            if cnt:
                res[f"{arm}_{k}_us"] = us
    rows_kernel_times(cfg, a, res)
    print(f"B={a.B} N={a.N} K={a.K}: ms per control step (best of {a.reps}), min clearance over the batch at percentiles {Q}")
    for arm in arms:
        print(f"  {arm:22s} {res[f'{arm}_ms_per_step']:.3f} ms/step  clearance "
              f"{list(res[f'{arm}_min_clearance_percentiles'].values())}  collided {res[f'{arm}_collided']}")
    net = res.get("static_blind_sdf_hoist_us", 0.0) + res.get("static_blind_sdf_mlp_us", 0.0)
    print(f"per step in a timed rollout: sdf_hoist + sdf_mlp {net:.1f} us; scene_sdf_rows "
          f"{res.get('static_exact_scene_sdf_rows_us', float('nan')):.1f} us.  scene_sdf_rows alone over {res['rows']} rows, "
          f"16 primitives: static {res['scene_sdf_rows_static_us']:.1f} us, dynamic {res['scene_sdf_rows_dynamic_us']:.1f} us, "
          f"dynamic with tau {res['scene_sdf_rows_dynamic_tau_us']:.1f} us")
    print(json.dumps(res))
    if res["static_exact_ms_per_step"] > res["static_blind_ms_per_step"]:
        print("NOTE: the step with the scene source was slower than the step with the network in this run")


if __name__ == "__main__":
    main()
