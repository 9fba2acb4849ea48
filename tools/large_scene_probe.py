"""What does the grid index of a large scene (Scene(..., grid=True), csrc/scene_grid.hip) cost and buy?  Forests of
n = 32, 256, 1024, 4096 upright cylinders at a fixed density (--density per square metre: the world grows with n, the
clutter around a camera does not), queried from --B poses spread over the forest at the config's image shape:

    render      one launch, B images                       "scene_render_grid"
    distance    one launch, B K points                     "scene_dist_grid"
    SDF rows    one launch, B (N + 1) node rows            "scene_sdf_rows_grid"

each against the only thing a plain scene offers for more than 32 primitives: ceil(n / 32) launches of the brute-force
kernel on chunks of 32 ("scene_render", "scene_dist", "scene_sdf_rows") plus the elementwise minimum of their outputs
(timed with torch on arrays of the same shape: chunks - 1 passes; for the rows a compare and two selects per pass).
All kernel times are HIP-event times from sdfnmpc_ctx_kernel_stats, the mean of --reps launches after a warm-up.  The
images of the two ways are compared bit for bit.  Then one rollout(scene=, vae=, perceive_every=1) of --K steps in
the 1024-cylinder forest (--no-rollout skips it): ms per step and the distribution of the minimum clearance.

    timeout 900 python tools/large_scene_probe.py --B 1024 --N 40 --K 50
Prints a table and a JSON line.  Diagnostic."""
import argparse
import json
import os
import sys
import time
import warnings

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from sdf_nmpc_amd import _lib
from sdf_nmpc_amd.config import Config
from sdf_nmpc_amd.scene import Scene
from sdf_nmpc_amd.vae import VaeWrapper
from rollout_probe import controller

SIZES = (32, 256, 1024, 4096)
CHUNK = 32
Z = (-2.0, 2.5)
CLEAR = ((0.0, 0.0), 2.2)  # rollout_probe.controller starts in [-1, 1]^3


def forest(n, density, seed=0):
    half = 0.5 * np.sqrt(n / density)
    return Scene.forest(n, (-half, -half, Z[0]), (half, half, Z[1]), radius=(0.15, 0.4), seed=seed, keep_clear=CLEAR), half


def mean_ms(ctx, name, reps):
    ms, cnt = ctx.kernel_stats(name)
    assert cnt % reps == 0 and cnt > 0, (name, cnt)
    return ms / reps  # per repetition: one grid launch, or all chunk launches


def torch_ms(fn, reps):
    import torch
    fn()
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(reps):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / reps


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--B", type=int, default=1024)
    ap.add_argument("--N", type=int, default=40)
    ap.add_argument("--K", type=int, default=50)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--density", type=float, default=0.25)
    ap.add_argument("--sizes", type=int, nargs="*", default=list(SIZES))
    ap.add_argument("--no-rollout", action="store_true")
    a = ap.parse_args()
    warnings.simplefilter("ignore")
    import torch
    cfg = Config(mpc__N=a.N)
    h, w = (int(v) for v in cfg.sensor.shape_imgs[-2:])
    B, N, K, NP = a.B, a.N, a.K, 17
    ctx = _lib.Context(0, stream=torch.cuda.current_stream().cuda_stream)
    ctx.enable_timing(True)
    dev = torch.device("cuda:0")
    res = {"B": B, "N": N, "K": K, "shape": [h, w], "density": a.density, "sizes": {}}
    # the elementwise minimum the chunked way needs, per pass over outputs of the launch's shape
    ia, ib = torch.rand(B, h, w, device=dev), torch.rand(B, h, w, device=dev)
    da, db = torch.rand(B * K, device=dev, dtype=torch.float64), torch.rand(B * K, device=dev, dtype=torch.float64)
    ha, hb = (torch.rand(B * (N + 1), device=dev, dtype=torch.float64) for _ in range(2))
    Ja, Jb = (torch.rand(B * (N + 1), 3, device=dev, dtype=torch.float64) for _ in range(2))

    def rows_min():
        lower = hb < ha
        return torch.where(lower, hb, ha), torch.where(lower[:, None], Jb, Ja)

    min_ms = dict(render=torch_ms(lambda: torch.minimum(ia, ib), a.reps), dist=torch_ms(lambda: torch.minimum(da, db), a.reps),
                  rows=torch_ms(rows_min, a.reps))
    res["min_pass_ms"] = min_ms
    del ia, ib, Ja, Jb
    print(f"B = {B}, image {h} x {w}, {B * K} points, {B * (N + 1)} rows; one minimum pass: render {min_ms['render']:.3f} ms, "
          f"distance {min_ms['dist']:.4f} ms, rows {min_ms['rows']:.4f} ms")
    print(f"{'n':>5} {'forest':>13} {'render grid':>12} {'chunked':>9} {'x':>6} {'dist grid':>10} {'chunked':>9} {'x':>6} "
          f"{'rows grid':>10} {'chunked':>9} {'x':>6}   [ms per launch]")
    for n in a.sizes:
        prims, half = forest(n, a.density)
        rng = np.random.default_rng(1)
        pos = rng.uniform([-half, -half, -1.0], [half, half, 1.0], (B, 3))
        yaw = rng.uniform(-np.pi, np.pi, B)
        Rm = np.zeros((B, 3, 3))
        Rm[:, 0, 0], Rm[:, 0, 1], Rm[:, 1, 0], Rm[:, 1, 1], Rm[:, 2, 2] = np.cos(yaw), -np.sin(yaw), np.sin(yaw), np.cos(yaw), 1.0
        dP, dR = _lib.DeviceArray.from_numpy(ctx, pos), _lib.DeviceArray.from_numpy(ctx, Rm.reshape(B, 9))
        pts = _lib.DeviceArray.from_numpy(ctx, rng.uniform([-half, -half, -1.0], [half, half, 1.0], (B * K, 3)))
        x = rng.normal(0, 1, (B, N + 1, 10))
        x[..., :3] = rng.uniform([-half, -half, -1.0], [half, half, 1.0], (B, N + 1, 3))
        p = np.ones((B, N + 1, NP))
        dx, dp = _lib.DeviceArray.from_numpy(ctx, x), _lib.DeviceArray.from_numpy(ctx, p)
        dh, dJ = _lib.DeviceArray(ctx, (B, N + 1, 3)), _lib.DeviceArray(ctx, (B, N + 1, 10, 3))
        dist = _lib.DeviceArray(ctx, (B * K,), np.float64)
        img = _lib.DeviceArray(ctx, (B, h, w), np.float32)
        max_df = 1.0
        grid = Scene(ctx, prims, grid=True)
        plain = [Scene(ctx, prims[i:i + CHUNK]) for i in range(0, n, CHUNK)]

        def queries(scene):
            scene.render(dP, dR, cfg, out=img)
            _lib.scene_distance(ctx, scene.h, pts, None, B * K, dist)
            _lib.scene_sdf_rows(ctx, scene.h, B, N, NP, dx, dp, dh, dJ, max_df)

        row = {"chunks": len(plain)}
        for way, scenes, names in (("grid", [grid], ("scene_render_grid", "scene_dist_grid", "scene_sdf_rows_grid")),
                                   ("chunked", plain, ("scene_render", "scene_dist", "scene_sdf_rows"))):
            for s in scenes:  # warm-up
                queries(s)
            ctx.synchronize()
            ctx.reset_stats()
            for _ in range(a.reps):
                for s in scenes:
                    queries(s)
            ctx.synchronize()
            for key, name in zip(("render", "dist", "rows"), names):
                extra = (len(scenes) - 1) * min_ms[key] if way == "chunked" else 0.0
                row[f"{key}_{way}_ms"] = mean_ms(ctx, name, a.reps) + extra
        # the two ways give the same images (the first 16 poses)
        got = grid.render(pos[:16], Rm[:16], cfg).numpy()
        want = np.full_like(got, np.inf)
        for s in plain:
            want = np.minimum(want, s.render(pos[:16], Rm[:16], cfg).numpy())
        row["images_equal"] = bool(np.array_equal(got, want))
        row["pixels_hit"] = float((want < 1.0).mean())
        for s in plain + [grid]:
            s.close()
        if n <= CHUNK:  # the plain kernel on the very primitives, next to the grid's render of them
            row["render_grid_over_plain"] = row["render_grid_ms"] / row["render_chunked_ms"]
        res["sizes"][str(n)] = row
        f = lambda k: f"{row[k + '_grid_ms']:>{12 if k == 'render' else 10}.4f} {row[k + '_chunked_ms']:>9.4f} " \
                      f"{row[k + '_chunked_ms'] / row[k + '_grid_ms']:>6.1f}"
        print(f"{n:>5} {2 * half:>6.1f} m wide {f('render')} {f('dist')} {f('rows')}   images equal: {row['images_equal']}, "
              f"{100 * row['pixels_hit']:.0f} % of the pixels hit")
    ctx.close()

    if not a.no_rollout:
        n, x0, wps = controller(cfg, B, seed=3)
        prims, half = forest(1024, a.density)
        scene = Scene(n.ocp.ctx, prims, grid=True)
        vae = VaeWrapper(cfg, batch=B, ctx=n.ocp.ctx)
        best = None
        for rep in range(2):  # repetition 0 warms up
            n.set_x0(x0)
            t = time.perf_counter()
            r = n.rollout(K, refs="wps", wps=wps, scene=scene, vae=vae, perceive_every=1)
            dt = (time.perf_counter() - t) * 1e3 / K
            best = dt if rep else None
        cmin = r.clearance.min(axis=1)
        pct = {f"p{q}": float(np.percentile(cmin, q)) for q in (0, 5, 25, 50, 75, 95, 100)}
        res["rollout_1024"] = dict(ms_per_step=best, min_clearance=pct, collided=float((cmin <= 0).mean()),
                                   converged=float((r.status == 0).mean()))
        print(f"rollout in the 1024-cylinder forest, perceiving every step: {best:.2f} ms per step; minimum clearance over "
              f"{K} steps, percentiles over {B} instances: " + ", ".join(f"{k} {v:.2f}" for k, v in pct.items()) +
              f" m; {100 * res['rollout_1024']['collided']:.1f} % touched an obstacle")
        n.ocp.close()
    print(json.dumps(res))


if __name__ == "__main__":
    main()
