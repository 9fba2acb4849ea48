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
Prints a table and a JSON line.  Diagnostic.

--movers m (1..32) asks the other question: what do m moving obstacles beside the forest cost (Scene(..., grid=True,
movers=Scene.crowd(m, ...)), the *_mixed kernels)?  For n = 256, 1024, 4096 it times the three mixed kernels against the
composition they replace -- the grid kernel on the forest, the dynamic kernel on the movers alone, and one elementwise
minimum (render, distance) or compare-and-select (rows) pass -- and beside them the grid kernel alone: the difference is
what the movers cost.  Every launch is timed on its own, --reps of them after a warm-up: the mean and the spread
(max - min) are printed.  The two ways are compared bit for bit before any time is reported.  Then one perceiving
rollout in the 1024-cylinder forest with Scene.crowd(16, ...).

    timeout 900 python tools/large_scene_probe.py --movers 4"""
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


def each_ms(ctx, name, launch, reps):
    """HIP-event time of every one of `reps` launches after a warm-up -> (mean, max - min) [ms]"""
    launch()
    ctx.synchronize()
    ms = []
    for _ in range(reps):
        ctx.reset_stats()
        launch()
        ctx.synchronize()
        t, cnt = ctx.kernel_stats(name)
        assert cnt == 1, (name, cnt)
        ms.append(t)
    return float(np.mean(ms)), float(np.max(ms) - np.min(ms))


def mixed_main(a):
    """--movers: the mixed kernels against grid + dynamic + one combining pass"""
    import torch
    cfg = Config(mpc__N=a.N)
    h, w = (int(v) for v in cfg.sensor.shape_imgs[-2:])
    B, N, K, NP, m = a.B, a.N, a.K, 17, a.movers
    T, max_df = 0.7, 1.0
    ctx = _lib.Context(0, stream=torch.cuda.current_stream().cuda_stream)
    ctx.enable_timing(True)
    dev = torch.device("cuda:0")
    res = {"B": B, "N": N, "K": K, "shape": [h, w], "density": a.density, "movers": m, "reps": a.reps, "sizes": {}}
    ia, ib = torch.rand(B, h, w, device=dev), torch.rand(B, h, w, device=dev)
    da, db = torch.rand(B * K, device=dev, dtype=torch.float64), torch.rand(B * K, device=dev, dtype=torch.float64)
    ha, hb = (torch.rand(B * (N + 1), device=dev, dtype=torch.float64) for _ in range(2))
    Ja, Jb = (torch.rand(B * (N + 1), 3, device=dev, dtype=torch.float64) for _ in range(2))

    def rows_min():
        lower = hb < ha
        return torch.where(lower, hb, ha), torch.where(lower[:, None], Jb, Ja)

    comb = dict(render=torch_ms(lambda: torch.minimum(ia, ib), a.reps), dist=torch_ms(lambda: torch.minimum(da, db), a.reps),
                rows=torch_ms(rows_min, a.reps))
    res["combine_pass_ms"] = comb
    del ia, ib, Ja, Jb
    print(f"{m} movers; B = {B}, image {h} x {w}, {B * K} points, {B * (N + 1)} rows; one combining pass: render "
          f"{comb['render']:.3f} ms, distance {comb['dist']:.4f} ms, rows {comb['rows']:.4f} ms; mean (spread) of {a.reps} launches [ms]")
    print(f"{'n':>5} {'query':>8} {'mixed':>16} {'grid + dyn + pass':>34} {'grid alone':>16} {'mixed / composition':>20}")
    for n in a.sizes:
        prims, half = forest(n, a.density)
        movers = Scene.crowd(m, (-half, -half, Z[0]), (half, half, Z[1]), seed=1)
        rng = np.random.default_rng(1)
        pos = rng.uniform([-half, -half, -1.0], [half, half, 1.0], (B, 3))
        yaw = rng.uniform(-np.pi, np.pi, B)
        Rm = np.zeros((B, 3, 3))
        Rm[:, 0, 0], Rm[:, 0, 1], Rm[:, 1, 0], Rm[:, 1, 1], Rm[:, 2, 2] = np.cos(yaw), -np.sin(yaw), np.sin(yaw), np.cos(yaw), 1.0
        dP, dR = _lib.DeviceArray.from_numpy(ctx, pos), _lib.DeviceArray.from_numpy(ctx, Rm.reshape(B, 9))
        pts = _lib.DeviceArray.from_numpy(ctx, rng.uniform([-half, -half, -1.0], [half, half, 1.0], (B * K, 3)))
        times = _lib.DeviceArray.from_numpy(ctx, rng.uniform(0.0, 2.0, B * K))
        x = rng.normal(0, 1, (B, N + 1, 10))
        x[..., :3] = rng.uniform([-half, -half, -1.0], [half, half, 1.0], (B, N + 1, 3))
        dx, dp = _lib.DeviceArray.from_numpy(ctx, x), _lib.DeviceArray.from_numpy(ctx, np.ones((B, N + 1, NP)))
        tau = _lib.DeviceArray.from_numpy(ctx, 0.05 * np.arange(N + 1))
        scenes = dict(mixed=Scene(ctx, prims, grid=True, movers=movers), grid=Scene(ctx, prims, grid=True),
                      dyn=Scene(ctx, movers))
        out = {k: dict(img=_lib.DeviceArray(ctx, (B, h, w), np.float32), dist=_lib.DeviceArray(ctx, (B * K,), np.float64),
                       h=_lib.DeviceArray(ctx, (B, N + 1, 3)), J=_lib.DeviceArray(ctx, (B, N + 1, 10, 3))) for k in scenes}
        launch = dict(
            render=lambda k: scenes[k].render(dP, dR, cfg, out=out[k]["img"], t=T),
            dist=lambda k: _lib.scene_distance_at(ctx, scenes[k].h, pts, None, times, B * K, out[k]["dist"]),
            rows=lambda k: _lib.scene_sdf_rows(ctx, scenes[k].h, B, N, NP, dx, dp, out[k]["h"], out[k]["J"], max_df, t0=T, tau=tau))
        names = dict(render=dict(mixed="scene_render_mixed", grid="scene_render_grid", dyn="scene_render_dyn"),
                     dist=dict(mixed="scene_dist_mixed", grid="scene_dist_grid", dyn="scene_dist_dyn"),
                     rows=dict(mixed="scene_sdf_rows_mixed", grid="scene_sdf_rows_grid", dyn="scene_sdf_rows"))
        row = {}
        for q in ("render", "dist", "rows"):
            for k in scenes:
                row[f"{q}_{k}_ms"], row[f"{q}_{k}_spread_ms"] = each_ms(ctx, names[q][k], lambda: launch[q](k), a.reps)
            row[f"{q}_composition_ms"] = row[f"{q}_grid_ms"] + row[f"{q}_dyn_ms"] + comb[q]
        # the two ways give the same bits: the images of the first 16 poses, every distance, every row
        img = {k: scenes[k].render(pos[:16], Rm[:16], cfg, t=T).numpy() for k in scenes}
        d = {k: out[k]["dist"].numpy() for k in scenes}
        hh = {k: out[k]["h"].numpy()[..., 2] for k in scenes}
        JJ = {k: out[k]["J"].numpy()[..., 2] for k in scenes}
        lower = hh["dyn"] < hh["grid"]
        equal = (np.array_equal(img["mixed"], np.minimum(img["grid"], img["dyn"])) and
                 np.array_equal(d["mixed"], np.minimum(d["grid"], d["dyn"])) and
                 np.array_equal(hh["mixed"], np.where(lower, hh["dyn"], hh["grid"])) and
                 np.array_equal(JJ["mixed"], np.where(lower[..., None], JJ["dyn"], JJ["grid"])))
        assert equal, f"n = {n}: the mixed kernels and the composition differ"
        row["bitwise_equal"] = True
        row["pixels_from_movers"] = float((img["dyn"] < img["grid"]).mean())
        row["rows_from_movers"] = float(lower.mean())
        for s in scenes.values():
            s.close()
        res["sizes"][str(n)] = row
        for q in ("render", "dist", "rows"):
            g = lambda k: f"{row[f'{q}_{k}_ms']:.4f} ({row[f'{q}_{k}_spread_ms']:.4f})"
            print(f"{n:>5} {q:>8} {g('mixed'):>16} {row[f'{q}_composition_ms']:>8.4f} = {g('grid')} + {row[f'{q}_dyn_ms']:.4f} + "
                  f"{comb[q]:.4f} {g('grid'):>16} {row[f'{q}_mixed_ms'] / row[f'{q}_composition_ms']:>12.2f}")
        print(f"      bitwise equal; {100 * row['pixels_from_movers']:.1f} % of the pixels and {100 * row['rows_from_movers']:.1f} % "
              f"of the rows come from a mover")
    ctx.close()

    if not a.no_rollout:
        n, x0, wps = controller(cfg, B, seed=3)
        prims, half = forest(1024, a.density)
        scene = Scene(n.ocp.ctx, prims, grid=True, movers=Scene.crowd(16, (-half, -half, Z[0]), (half, half, Z[1]), seed=1))
        vae = VaeWrapper(cfg, batch=B, ctx=n.ocp.ctx)
        best = None
        for rep in range(2):  # repetition 0 warms up
            n.set_x0(x0)
            t = time.perf_counter()
            r = n.rollout(K, refs="wps", wps=wps, scene=scene, vae=vae, perceive_every=1)
            best = (time.perf_counter() - t) * 1e3 / K if rep else None
        cmin = r.clearance.min(axis=1)
        res["rollout_1024_crowd16"] = dict(ms_per_step=best, converged=float((r.status == 0).mean()),
                                           collided=float((cmin <= 0).mean()), min_clearance_p50=float(np.median(cmin)))
        print(f"rollout in the 1024-cylinder forest with a crowd of 16, perceiving every step: {best:.2f} ms per step; "
              f"{100 * res['rollout_1024_crowd16']['converged']:.2f} % of the QPs converged; {100 * res['rollout_1024_crowd16']['collided']:.1f} % "
              f"of the instances touched an obstacle (synthetic weights: this says nothing about the controller)")
        n.ocp.close()
    print(json.dumps(res))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--B", type=int, default=1024)
    ap.add_argument("--N", type=int, default=40)
    ap.add_argument("--K", type=int, default=50)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--density", type=float, default=0.25)
    ap.add_argument("--sizes", type=int, nargs="*", default=None)
    ap.add_argument("--no-rollout", action="store_true")
    ap.add_argument("--movers", type=int, default=0, help="1..32: time the mixed kernels with that many movers instead")
    a = ap.parse_args()
    warnings.simplefilter("ignore")
    if a.movers:
        a.sizes = a.sizes or [256, 1024, 4096]
        return mixed_main(a)
    a.sizes = a.sizes or list(SIZES)
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
