"""What do the three mesh kernels cost, and what does the hierarchy buy?  On a heightfield of --grid x --grid vertices
(about 20 k triangles at the default 101) and on a tunnel of comparable size it times, by HIP events,

  * scene_render_mesh over --B images of the config's sensor shape, cameras above the terrain / inside the tunnel;
  * scene_dist_mesh over --points points around the surface;
  * scene_swept_mesh over --chords chords of about a metre (eps 1e-3, at most --max-evals evaluations each),

with the hierarchy (the default leaf size, and --leaf) against leaf_size = -1, the same kernels over one leaf that holds
every triangle -- and checks that both give the same bits.  Beside them the same three queries of a forest of as many
cylinders behind the grid index (Scene.forest, grid=True): another world, so the comparison says what a scene of that
many elements costs in either representation, not which is better.  The library has no diagnostic build that counts
node visits, so none are printed.  The last line is the JSON of everything printed."""
import argparse
import json
import os
import sys
import warnings

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from sdf_nmpc_amd import _lib
from sdf_nmpc_amd.config import Config
from sdf_nmpc_amd.mesh import Mesh
from sdf_nmpc_amd.scene import Scene
from large_scene_probe import each_ms


def terrain(g):
    i, j = np.meshgrid(np.arange(g), np.arange(g), indexing="ij")
    d = 20.0 / (g - 1)
    return Mesh.heightfield(-10.0, -10.0, d, d, -1.5 + 0.5 * np.sin(0.9 * d * i) * np.cos(0.7 * d * j) + 0.15 * np.sin(3.1 * d * (i + j)))


def tunnel(ntri):
    seg = 40
    rings = max(ntri // (2 * seg) + 1, 2)
    s = np.linspace(0.0, 60.0, rings)
    return Mesh.tunnel(np.stack([s, 2.0 * np.sin(0.2 * s), 0.8 * np.cos(0.15 * s)], 1), 2.0, segments=seg, roughness=0.2, seed=7)


def queries(rng, a, kind):
    """Camera poses, points and chords near the surface: above the terrain, or along the tunnel's axis."""
    if kind == "tunnel":
        s = rng.uniform(2.0, 58.0, a.B)
        cam = np.stack([s, 2.0 * np.sin(0.2 * s), 0.8 * np.cos(0.15 * s)], 1)
        s = rng.uniform(0.0, 60.0, a.points)
        pts = np.stack([s, 2.0 * np.sin(0.2 * s), 0.8 * np.cos(0.15 * s)], 1) + rng.uniform(-1.2, 1.2, (a.points, 3))
    else:
        cam = np.column_stack([rng.uniform(-8, 8, (a.B, 2)), rng.uniform(-0.5, 0.5, a.B)])
        pts = np.column_stack([rng.uniform(-10, 10, (a.points, 2)), rng.uniform(-2.0, 0.5, a.points)])
    yaw = rng.uniform(-0.3, 0.3, a.B) if kind == "tunnel" else rng.uniform(-np.pi, np.pi, a.B)
    R = np.stack([[[np.cos(y), -np.sin(y), 0], [np.sin(y), np.cos(y), 0], [0, 0, 1.0]] for y in yaw])
    p0 = pts[:a.chords]
    e = rng.normal(0, 1, (a.chords, 3))
    p1 = p0 + e / np.linalg.norm(e, axis=1, keepdims=True) * rng.uniform(0.5, 1.5, (a.chords, 1))
    return cam, R, pts, p0, p1


def time_scene(ctx, cfg, scene, q, a, names):
    cam, R, pts, p0, p1 = q
    h, w = (int(v) for v in cfg.sensor.shape_imgs[-2:])
    dev = lambda x, dt=np.float64: _lib.DeviceArray.from_numpy(ctx, np.ascontiguousarray(x, dtype=dt))
    dp, dR, dpts, d0, d1 = dev(cam), dev(R.reshape(-1, 9)), dev(pts), dev(p0), dev(p1)
    img = _lib.DeviceArray(ctx, (a.B, h, w), np.float32)
    dist = _lib.DeviceArray(ctx, (a.points,))
    dmin, s, gap = (_lib.DeviceArray(ctx, (a.chords,)) for _ in range(3))
    evals = _lib.DeviceArray(ctx, (a.chords,), np.int32)
    o = Scene.img_opts(cfg)
    r_ms, r_sp = each_ms(ctx, names[0], lambda: _lib.scene_render(ctx, scene.h, None, o, h, w, 1.0, a.B, dp, dR, img), a.reps)
    d_ms, d_sp = each_ms(ctx, names[1], lambda: _lib.scene_distance(ctx, scene.h, dpts, None, a.points, dist), a.reps)
    s_ms, s_sp = each_ms(ctx, names[2], lambda: _lib.scene_swept_distance(ctx, scene.h, d0, d1, None, None, None, a.chords, 1e-3,
                                                                           a.max_evals, dmin, s, gap, evals), a.reps)
    out = dict(render_ms=r_ms, render_spread_ms=r_sp, dist_ms=d_ms, dist_spread_ms=d_sp, swept_ms=s_ms, swept_spread_ms=s_sp,
               evals_mean=float(evals.numpy().mean()), hit_share=float((img.numpy() < float(cfg.sensor.dmax)).mean()))
    return out, (img.numpy(), dist.numpy(), dmin.numpy(), s.numpy(), gap.numpy(), evals.numpy())


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--grid", type=int, default=101, help="vertices per side of the heightfield: 2 (grid - 1)^2 triangles")
    ap.add_argument("--B", type=int, default=8)
    ap.add_argument("--points", type=int, default=16384)
    ap.add_argument("--chords", type=int, default=4096)
    ap.add_argument("--max-evals", type=int, default=256)
    ap.add_argument("--leaf", type=int, nargs="*", default=[1, 8], help="leaf sizes timed beside the default")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--no-brute", action="store_true", help="skip leaf_size = -1 (and the check against it)")
    a = ap.parse_args()
    warnings.filterwarnings("ignore")
    import torch
    cfg = Config()
    ctx = _lib.Context(0, stream=torch.cuda.current_stream().cuda_stream)
    ctx.enable_timing(True)
    mesh_names = ("scene_render_mesh", "scene_dist_mesh", "scene_swept_mesh")
    res = dict(B=a.B, shape=[int(v) for v in cfg.sensor.shape_imgs[-2:]], points=a.points, chords=a.chords,
               max_evals=a.max_evals, reps=a.reps, scenes={})
    ter = terrain(a.grid)
    for kind, mesh in (("heightfield", ter), ("tunnel", tunnel(ter.tris.shape[0]))):
        q = queries(np.random.default_rng(2), a, kind)
        rows, base = {}, None
        for leaf in ([] if a.no_brute else [-1]) + [0] + list(a.leaf):
            scene = Scene.mesh(ctx, mesh, leaf_size=leaf)
            rows[str(leaf)], got = time_scene(ctx, cfg, scene, q, a, mesh_names)
            scene.close()
            if leaf == -1:
                base = got
            elif base is not None:
                assert all(np.array_equal(x, y) for x, y in zip(got, base)), f"{kind}: leaf_size {leaf} differs from -1"
        res["scenes"][kind] = dict(triangles=int(mesh.tris.shape[0]), leaf=rows)
        print(f"{kind}: {mesh.tris.shape[0]} triangles; {a.B} images of {res['shape']}, {a.points} points, {a.chords} chords")
        for leaf, r in rows.items():
            label = {"-1": "no hierarchy", "0": "default leaf"}.get(leaf, f"leaf {leaf}")
            print(f"  {label:13s} render {r['render_ms']:9.4f} ms (spread {r['render_spread_ms']:.4f})  distance {r['dist_ms']:9.4f} ms "
                  f"({r['dist_spread_ms']:.4f})  swept {r['swept_ms']:9.4f} ms ({r['swept_spread_ms']:.4f}; {r['evals_mean']:.1f} "
                  f"evaluations per chord); {100 * r['hit_share']:.0f} % of the pixels hit")
    n = ter.tris.shape[0]
    half = 0.5 * np.sqrt(n / 0.25)
    forest = Scene.forest(min(n, 65536), (-half, -half, -2.0), (half, half, 2.5), radius=(0.15, 0.4), seed=0, keep_clear=((0.0, 0.0), 2.2))
    scene = Scene(ctx, forest, grid=True)
    rng = np.random.default_rng(2)
    cam = np.column_stack([rng.uniform(-1, 1, (a.B, 2)), rng.uniform(-0.5, 0.5, a.B)])
    yaw = rng.uniform(-np.pi, np.pi, a.B)
    R = np.stack([[[np.cos(y), -np.sin(y), 0], [np.sin(y), np.cos(y), 0], [0, 0, 1.0]] for y in yaw])
    pts = np.column_stack([rng.uniform(-half, half, (a.points, 2)), rng.uniform(-2.0, 2.5, a.points)])
    e = rng.normal(0, 1, (a.chords, 3))
    p1 = pts[:a.chords] + e / np.linalg.norm(e, axis=1, keepdims=True) * rng.uniform(0.5, 1.5, (a.chords, 1))
    r, _ = time_scene(ctx, cfg, scene, (cam, R, pts, pts[:a.chords], p1), a, ("scene_render_grid", "scene_dist_grid", "scene_swept_grid"))
    scene.close()
    res["scenes"]["forest_grid"] = dict(primitives=len(forest), **r)
    print(f"forest of {len(forest)} cylinders behind the grid index: render {r['render_ms']:.4f} ms  distance {r['dist_ms']:.4f} ms  "
          f"swept {r['swept_ms']:.4f} ms ({r['evals_mean']:.1f} evaluations per chord); {100 * r['hit_share']:.0f} % of the pixels hit")
    ctx.enable_timing(False)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
