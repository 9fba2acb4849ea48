"""What do the three mesh kernels cost, and what does the hierarchy buy?  On a heightfield of --grid x --grid vertices
(about 20 k triangles at the default 101) and on a tunnel of comparable size it times, by HIP events,

  * scene_render_mesh over --B images of the config's sensor shape, cameras above the terrain / inside the tunnel;
  * scene_dist_mesh over --points points around the surface;
  * scene_swept_mesh over --chords chords of about a metre (eps 1e-3, at most --max-evals evaluations each),

with the hierarchy (the default leaf size, and --leaf) against leaf_size = -1, the same kernels over one leaf that holds
every triangle -- and checks that both give the same bits.  Beside them the same three queries of a forest of as many
cylinders behind the grid index (Scene.forest, grid=True): another world, so the comparison says what a scene of that
many elements costs in either representation, not which is better.  The library has no diagnostic build that counts
node visits, so none are printed.  The last line is the JSON of everything printed.

--sdf: what does the mesh as the controller's exact SDF cost (scene_sdf_rows_mesh)?  On the same tunnel and heightfield,
at N = 40 and B = 256 and 1024, the node positions are the iterate of a short rollout with the mesh source, so the rows
of an instance are neighbours on a trajectory.  It times scene_sdf_rows_mesh on them -- the open set (searched within
max_df only) and the same surface closed by cones over its boundary loops (the full search) -- at leaf sizes 1, 4 and -1,
beside scene_dist_mesh on the same points and sets, the yardstick; then the time per step of a rollout with the network
(perceiving the tunnel through the encoder, default weights) and with the mesh source, and the minimum clearance of both
arms.  Writes profiles/mesh_sdf_probe.json.

--movers m: what do m movers beside the mesh cost (Scene.mesh(..., movers=), the four *_mesh_mixed kernels)?  On the same
tunnel and heightfield with a Scene.crowd of m inside the mesh's bounds: --B images at t = 0.7, --points points with
times, rows at B = 1024, N = 40 with tau, --chords chords with times.  Each of scene_render_mesh_mixed,
scene_dist_mesh_mixed and scene_sdf_rows_mesh_mixed is set against the composition it replaces, from kernels the feature
left alone in the same process: the *_mesh kernel on the mesh alone, the dynamic kernel on the movers alone and the
combining pass, timed with torch -- after an assertion that both give the same bits.  The swept kernel has no
composition: it stands beside scene_swept_mesh on the mesh alone, with the evaluations per chord.  Also printed: how often
a mover is the nearest thing.  Writes profiles/mesh_mixed_probe.json (one file for every m it is run with).

--instances n: what do n instances of one part cost (Scene.instanced, the four *_inst kernels), against what they
replace?  The part is a tree of about 1 300 triangles; n of them stand in a field (Scene.scatter), and --B images, --points
points, rows at B = 128, N = 40 and --chords chords are timed
  * static: against the welded Scene.mesh(Mesh.merge(...)) of the same n trees -- another hierarchy over the same
    triangles, whose fp32 vertices are rounded after the placement, so the results agree to that rounding and not to the
    bit -- with the bytes of the triangle arrays of both beside the times;
  * moving (every tree drifts and yaws): against n single-instance scenes, queried in one launch over n times the
    queries, and one combining pass (torch) -- after an assertion that both give the same bits;
and the instanced kernels again at n / 4, for the cost per instance.  Writes profiles/mesh_inst_probe.json."""
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
from large_scene_probe import each_ms, torch_ms


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


def closed_by_cones(mesh, flip=False, apex_shift=(0.0, 0.0, 0.0)):
    """The surface made a closed, consistently oriented manifold: every boundary loop coned to one new vertex (the mean
    of the loop, shifted by apex_shift).  flip: every triangle reversed first."""
    t = mesh.tris[:, ::-1] if flip else mesh.tris
    e = set()
    for a, b, c in t.tolist():
        e.update(((a, b), (b, c), (c, a)))
    nxt = {a: b for a, b in e if (b, a) not in e}
    verts, tris = [mesh.verts], [t]
    nv = mesh.verts.shape[0]
    while nxt:
        a0 = next(iter(nxt))
        loop = [a0]
        while True:
            b = nxt.pop(loop[-1])
            if b == a0:
                break
            loop.append(b)
        verts.append(mesh.verts[loop].mean(0, keepdims=True) + np.asarray(apex_shift, float))
        tris.append(np.array([(v, u, nv) for u, v in zip(loop, loop[1:] + loop[:1])], np.int32))
        nv += 1
    out = Mesh(np.concatenate(verts, 0), np.concatenate(tris, 0))
    assert out.is_closed()
    return out


def sdf_starts(rng, B, kind):
    """Start states [B, 10] flying along +x at 1.5 m/s, and a goal 8 m ahead: on the tunnel's axis, or 1 m above the terrain"""
    x0 = np.zeros((B, 10))
    x0[:, 3], x0[:, 7] = 1.0, 1.5
    if kind == "tunnel":
        s = rng.uniform(2.0, 45.0, B)
        axis = lambda s: np.stack([s, 2.0 * np.sin(0.2 * s), 0.8 * np.cos(0.15 * s)], 1)
        x0[:, :3] = axis(s) + rng.uniform(-0.8, 0.8, (B, 3))
        goal = axis(s + 8.0)
    else:
        x0[:, :2] = rng.uniform(-8.0, 0.0, (B, 2))
        x0[:, 2] = -0.4 + rng.uniform(-0.2, 0.2, B)
        goal = x0[:, :3] + np.array([8.0, 0.0, 0.0])
    return x0, goal


def sdf_main(a):
    import time
    import torch
    from sdf_nmpc_amd.controller import Nmpc
    from sdf_nmpc_amd.reference import yaw2quat
    from sdf_nmpc_amd.vae import VaeWrapper
    N, K, max_df, name, yard = 40, 6, 1.0, "scene_sdf_rows_mesh", "scene_dist_mesh"
    cfg = Config(mpc__N=N)
    ter = terrain(a.grid)
    opens = {"tunnel": tunnel(ter.tris.shape[0]), "heightfield": ter}
    closeds = {"tunnel": closed_by_cones(opens["tunnel"], flip=True),  # the free space inside the tube is outside the solid
               "heightfield": closed_by_cones(ter, apex_shift=(0.0, 0.0, -8.0))}
    res = dict(N=N, max_df=max_df, reps=a.reps, rollout_steps=K, cases=[], steps=[])
    for kind in ("tunnel", "heightfield"):
        for B in (256, 1024):
            n = Nmpc(cfg, batch=B)
            ctx = n.ocp.ctx
            ctx.enable_timing(True)
            x0, goal = sdf_starts(np.random.default_rng(3), B, kind)
            wps = (goal[:, None, :], np.tile(yaw2quat(0.0), (B, 1, 1)))
            n.set_sdf_flag(1.0)
            src = Scene.mesh(ctx, opens[kind], sdf_source=True)
            n.set_sdf_scene(src, max_df=max_df)
            n.set_x0(x0)
            n.rollout(2, refs="wps", wps=wps)  # warm-up
            n.set_x0(x0)
            ctx.synchronize()
            t = time.perf_counter()
            r = n.rollout(K, refs="wps", wps=wps)
            mesh_ms = 1e3 * (time.perf_counter() - t) / K
            clear_mesh = r.clearance.min(1)
            x = n.ocp.download("x")                      # the iterate: [B, N+1, 10]
            dx = _lib.DeviceArray.from_numpy(ctx, x)
            dpts = _lib.DeviceArray.from_numpy(ctx, np.ascontiguousarray(x[..., :3]).reshape(-1, 3))
            rows = B * (N + 1)
            p = np.zeros((B, N + 1, 17))
            p[..., 0] = 1.0
            dp, dh, dJ = _lib.DeviceArray.from_numpy(ctx, p), _lib.DeviceArray(ctx, (B, N + 1, 3)), _lib.DeviceArray(ctx, (B, N + 1, 10, 3))
            dist = _lib.DeviceArray(ctx, (rows,))
            n.set_sdf_scene(None)
            src.close()
            base = {}
            for closed, meshes in ((False, opens), (True, closeds)):
                for leaf in (1, 4, -1):
                    sc = Scene.mesh(ctx, meshes[kind], closed=closed, leaf_size=leaf, sdf_source=True)
                    ms, sp = each_ms(ctx, name, lambda: _lib.scene_sdf_rows(ctx, sc.h, B, N, 17, dx, dp, dh, dJ, max_df), a.reps)
                    yms, ysp = each_ms(ctx, yard, lambda: _lib.scene_distance(ctx, sc.h, dpts, None, rows, dist), a.reps)
                    h2, d = dh.numpy()[..., 2].ravel(), dist.numpy()
                    assert np.array_equal(h2, np.where(d < max_df, d, max_df)), "rows differ from Scene.distance"
                    got = (h2, dJ.numpy()[..., 2])
                    if leaf == 1:
                        base[closed] = got
                    else:
                        assert all(np.array_equal(u, v) for u, v in zip(got, base[closed])), f"leaf_size {leaf} differs from 1"
                    sc.close()
                    case = dict(scene=kind, B=B, rows=rows, closed=closed, pruned=not closed, leaf=leaf,
                                triangles=int(meshes[kind].tris.shape[0]), rows_ms=ms, rows_spread_ms=sp, dist_ms=yms,
                                dist_spread_ms=ysp, near_share=float((h2 < max_df).mean()))
                    res["cases"].append(case)
                    print(f"{kind:11s} B={B:4d} {'closed' if closed else 'open, pruned':12s} leaf {leaf:2d}: {name} {ms:9.4f} ms "
                          f"(max - min {sp:.4f})   {yard} {yms:9.4f} ms ({ysp:.4f})   {100 * case['near_share']:.0f} % of the rows near")
            if kind == "tunnel":  # the two arms flying the tunnel: the mesh source above, and the network perceiving the mesh
                vae = VaeWrapper(cfg, batch=B, ctx=ctx)
                view = Scene.mesh(ctx, opens[kind])
                n.reset()
                n.set_sdf_flag(1.0)
                n.set_x0(x0)
                n.rollout(2, refs="wps", wps=wps, scene=view, vae=vae)
                n.set_x0(x0)
                ctx.synchronize()
                t = time.perf_counter()
                r = n.rollout(K, refs="wps", wps=wps, scene=view, vae=vae)
                net_ms = 1e3 * (time.perf_counter() - t) / K
                pc = lambda c: [float(v) for v in np.percentile(c, (0, 5, 50))]
                step = dict(scene=kind, B=B, K=K, mesh_source_ms_per_step=mesh_ms, network_ms_per_step=net_ms,
                            min_clearance_p0_p5_p50_mesh_source=pc(clear_mesh), min_clearance_p0_p5_p50_network=pc(r.clearance.min(1)))
                res["steps"].append(step)
                print(f"{kind} B={B}: {mesh_ms:.3f} ms per step with the mesh source, {net_ms:.3f} ms with the network (perceiving every "
                      f"step); minimum clearance p0 / p5 / p50 [m]: mesh source {np.round(pc(clear_mesh), 3).tolist()}, network "
                      f"{np.round(step['min_clearance_p0_p5_p50_network'], 3).tolist()}")
                view.close()
            ctx.enable_timing(False)
            n.ocp.close()
    os.makedirs(os.path.join(ROOT, "profiles"), exist_ok=True)
    with open(a.out or os.path.join(ROOT, "profiles", "mesh_sdf_probe.json"), "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(json.dumps(res))


def movers_main(a):
    import torch
    N, RB, NP, T, max_df, m = 40, 1024, 17, 0.7, 1.0, a.movers
    cfg = Config(mpc__N=N)
    h, w = (int(v) for v in cfg.sensor.shape_imgs[-2:])
    ctx = _lib.Context(0, stream=torch.cuda.current_stream().cuda_stream)
    ctx.enable_timing(True)
    dev = torch.device("cuda:0")
    ia, ib = torch.rand(a.B, h, w, device=dev), torch.rand(a.B, h, w, device=dev)
    da, db = (torch.rand(a.points, device=dev, dtype=torch.float64) for _ in range(2))
    ha, hb = (torch.rand(RB * (N + 1), device=dev, dtype=torch.float64) for _ in range(2))
    Ja, Jb = (torch.rand(RB * (N + 1), 3, device=dev, dtype=torch.float64) for _ in range(2))

    def rows_min():
        lower = hb < ha
        return torch.where(lower, hb, ha), torch.where(lower[:, None], Jb, Ja)

    comb = dict(render=torch_ms(lambda: torch.minimum(ia, ib), a.reps), dist=torch_ms(lambda: torch.minimum(da, db), a.reps),
                rows=torch_ms(rows_min, a.reps))
    res = dict(movers=m, B=a.B, shape=[h, w], points=a.points, rows=RB * (N + 1), N=N, chords=a.chords, max_evals=a.max_evals,
               reps=a.reps, t=T, max_df=max_df, combine_pass_ms=comb, scenes={})
    print(f"{m} movers; {a.B} images of {h} x {w}, {a.points} points, {RB * (N + 1)} rows, {a.chords} chords; one combining pass: "
          f"render {comb['render']:.4f} ms, distance {comb['dist']:.4f} ms, rows {comb['rows']:.4f} ms; mean (max - min) of {a.reps} "
          f"launches [ms]")
    ter = terrain(a.grid)
    names = dict(render=dict(mixed="scene_render_mesh_mixed", mesh="scene_render_mesh", dyn="scene_render_dyn"),
                 dist=dict(mixed="scene_dist_mesh_mixed", mesh="scene_dist_mesh", dyn="scene_dist_dyn"),
                 rows=dict(mixed="scene_sdf_rows_mesh_mixed", mesh="scene_sdf_rows_mesh", dyn="scene_sdf_rows"),
                 swept=dict(mixed="scene_swept_mesh_mixed", mesh="scene_swept_mesh"))
    for kind, mesh in (("tunnel", tunnel(ter.tris.shape[0])), ("heightfield", ter)):
        rng = np.random.default_rng(2)
        cam, R, pts, p0, p1 = queries(rng, a, kind)
        lo, hi = mesh.verts.min(0), mesh.verts.max(0)
        if kind == "tunnel":  # the crowd walks the tunnel's floor region, inside the tube
            lo, hi = np.array([lo[0], -1.5, -1.5]), np.array([hi[0], 1.5, 1.0])
        else:
            hi = np.array([hi[0], hi[1], hi[2] + 2.0])
        movers = Scene.crowd(m, lo, hi, seed=1)
        dv = lambda x, dt=np.float64: _lib.DeviceArray.from_numpy(ctx, np.ascontiguousarray(x, dtype=dt))
        dP, dR, dpts, d0, d1 = dv(cam), dv(R.reshape(-1, 9)), dv(pts), dv(p0), dv(p1)
        times = dv(rng.uniform(0.0, 2.0, a.points))
        c0 = rng.uniform(0.0, 2.0, a.chords)
        dc0, dc1 = dv(c0), dv(c0 + 0.1)
        x = rng.normal(0, 1, (RB, N + 1, 10))
        x[..., :3] = pts[rng.integers(0, a.points, RB)][:, None, :] + 0.075 * np.arange(N + 1)[None, :, None] * np.array([1.0, 0.0, 0.0])
        dx, dp = dv(x), dv(np.ones((RB, N + 1, NP)))
        tau = dv(0.05 * np.arange(N + 1))
        scenes = dict(mixed=Scene.mesh(ctx, mesh, sdf_source=True, movers=movers), mesh=Scene.mesh(ctx, mesh, sdf_source=True),
                      dyn=Scene(ctx, movers))
        out = {k: dict(img=_lib.DeviceArray(ctx, (a.B, h, w), np.float32), dist=_lib.DeviceArray(ctx, (a.points,)),
                       h=_lib.DeviceArray(ctx, (RB, N + 1, 3)), J=_lib.DeviceArray(ctx, (RB, N + 1, 10, 3)),
                       sw=[_lib.DeviceArray(ctx, (a.chords,)) for _ in range(3)] + [_lib.DeviceArray(ctx, (a.chords,), np.int32)])
               for k in scenes}
        launch = dict(
            render=lambda k: scenes[k].render(dP, dR, cfg, out=out[k]["img"], t=T),
            dist=lambda k: _lib.scene_distance_at(ctx, scenes[k].h, dpts, None, times, a.points, out[k]["dist"]),
            rows=lambda k: _lib.scene_sdf_rows(ctx, scenes[k].h, RB, N, NP, dx, dp, out[k]["h"], out[k]["J"], max_df, t0=T, tau=tau),
            swept=lambda k: _lib.scene_swept_distance(ctx, scenes[k].h, d0, d1, None, dc0, dc1, a.chords, 1e-3, a.max_evals,
                                                      *out[k]["sw"]))
        row = dict(triangles=int(mesh.tris.shape[0]))
        for q in ("render", "dist", "rows", "swept"):
            for k in names[q]:
                row[f"{q}_{k}_ms"], row[f"{q}_{k}_spread_ms"] = each_ms(ctx, names[q][k], lambda: launch[q](k), a.reps)
            if q != "swept":
                row[f"{q}_composition_ms"] = row[f"{q}_mesh_ms"] + row[f"{q}_dyn_ms"] + comb[q]
                row[f"{q}_composition_spread_ms"] = row[f"{q}_mesh_spread_ms"] + row[f"{q}_dyn_spread_ms"]
        img = {k: out[k]["img"].numpy() for k in scenes}
        d = {k: out[k]["dist"].numpy() for k in scenes}
        hh = {k: out[k]["h"].numpy()[..., 2] for k in scenes}
        JJ = {k: out[k]["J"].numpy()[..., 2] for k in scenes}
        lower = hh["dyn"] < hh["mesh"]
        assert (np.array_equal(img["mixed"], np.minimum(img["mesh"], img["dyn"])) and
                np.array_equal(d["mixed"], np.minimum(d["mesh"], d["dyn"])) and
                np.array_equal(hh["mixed"], np.where(lower, hh["dyn"], hh["mesh"])) and
                np.array_equal(JJ["mixed"], np.where(lower[..., None], JJ["dyn"], JJ["mesh"]))), \
            f"{kind}: the mesh-with-movers kernels and the composition differ"
        row.update(bitwise_equal=True, pixels_from_movers=float((img["dyn"] < img["mesh"]).mean()),
                   points_from_movers=float((d["dyn"] < d["mesh"]).mean()), rows_from_movers=float(lower.mean()),
                   rows_near=float((hh["mixed"] < max_df).mean()),
                   swept_evals_mixed=float(out["mixed"]["sw"][3].numpy().mean()), swept_evals_mesh=float(out["mesh"]["sw"][3].numpy().mean()))
        for s in scenes.values():
            s.close()
        res["scenes"][kind] = row
        print(f"{kind}: {row['triangles']} triangles")
        for q in ("render", "dist", "rows"):
            g = lambda k: f"{row[f'{q}_{k}_ms']:.4f} ({row[f'{q}_{k}_spread_ms']:.4f})"
            over = row[f"{q}_mixed_ms"] - row[f"{q}_composition_ms"]
            verdict = "within" if over <= row[f"{q}_composition_spread_ms"] else f"ABOVE the composition by {over:.4f} ms, beyond"
            print(f"  {q:>6}: mixed {g('mixed'):>18}   composition {row[f'{q}_composition_ms']:.4f} = mesh {g('mesh')} + dyn {g('dyn')} + "
                  f"pass {comb[q]:.4f}   ratio {row[f'{q}_mixed_ms'] / row[f'{q}_composition_ms']:.2f}: {verdict} its max - min "
                  f"{row[f'{q}_composition_spread_ms']:.4f}")
        print(f"   swept: mixed {row['swept_mixed_ms']:.4f} ({row['swept_mixed_spread_ms']:.4f}), {row['swept_evals_mixed']:.1f} evaluations "
              f"per chord; scene_swept_mesh on the mesh alone {row['swept_mesh_ms']:.4f} ({row['swept_mesh_spread_ms']:.4f}), "
              f"{row['swept_evals_mesh']:.1f} evaluations")
        print(f"  bitwise equal; a mover is the nearest thing in {100 * row['pixels_from_movers']:.1f} % of the pixels, "
              f"{100 * row['points_from_movers']:.1f} % of the points and {100 * row['rows_from_movers']:.1f} % of the rows "
              f"({100 * row['rows_near']:.0f} % of the rows are within max_df)")
    ctx.enable_timing(False)
    path = a.out or os.path.join(ROOT, "profiles", "mesh_mixed_probe.json")
    os.makedirs(os.path.dirname(path), exist_ok=True)
    allres = {}
    if os.path.exists(path):
        with open(path) as f:
            allres = json.load(f)
    allres[f"movers_{m}"] = res
    with open(path, "w") as f:
        json.dump(allres, f, indent=1)
        f.write("\n")
    print(json.dumps(res))


def tree():
    """a trunk and a crown, both closed: 64 + 1280 triangles"""
    return Mesh.merge(Mesh.cylinder((0.0, 0.0), 0.15, -1.5, 0.5, 16), Mesh.icosphere((0.0, 0.0, 1.0), 0.8, 3))


def inst_main(a):
    import torch
    n, N, RB, NP, T, max_df = a.instances, 40, 128, 17, 0.7, 1.0
    cfg = Config(mpc__N=N)
    h, w = (int(v) for v in cfg.sensor.shape_imgs[-2:])
    ctx = _lib.Context(0, stream=torch.cuda.current_stream().cuda_stream)
    ctx.enable_timing(True)
    part = tree()
    ntri = int(part.tris.shape[0])
    half = 2.0 * np.sqrt(n)  # a quarter of a tree per square metre
    lo, hi = (-half, -half, 0.0), (half, half, 0.0)
    rng = np.random.default_rng(2)
    cam = np.column_stack([rng.uniform(-0.5 * half, 0.5 * half, (a.B, 2)), rng.uniform(-0.5, 0.5, a.B)])
    yaw = rng.uniform(-np.pi, np.pi, a.B)
    R = np.stack([[[np.cos(y), -np.sin(y), 0], [np.sin(y), np.cos(y), 0], [0, 0, 1.0]] for y in yaw])
    pts = np.column_stack([rng.uniform(-half, half, (a.points, 2)), rng.uniform(-1.5, 2.0, a.points)])
    e = rng.normal(0, 1, (a.chords, 3))
    p0 = pts[:a.chords]
    p1 = p0 + e / np.linalg.norm(e, axis=1, keepdims=True) * rng.uniform(0.5, 1.5, (a.chords, 1))
    x = rng.normal(0, 1, (RB, N + 1, 10))
    x[..., :3] = pts[rng.integers(0, a.points, RB)][:, None, :] + 0.075 * np.arange(N + 1)[None, :, None] * np.array([1.0, 0.0, 0.0])
    dv = lambda v, dt=np.float64: _lib.DeviceArray.from_numpy(ctx, np.ascontiguousarray(v, dtype=dt))
    tau = dv(0.05 * np.arange(N + 1))
    names = dict(inst=("scene_render_inst", "scene_dist_inst", "scene_sdf_rows_inst", "scene_swept_inst"),
                 mesh=("scene_render_mesh", "scene_dist_mesh", "scene_sdf_rows_mesh", "scene_swept_mesh"))

    def four(scene, kind, rep_q=1, scene_of=None):
        """the four queries of `scene`, every array repeated rep_q times (scene k of a set of rep_q takes the k-th copy)
        -> times (mean, max - min) and results"""
        tile = lambda v: np.tile(v, (rep_q,) + (1,) * (np.ndim(v) - 1))
        dP, dR, dpts, d0, d1 = dv(tile(cam)), dv(tile(R.reshape(-1, 9))), dv(tile(pts)), dv(tile(p0)), dv(tile(p1))
        nB, npts, nch, nRB = a.B * rep_q, a.points * rep_q, a.chords * rep_q, RB * rep_q
        so = None if scene_of is None else dv(np.repeat(np.arange(rep_q), a.B), np.int32)
        sor = None if scene_of is None else dv(np.repeat(np.arange(rep_q), RB), np.int32)
        times, c0, c1 = dv(np.full(npts, T)), dv(np.full(nch, T)), dv(np.full(nch, T + 0.1))
        dx, dp = dv(tile(x)), dv(np.ones((nRB, N + 1, NP)))
        img, dist = _lib.DeviceArray(ctx, (nB, h, w), np.float32), _lib.DeviceArray(ctx, (npts,))
        hh, JJ = _lib.DeviceArray(ctx, (nRB, N + 1, 3)), _lib.DeviceArray(ctx, (nRB, N + 1, 10, 3))
        sw = [_lib.DeviceArray(ctx, (nch,)) for _ in range(3)] + [_lib.DeviceArray(ctx, (nch,), np.int32)]
        o = Scene.img_opts(cfg)
        launch = (lambda: _lib.scene_render_at(ctx, scene.h, so, o, h, w, 1.0, nB, dP, dR, T, img),
                  lambda: _lib.scene_distance_at(ctx, scene.h, dpts, None, times, npts, dist),
                  lambda: _lib.scene_sdf_rows(ctx, scene.h, nRB, N, NP, dx, dp, hh, JJ, max_df, scene_of=sor, t0=T, tau=tau),
                  lambda: _lib.scene_swept_distance(ctx, scene.h, d0, d1, None, c0, c1, nch, 1e-3, a.max_evals, *sw))
        ms = {q: each_ms(ctx, nm, fn, a.reps) for q, nm, fn in zip(("render", "dist", "rows", "swept"), names[kind], launch)}
        return ms, dict(img=img.numpy(), dist=dist.numpy(), h=hh.numpy()[..., 2], J=JJ.numpy()[..., 2], dmin=sw[0].numpy(),
                        evals=sw[3].numpy())

    def line(label, ms, extra=""):
        print(f"  {label:34s}" + "  ".join(f"{q} {ms[q][0]:9.4f} ({ms[q][1]:.4f})" for q in ("render", "dist", "rows", "swept")) + extra)

    res = dict(instances=n, part_triangles=ntri, B=a.B, shape=[h, w], points=a.points, rows=RB * (N + 1), chords=a.chords,
               max_evals=a.max_evals, reps=a.reps, t=T, max_df=max_df, field_half_m=half)
    print(f"{n} instances of a part of {ntri} triangles in a field of {2 * half:.0f} m; {a.B} images of {h} x {w}, {a.points} points, "
          f"{RB * (N + 1)} rows, {a.chords} chords; mean (max - min) of {a.reps} launches [ms]")
    # ---- static: instanced against welded
    static = Scene.scatter(n, lo, hi, parts=1, seed=1, keep_clear=((0.0, 0.0), 1.0))
    placed = []
    for _, _, pos, m in static:
        q0, _, _, q3 = m["q"]
        c, s_ = q0 * q0 - q3 * q3, 2.0 * q0 * q3
        placed.append(part.transformed(R=[[c, -s_, 0.0], [s_, c, 0.0], [0.0, 0.0, 1.0]], t=pos))
    sc_i = Scene.instanced(ctx, part, static, sdf_source=True)
    sc_w = Scene.mesh(ctx, Mesh.merge(*placed), sdf_source=True)
    ms_i, r_i = four(sc_i, "inst")
    ms_w, r_w = four(sc_w, "mesh")
    sc_c = Scene.instanced(ctx, part, static, closed=True, sdf_source=True)
    ms_c, _ = four(sc_c, "inst")
    quarter = Scene.instanced(ctx, part, static[:max(n // 4, 1)], sdf_source=True)
    ms_q, _ = four(quarter, "inst")
    for s_ in (sc_i, sc_w, sc_c, quarter):
        s_.close()
    tri_b = 64 + 80  # MeshTriF + MeshTriD per triangle of an open set (a closed one adds 168)
    bytes_w, bytes_i = n * ntri * tri_b, ntri * tri_b + n * 200
    agree = dict(img=float(np.abs(r_i["img"] - r_w["img"]).max()), img_differ_share=float((np.abs(r_i["img"] - r_w["img"]) > 1e-4).mean()),
                 dist=float(np.abs(r_i["dist"] - r_w["dist"]).max()), h=float(np.abs(r_i["h"] - r_w["h"]).max()),
                 dmin=float(np.abs(r_i["dmin"] - r_w["dmin"]).max()))
    assert agree["dist"] <= 1e-5 and agree["h"] <= 1e-5 and agree["dmin"] <= 2e-3 and agree["img_differ_share"] <= 0.05, agree
    res["static"] = dict(instanced_ms=ms_i, welded_ms=ms_w, instanced_closed_ms=ms_c, instanced_quarter_ms=ms_q,
                         triangle_bytes_welded=bytes_w, triangle_bytes_instanced=bytes_i, max_abs_difference=agree,
                         hit_share=float((r_i["img"] < float(cfg.sensor.dmax)).mean()), rows_near=float((r_i["h"] < max_df).mean()),
                         swept_evals_instanced=float(r_i["evals"].mean()), swept_evals_welded=float(r_w["evals"].mean()))
    print(f"static, open: triangle arrays {bytes_w / 1e6:.2f} MB welded, {bytes_i / 1e6:.3f} MB instanced; largest difference "
          f"distance {agree['dist']:.1e} m, rows {agree['h']:.1e}, swept dmin {agree['dmin']:.1e}, image {agree['img']:.1e} m "
          f"({100 * agree['img_differ_share']:.3f} % of the pixels beyond 1e-4: silhouettes); {100 * res['static']['hit_share']:.0f} % "
          f"of the pixels hit, {100 * res['static']['rows_near']:.0f} % of the rows within max_df")
    line(f"instanced, {n}", ms_i, f"  ({res['static']['swept_evals_instanced']:.1f} evaluations per chord)")
    line("welded mesh", ms_w, f"  ({res['static']['swept_evals_welded']:.1f})")
    line(f"instanced, closed, {n}", ms_c)
    line(f"instanced, {max(n // 4, 1)}", ms_q)
    # ---- moving: instanced against n single-instance scenes and a combining pass
    rngm = np.random.default_rng(3)
    moving = [Scene.instance(0, pos, q=m["q"], v=tuple(rngm.uniform(-0.5, 0.5, 2)) + (0.0,), yaw_rate=rngm.uniform(-0.5, 0.5))
              for _, _, pos, m in static]
    sc_m = Scene.instanced(ctx, part, moving, sdf_source=True)
    ms_m, r_m = four(sc_m, "inst")
    sc_m.close()
    singles = Scene.instanced(ctx, part, [[i] for i in moving], sdf_source=True)
    ms_s, r_s = four(singles, "inst", rep_q=n, scene_of=True)
    singles.close()
    dev = torch.device("cuda:0")
    ti = torch.rand(n, a.B, h, w, device=dev)
    td = torch.rand(n, a.points, device=dev, dtype=torch.float64)
    th, tJ = torch.rand(n, RB * (N + 1), device=dev, dtype=torch.float64), torch.rand(n, RB * (N + 1), 3, device=dev, dtype=torch.float64)

    def rows_min():
        k = th.argmin(0)
        return th.gather(0, k[None])[0], tJ.gather(0, k[None, :, None].expand(1, -1, 3))[0]

    comb = dict(render=torch_ms(lambda: ti.amin(0), a.reps), dist=torch_ms(lambda: td.amin(0), a.reps), rows=torch_ms(rows_min, a.reps),
                swept=torch_ms(lambda: td[:, :a.chords].amin(0), a.reps))
    each = r_s["h"].reshape(n, RB, N + 1)
    k = each.argmin(0)  # the first of equal values: the lowest index keeps a tie
    assert (np.array_equal(r_m["img"], r_s["img"].reshape(n, a.B, h, w).min(0)) and
            np.array_equal(r_m["dist"], r_s["dist"].reshape(n, -1).min(0)) and
            np.array_equal(r_m["h"], np.take_along_axis(each, k[None], 0)[0]) and
            np.array_equal(r_m["J"], np.take_along_axis(r_s["J"].reshape(n, RB, N + 1, 10), k[None, ..., None], 0)[0])), \
        "the instanced kernels and the composition of single-instance scenes differ"
    res["moving"] = dict(instanced_ms=ms_m, singles_ms=ms_s, combine_pass_ms=comb, bitwise_equal=True,
                         swept_evals_instanced=float(r_m["evals"].mean()))
    print(f"moving, open: bitwise equal to the minimum over {n} single-instance scenes; one combining pass: " +
          ", ".join(f"{q} {comb[q]:.4f}" for q in comb) + " ms")
    line(f"instanced, {n}", ms_m, f"  ({res['moving']['swept_evals_instanced']:.1f} evaluations per chord)")
    line(f"{n} single-instance scenes", ms_s)
    per = {q: 1e6 * ms_i[q][0] / (n * cnt) for q, cnt in (("render", a.B * h * w), ("dist", a.points), ("rows", RB * (N + 1)))}
    res["per_instance_ns"] = per
    print("static, per instance and query [ns]: " + ", ".join(f"{q} {v:.3f}" for q, v in per.items()))
    ctx.enable_timing(False)
    path = a.out or os.path.join(ROOT, "profiles", "mesh_inst_probe.json")
    os.makedirs(os.path.dirname(path), exist_ok=True)
    allres = {}
    if os.path.exists(path):
        with open(path) as f:
            allres = json.load(f)
    allres[f"instances_{n}"] = res
    with open(path, "w") as f:
        json.dump(allres, f, indent=1)
        f.write("\n")
    print(json.dumps(res))


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
    ap.add_argument("--sdf", action="store_true", help="the mesh as the controller's SDF source: scene_sdf_rows_mesh")
    ap.add_argument("--movers", type=int, default=None, help="movers beside the mesh: the four *_mesh_mixed kernels")
    ap.add_argument("--instances", type=int, default=None, help="instances of one part: the four *_inst kernels (1..256)")
    ap.add_argument("--out", default=None, help="--sdf, --movers, --instances: where the JSON goes (profiles/mesh_sdf_probe.json, "
                                                "profiles/mesh_mixed_probe.json, profiles/mesh_inst_probe.json)")
    a = ap.parse_args()
    warnings.filterwarnings("ignore")
    if a.sdf:
        return sdf_main(a)
    if a.movers is not None:
        return movers_main(a)
    if a.instances is not None:
        return inst_main(a)
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
