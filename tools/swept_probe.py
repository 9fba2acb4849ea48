"""What does the clearance between the log rows cost, and what does it find?  Rollouts of --B instances, --K steps, in a
forest of --n cylinders (Scene.forest, grid index) and in the same forest with --movers moving cylinders beside it
(Scene.crowd, in a box of --crowd-half metres to either side of the origin, where the flights are), flown on the
scene's exact distance (Nmpc.set_sdf_scene; with movers predict=True) with swept=True.  Per scene it prints

  * the HIP-event time of the swept launch over the log's B K chords beside the clearance launch over its B (K + 1)
    rows, both from device arrays (mean and spread of --reps launches);
  * the distribution of the distance evaluations per chord (the clearance launch makes one per row), and the largest gap;
  * the number of chords with swept_clearance < robot.size.xy while both end rows are at or above it: contacts that the
    rows alone do not show.

The weights are synthetic: the numbers say what the query costs and how often the rows miss a contact on such paths,
nothing about the controller.  The last line is the JSON of everything printed."""
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
from sdf_nmpc_amd.scene import Scene
from large_scene_probe import Z, each_ms, forest
from rollout_probe import controller


def probe(cfg, a, movers):
    B, K = a.B, a.K
    n, x0, wps = controller(cfg, B, seed=3)
    ctx = n.ocp.ctx
    prims, half = forest(a.n, a.density)
    # the movers swing inside the box the flights stay in (starts in [-1, 1]^3, waypoints within 3 m of them), not
    # over the whole forest, so that they cross the paths
    ch = min(a.crowd_half, half)
    crowd = Scene.crowd(movers, (-ch, -ch, Z[0]), (ch, ch, Z[1]), seed=1) if movers else None
    scene = Scene(ctx, prims, grid=True, movers=crowd)
    n.set_sdf_scene(scene, predict=bool(movers))
    n.set_x0(x0)
    r = n.rollout(K, refs="wps", wps=wps, swept=True)
    # the two launches over the same log, from device arrays
    rows = _lib.DeviceArray.from_numpy(ctx, np.ascontiguousarray(r.x[:, :, :3]).reshape(-1, 3))
    times = _lib.DeviceArray.from_numpy(ctx, np.tile(r.t, B))
    p0 = _lib.DeviceArray.from_numpy(ctx, np.ascontiguousarray(r.x[:, :-1, :3]).reshape(-1, 3))
    p1 = _lib.DeviceArray.from_numpy(ctx, np.ascontiguousarray(r.x[:, 1:, :3]).reshape(-1, 3))
    t0, t1 = (_lib.DeviceArray.from_numpy(ctx, np.tile(t, B)) for t in (r.t[:-1], r.t[1:]))
    dist = _lib.DeviceArray(ctx, (B * (K + 1),))
    dmin, s, gap = (_lib.DeviceArray(ctx, (B * K,)) for _ in range(3))
    evals = _lib.DeviceArray(ctx, (B * K,), np.int32)
    suffix = "_mixed" if movers else "_grid"
    ctx.enable_timing(True)
    c_ms, c_sp = each_ms(ctx, "scene_dist" + suffix,
                         lambda: _lib.scene_distance_at(ctx, scene.h, rows, None, times, B * (K + 1), dist), a.reps)
    s_ms, s_sp = each_ms(ctx, "scene_swept" + suffix,
                         lambda: _lib.scene_swept_distance(ctx, scene.h, p0, p1, None, t0, t1, B * K, 1e-3, 4096, dmin, s,
                                                           gap, evals), a.reps)
    ctx.enable_timing(False)
    assert np.array_equal(dmin.numpy().reshape(B, K), r.swept_clearance) and np.array_equal(dist.numpy().reshape(B, K + 1), r.clearance)
    ev, size = evals.numpy(), float(cfg.robot.size.xy)
    ends = np.minimum(r.clearance[:, :-1], r.clearance[:, 1:])
    missed = (r.swept_clearance < size) & (ends >= size)
    step = np.linalg.norm(np.diff(r.x[:, :, :3], axis=1), axis=2)
    res = dict(primitives=a.n, movers=movers, speed_bound=float(scene.speed_bound[0]), chords=B * K, clearance_ms=c_ms,
               clearance_spread_ms=c_sp, swept_ms=s_ms, swept_spread_ms=s_sp,
               evals=dict(mean=float(ev.mean()), p50=float(np.percentile(ev, 50)), p90=float(np.percentile(ev, 90)),
                          p99=float(np.percentile(ev, 99)), max=int(ev.max())),
               gap_max=float(r.swept_gap.max()), chord_p50=float(np.median(step)), chord_max=float(step.max()),
               rows_below_size=int((r.clearance < size).sum()), chords_below_size=int((r.swept_clearance < size).sum()),
               chords_below_size_with_both_rows_clear=int(missed.sum()),
               largest_dip_below_rows=float((ends - r.swept_clearance).max()), converged=float((r.status == 0).mean()))
    e = res["evals"]
    print(f"{a.n} cylinders, {movers} movers (V = {res['speed_bound']:.2f} m/s), {B} x {K} chords of median {res['chord_p50']:.3f} m "
          f"(longest {res['chord_max']:.3f} m); {100 * res['converged']:.1f} % of the QPs converged")
    print(f"  clearance launch over {B * (K + 1)} rows {c_ms:.4f} ms (spread {c_sp:.4f}); swept launch over {B * K} chords "
          f"{s_ms:.4f} ms (spread {s_sp:.4f}): {s_ms / c_ms:.1f} x")
    print(f"  evaluations per chord: mean {e['mean']:.1f}, p50 {e['p50']:.0f}, p90 {e['p90']:.0f}, p99 {e['p99']:.0f}, max {e['max']}; "
          f"largest gap {res['gap_max']:.2e} m")
    print(f"  below robot.size.xy = {size} m: {res['rows_below_size']} rows, {res['chords_below_size']} chords, of which "
          f"{res['chords_below_size_with_both_rows_clear']} with both end rows at or above it; the largest dip of a chord below its "
          f"rows {res['largest_dip_below_rows']:.4f} m")
    scene.close()
    n.ocp.close()
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--B", type=int, default=1024)
    ap.add_argument("--N", type=int, default=20)
    ap.add_argument("--K", type=int, default=50)
    ap.add_argument("--n", type=int, default=1024)
    ap.add_argument("--movers", type=int, default=16)
    ap.add_argument("--density", type=float, default=0.25)
    ap.add_argument("--crowd-half", type=float, default=5.0, help="the movers' box is +-this many metres in x and y")
    ap.add_argument("--reps", type=int, default=5)
    a = ap.parse_args()
    warnings.filterwarnings("ignore")
    cfg = Config(mpc__N=a.N)
    print(json.dumps(dict(B=a.B, N=a.N, K=a.K, scenes=[probe(cfg, a, 0), probe(cfg, a, a.movers)])))


if __name__ == "__main__":
    main()
