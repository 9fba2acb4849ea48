"""What does perceiving inside the device loop buy?  The same K-step closed loop with a new image of an analytic
scene every `--every`-th step, run two ways on one controller configuration: as Nmpc.rollout(scene=, vae=) (one
launch sequence, one wait), and as the host-driven loop built from the public pieces (render_from_state -> set_img ->
encode_to -> set_x0 -> gen_refs_device -> solve -> plant_step -> download the state).  Both use the same kernels, so
the loops compute the same bits (checked) and the difference is the host's.  Also the three scene kernels' own times
(HIP events): scene_render at 270 x 480 with 16 primitives next to its floors, scene_pose, scene_dist -- and the
dynamic kernels on the same scene with every primitive moving, from the same run.  --moving gives the loops' scene
those motions (the host-driven loop renders at t = k * dt, the device loop runs the scene's clock);
--kernels-only skips the loops.  --sensor runs the loops under the reference's training augmentation as a sensor model
(SensorModel.reference_augment with the outlier removal behind it): the device loop against the host-driven loop that
calls SensorModel.apply between the render and the encoder (same bits, checked), the distribution of the minimum
clearance over the batch with and without the sensor model, and per launch the sensor stage's kernels next to
scene_render and the encoder's from one timed rollout, plus the general morphology kernel with the radius-10 disc.
--vehicle runs the device loop with and without a vehicle model of moderate size (rollout_probe.VEHICLE: two periods of
input delay, thrust lag, rotor drag, gusts, noise on the state estimate) and prints the distribution of the minimum
clearance of the true vehicle over the batch for both, and the rollout's ms per step.  --vehicle --body adds the same
model as a rigid body (rollout_probe.BODY: attitude and rate loop, rotor lag and limits instead of the thrust lag) at
16 plant substeps.  With synthetic network weights the distributions compare vehicles, not controllers.

One configuration per run (give every run its own time limit):
    timeout 600 python tools/perceive_probe.py --B 1024 --N 40 --every 1
    timeout 600 python tools/perceive_probe.py --B 1024 --N 40 --every 5
    timeout 200 python tools/perceive_probe.py --B 1 --N 40 --every 1
    timeout 600 python tools/perceive_probe.py --B 256 --N 40 --every 1 --sensor
    timeout 600 python tools/perceive_probe.py --B 256 --N 40 --every 1 --vehicle
    timeout 600 python tools/perceive_probe.py --B 256 --N 40 --every 1 --vehicle --body
Prints ms per control step of both loops (best of --reps repetitions after a warm-up) and a JSON line.  Diagnostic."""
import argparse
import json
import os
import sys
import time
import warnings

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from sdf_nmpc_amd import _lib
from sdf_nmpc_amd.config import Config
from sdf_nmpc_amd.scene import Scene
from sdf_nmpc_amd.sensor import SensorModel
from sdf_nmpc_amd.vae import VaeWrapper
from sdf_nmpc_amd.vehicle import VehicleModel
from rollout_probe import BODY_SUBSTEPS, VEHICLE, body_vehicle, controller

# vector instructions executed per ray-primitive test, from the loop body in the -save-temps assembly: 38 (box), 39
# (sphere), 51 (cylinder); the probe's forest is one box, ten cylinders and five spheres
INSTR_PER_TEST = (38 + 10 * 51 + 5 * 39) / 16
LANE_INSTR_PER_S = 39e12  # 256 CUs x 4 SIMDs x 16 lanes x 2.4 GHz: one wave per SIMD
LANE_INSTR_PER_S_2 = 2 * LANE_INSTR_PER_S  # two or more waves per SIMD: a wave64 instruction issues in 2 cycles, not 4
HBM_BYTES_PER_S = 8e12


def forest(n_prims, seed=3):
    """A floor and n_prims - 1 pillars and balls ahead of the start box of rollout_probe.controller."""
    rng = np.random.default_rng(seed)
    prims = [Scene.box((-20, -20, -2.1), (20, 20, -2.0))]
    while len(prims) < n_prims:
        c = rng.uniform([2.0, -4.0], [7.0, 4.0])
        prims.append(Scene.cylinder(c, rng.uniform(0.15, 0.4), -2.0, 2.5) if len(prims) % 3 else
                     Scene.sphere((c[0], c[1], rng.uniform(-1, 1)), rng.uniform(0.2, 0.5)))
    return prims


def moving_forest(n_prims, seed=3):
    """The forest with every primitive moving: the floor slides, the pillars lean, drift and turn, the balls drift and
    bob."""
    rng = np.random.default_rng(seed + 100)
    prims = forest(n_prims, seed)
    out = [Scene.moving(prims[0], v=(0.1, 0.05, 0.0))]
    for p in prims[1:]:
        out.append(Scene.moving(p, v=(*rng.uniform(-0.3, 0.3, 2), 0.0), rpy=(*rng.uniform(-0.3, 0.3, 2), 0.0),
                                yaw_rate=rng.uniform(-0.5, 0.5), amp=(0.0, 0.0, rng.uniform(0.0, 0.3)), omega=1.5,
                                phase=rng.uniform(0.0, 6.0)))
    return out


def host_loop(n, vae, scene, x0, wps, K, every, plant, sensor=None):
    B, ctx = max(n.B, 1), n.ocp.ctx
    dx = _lib.DeviceArray(ctx, (B, 10))
    x, xs = np.reshape(x0, (B, 10)).copy(), []
    sq = (lambda a: a) if n.B > 1 else (lambda a: a[0])
    for k in range(K):
        n.set_x0(sq(x))
        if k % every == 0:
            img = scene.render_from_state(x, n.cfg, normalized=False, t=0.0 + k * plant.dt)
            if sensor is not None:
                sensor.apply(img, frame=k, normalized=False)
            vae.set_img(img)
            vae.encode_to(n, img.pose["W_p_Bo"], img.pose["W_R_Bo"])
        n.gen_refs_device("wps", wps=wps)
        n.solve()
        dx.upload(x)
        _lib.plant_step(ctx, plant, B, dx, n.ocp.field("u0"), dx)
        x = dx.numpy()
        xs.append(x)
    return np.stack(xs, 1)


def kernel_times(ctx, cfg, B, res):
    """HIP events around each launch of the scene kernels (16 primitives, the sensor's 270 x 480 image): the static
    ones on the static forest, the dynamic ones on the same forest with every primitive moving."""
    scene, dyn = Scene(ctx, forest(16)), Scene(ctx, moving_forest(16))
    rng = np.random.default_rng(0)
    x = np.zeros((B, 10))
    x[:, :3] = rng.uniform(-1, 1, (B, 3))
    x[:, 3] = 1.0
    x[:, 6] = rng.uniform(-0.3, 0.3, B)
    dx = _lib.DeviceArray.from_numpy(ctx, x)
    h, w = (int(v) for v in cfg.sensor.shape_imgs[-2:])
    out = _lib.DeviceArray(ctx, (B, h, w), np.float32)
    ps = scene.pose(dx, cfg)
    pts = _lib.DeviceArray.from_numpy(ctx, np.tile(x[:, None, :3], (1, 51, 1)).reshape(-1, 3))
    dist = _lib.DeviceArray(ctx, (B * 51,))
    times = _lib.DeviceArray.from_numpy(ctx, np.tile(np.arange(51) * 0.05, B))
    calls = {"scene_render": lambda: scene.render(ps["W_p_C"], ps["W_R_C"], cfg, out=out),
             "scene_pose": lambda: _lib.scene_pose(ctx, cfg.sensor.B_p_C, cfg.sensor.B_R_C, B, dx, *ps.values()),
             "scene_dist": lambda: _lib.scene_distance(ctx, scene.h, pts, None, B * 51, dist),
             "scene_render_dyn": lambda: dyn.render(ps["W_p_C"], ps["W_R_C"], cfg, out=out, t=1.3),
             "scene_dist_dyn": lambda: _lib.scene_distance_at(ctx, dyn.h, pts, None, times, B * 51, dist)}
    for name, fn in calls.items():
        for _ in range(5):
            fn()
        ctx.synchronize()
        ctx.reset_stats()
        ctx.enable_timing(True)
        for _ in range(20):
            fn()
        ms, cnt = ctx.kernel_stats(name)
        ctx.enable_timing(False)
        ctx.reset_stats()
        res[f"{name}_us"] = ms / cnt * 1e3
    rays = B * h * w
    res["render_rays"] = rays
    res["render_floor_store_us"] = rays * 4 / HBM_BYTES_PER_S * 1e6
    res["render_floor_valu_us"] = rays * 16 * INSTR_PER_TEST / LANE_INSTR_PER_S * 1e6
    res["render_floor_valu_2cycle_us"] = rays * 16 * INSTR_PER_TEST / LANE_INSTR_PER_S_2 * 1e6
    res["render_dyn_over_static"] = res["scene_render_dyn_us"] / res["scene_render_us"]
    res["render_dyn_hit_share"] = float((out.numpy() < 1.0).mean())  # the last launches wrote the moving forest
    scene.render(ps["W_p_C"], ps["W_R_C"], cfg, out=out)
    res["render_hit_share"] = float((out.numpy() < 1.0).mean())


def sensor_probe(cfg, a, res):
    """The loops under a degraded camera, the clearance it costs, and the sensor stage's own time."""
    from sdf_nmpc_amd import preprocessing
    make = lambda ctx: SensorModel.reference_augment(cfg, ctx, 2024, outlier_rm=True, miss_invalid=True)
    runs = {}
    for name in ("sensor", "clean", "host"):
        n, x0, wps = controller(cfg, a.B, 1)
        ctx = n.ocp.ctx
        scene, vae = Scene(ctx, forest(16)), VaeWrapper(cfg, batch=a.B, ctx=ctx)
        plant = _lib.plant_opts(cfg, dt=float(n.ocp.dt[0]))
        if name == "host":
            runs[name] = host_loop(n, vae, scene, x0, wps, a.K, a.every, plant, sensor=make(ctx))
        else:
            n.set_x0(x0)
            if name == "sensor":
                ctx.enable_timing(True)
                ctx.reset_stats()
            runs[name] = n.rollout(a.K, refs="wps", wps=wps, plant=plant, scene=scene, vae=vae, perceive_every=a.every,
                                   sensor=make(ctx) if name == "sensor" else None)
            if name == "sensor":
                for k in ("scene_render", "sensor_degrade", "outlier_rm", "vae_pre", "vae_stem", "vae_conv", "vae_head"):
                    ms, cnt = ctx.kernel_stats(k)
                    res[f"{k}_us"], res[f"{k}_launches"] = ms / max(cnt, 1) * 1e3, cnt
                ctx.enable_timing(False)
                per = max(res["scene_render_launches"], 1)
                res["sensor_stage_us_per_perception"] = (res["sensor_degrade_us"] * res["sensor_degrade_launches"] +
                                                         res["outlier_rm_us"] * res["outlier_rm_launches"]) / per
                res["vae_encode_us_per_perception"] = sum(res[f"{k}_us"] * res[f"{k}_launches"] for k in
                                                          ("vae_pre", "vae_stem", "vae_conv", "vae_head")) / per
                # the general kernel with the reference's disc of radius 10 on the batch's images (Erode, ignore_zeros)
                h, w = (int(v) for v in cfg.sensor.shape_imgs[-2:])
                img = _lib.DeviceArray.from_numpy(ctx, np.random.default_rng(0).uniform(0, 1, (max(n.B, 1), h, w)).astype(np.float32))
                r = np.arange(-10, 11)
                er = preprocessing.Erode((r[:, None] ** 2 + r[None] ** 2 <= 100), True, ctx=ctx)
                er(img)
                ctx.reset_stats()
                ctx.enable_timing(True)
                for _ in range(5):
                    er(img)
                ms, cnt = ctx.kernel_stats("morph")
                ctx.enable_timing(False)
                res["morph_disc10_us"] = ms / cnt * 1e3
        vae.vae.close()
        n.ocp.close()
    res["same_bits"] = bool(np.array_equal(runs["sensor"].x[:, 1:], runs["host"]))
    q = (0, 5, 25, 50, 75, 95, 100)
    for name in ("sensor", "clean"):
        mc = runs[name].clearance.min(axis=1)
        res[f"min_clearance_{name}_percentiles"] = dict(zip(map(str, q), np.percentile(mc, q).round(4).tolist()))
        res[f"collided_{name}"] = int((mc < 0).sum())
    print(f"B={a.B} N={a.N} K={a.K} every={a.every} under reference_augment + outlier removal: device loop == host loop: "
          f"{res['same_bits']}; per perceiving step scene_render {res['scene_render_us']:.1f} us, sensor stage "
          f"{res['sensor_stage_us_per_perception']:.1f} us (sensor_degrade {res['sensor_degrade_us']:.1f} + outlier_rm "
          f"{res['outlier_rm_us']:.1f} + a copy), encoder {res['vae_encode_us_per_perception']:.1f} us; Erode with the "
          f"radius-10 disc {res['morph_disc10_us']:.1f} us")
    print("min clearance over the batch, percentiles", q)
    for name in ("clean", "sensor"):
        print(f"  {name:6s}", list(res[f"min_clearance_{name}_percentiles"].values()), "collided:", res[f"collided_{name}"])
    print(json.dumps(res))


def vehicle_probe(cfg, a, res):
    """The perceiving device loop under an imperfect vehicle and estimator, and the clearance it costs."""
    def run(name):
        n, x0, wps = controller(cfg, a.B, 1)
        ctx = n.ocp.ctx
        scene, vae = Scene(ctx, forest(16)), VaeWrapper(cfg, batch=a.B, ctx=ctx)
        plant = _lib.plant_opts(cfg, dt=float(n.ocp.dt[0]), substeps=BODY_SUBSTEPS[-1] if name == "body" else 1)
        m = VehicleModel(cfg, ctx, max(a.B, 1), seed=2024, **VEHICLE) if name == "vehicle" else None
        if name == "body":
            m = body_vehicle(cfg, ctx, max(a.B, 1), 2024)
        n.set_x0(x0)
        ctx.synchronize()
        t0 = time.perf_counter()
        r = n.rollout(a.K, refs="wps", wps=wps, plant=plant, scene=scene, vae=vae, perceive_every=a.every, vehicle=m)
        ms = (time.perf_counter() - t0) / a.K * 1e3
        if m is not None:
            m.close()
        vae.vae.close()
        n.ocp.close()
        return r, ms

    names = ("perfect", "vehicle", "body") if a.body else ("perfect", "vehicle")
    run(names[-1])  # warms up (workspaces, code objects) and is not timed
    runs = {}
    for name in names:
        runs[name], res[f"rollout_ms_per_step_{name}"] = run(name)
    q = (0, 5, 25, 50, 75, 95, 100)
    for name in names:
        mc = runs[name].clearance.min(axis=1)
        res[f"min_clearance_{name}_percentiles"] = dict(zip(map(str, q), np.percentile(mc, q).round(4).tolist()))
        res[f"collided_{name}"] = int((mc < 0).sum())
    err = runs["vehicle"].xhat - runs["vehicle"].x
    res["est_pos_err_std"] = float(err[..., :3].std())
    print(f"B={a.B} N={a.N} K={a.K} every={a.every} with the vehicle model {VEHICLE}: rollout "
          f"{res['rollout_ms_per_step_perfect']:.3f} ms/step without it, {res['rollout_ms_per_step_vehicle']:.3f} ms/step "
          f"with it; std of the position estimate's error {res['est_pos_err_std']:.4f} m")
    if a.body:
        print(f"as a rigid body ({BODY_SUBSTEPS[-1]} plant substeps): {res['rollout_ms_per_step_body']:.3f} ms/step; rotors within "
              f"{float(runs['body'].rotor.min()):.2f}..{float(runs['body'].rotor.max()):.2f}")
    print("min clearance of the true vehicle over the batch, percentiles", q)
    for name in names:
        print(f"  {name:8s}", list(res[f"min_clearance_{name}_percentiles"].values()), "collided:", res[f"collided_{name}"])
    print(json.dumps(res))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--B", type=int, default=1024)
    ap.add_argument("--N", type=int, default=40)
    ap.add_argument("--K", type=int, default=50)
    ap.add_argument("--every", type=int, default=1)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--moving", action="store_true", help="the loops' scene moves (moving_forest)")
    ap.add_argument("--kernels-only", action="store_true", help="only the scene kernels' own times")
    ap.add_argument("--sensor", action="store_true", help="the loops under SensorModel.reference_augment")
    ap.add_argument("--vehicle", action="store_true", help="the device loop with and without a vehicle model")
    ap.add_argument("--body", action="store_true", help="with --vehicle: also the model as a rigid body")
    a = ap.parse_args()
    if a.body and not a.vehicle:
        ap.error("--body goes with --vehicle")
    warnings.simplefilter("ignore")
    cfg = Config(mpc__N=a.N)
    res = {"B": a.B, "N": a.N, "K": a.K, "every": a.every, "moving": a.moving}
    if a.sensor:
        sensor_probe(cfg, a, res)
        return
    if a.vehicle:
        vehicle_probe(cfg, a, res)
        return
    if a.kernels_only:
        ctx = _lib.Context(0)
        kernel_times(ctx, cfg, a.B, res)
        print(f"B={a.B}: scene_render {res['scene_render_us']:.1f} us, scene_render_dyn {res['scene_render_dyn_us']:.1f} us "
              f"({res['render_dyn_over_static']:.2f}x), scene_dist {res['scene_dist_us']:.1f} us, scene_dist_dyn "
              f"{res['scene_dist_dyn_us']:.1f} us")
        print(json.dumps(res))
        return
    make_forest = moving_forest if a.moving else forest
    t_roll, t_host, xr, xh = [], [], None, None
    for rep in range(a.reps + 1):  # repetition 0 warms up (workspaces, code objects) and is not timed
        n, x0, wps = controller(cfg, a.B, 1)
        ctx = n.ocp.ctx
        scene, vae = Scene(ctx, make_forest(16)), VaeWrapper(cfg, batch=a.B, ctx=ctx)
        plant = _lib.plant_opts(cfg, dt=float(n.ocp.dt[0]))
        n.set_x0(x0)
        ctx.synchronize()
        t0 = time.perf_counter()
        r = n.rollout(a.K, refs="wps", wps=wps, plant=plant, scene=scene, vae=vae, perceive_every=a.every)
        t1 = time.perf_counter()
        vae.vae.close()
        n.ocp.close()
        n, x0, wps = controller(cfg, a.B, 1)
        ctx = n.ocp.ctx
        scene, vae = Scene(ctx, make_forest(16)), VaeWrapper(cfg, batch=a.B, ctx=ctx)
        plant = _lib.plant_opts(cfg, dt=float(n.ocp.dt[0]))
        ctx.synchronize()
        t2 = time.perf_counter()
        xh = host_loop(n, vae, scene, x0, wps, a.K, a.every, plant)
        t3 = time.perf_counter()
        xr = r.x[:, 1:]
        if rep:
            t_roll.append((t1 - t0) / a.K * 1e3)
            t_host.append((t3 - t2) / a.K * 1e3)
        vae.vae.close()
        if rep < a.reps:
            n.ocp.close()
    res["same_bits"] = bool(np.array_equal(xr, xh))
    res["rollout_ms_per_step"], res["host_loop_ms_per_step"] = min(t_roll), min(t_host)
    res["rollout_ms_all"], res["host_loop_ms_all"] = [round(t, 3) for t in t_roll], [round(t, 3) for t in t_host]  # the spread
    res["qp_iters_mean"] = float(r.iters.mean())
    res["min_clearance"] = float(r.clearance.min())
    kernel_times(n.ocp.ctx, cfg, max(n.B, 1), res)
    n.ocp.close()
    print(f"B={a.B} N={a.N} K={a.K} every={a.every}: rollout with perception {res['rollout_ms_per_step']:.3f} ms/step, "
          f"host-driven loop {res['host_loop_ms_per_step']:.3f} ms/step (same bits: {res['same_bits']}); scene_render "
          f"{res['scene_render_us']:.1f} us (floors: store {res['render_floor_store_us']:.1f} us, vector ALU "
          f"{res['render_floor_valu_us']:.1f} us at 39 T lane-instructions/s, {res['render_floor_valu_2cycle_us']:.1f} us "
          f"at twice that), scene_pose {res['scene_pose_us']:.1f} us, scene_dist "
          f"{res['scene_dist_us']:.1f} us; on the moving forest scene_render_dyn {res['scene_render_dyn_us']:.1f} us "
          f"({res['render_dyn_over_static']:.2f}x), scene_dist_dyn {res['scene_dist_dyn_us']:.1f} us")
    print(json.dumps(res))
    if res["rollout_ms_per_step"] > res["host_loop_ms_per_step"]:
        print("NOTE: the rollout was not faster than the host-driven loop in this run")


if __name__ == "__main__":
    main()
