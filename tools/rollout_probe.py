"""What does keeping a closed loop on the device buy?  The same K-step loop -- references from the plant state
(waypoint mode), shift, one SQP-RTI iteration, the plant advanced by u_0 -- run two ways on one controller
configuration: as Nmpc.rollout (one launch sequence, one wait), and as the host-driven loop a user writes without
it (set_x0 -> gen_refs_device -> solve -> plant_step -> download the state), which pays two synchronisations and
three copies per step.  Both use the plant kernel, so the loops compute the same bits (checked) and the difference
is the host's.  Also the plant kernel's own time (HIP events) at substeps 1 and 10.  With --vehicle: the same for
the vehicle model's kernel ("plant_vehicle": delay, thrust lag, drag, gusts, estimate noise all on) beside "plant",
and the rollout's ms per step with and without the model.  With --vehicle --body: the rigid-body kernel
("plant_vehicle_body": the same model with a RigidBody instead of the thrust lag) beside "plant_vehicle" at 8 and 16
substeps, the rollout's ms per step with it (16 substeps), and the kernel's share of that step.

One configuration per run (give every run its own time limit):
    timeout 300 python tools/rollout_probe.py --B 1024 --N 40      # C3
    timeout 120 python tools/rollout_probe.py --B 1 --N 40
    timeout 300 python tools/rollout_probe.py --B 1024 --N 40 --vehicle
    timeout 300 python tools/rollout_probe.py --B 1024 --N 40 --vehicle --body
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
from sdf_nmpc_amd.controller import Nmpc
from sdf_nmpc_amd.reference import yaw2quat
from sdf_nmpc_amd.vehicle import RigidBody, VehicleModel

# a model of moderate size with every term on: what the "plant_vehicle" figures are measured under
VEHICLE = dict(delay=2, thrust_tau=0.05, drag=(0.3, 0.3, 0.1), gust_std=0.5, gust_tau=1.0, est_std_pos=0.03,
               est_std_vel=0.05, est_std_yaw=0.01)
# the reference's default.yaml robot.* (mass, inertia, alloc, limits.wp) under RigidBody's default inner loop
BODY = dict(mass=1.46, inertia=(0.017, 0.018, 0.028), cf=0.02246, ct=0.00020673, wp_max=25.0,
            motors=[[0.09, -0.09, -0.005, 0, 0, -1], [-0.09, 0.09, -0.005, 0, 0, -1], [0.09, 0.09, -0.005, 0, 0, 1],
                    [-0.09, -0.09, -0.005, 0, 0, 1]])
BODY_SUBSTEPS = (8, 16)


def body_vehicle(cfg, ctx, B, seed):
    """VEHICLE with a rigid body: the rotor lag replaces the thrust lag."""
    return VehicleModel(cfg, ctx, B, seed=seed, body=RigidBody(**BODY), **{k: v for k, v in VEHICLE.items() if k != "thrust_tau"})


def controller(cfg, B, seed):
    rng = np.random.default_rng(seed)
    n = Nmpc(cfg, batch=B)
    x0 = np.zeros((B, 10))
    x0[:, :3] = rng.uniform(-1, 1, (B, 3))
    x0[:, 3:7] = np.stack([yaw2quat(y) for y in rng.uniform(-np.pi, np.pi, B)])
    x0[:, 7:] = rng.normal(0, 0.3, (B, 3))
    sq = (lambda a: a[0]) if B == 1 else (lambda a: a)
    n.set_sdf_flag(1.0)
    n.set_latent(sq(rng.normal(0, 1, (B, 128))), sq(x0[:, :3] + rng.normal(0, 0.2, (B, 3))), sq(np.stack([np.eye(3)] * B)))
    wps = (x0[:, None, :3] + rng.uniform(-3, 3, (B, 2, 3)), np.stack([[yaw2quat(a) for a in r] for r in rng.uniform(-1, 1, (B, 2))]))
    return n, sq(x0), wps


def host_loop(n, x0, wps, K, plant):
    B, ctx = max(n.B, 1), n.ocp.ctx
    dx = _lib.DeviceArray(ctx, (B, 10))
    x, xs = np.reshape(x0, (B, 10)).copy(), []
    for _ in range(K):
        n.set_x0(x if n.B > 1 else x[0])
        n.gen_refs_device("wps", wps=wps)
        n.solve()
        dx.upload(x)
        _lib.plant_step(ctx, plant, B, dx, n.ocp.field("u0"), dx)
        x = dx.numpy()
        xs.append(x)
    return np.stack(xs, 1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--B", type=int, default=1024)
    ap.add_argument("--N", type=int, default=40)
    ap.add_argument("--K", type=int, default=50)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--vehicle", action="store_true", help="also time the vehicle model's kernel and a rollout with it")
    ap.add_argument("--body", action="store_true", help="with --vehicle: also the rigid-body kernel and a rollout with it")
    a = ap.parse_args()
    if a.body and not a.vehicle:
        ap.error("--body goes with --vehicle")
    warnings.simplefilter("ignore")
    cfg = Config(mpc__N=a.N)
    res = {"B": a.B, "N": a.N, "K": a.K}
    t_roll, t_host, xr, xh = [], [], None, None
    for rep in range(a.reps + 1):  # repetition 0 warms up (workspaces, code objects) and is not timed
        n, x0, wps = controller(cfg, a.B, 1)
        plant = _lib.plant_opts(cfg, dt=float(n.ocp.dt[0]))
        n.set_x0(x0)
        n.ocp.ctx.synchronize()
        t0 = time.perf_counter()
        r = n.rollout(a.K, refs="wps", wps=wps, plant=plant)
        t1 = time.perf_counter()
        n.ocp.close()
        n, x0, wps = controller(cfg, a.B, 1)
        plant = _lib.plant_opts(cfg, dt=float(n.ocp.dt[0]))
        n.ocp.ctx.synchronize()
        t2 = time.perf_counter()
        xh = host_loop(n, x0, wps, a.K, plant)
        t3 = time.perf_counter()
        xr = r.x[:, 1:]
        if rep:
            t_roll.append((t1 - t0) / a.K * 1e3)
            t_host.append((t3 - t2) / a.K * 1e3)
        if rep < a.reps:
            n.ocp.close()
    res["same_bits"] = bool(np.array_equal(xr, xh))
    res["rollout_ms_per_step"], res["host_loop_ms_per_step"] = min(t_roll), min(t_host)
    res["qp_iters_mean"] = float(r.iters.mean())
    # the plant kernel alone, HIP events around each launch
    ctx, B = n.ocp.ctx, max(n.B, 1)
    dx, du = _lib.DeviceArray.from_numpy(ctx, xh[:, -1]), _lib.DeviceArray.from_numpy(ctx, r.u[:, -1])
    out = _lib.DeviceArray(ctx, (B, 10))
    for sub in (1, 10):
        o = _lib.plant_opts(cfg, dt=float(n.ocp.dt[0]), substeps=sub)
        for _ in range(20):
            _lib.plant_step(ctx, o, B, dx, du, out)
        ctx.synchronize()
        ctx.reset_stats()
        ctx.enable_timing(True)
        for _ in range(200):
            _lib.plant_step(ctx, o, B, dx, du, out)
        ms, cnt = ctx.kernel_stats("plant")
        ctx.enable_timing(False)
        ctx.reset_stats()
        res[f"plant_us_substeps{sub}"] = ms / cnt * 1e3
    if a.vehicle:
        m = VehicleModel(cfg, ctx, B, seed=1, **VEHICLE)
        est = _lib.DeviceArray.from_numpy(ctx, xh[:, -1])
        m.begin(est, 0)
        for sub in (1, 10):
            o = _lib.plant_opts(cfg, dt=float(n.ocp.dt[0]), substeps=sub)
            for f in range(20):
                m.step(o, du, f, est)
            ctx.synchronize()
            ctx.reset_stats()
            ctx.enable_timing(True)
            for f in range(200):
                m.step(o, du, 20 + f, est)
            ms, cnt = ctx.kernel_stats("plant_vehicle")
            ctx.enable_timing(False)
            ctx.reset_stats()
            res[f"plant_vehicle_us_substeps{sub}"] = ms / cnt * 1e3
        m.close()
    if a.body:  # both vehicle kernels at the substeps a rigid body needs
        for name, m in (("plant_vehicle", VehicleModel(cfg, ctx, B, seed=1, **VEHICLE)), ("plant_vehicle_body", body_vehicle(cfg, ctx, B, 1))):
            est = _lib.DeviceArray.from_numpy(ctx, xh[:, -1])
            m.begin(est, 0)
            for sub in BODY_SUBSTEPS:
                o = _lib.plant_opts(cfg, dt=float(n.ocp.dt[0]), substeps=sub)
                for f in range(20):
                    m.step(o, du, f, est)
                ctx.synchronize()
                ctx.reset_stats()
                ctx.enable_timing(True)
                for f in range(200):
                    m.step(o, du, 20 + f, est)
                ms, cnt = ctx.kernel_stats(name)
                ctx.enable_timing(False)
                ctx.reset_stats()
                res[f"{name}_us_substeps{sub}"] = ms / cnt * 1e3
            m.close()
    n.ocp.close()
    if a.vehicle:  # the rollout of the first part again, alternating without and with the model
        t_off, t_on = [], []
        for rep in range(a.reps + 1):
            for with_model in (False, True):
                n, x0, wps = controller(cfg, a.B, 1)
                plant = _lib.plant_opts(cfg, dt=float(n.ocp.dt[0]))
                m = VehicleModel(cfg, n.ocp.ctx, max(a.B, 1), seed=1, **VEHICLE) if with_model else None
                n.set_x0(x0)
                n.ocp.ctx.synchronize()
                t0 = time.perf_counter()
                n.rollout(a.K, refs="wps", wps=wps, plant=plant, vehicle=m)
                t1 = time.perf_counter()
                if rep:
                    (t_on if with_model else t_off).append((t1 - t0) / a.K * 1e3)
                if m is not None:
                    m.close()
                n.ocp.close()
        res["rollout_ms_per_step_no_vehicle"], res["rollout_ms_per_step_vehicle"] = min(t_off), min(t_on)
    if a.body:  # and with the rigid body, at the finer plant step it needs
        t_body = []
        for rep in range(a.reps + 1):
            n, x0, wps = controller(cfg, a.B, 1)
            plant = _lib.plant_opts(cfg, dt=float(n.ocp.dt[0]), substeps=BODY_SUBSTEPS[-1])
            m = body_vehicle(cfg, n.ocp.ctx, max(a.B, 1), 1)
            n.set_x0(x0)
            n.ocp.ctx.synchronize()
            t0 = time.perf_counter()
            rb = n.rollout(a.K, refs="wps", wps=wps, plant=plant, vehicle=m)
            t1 = time.perf_counter()
            if rep:
                t_body.append((t1 - t0) / a.K * 1e3)
            m.close()
            n.ocp.close()
        res["rollout_ms_per_step_body"] = min(t_body)
        res["body_share_of_step"] = res[f"plant_vehicle_body_us_substeps{BODY_SUBSTEPS[-1]}"] * 1e-3 / min(t_body)
        res["body_rotor_range"] = [float(rb.rotor.min()), float(rb.rotor.max())]
    print(f"B={a.B} N={a.N} K={a.K}: rollout {res['rollout_ms_per_step']:.3f} ms/step, host-driven loop "
          f"{res['host_loop_ms_per_step']:.3f} ms/step (same bits: {res['same_bits']}); plant kernel "
          f"{res['plant_us_substeps1']:.1f} us at substeps 1, {res['plant_us_substeps10']:.1f} us at substeps 10")
    if a.vehicle:
        print(f"vehicle model: plant_vehicle kernel {res['plant_vehicle_us_substeps1']:.1f} us at substeps 1, "
              f"{res['plant_vehicle_us_substeps10']:.1f} us at substeps 10; rollout "
              f"{res['rollout_ms_per_step_no_vehicle']:.3f} ms/step without the model, "
              f"{res['rollout_ms_per_step_vehicle']:.3f} ms/step with it")
    if a.body:
        print("rigid body: " + ", ".join(f"plant_vehicle_body {res[f'plant_vehicle_body_us_substeps{s}']:.1f} us beside plant_vehicle "
                                          f"{res[f'plant_vehicle_us_substeps{s}']:.1f} us at substeps {s}" for s in BODY_SUBSTEPS) +
              f"; rollout {res['rollout_ms_per_step_body']:.3f} ms/step with it ({BODY_SUBSTEPS[-1]} substeps), the kernel "
              f"{100 * res['body_share_of_step']:.1f} % of a step; rotors within {res['body_rotor_range']}")
    print(json.dumps(res))
    if res["rollout_ms_per_step"] > res["host_loop_ms_per_step"]:
        print("NOTE: the rollout was not faster than the host-driven loop in this run")


if __name__ == "__main__":
    main()
