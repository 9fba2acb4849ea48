"""The parity cases of the rigid-body vehicle, shared by tests/test_rigid_body_ref.py (which checks on the CPU that
they reach both rotor limits) and tests/test_gpu_vehicle_body.py (which runs them on the device).  The restatement's
result of a case is computed once per process and handed out read-only.

One call: random tilted states with body rates and rotor speeds away from hover, every third quaternion with
q0 < 0; B = 3, 64, 65; substeps 1 and 4; with and without acc_dist, gamma_scale and drag; tau_mot = 0 and > 0; random
commands and the saturating command u = (1, 1, -1, 1) from a fast-rotating state.  dt is chosen per substeps so that
(dt / substeps) max(1 / tau_mot, k_rate, 2 / tau_att) <= 1.
Six calls: delay 2, gust and estimate noise on, commands that change every call, the third one saturating."""
import functools

import numpy as np

import rigid_body_ref as RB
from sdf_nmpc_amd.config import Config

BATCHES = (3, 64, 65)
SUBSTEPS = (1, 4)
DT = {1: 0.02, 4: 0.075}
SAT_U = np.array([1.0, 1.0, -1.0, 1.0])
SEQ = dict(seed=0xb0d1e5, delay=2, gust_std=0.8, gust_tau=0.4, est_std_pos=0.05, est_std_vel=0.1, est_std_yaw=0.02)
SEQ_CALLS, SEQ_SUBSTEPS, SEQ_DT = 6, 4, 0.075

# (name, tau_mot, mismatch and drag, saturating)
ONE_CALL = [(f"{'lag' if tm else 'nolag'}-{'mis' if mis else 'plain'}-{'sat' if sat else 'rand'}", tm, mis, sat)
            for tm in (RB.LOOP["tau_mot"], 0.0) for mis in (False, True) for sat in (False, True)]


def body_kw(tau_mot=RB.LOOP["tau_mot"]):
    return dict(RB.DEFAULT, **dict(RB.LOOP, tau_mot=tau_mot))


def one_call_inputs(B, substeps, name):
    _, tau_mot, mis, sat = next(c for c in ONE_CALL if c[0] == name)
    rng = np.random.default_rng(7000 + 100 * B + 10 * substeps + [c[0] for c in ONE_CALL].index(name))
    x, u, om, ro = RB.tilted_states(rng, B, rate=6.0 if sat else 1.0)
    if sat:
        u = np.tile(SAT_U, (B, 1))
    acc = rng.uniform(-2, 2, (B, 3)) if mis else None
    gs = rng.uniform(0.8, 1.2, B) if mis else None
    drag = (0.3, 0.2, 0.1) if mis else (0, 0, 0)
    return dict(x=x, u=u, omega=om, rotor=ro, acc=acc, gs=gs, drag=drag, tau_mot=tau_mot, dt=DT[substeps])


def _freeze(d):
    for v in d.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return d


@functools.lru_cache(maxsize=None)
def one_call_ref(B, substeps, name):
    """The restatement's (x_true, omega, rotor, estimate) after the call, and whether a rotor was clipped at either end."""
    i = one_call_inputs(B, substeps, name)
    r = RB.RigidBodyVehicle(Config(), B, drag=i["drag"], **body_kw(i["tau_mot"]))
    r.begin(i["x"], 0)
    r.omega, r.rotor = i["omega"].copy(), i["rotor"].copy()
    est = r.step("att", i["u"], 0, i["dt"], substeps, i["acc"], i["gs"])
    return _freeze(dict(x=r.x_true, omega=r.omega, rotor=r.rotor, est=est, idle=r.clipped_idle, max=r.clipped_max))


def seq_inputs(B):
    rng = np.random.default_rng(8100 + B)
    x, _, om, ro = RB.tilted_states(rng, B)
    us = [RB.tilted_states(rng, B)[1] for _ in range(SEQ_CALLS)]
    us[2] = np.tile(SAT_U, (B, 1))
    stream = (np.arange(B)[::-1] * 3 + 1).astype(np.int32)
    return dict(x=x, omega=om, rotor=ro, us=us, stream=stream)


def seq_run(B):
    """The restatement over the six calls: per call (x_true, estimate, u_applied, omega, rotor)."""
    i = seq_inputs(B)
    x, us = i["x"], i["us"]
    r = RB.RigidBodyVehicle(Config(), B, stream_id=i["stream"], **SEQ, **body_kw())
    est0 = r.begin(x, 0)
    r.omega, r.rotor = i["omega"].copy(), i["rotor"].copy()
    rows = []
    for f, u in enumerate(us):
        est = r.step("att", u, f, SEQ_DT, SEQ_SUBSTEPS)
        rows.append(dict(x=r.x_true.copy(), est=est, u_app=r.u_app.copy(), omega=r.omega.copy(), rotor=r.rotor.copy()))
    return est0, rows, (r.clipped_idle, r.clipped_max)


@functools.lru_cache(maxsize=None)
def seq_ref(B):
    est0, rows, clipped = seq_run(B)
    est0.setflags(write=False)
    return est0, tuple(_freeze(r) for r in rows), clipped
