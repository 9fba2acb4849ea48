"""CPU truth of the closed-loop plant (csrc/plant.hip): a numpy fp64 restatement of both models' f_expl --
'att' (sdf_nmpc/model/quad_rollpitchyawrate.py:19-55 with utils/math.py euler2rot, quat2rot, hamilton_prod) and
'att_tau' (quad_rollpitchyawrate_tau.py:19-58) -- written from the model equations, not from the kernel's
operation order, integrated with `substeps` classic RK4 steps of dt / substeps, plus the two mismatch terms of
sdfnmpc_plant_opts: acc_dist [B, 3], a world-frame acceleration added to dv/dt, and gamma_scale [B], a factor on
the thrust input.  tests/test_plant_ref.py pins it to the C oracle's integrator ('att') and to
tests/att_tau_ref.py ('att_tau') at substeps = 1 without mismatch."""
import numpy as np

G = 9.81
TAU_ROLL = TAU_PITCH = 0.12  # quad_rollpitchyawrate_tau.py:19-20
KINDS = {"att": 0, "att_tau": 1}


def limits(cfg):
    L = cfg.robot.limits
    return float(L.gamma), float(L.roll), float(L.pitch), float(L.wz)


def _hprod(a, b):
    a0, a1, a2, a3 = np.moveaxis(a, -1, 0)
    b0, b1, b2, b3 = np.moveaxis(b, -1, 0)
    return np.stack([a0 * b0 - a1 * b1 - a2 * b2 - a3 * b3,
                     a0 * b1 + a1 * b0 + a2 * b3 - a3 * b2,
                     a0 * b2 - a1 * b3 + a2 * b0 + a3 * b1,
                     a0 * b3 + a1 * b2 - a2 * b1 + a3 * b0], -1)


def f_expl(kind, x, u, lim, acc_dist=None, gamma_scale=None):
    """x [B, 10], u [B, 4] -> dx/dt [B, 10]."""
    q = x[:, 3:7] / np.linalg.norm(x[:, 3:7], axis=-1, keepdims=True)
    q0, q1, q2, q3 = q.T
    gamma, roll_c, pitch_c, wz = u[:, 0] * lim[0], u[:, 1] * lim[1], u[:, 2] * lim[2], u[:, 3] * lim[3]
    if gamma_scale is not None:
        gamma = gamma * gamma_scale
    zero = np.zeros_like(wz)
    if kind == 0:
        # W_R_B = quat2rot([cos tz, 0, 0, sin tz]) @ euler2rot([roll, pitch, 0]); its third column times gamma
        tz = np.arctan2(q3, q0)
        cy, sy = np.cos(tz), np.sin(tz)
        cr, sr, cp, sp = np.cos(roll_c), np.sin(roll_c), np.cos(pitch_c), np.sin(pitch_c)
        bz = np.stack([cr * sp, -sr, cr * cp], -1)  # euler2rot(roll, pitch, 0) e_z
        Rz = np.zeros(x.shape[:1] + (3, 3))
        Rz[:, 0, 0] = cy * cy - sy * sy
        Rz[:, 0, 1] = -2 * cy * sy
        Rz[:, 1, 0] = 2 * cy * sy
        Rz[:, 1, 1] = cy * cy - sy * sy
        Rz[:, 2, 2] = cy * cy + sy * sy
        W_a = np.einsum("bij,bj->bi", Rz, bz) * gamma[:, None]
        w = np.stack([zero, zero, zero, wz], -1)
    else:
        roll = np.arctan2(2 * (q0 * q1 + q2 * q3), 1 - 2 * (q1 * q1 + q2 * q2))
        pitch = np.arcsin(2 * (q0 * q2 - q3 * q1))
        W_a = np.stack([2 * (q1 * q3 + q0 * q2), 2 * (q2 * q3 - q0 * q1), q0 ** 2 - q1 ** 2 - q2 ** 2 + q3 ** 2],
                       -1) * gamma[:, None]
        d_roll, d_pitch = (roll_c - roll) / TAU_ROLL, (pitch_c - pitch) / TAU_PITCH
        w0 = d_roll + np.sin(pitch) * np.sin(roll) / np.cos(pitch) * d_pitch
        w1 = np.cos(roll) * d_pitch
        w = np.stack([zero, w0, w1, wz], -1)
    W_a = W_a - np.array([0.0, 0.0, G])
    if acc_dist is not None:
        W_a = W_a + acc_dist
    return np.concatenate([x[:, 7:10], _hprod(q, w) / 2, W_a], -1)


def step(cfg, kind, x, u, dt, substeps=1, acc_dist=None, gamma_scale=None):
    """x_next [B, 10] = `substeps` RK4 steps of dt / substeps from x [B, 10] under u [B, 4]; kind 0 / 1 or a name."""
    kind = KINDS.get(kind, kind)
    lim = limits(cfg)
    x = np.array(x, dtype=np.float64)
    u = np.asarray(u, dtype=np.float64)
    f = lambda z: f_expl(kind, z, u, lim, acc_dist, gamma_scale)
    h = dt / substeps
    for _ in range(substeps):
        k1 = f(x)
        k2 = f(x + h / 2 * k1)
        k3 = f(x + h / 2 * k2)
        k4 = f(x + h * k3)
        x = x + h / 6 * (k1 + 2 * k2 + 2 * k3 + k4)
    return x


def states(rng, B):
    """Random plant states [B, 10] and inputs [B, 4] inside the box: any yaw, roll and pitch within 0.6 rad (away
    from the 'att_tau' model's singularity at |pitch| = pi / 2), quaternion norms 0.9..1.1 (the models normalise)."""
    x = np.zeros((B, 10))
    x[:, :3] = rng.uniform(-2, 2, (B, 3))
    yaw, pitch, roll = rng.uniform(-np.pi, np.pi, B), rng.uniform(-0.6, 0.6, B), rng.uniform(-0.6, 0.6, B)
    qz = np.stack([np.cos(yaw / 2), 0 * yaw, 0 * yaw, np.sin(yaw / 2)], -1)
    qy = np.stack([np.cos(pitch / 2), 0 * yaw, np.sin(pitch / 2), 0 * yaw], -1)
    qx = np.stack([np.cos(roll / 2), np.sin(roll / 2), 0 * yaw, 0 * yaw], -1)
    x[:, 3:7] = _hprod(_hprod(qz, qy), qx) * rng.uniform(0.9, 1.1, (B, 1))
    x[:, 7:] = rng.normal(0, 1.0, (B, 3))
    u = np.concatenate([rng.uniform(0.2, 0.9, (B, 1)), rng.uniform(-0.8, 0.8, (B, 3))], 1)
    return x, u
