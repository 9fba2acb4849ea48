"""CPU truth of the 'att_tau' model (first-order roll / pitch lag): a torch fp64 restatement of
sdf_nmpc/model/quad_rollpitchyawrate_tau.py:19-58 with utils/math.py quat2euler :57-70, quat2rot :7-23,
deuler_avel_map :210-226 (row 1 = [0, cos(roll), -sin(pitch)], as the reference writes it), hamilton_prod
and invert, batched over leading dimensions; Jacobians by autograd.

tests/golden/make_tau_golden.py pins it to the reference's own numpy helpers (values to 1e-13, Jacobians
by central differences) and records tests/golden/tau_golden.npz.  The C oracle knows the 'att' model only:
`lin` takes what does not depend on the dynamics (h, J_h, y_N, J_yN) from oracle.linearize_batch and
overwrites x_next, [A|B], y and J_y, which gives the dict qp_ipm_batch and stage_qp accept."""
import numpy as np
import torch

G = 9.81
TAU_ROLL = TAU_PITCH = 0.12  # quad_rollpitchyawrate_tau.py:19-20


def limits(cfg):
    L = cfg.robot.limits
    return float(L.gamma), float(L.roll), float(L.pitch), float(L.wz)


def _hprod(a, b):
    a0, a1, a2, a3 = a.unbind(-1)
    b0, b1, b2, b3 = b.unbind(-1)
    return torch.stack([a0 * b0 - a1 * b1 - a2 * b2 - a3 * b3,
                        a0 * b1 + a1 * b0 + a2 * b3 - a3 * b2,
                        a0 * b2 - a1 * b3 + a2 * b0 + a3 * b1,
                        a0 * b3 + a1 * b2 - a2 * b1 + a3 * b0], -1)


def f_expl(x, u, lim):
    """(..., 10), (..., 4) -> f (..., 10), W_a (..., 3)."""
    q = x[..., 3:7] / torch.linalg.norm(x[..., 3:7], dim=-1, keepdim=True)
    q0, q1, q2, q3 = q.unbind(-1)
    roll = torch.atan2(2 * (q0 * q1 + q2 * q3), 1 - 2 * (q1 * q1 + q2 * q2))
    pitch = torch.asin(2 * (q0 * q2 - q3 * q1))
    gamma, roll_des, pitch_des, wz = u[..., 0] * lim[0], u[..., 1] * lim[1], u[..., 2] * lim[2], u[..., 3] * lim[3]
    r13 = 2 * (q1 * q3 + q0 * q2)
    r23 = 2 * (q2 * q3 - q0 * q1)
    r33 = q0 ** 2 - q1 ** 2 - q2 ** 2 + q3 ** 2
    W_a = torch.stack([r13 * gamma, r23 * gamma, r33 * gamma - G], -1)
    dot_roll = (roll_des - roll) / TAU_ROLL
    dot_pitch = (pitch_des - pitch) / TAU_PITCH
    w0 = dot_roll + torch.sin(pitch) * torch.sin(roll) / torch.cos(pitch) * dot_pitch
    w1 = torch.cos(roll) * dot_pitch
    dq = _hprod(q, torch.stack([torch.zeros_like(wz), w0, w1, wz], -1)) / 2
    return torch.cat([x[..., 7:10], dq, W_a], -1), W_a


def rk4(x, u, dt, lim):
    """dt broadcasts against x[..., 0]."""
    dt = torch.as_tensor(dt, dtype=x.dtype)[..., None]
    f = lambda z: f_expl(z, u, lim)[0]
    k1 = f(x)
    k2 = f(x + dt / 2 * k1)
    k3 = f(x + dt / 2 * k2)
    k4 = f(x + dt * k3)
    return x + dt / 6 * (k1 + 2 * k2 + 2 * k3 + k4)


def y_stage(x, u, qd, lim):
    """[p, q_e[3], v, roll_des, pitch_des, wz, W_a[2]] (quad_rollpitchyawrate_tau.py:51-53)."""
    q = x[..., 3:7] / torch.linalg.norm(x[..., 3:7], dim=-1, keepdim=True)
    qi = q * torch.tensor([1.0, -1.0, -1.0, -1.0], dtype=x.dtype) / torch.linalg.norm(q, dim=-1, keepdim=True)
    q_e = _hprod(qd, qi)
    _, W_a = f_expl(x, u, lim)
    scale = torch.tensor(lim[1:], dtype=x.dtype)
    return torch.cat([x[..., :3], q_e[..., 3:4], x[..., 7:10], u[..., 1:4] * scale, W_a[..., 2:3]], -1)


def _jac(fun, xu, nout):
    """d fun(xu)[..., i] / d xu[..., j] for a function acting row by row: [..., j, i] (column-major blocks)."""
    xu = xu.detach().requires_grad_(True)
    out = fun(xu)
    cols = [torch.autograd.grad(out[..., i].sum(), xu, retain_graph=i + 1 < nout)[0] for i in range(nout)]
    return out.detach(), torch.stack(cols, -1)


def dynamics(cfg, x, u, p, dt):
    """x (..., 10), u (..., 4), p (..., np), dt broadcastable to the leading dims ->
    xn (..., 10), AB (..., 14, 10), y (..., 11), Jy (..., 14, 11): the layouts of include/sdfnmpc.h."""
    lim = limits(cfg)
    xu = torch.from_numpy(np.ascontiguousarray(np.concatenate([x, u], -1), dtype=np.float64))
    qd = torch.from_numpy(np.ascontiguousarray(p[..., 13:17], dtype=np.float64))
    dtt = torch.from_numpy(np.broadcast_to(np.asarray(dt, np.float64), x.shape[:-1]).copy())
    xn, AB = _jac(lambda z: rk4(z[..., :10], z[..., 10:], dtt, lim), xu, 10)
    y, Jy = _jac(lambda z: y_stage(z[..., :10], z[..., 10:], qd, lim), xu, 11)
    return xn.numpy(), AB.numpy(), y.numpy(), Jy.numpy()


def step(cfg, x, u, dt):
    """The plant: x_next = RK4(x, u, dt), one instance per row."""
    with torch.no_grad():
        return rk4(torch.from_numpy(np.ascontiguousarray(x, dtype=np.float64)),
                   torch.from_numpy(np.ascontiguousarray(u, dtype=np.float64)), float(dt), limits(cfg)).numpy()


def lin(O, cfg, onet, x, u, p, dt, nthreads=4):
    """The preparation phase's outputs for x [B][N+1][10], u [B][N][4], p [B][N+1][np], dt [N]."""
    out = O.linearize_batch(O.quad_model(cfg), onet, x, u, p, dt, nthreads)
    out["xn"], out["AB"], out["y"], out["Jy"] = dynamics(cfg, x[:, :-1], u, p[:, :-1], np.asarray(dt)[None, :])
    return out
