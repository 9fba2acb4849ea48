"""Regenerates tests/golden/tau_golden.npz: 64 linearisation cases of the 'att_tau' model.

    python tests/golden/make_tau_golden.py <path of the reference checkout>

The inputs (x, u, p, dt) and everything that does not depend on the dynamics (h, J_h, y_N, J_yN) are
lin_golden.npz's (make_golden.py:lin_golden: seed 4321, roll and pitch in +-0.3, |q| in 0.9..1.1, the four
dt values).  f_expl, the RK4 step and the stage residual are assembled here from the reference's own numpy
helpers (utils/math.py quat2euler, quat2rot, deuler_avel_map, hamilton_prod, invert, imported with a
no-op ``casadi`` module) as quad_rollpitchyawrate_tau.py:19-58 composes them; the Jacobians come from the
torch fp64 restatement tests/att_tau_ref.py, which is pinned here to the helper version: values to 1e-13,
Jacobians by central differences at lin_golden's bars.  Arrays only are written.
"""
import os
import sys
import types

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import att_tau_ref as T  # noqa: E402
from sdf_nmpc_amd.config import Config  # noqa: E402

G, TAU_ROLL, TAU_PITCH = 9.81, 0.12, 0.12  # base_model.py:10, quad_rollpitchyawrate_tau.py:19-20


def reference_math(ref_root):
    sys.modules.setdefault("casadi", types.ModuleType("casadi"))  # imported by utils/math.py:3, unused by the numpy branches
    sys.path.insert(0, ref_root)
    from sdf_nmpc.utils import math as rmath
    return rmath


def main(ref_root):
    rmath = reference_math(ref_root)
    cfg = Config()
    LIM = cfg.robot.limits

    def f_expl_np(x, u):
        q = x[3:7] / np.linalg.norm(x[3:7])
        eta = rmath.quat2euler(q)
        gamma, roll_des, pitch_des, wz = u[0] * LIM.gamma, u[1] * LIM.roll, u[2] * LIM.pitch, u[3] * LIM.wz
        W_a = rmath.quat2rot(q) @ np.array([0, 0, gamma]) + np.array([0, 0, -G])
        dot_roll = (roll_des - eta[0]) / TAU_ROLL
        dot_pitch = (pitch_des - eta[1]) / TAU_PITCH
        w = rmath.deuler_avel_map(eta) @ np.array([dot_roll, dot_pitch, 0])
        dq = rmath.hamilton_prod(q, np.array([0, w[0], w[1], wz])) / 2
        return np.concatenate([x[7:10], dq, W_a]), W_a

    def rk4_np(x, u, dt):
        f = lambda z: f_expl_np(z, u)[0]
        k1 = f(x); k2 = f(x + dt / 2 * k1); k3 = f(x + dt / 2 * k2); k4 = f(x + dt * k3)
        return x + dt / 6 * (k1 + 2 * k2 + 2 * k3 + k4)

    def y_np(x, u, p):
        q = x[3:7] / np.linalg.norm(x[3:7])
        q_e = rmath.hamilton_prod(p[13:17], rmath.invert(q))
        _, W_a = f_expl_np(x, u)
        return np.concatenate([x[:3], [q_e[3]], x[7:10], [u[1] * LIM.roll, u[2] * LIM.pitch, u[3] * LIM.wz, W_a[2]]])

    L = np.load(os.path.join(HERE, "lin_golden.npz"))
    X, U, P, DT = L["x"], L["u"], L["p"], L["dt"]
    n = len(X)
    xn, AB, y, Jy = T.dynamics(cfg, X, U, P, DT)
    A_B, J_y = AB.transpose(0, 2, 1), Jy.transpose(0, 2, 1)  # [n][10][14], [n][11][14] as lin_golden stores them
    f = np.array([f_expl_np(X[i], U[i])[0] for i in range(n)])
    pin_v = pin_fd = 0.0
    eps = 1e-6
    for i in range(n):
        x, u, p, dt = X[i], U[i], P[i], float(DT[i])
        # value pins: the torch restatement == the reference helpers
        ev = max(np.abs(xn[i] - rk4_np(x, u, dt)).max(), np.abs(y[i] - y_np(x, u, p)).max())
        pin_v = max(pin_v, ev)
        assert ev <= 1e-13, (i, ev)
        # derivative pins: central finite differences of the reference-helper functions
        xu = np.concatenate([x, u])
        for j in range(14):
            d = np.zeros(14); d[j] = eps
            xp, up, xm, um = (xu + d)[:10], (xu + d)[10:], (xu - d)[:10], (xu - d)[10:]
            fd = (rk4_np(xp, up, dt) - rk4_np(xm, um, dt)) / (2 * eps)
            sa = max(1, np.abs(A_B[i]).max())
            assert np.allclose(fd, A_B[i][:, j], rtol=1e-5, atol=2e-7 * sa), (i, j)
            fdy = (y_np(xp, up, p) - y_np(xm, um, p)) / (2 * eps)
            sy = max(1, np.abs(J_y[i]).max())
            assert np.allclose(fdy, J_y[i][:, j], rtol=1e-5, atol=2e-6 * sy), (i, j)
            pin_fd = max(pin_fd, np.abs(fd - A_B[i][:, j]).max() / sa, np.abs(fdy - J_y[i][:, j]).max() / sy)
    # the terminal residual [p, q_e[3]] is the stage residual's first four rows in both models
    assert np.abs(y[:, :4] - L["yN"]).max() <= 1e-13
    out = dict(x=X, u=U, p=P, dt=DT, f=f, xn=xn, A=A_B[:, :, :10], B=A_B[:, :, 10:], y=y, Jy=J_y, yN=L["yN"],
               JyN=L["JyN"], h=L["h"], Jh=L["Jh"])
    np.savez_compressed(os.path.join(HERE, "tau_golden.npz"), **out)
    print(f"tau_golden.npz: {n} cases; value pin {pin_v:.1e}, worst finite-difference residual {pin_fd:.1e} (relative)")
    print({k: v.shape for k, v in out.items()})


if __name__ == "__main__":
    if len(sys.argv) != 2:
        sys.exit(__doc__)
    main(sys.argv[1])
