"""Regenerates tests/golden/body_golden.npz: the allocation matrices and 64 evaluations of the rigid-body f_expl.

    python tests/golden/make_body_golden.py <path of the reference checkout>

Gf and Gt are formed as model/quad_props.py:20-27 forms them, with the reference's own numpy helpers (utils/math.py
axis_rot, GTMRP_matrix, imported with a no-op ``casadi`` module) from the robot.* entries of its config/default.yaml.
f_expl is assembled from its quat2rot and hamilton_prod as quad_props.py:41-48 composes them, at 64 random states
(p, q, v, omega) [13] and rotor commands u in (0, 1), wp = u * robot.limits.wp: |q| in 0.9..1.1, every third case with
q0 < 0.  Arrays only are written.
"""
import os
import sys
import types

import numpy as np
import yaml

HERE = os.path.dirname(os.path.abspath(__file__))
G = 9.81  # base_model.py:10


def reference_math(ref_root):
    sys.modules.setdefault("casadi", types.ModuleType("casadi"))  # imported by utils/math.py:3, unused by the numpy branches
    sys.path.insert(0, ref_root)
    from sdf_nmpc.utils import math as rmath
    return rmath


def main(ref_root):
    rmath = reference_math(ref_root)
    with open(os.path.join(ref_root, "sdf_nmpc", "config", "default.yaml")) as f:
        robot = yaml.safe_load(f)["robot"]
    alloc, wp_max, m = robot["alloc"], float(robot["limits"]["wp"]), float(robot["mass"])
    J = np.diag(robot["inertia"]).astype(float)
    Jinv = np.linalg.inv(J)

    # the allocation as quad_props.py:20-27 composes the helpers: rotor i turned about z by i pi / (n / 2), then by its
    # beta about y and its alternating alpha about x; one coefficient pair for every rotor; both matrices times cf
    motors = np.array(alloc["motors"], float)
    n_rot = len(motors)
    turns = []
    for i, (_, _, _, a_i, b_i, _) in enumerate(motors):
        turns.append(rmath.axis_rot("z", i * (rmath.pi / (n_rot / 2))) @ rmath.axis_rot("y", b_i)
                     @ rmath.axis_rot("x", (-1) ** i * a_i))
    cfs, cts = [alloc["cf"]] * n_rot, [alloc["ct"]] * n_rot
    Gf, Gt = rmath.GTMRP_matrix(turns, motors[:, :3], list(motors[:, 5]), cfs, cts)
    Gf, Gt = alloc["cf"] * Gf, alloc["cf"] * Gt

    def f_expl(x, u):  # quad_props.py:30-48
        q = x[3:7] / np.linalg.norm(x[3:7])
        v, w = x[7:10], x[10:]
        wp = u * wp_max
        W_a = rmath.quat2rot(q) @ Gf @ wp**2 / m + np.array([0, 0, -G])
        return np.concatenate([v, rmath.hamilton_prod(q, np.concatenate([[0], w])) / 2, W_a,
                               Jinv @ (Gt @ wp**2 - np.cross(w, J @ w))])

    rng = np.random.default_rng(1313)
    n = 64
    X = np.zeros((n, 13))
    X[:, :3] = rng.uniform(-2, 2, (n, 3))
    q = rng.normal(size=(n, 4))
    q *= rng.uniform(0.9, 1.1, (n, 1)) / np.linalg.norm(q, axis=1, keepdims=True)
    q[:, 0] = np.abs(q[:, 0])
    q[::3] *= -1.0
    X[:, 3:7] = q
    X[:, 7:10] = rng.normal(0, 1.0, (n, 3))
    X[:, 10:] = rng.normal(0, 2.0, (n, 3))
    U = rng.uniform(0.05, 1.0, (n, 4))
    F = np.array([f_expl(X[i], U[i]) for i in range(n)])
    out = dict(mass=np.array(m), inertia=np.array(robot["inertia"], float), motors=np.array(alloc["motors"], float),
               cf=np.array(float(alloc["cf"])), ct=np.array(float(alloc["ct"])), wp_max=np.array(wp_max), Gf=Gf, Gt=Gt,
               x=X, wp=U * wp_max, f=F)
    np.savez_compressed(os.path.join(HERE, "body_golden.npz"), **out)
    print(f"body_golden.npz: {n} cases, {(q[:, 0] < 0).sum()} with q0 < 0; |f| up to {np.abs(F).max():.3g}")
    print({k: v.shape for k, v in out.items()})


if __name__ == "__main__":
    if len(sys.argv) != 2:
        sys.exit(__doc__)
    main(sys.argv[1])
