"""fp64 numpy reference for the dynamic kernels of csrc/scene.hip: primitives with a rigid frame that is a function of
time,

    c(t) = c0 + v t + amp sin(omega t + phase)        R(t) = Rz(yaw_rate t) R0

about the reference point c0 (sphere: centre; box: (lo + hi) / 2; cylinder: (cx, cy, (z0 + z1) / 2)).  Per primitive
the ray or the point is carried into the primitive's frame and tests/scene_ref.py (imported unchanged) does the rest on
the canonical centred shape: its face-by-face `_hit_faces` / `_inside` and its closed-form distances.  A primitive
without motion goes to scene_ref as it is, in the world frame.

Also the one dynamic fixture every test of moving scenes uses (SPEC, TIMES)."""
import numpy as np

import scene_ref as R

# ---- the fixed inputs: scene_ref.SCENE with motions, as keyword arguments of sdf_nmpc_amd.scene.Scene.moving
SPEC = [(R.SCENE[0], dict(v=(0.0, 0.4, 0.0))),
        (R.SCENE[1], dict(rpy=(0.2, -0.3, 0.5), yaw_rate=0.6, amp=(0.0, 0.8, 0.0), omega=1.5, phase=0.3)),
        (R.SCENE[2], dict(rpy=(0.4, 0.2, 0.0), v=(-0.3, 0.0, 0.0))),
        (R.SCENE[3], None)]                                  # the floor stays
TIMES = (0.0, 0.7, 2.3)


def moving(prim, v=(0.0, 0.0, 0.0), q=None, rpy=None, yaw_rate=0.0, amp=(0.0, 0.0, 0.0), omega=0.0, phase=0.0):
    """(kind, values, motion): the orientation as a matrix, from q = (w, x, y, z) or ZYX roll-pitch-yaw."""
    assert q is None or rpy is None
    R0 = R.quat2rot(q) if q is not None else R.rpy2rot(*rpy) if rpy is not None else np.eye(3)
    return (prim[0], list(prim[1]), dict(R0=R0, v=np.asarray(v, float), amp=np.asarray(amp, float),
                                         yaw_rate=float(yaw_rate), omega=float(omega), phase=float(phase)))


def scene(spec=SPEC):
    return [moving(p, **kw) if kw is not None else p for p, kw in spec]


def canonical(kind, a):
    """-> the reference point c0 and the primitive centred on the origin"""
    a = np.asarray(a, float)
    if kind == "sphere":
        return a[:3].copy(), np.array([0.0, 0.0, 0.0, a[3]])
    if kind == "box":
        h = (a[3:6] - a[:3]) / 2
        return (a[:3] + a[3:6]) / 2, np.concatenate([-h, h])
    hz = (a[4] - a[3]) / 2
    return np.array([a[0], a[1], (a[3] + a[4]) / 2]), np.array([0.0, 0.0, a[2], -hz, hz])


def frame(c0, m, t):
    """c(t) [..., 3] and R(t) [..., 3, 3] for times t [...]"""
    t = np.asarray(t, float)
    c = c0 + m["v"] * t[..., None] + m["amp"] * np.sin(m["omega"] * t + m["phase"])[..., None]
    cy, sy, z, o = np.cos(m["yaw_rate"] * t), np.sin(m["yaw_rate"] * t), np.zeros_like(t), np.ones_like(t)
    Rz = np.stack([np.stack([cy, -sy, z], -1), np.stack([sy, cy, z], -1), np.stack([z, z, o], -1)], -2)
    return c, Rz @ m["R0"]


def cast(prims, o, d, t=0.0):
    """scene_ref.cast of the scene at time t: 0 when o lies inside a primitive, else the nearest face crossing."""
    o, d = np.asarray(o, float), np.asarray(d, float).reshape(-1, 3)
    best = np.full(d.shape[0], np.inf)
    for kind, a, *mo in prims:
        a = np.asarray(a, float)
        if mo:
            c0, a = canonical(kind, a)
            c, Rt = frame(c0, mo[0], t)
            ol, dl = Rt.T @ (o - c), d @ Rt
        else:
            ol, dl = o, d
        if R._inside(kind, a, ol):
            return np.zeros(d.shape[0])
        best = np.minimum(best, R._hit_faces(kind, a, ol, dl))
    return best


def values(prims, W_p_C, W_R_C, h, w, hfov, vfov, dmax, t=0.0, is_depth=False, is_spherical=False, du=0.0, dv=0.0):
    """scene_ref.values of the scene at time t: metres [B, h, w]."""
    dc = R.ray_dirs(h, w, hfov, vfov, is_spherical, du, dv).reshape(-1, 3)
    out = []
    for p, Rm in zip(np.reshape(W_p_C, (-1, 3)), np.reshape(W_R_C, (-1, 3, 3))):
        r = cast(prims, p, dc @ Rm.T, t)
        val = r * dc[:, 0] if is_depth else r
        out.append(np.where(np.isfinite(r), np.minimum(val, dmax), dmax).reshape(h, w))
    return np.stack(out)


def decided(prims, W_p_C, W_R_C, h, w, hfov, vfov, dmax, t=0.0, **kw):
    """scene_ref.decided's rule on the scene at time t."""
    v0 = values(prims, W_p_C, W_R_C, h, w, hfov, vfov, dmax, t, **kw)
    ok = np.ones(v0.shape, bool)
    for su in (-1.0, 1.0):
        for sv in (-1.0, 1.0):
            v = values(prims, W_p_C, W_R_C, h, w, hfov, vfov, dmax, t, du=su * R.DECIDE_EPS, dv=sv * R.DECIDE_EPS, **kw)
            ok &= np.abs(v - v0) <= R.DECIDE_TOL
    return ok


def distance(prims, pts, t=0.0):
    """Signed distance [n] from points [n, 3] to the scene, point j at time t (a scalar) or t[j]."""
    pts = np.asarray(pts, float).reshape(-1, 3)
    t = np.broadcast_to(np.asarray(t, float), (pts.shape[0],))
    best = np.full(pts.shape[0], np.inf)
    for kind, a, *mo in prims:
        if mo:
            c0, a = canonical(kind, a)
            c, Rt = frame(c0, mo[0], t)                       # [n, 3], [n, 3, 3]
            q = np.einsum("nij,ni->nj", Rt, pts - c)          # R(t)^T (p - c(t))
        else:
            q = pts
        best = np.minimum(best, R.distance([(kind, a)], q))
    return best
