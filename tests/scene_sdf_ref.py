"""fp64 numpy reference for csrc/scene_sdf.hip: the exact signed distance of a scene and its gradient written as the
SDF row of the preparation phase (column 2 of h and J_h), from the geometry and not from the kernel.

Per primitive the point is taken into the primitive's frame -- q = R(t)^T (p - c(t)) with scene_dyn_ref's `canonical`
and `frame`; a primitive without motion keeps the world axes, q = p - c0 -- and the distance d and its gradient g are
those of the centred shape:

  sphere            d = |q| - r                 g = q / |q|                         ((0, 0, 1) at q = 0)
  box               a = |q| - h                 outside (max a > 0): g_i = sign(q_i) max(a_i, 0) / |max(a, 0)|
                                                inside: g = sign(q_m) e_m, m the largest a_i (lowest index on a tie)
  capped cylinder   a = (rho - r, |q_z| - h_z)  outside: (max(a_0, 0) e_rho + max(a_1, 0) sign(q_z) e_z) / |max(a, 0)|
                                                inside: e_rho when a_0 >= a_1, else sign(q_z) e_z
  both              d = |max(a, 0)| + min(max a, 0)

with sign(0) = +1 and e_rho = (q_x, q_y, 0) / rho ((1, 0, 0) at rho = 0).  The scene's distance is the minimum over the
primitives (the lowest index on a tie), its world gradient R(t) g of that primitive.  Truncation: d < max_df keeps
(d, grad), anything else -- an empty scene too -- gives (max_df, 0).  The row: h2 = flag df + (1 - flag) max_df, J_h2 =
flag grad in columns 0..2 and 0 in 3..9, flag = p[..., 0] (gen_model.py:46-61).

`decided` marks the rows a last-bit difference cannot move: away from the ties between two primitives, from the
truncation distance, and from the kinks of a primitive (edges' bisectors, the medial axis inside), where the analytic
gradient is one of several one-sided values."""
import numpy as np

import scene_dyn_ref as D
import scene_ref as R

# the region every test draws its positions from: around scene_ref.SCENE / scene_dyn_ref.SPEC
LO, HI = np.array([-0.5, -3.0, -1.4]), np.array([6.0, 3.0, 2.0])
TIE_EPS, FD_STEP, FD_TOL = 1e-6, 1e-6, 1e-4


def draw(n, seed):
    """n positions uniform in the box [LO, HI]"""
    return LO + (HI - LO) * np.random.default_rng(seed).random((n, 3))


def _sign1(v):
    return np.where(v < 0.0, -1.0, 1.0)


def shape_sd(kind, shape, q):
    """Distance [n] and gradient [n, 3] of the centred shape `shape` (scene_dyn_ref.canonical) at q [n, 3]."""
    n = q.shape[0]
    g = np.zeros((n, 3))
    with np.errstate(divide="ignore", invalid="ignore"):
        if kind == "sphere":
            nq = np.linalg.norm(q, axis=1)
            z = nq == 0.0
            g = np.where(z[:, None], np.array([0.0, 0.0, 1.0]), q / np.where(z, 1.0, nq)[:, None])
            return nq - shape[3], g
        if kind == "box":
            a = np.abs(q) - shape[3:6]
            pos = np.maximum(a, 0.0)
            ln = np.linalg.norm(pos, axis=1)
            out = a.max(axis=1) > 0.0
            g_out = _sign1(q) * pos / np.where(out, ln, 1.0)[:, None]
            m = np.argmax(a, axis=1)  # the first of equal maxima
            g_in = np.zeros((n, 3))
            g_in[np.arange(n), m] = _sign1(q[np.arange(n), m])
            return ln + np.minimum(a.max(axis=1), 0.0), np.where(out[:, None], g_out, g_in)
        r, hz = shape[2], shape[4]
        rho = np.hypot(q[:, 0], q[:, 1])
        z = rho == 0.0
        e_rho = np.stack([np.where(z, 1.0, q[:, 0] / np.where(z, 1.0, rho)), np.where(z, 0.0, q[:, 1] / np.where(z, 1.0, rho)),
                          np.zeros(n)], 1)
        e_z = np.stack([np.zeros(n), np.zeros(n), _sign1(q[:, 2])], 1)
        a = np.stack([rho - r, np.abs(q[:, 2]) - hz], 1)
        pos = np.maximum(a, 0.0)
        ln = np.linalg.norm(pos, axis=1)
        out = a.max(axis=1) > 0.0
        g_out = (pos[:, :1] * e_rho + pos[:, 1:] * e_z) / np.where(out, ln, 1.0)[:, None]
        g_in = np.where((a[:, 0] >= a[:, 1])[:, None], e_rho, e_z)
        return ln + np.minimum(a.max(axis=1), 0.0), np.where(out[:, None], g_out, g_in)


def dist_grad(prims, pts, t=0.0):
    """The scene's untruncated distance [n], its world gradient [n, 3] and the second smallest primitive distance [n]
    (inf with fewer than two primitives), point j at time t (a scalar) or t[j]."""
    pts = np.asarray(pts, float).reshape(-1, 3)
    n = pts.shape[0]
    t = np.broadcast_to(np.asarray(t, float), (n,))
    best, second, grad = np.full(n, np.inf), np.full(n, np.inf), np.zeros((n, 3))
    for kind, a, *mo in prims:
        c0, shape = D.canonical(kind, a)
        if mo:
            c, Rt = D.frame(c0, mo[0], t)                          # [n, 3], [n, 3, 3]
            q = np.einsum("nij,ni->nj", Rt, pts - c)               # R(t)^T (p - c(t))
        else:
            q = pts - c0
        d, g = shape_sd(kind, shape, q)
        gw = np.einsum("nij,nj->ni", Rt, g) if mo else g
        win = d < best                                             # strict: the lowest index keeps a tie
        second = np.where(win, best, np.minimum(second, d))
        grad = np.where(win[:, None], gw, grad)
        best = np.where(win, d, best)
    return best, grad, second


def _times(shape, t0, tau):
    """The time of every node row of a [..., N+1] batch: t0 + tau[k], or t0"""
    t = np.full(shape, float(t0))
    return t if tau is None else t + np.asarray(tau, float)


def sdf_rows(prims, x, p, max_df, t0=0.0, tau=None):
    """Column 2 of h [..., N+1] and of J_h [..., N+1, 10] for node positions x [..., N+1, >= 3] and parameters p
    [..., N+1, np] (the flag is p[..., 0]); node k sees the scene at t0 + tau[k] (tau None: every node at t0)."""
    x, p = np.asarray(x, float), np.asarray(p, float)
    lead = x.shape[:-1]
    d, g, _ = dist_grad(prims, x[..., :3].reshape(-1, 3), _times(lead, t0, tau).ravel())
    near = d < max_df
    df = np.where(near, d, max_df).reshape(lead)
    g = np.where(near[:, None], g, 0.0).reshape(lead + (3,))
    flag = p[..., 0]
    J = np.zeros(lead + (10,))
    J[..., :3] = flag[..., None] * g
    return flag * df + (1.0 - flag) * max_df, J


def decided(prims, x, max_df, t0=0.0, tau=None):
    """Rows [..., N+1] bool: the two smallest primitive distances differ by more than TIE_EPS, |d - max_df| > TIE_EPS,
    and the analytic gradient agrees per component within FD_TOL with the central difference (step FD_STEP) of
    scene_ref.distance / scene_dyn_ref.distance."""
    x = np.asarray(x, float)
    lead = x.shape[:-1]
    pts, t = x[..., :3].reshape(-1, 3), _times(lead, t0, tau).ravel()
    d, g, second = dist_grad(prims, pts, t)
    dyn = any(len(pr) > 2 for pr in prims)
    dist = (lambda q: D.distance(prims, q, t)) if dyn else (lambda q: R.distance(prims, q))
    ok = (second - d > TIE_EPS) & (np.abs(d - max_df) > TIE_EPS)
    for i in range(3):
        e = np.zeros(3)
        e[i] = FD_STEP
        fd = (dist(pts + e) - dist(pts - e)) / (2.0 * FD_STEP)
        ok &= np.abs(fd - g[:, i]) <= FD_TOL
    return ok.reshape(lead)
