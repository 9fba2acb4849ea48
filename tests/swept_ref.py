"""fp64 numpy restatement of the swept-clearance query (csrc/scene_swept.hip), on the distance functions of scene_ref /
scene_dyn_ref (imported unchanged): the minimum over s in [0, 1] of

    D(s) = distance(scene at t(s), p(s)),    p(s) = p0 + s (p1 - p0),    t(s) = t0 + s (t1 - t0)

`speed_bound` is V, the bound on the speed of any surface point of any mover; `lipschitz` the constant L = |p1 - p0| +
V |t1 - t0| of D; `bnb` the deterministic Lipschitz branch and bound on dyadic intervals for one segment, with its
certificate; `dense` the minimum over M + 1 uniform samples, the yardstick both certificates are tested against:

    dense - L / (2 M) <= true minimum <= dense        (D is L-Lipschitz; a sample lies within 1 / (2 M) of every s)
    dmin - gap        <= true minimum <= dmin         (the certificate)

so dense - L / (2 M) <= dmin and dmin - gap <= dense, whatever the algorithm did.

Primitives are scene_dyn_ref's: (kind, values) or (kind, values, motion) with motion from scene_dyn_ref.moving."""
import numpy as np

import scene_dyn_ref as D

DEPTH = 20  # the narrowest interval is 2^-20 of the segment


def distance(prims, pts, t=0.0):
    """The scene's signed distance at points [n, 3] and times t (a scalar or [n]); +inf without primitives."""
    return D.distance(prims, pts, t)


def speed_bound(prims):
    """V = max over the movers of |v| + |omega| |amp| + |yaw_rate| rho, Euclidean norms, inflated by 1 + 1e-12; rho is
    the largest distance of a point of the shape from its reference point: 0 for a sphere, the half diagonal of a box,
    sqrt(r^2 + hz^2) for a cylinder.  0 without movers."""
    V = 0.0
    for kind, a, *mo in prims:
        if not mo:
            continue
        m = mo[0]
        _, shape = D.canonical(kind, a)
        rho = 0.0 if kind == "sphere" else np.linalg.norm(shape[3:6]) if kind == "box" else np.hypot(shape[2], shape[4])
        V = max(V, np.linalg.norm(m["v"]) + abs(m["omega"]) * np.linalg.norm(m["amp"]) + abs(m["yaw_rate"]) * rho)
    return V * (1.0 + 1e-12)


def lipschitz(prims, p0, p1, t0=0.0, t1=0.0):
    return float(np.linalg.norm(np.asarray(p1, float) - np.asarray(p0, float)) + speed_bound(prims) * abs(t1 - t0))


def bnb(prims, p0, p1, t0=0.0, t1=0.0, eps=1e-3, max_evals=4096):
    """-> dmin, s, gap, evals for one segment.  An interval [a, b] of width w holds no value below lb = (D(a) + D(b) -
    L w) / 2; one with lb >= best - eps is dropped, any other halved at its midpoint, the left half first, down to a
    width of 2^-DEPTH and until max_evals evaluations are used.  gap = max(0, best - the smallest lb of any interval
    dropped): at most eps when neither limit was met."""
    p0, p1 = np.asarray(p0, float), np.asarray(p1, float)
    if not (np.isfinite(p0).all() and np.isfinite(p1 - p0).all() and np.isfinite(t0) and np.isfinite(t1 - t0)):
        return np.nan, np.nan, np.nan, 0
    L = lipschitz(prims, p0, p1, t0, t1)

    def at(s):
        return float(distance(prims, (p0 + s * (p1 - p0))[None], t0 + s * (t1 - t0))[0])

    best, sbest, evals = at(0.0), 0.0, 1
    if not L > 0.0:
        return best, 0.0, 0.0, 1
    d1 = at(1.0)
    evals = 2
    stack = [(0, 0, best, d1)]  # level, index, D at the two ends: the interval [index, index + 1] 2^-level
    if d1 < best:
        best, sbest = d1, 1.0
    lbmin = np.inf
    while stack:
        level, idx, da, db = stack.pop()
        lb = 0.5 * (da + db - L * 2.0 ** -level)
        if not (lb < best - eps and level < DEPTH and evals < max_evals):
            lbmin = min(lbmin, lb)
            continue
        sm = (2 * idx + 1) * 2.0 ** -(level + 1)
        dm = at(sm)
        evals += 1
        if dm < best or (dm == best and sm < sbest):
            best, sbest = dm, sm
        stack.append((level + 1, 2 * idx + 1, dm, db))
        stack.append((level + 1, 2 * idx, da, dm))
    return best, sbest, (best - lbmin if lbmin < best else 0.0), evals


def relevant(prims, p0, p1):
    """bool [n, len(prims)]: the primitives that can hold the minimum over each of the segments p0 -> p1 [n, 3]: every
    mover, and a static primitive unless its distance at p0 exceeds the static primitives' there by more than twice the
    segment's length -- its distance is 1-Lipschitz in space, so along the segment it stays above d_i(p0) - len while the
    scene's stays below min_i d_i(p0) + len.  What `dense` evaluates for a scene of hundreds of static primitives."""
    p0 = np.asarray(p0, float).reshape(-1, 3)
    ln = np.linalg.norm(np.asarray(p1, float).reshape(-1, 3) - p0, axis=1)
    keep = np.ones((p0.shape[0], len(prims)), bool)
    static = [i for i, pr in enumerate(prims) if len(pr) == 2]
    if static:
        d0 = np.stack([distance([prims[i]], p0) for i in static], 1)  # [n, static]
        keep[:, static] = d0 <= (d0.min(axis=1) + 2.0 * ln + 1e-9)[:, None]
    return keep


def dense(prims, p0, p1, t0=0.0, t1=0.0, M=4096, cull=True):
    """-> [n], [n]: the minimum of D over the M + 1 uniform samples s = i / M of each of the segments p0 -> p1 [n, 3]
    between the times t0, t1 (scalars or [n]), and the s of the first sample that attains it."""
    p0, p1 = np.asarray(p0, float).reshape(-1, 3), np.asarray(p1, float).reshape(-1, 3)
    n = p0.shape[0]
    t0, t1 = np.broadcast_to(np.asarray(t0, float), (n,)), np.broadcast_to(np.asarray(t1, float), (n,))
    keep = relevant(prims, p0, p1) if cull else np.ones((n, len(prims)), bool)
    s = np.arange(M + 1) / M
    dmin, smin = np.empty(n), np.empty(n)
    for j in range(n):
        d = distance([pr for pr, k in zip(prims, keep[j]) if k], p0[j] + s[:, None] * (p1[j] - p0[j]),
                     t0[j] + s * (t1[j] - t0[j]))
        i = int(np.argmin(d))
        dmin[j], smin[j] = d[i], s[i]
    return dmin, smin
