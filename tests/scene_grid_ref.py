"""fp64 numpy restatement of the uniform grid of an indexed scene (sdfnmpc_scene_create_large, csrc/engine.cpp) and of
the two searches of csrc/scene_grid.hip with their stop rules: the DDA of a ray and the ring search of a point.  Written
to be examined, not to be fast: a search returns the set of primitives it visited and the minimum over them, and
tests/test_scene_grid_ref.py holds that minimum against tests/scene_ref.py's brute force over all primitives.

Also the chunked brute force the GPU tests hold the grid kernels against: the parent kernels on at most 32 primitives
at a time, combined by the elementwise minimum."""
import numpy as np

import scene_ref as R

MAX_AXIS, MAX_CELLS = 1024, 1 << 22
CHUNK = 32


def bbox(prim):
    kind, a = prim[0], np.asarray(prim[1], float)
    if kind == "sphere":
        return a[:3] - a[3], a[:3] + a[3]
    if kind == "box":
        return a[:3].copy(), a[3:6].copy()
    return np.array([a[0] - a[2], a[1] - a[2], a[3]]), np.array([a[0] + a[2], a[1] + a[2], a[4]])


def build(prims, cell=None):
    """The grid of one scene: org [3], cell, n [3], infl, and the CSR lists start [cells + 1], items (ascending
    primitive index within a cell; cell id = (k n[1] + j) n[0] + i)."""
    n = len(prims)
    if n == 0:
        return dict(org=np.zeros(3), cell=1.0, n=np.ones(3, int), infl=0.0, start=np.zeros(2, int), items=np.zeros(0, int))
    boxes = [bbox(p) for p in prims]
    lo = np.min([b[0] for b in boxes], axis=0)
    hi = np.max([b[1] for b in boxes], axis=0)
    Rm = max(np.abs(lo).max(), np.abs(hi).max())
    ext = hi - lo
    c = float(cell) if cell is not None else max(np.cbrt(np.prod(ext) / (4.0 * n)), (ext.max() + Rm * 2.0 ** -10) / 250.0)
    c = float(np.float32(c))
    infl = c * 2.0 ** -10 + Rm * 2.0 ** -12
    org = np.zeros(3)
    dims = np.zeros(3, int)
    for k in range(3):
        o = np.float32(lo[k] - 2 * infl)
        if float(o) > lo[k] - 2 * infl:
            o = np.nextafter(o, np.float32(-np.inf))
        org[k] = float(o)
        top = hi[k] + 2 * infl
        dims[k] = max(1, int(np.ceil((top - org[k]) / c)))
        while org[k] + dims[k] * c < top:
            dims[k] += 1
    if dims.max() > MAX_AXIS or int(np.prod(dims)) > MAX_CELLS:
        raise ValueError("grid too large")
    lists = [[] for _ in range(int(np.prod(dims)))]
    for i, (bl, bh) in enumerate(boxes):
        q0 = np.clip(np.floor((bl - infl - org) / c).astype(int), 0, dims - 1)
        q1 = np.clip(np.floor((bh + infl - org) / c).astype(int), 0, dims - 1)
        for z in range(q0[2], q1[2] + 1):
            for y in range(q0[1], q1[1] + 1):
                for x in range(q0[0], q1[0] + 1):
                    lists[(z * dims[1] + y) * dims[0] + x].append(i)
    start = np.concatenate([[0], np.cumsum([len(l) for l in lists])]).astype(int)
    items = np.array([i for l in lists for i in l], int)
    return dict(org=org, cell=c, n=dims, infl=infl, start=start, items=items)


def _cell(u, n):
    return n - 1 if u >= n - 1 else (int(u) if u > 0 else 0)


def _slab(lo, hi, o, d, tn, tf):
    with np.errstate(divide="ignore", invalid="ignore"):
        t1, t2 = np.float64(lo - o) / d, np.float64(hi - o) / d
    if np.isnan(t1) or np.isnan(t2):  # on the plane with d == 0: fmin / fmax drop the NaN
        t1 = t2 = t2 if np.isnan(t1) else t1
    return max(tn, min(t1, t2)), min(tf, max(t1, t2))


def ray_search(G, o, d, tstop, hit):
    """The DDA of scene_render_grid_kernel for the ray o + t d: hit(i) is primitive i's hit parameter (inf: none).
    -> (best, the set of primitives tested, the number of cells visited)."""
    o, d = np.asarray(o, float), np.asarray(d, float)
    org, c, n = G["org"], G["cell"], G["n"]
    best, seen, tn, tf = np.inf, set(), -np.inf, np.inf
    for k in range(3):
        tn, tf = _slab(org[k], org[k] + n[k] * c, o[k], d[k], tn, tf)
    t0 = max(tn, 0.0)
    if len(G["items"]) == 0 or not (tn <= tf and tf >= 0.0 and t0 <= tstop):
        return best, seen, 0
    ci = [_cell((o[k] + t0 * d[k] - org[k]) / c, n[k]) for k in range(3)]
    step = [1 if d[k] > 0 else -1 for k in range(3)]
    fwd = [1 if d[k] > 0 else 0 for k in range(3)]
    plane = lambda k: (org[k] + (ci[k] + fwd[k]) * c - o[k]) / d[k] if abs(d[k]) > 0 else np.inf
    t = [plane(k) for k in range(3)]
    cells = 0
    for _ in range(int(n.sum()) + 3):
        cid = (ci[2] * n[1] + ci[1]) * n[0] + ci[0]
        cells += 1
        for i in G["items"][G["start"][cid]:G["start"][cid + 1]]:
            seen.add(int(i))
            best = min(best, hit(int(i)))
        te = min(t)
        if not te * (1.0 - 2.0 ** -16) < min(best, tstop):
            break
        k = 0 if (t[0] <= t[1] and t[0] <= t[2]) else (1 if t[1] <= t[2] else 2)
        ci[k] += step[k]
        if not 0 <= ci[k] < n[k]:
            break
        t[k] = plane(k)
    return best, seen, cells


def point_search(G, p, dist, cap=np.inf):
    """The ring search of scene_distance_grid_kernel (cap = inf) and scene_sdf_rows_grid_kernel (cap = max_df) for the
    point p: dist(i) is primitive i's signed distance.  -> (best, the set of primitives tested, the number of rounds)."""
    p = np.asarray(p, float)
    org, c, n = G["org"], G["cell"], G["n"]
    lo = np.array([_cell((p[k] - org[k]) / c, n[k]) for k in range(3)])
    hi = lo.copy()
    plo, phi = np.ones(3, int), np.zeros(3, int)
    best, seen = np.inf, set()
    rounds = 0
    for _ in range(int(n.max()) + 1):
        rounds += 1
        for z in range(lo[2], hi[2] + 1):
            for y in range(lo[1], hi[1] + 1):
                row = (z * n[1] + y) * n[0]
                inner = plo[2] <= z <= phi[2] and plo[1] <= y <= phi[1]
                runs = [(lo[0], hi[0] + 1)] if not inner else [(lo[0], plo[0]), (phi[0] + 1, hi[0] + 1)]
                for a, b in runs:
                    for i in G["items"][G["start"][row + a]:G["start"][row + b]]:
                        seen.add(int(i))
                        best = min(best, dist(int(i)))
        gap, grown = np.inf, False
        for k in range(3):
            if lo[k] > 0:
                gap = min(gap, p[k] - (org[k] + lo[k] * c))
                grown = True
            if hi[k] < n[k] - 1:
                gap = min(gap, org[k] + (hi[k] + 1) * c - p[k])
                grown = True
        if not grown or not min(best, cap) > gap:
            break
        plo, phi = lo.copy(), hi.copy()
        lo, hi = np.maximum(lo - 1, 0), np.minimum(hi + 1, n - 1)
    return best, seen, rounds


# ---- the chunked brute force of the GPU tests: the parent's kernels on <= 32 primitives at a time
def chunks(prims, size=CHUNK):
    return [prims[i:i + size] for i in range(0, len(prims), size)]


def chunked_render(ctx, prims, *args, **kw):
    """min over the chunks of Scene(ctx, chunk).render(*args, **kw) [B, h, w]; no primitive: a plain empty scene."""
    from sdf_nmpc_amd.scene import Scene
    out = None
    for ch in chunks(prims) or [[]]:
        sc = Scene(ctx, ch)
        img = sc.render(*args, **kw).numpy()
        sc.close()
        out = img if out is None else np.minimum(out, img)
    return out


def chunked_distance(ctx, prims, pts):
    from sdf_nmpc_amd.scene import Scene
    out = np.full(np.reshape(pts, (-1, 3)).shape[0], np.inf)
    for ch in chunks(prims):
        sc = Scene(ctx, ch)
        out = np.minimum(out, sc.distance(pts))
        sc.close()
    return out
