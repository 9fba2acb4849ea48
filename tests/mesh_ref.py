"""fp64 numpy reference for csrc/scene_mesh.hip, written from the geometry and not from the kernel: a brute-force ray
cast over all triangles (Moller-Trumbore), a brute-force closest point on a triangle (the plane's foot when it lies in
the triangle, else the nearest of the three sides), the sign by the angle-weighted pseudonormal of the nearest feature,
and the `decided` mask of the GPU comparison.

The library rounds the vertices to fp32 once; ``rounded`` does the same, so that a reference on its result sees the
mesh the kernels see.  The fixed scene is scene_ref.SCENE restated as meshes."""
import numpy as np

import scene_ref as R
from sdf_nmpc_amd.mesh import Mesh

NDOT_MIN = 0.1  # decided pixels: |n . d| at the reference hit


def fixed_scene():
    """scene_ref.SCENE as one mesh: icosphere subdiv 2, boxes, a cylinder of 24 segments."""
    parts = []
    for kind, a in R.SCENE:
        if kind == "sphere":
            parts.append(Mesh.icosphere(a[:3], a[3], 2))
        elif kind == "box":
            parts.append(Mesh.box(a[:3], a[3:6]))
        else:
            parts.append(Mesh.cylinder(a[:2], a[2], a[3], a[4], 24))
    return Mesh.merge(*parts)


def rounded(mesh):
    return Mesh(mesh.verts.astype(np.float32).astype(np.float64), mesh.tris)


# ---- rays
def cast(mesh, o, d):
    """Unit rays d [n, 3] from o [3]: (t [n], the smallest t >= 0 at which a ray meets a triangle, either face, inf
    for a miss; ndot [n], |n . d| for the unit normal of that triangle, 1 for a miss)."""
    o, d = np.asarray(o, float), np.asarray(d, float).reshape(-1, 3)
    v, tr = mesh.verts, mesh.tris
    best, ndot = np.full(d.shape[0], np.inf), np.ones(d.shape[0])
    if tr.shape[0] == 0:
        return best, ndot
    a, e1, e2 = v[tr[:, 0]], v[tr[:, 1]] - v[tr[:, 0]], v[tr[:, 2]] - v[tr[:, 0]]   # [m, 3]
    nrm = np.cross(e1, e2)
    nrm /= np.linalg.norm(nrm, axis=1, keepdims=True)
    s = o - a                                                                        # [m, 3]
    q = np.cross(s, e1)                                                              # [m, 3]
    with np.errstate(divide="ignore", invalid="ignore"):
        for lo in range(0, d.shape[0], 512):
            dd = d[lo:lo + 512]                                                      # [k, 3]
            p = np.cross(dd[:, None, :], e2[None])                                   # [k, m, 3]
            det = np.einsum("kmi,mi->km", p, e1)
            u = np.einsum("kmi,mi->km", p, s) / det
            w = np.einsum("ki,mi->km", dd, q) / det
            t = np.einsum("mi,mi->m", e2, q)[None] / det
            ok = (det != 0) & (u >= 0) & (w >= 0) & (u + w <= 1) & (t >= 0)
            t = np.where(ok, t, np.inf)
            k = t.argmin(axis=1)
            tt = t[np.arange(t.shape[0]), k]
            best[lo:lo + 512] = tt
            ndot[lo:lo + 512] = np.where(np.isfinite(tt), np.abs(np.einsum("ki,ki->k", dd, nrm[k])), 1.0)
    return best, ndot


def values(mesh, W_p_C, W_R_C, h, w, hfov, vfov, dmax, is_depth=False, is_spherical=False, du=0.0, dv=0.0, with_ndot=False):
    """The pixel values in metres [B, h, w]: min(range or depth, dmax), dmax for a miss (scene_ref.values)."""
    dc = R.ray_dirs(h, w, hfov, vfov, is_spherical, du, dv).reshape(-1, 3)
    out, nd = [], []
    for p, Rm in zip(np.reshape(W_p_C, (-1, 3)), np.reshape(W_R_C, (-1, 3, 3))):
        t, n = cast(mesh, p, dc @ Rm.T)
        val = t * dc[:, 0] if is_depth else t
        out.append(np.where(np.isfinite(t), np.minimum(val, dmax), dmax).reshape(h, w))
        nd.append(n.reshape(h, w))
    return (np.stack(out), np.stack(nd)) if with_ndot else np.stack(out)


def decided(mesh, W_p_C, W_R_C, h, w, hfov, vfov, dmax, **kw):
    """scene_ref.decided -- the value moves by at most DECIDE_TOL when the pixel coordinates are shifted by
    +-DECIDE_EPS -- further restricted to rays that meet their triangle at |n . d| >= NDOT_MIN."""
    v0, nd = values(mesh, W_p_C, W_R_C, h, w, hfov, vfov, dmax, with_ndot=True, **kw)
    ok = nd >= NDOT_MIN
    for su in (-1.0, 1.0):
        for sv in (-1.0, 1.0):
            v = values(mesh, W_p_C, W_R_C, h, w, hfov, vfov, dmax, du=su * R.DECIDE_EPS, dv=sv * R.DECIDE_EPS, **kw)
            ok &= np.abs(v - v0) <= R.DECIDE_TOL
    return ok


# ---- distance
def _pseudonormals(mesh):
    """face [m, 3] unit; edge {(a, b) undirected: sum of the adjacent unit face normals}; vertex [nv, 3] angle-weighted."""
    v, tr = mesh.verts, mesh.tris
    fn = np.cross(v[tr[:, 1]] - v[tr[:, 0]], v[tr[:, 2]] - v[tr[:, 0]])
    fn /= np.linalg.norm(fn, axis=1, keepdims=True)
    vn = np.zeros_like(v)
    en = {}
    for i, t in enumerate(tr):
        for k in range(3):
            p, q, r = v[t[k]], v[t[(k + 1) % 3]], v[t[(k + 2) % 3]]
            e1, e2 = q - p, r - p
            ang = np.arccos(np.clip(e1 @ e2 / (np.linalg.norm(e1) * np.linalg.norm(e2)), -1.0, 1.0))
            vn[t[k]] += ang * fn[i]
            key = (min(t[k], t[(k + 1) % 3]), max(t[k], t[(k + 1) % 3]))
            en[key] = en.get(key, 0.0) + fn[i]
    return fn, en, vn


def _segment(p, a, b):
    """Closest point of the segment a b to the points p [n, 3]: (point [n, 3], parameter [n] in [0, 1])."""
    ab = b - a
    s = np.clip((p - a) @ ab / (ab @ ab), 0.0, 1.0)
    return a + s[:, None] * ab, s


def distance(mesh, pts, signed=False):
    """Distance [n] from points [n, 3] to the mesh: brute force over the triangles, ties to the lower triangle index;
    signed: negative where (p - c) . n < 0 for the pseudonormal n of the feature the closest point c lies on (a closed,
    consistently oriented mesh).  +inf without triangles."""
    pts = np.asarray(pts, float).reshape(-1, 3)
    v, tr = mesh.verts, mesh.tris
    n = pts.shape[0]
    best, sign = np.full(n, np.inf), np.ones(n)
    if signed:
        fn, en, vn = _pseudonormals(mesh)
    for i, t in enumerate(tr):
        a, b, c = v[t[0]], v[t[1]], v[t[2]]
        nrm = np.cross(b - a, c - a)
        nrm /= np.linalg.norm(nrm)
        # the foot of p on the plane, in barycentric coordinates through the Gram matrix of the two sides
        e1, e2 = b - a, c - a
        G = np.array([[e1 @ e1, e1 @ e2], [e1 @ e2, e2 @ e2]])
        uv = np.linalg.solve(G, np.stack([(pts - a) @ e1, (pts - a) @ e2]))
        inside = (uv[0] >= 0) & (uv[1] >= 0) & (uv[0] + uv[1] <= 1)
        q = a + uv[0][:, None] * e1 + uv[1][:, None] * e2
        d2 = np.where(inside, ((pts - q) ** 2).sum(1), np.inf)
        feat = np.zeros((n, 3))
        if signed:
            feat[:] = fn[i]
        cp = q.copy()
        for k in range(3):
            pa, pb = t[k], t[(k + 1) % 3]
            qs, s = _segment(pts, v[pa], v[pb])
            ds = ((pts - qs) ** 2).sum(1)
            take = ~inside & (ds < d2)
            d2 = np.where(take, ds, d2)
            cp = np.where(take[:, None], qs, cp)
            if signed:
                f = np.where((s == 0)[:, None], vn[pa], np.where((s == 1)[:, None], vn[pb], en[(min(pa, pb), max(pa, pb))]))
                feat = np.where(take[:, None], f, feat)
        better = d2 < best
        best = np.where(better, d2, best)
        if signed:
            sg = np.where(((pts - cp) * feat).sum(1) < 0, -1.0, 1.0)
            sign = np.where(better, sg, sign)
    return sign * np.sqrt(best)
