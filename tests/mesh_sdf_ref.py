"""fp64 numpy reference for scene_sdf_rows_mesh_kernel (csrc/scene_mesh.hip): the distance of a triangle mesh and its
gradient written as the SDF row of the preparation phase (column 2 of h and J_h), from the geometry on mesh_ref and not
from the kernel.

Per triangle the closest point is the foot of p on the plane when it lies in the triangle, else the nearest point of
the three sides (mesh_ref's construction).  The foot is taken along the unit normal, c = p - ((p - a) . n) n, so that
p - c = ((p - a) . n) n carries the rounding error of one dot product and not that of a 2 x 2 solve: the gradient of a
row 1e-3 m off a face is then good to about 1e-13, where the barycentric foot loses two more digits (measured against
50-digit arithmetic on the GPU tests' rows: 6e-12).  The mesh's closest point c is that of the triangle with the smallest squared
distance, the lowest index on a tie.  The value is |p - c|, for a closed mesh (signed) negative where (p - c) . n < 0 for
the pseudonormal n of the feature c lies on.  Its world gradient:

  |p - c| > 0        (p - c) / |p - c|, negated where the sign is negative: a unit vector away from the surface
                     outside, towards it inside
  p on the surface   signed: the pseudonormal of the feature, normalised; unsigned: the unit face normal of the winning
                     triangle (a one-sided value)

Truncation: d < max_df keeps (d, grad); anything else -- a mesh without triangles and a position that is not finite
too -- gives (max_df, 0).  The row: h2 = flag df + (1 - flag) max_df, J_h2 = flag grad in columns 0..2 and 0 in 3..9,
flag = p[..., 0] (scene_sdf_ref's contract).

`decided` marks the rows a last-bit difference cannot move, by scene_sdf_ref's rules: away from the truncation
distance, away from the surface, and where the analytic gradient agrees with the central difference of
mesh_ref.distance (off the medial axis and the ties between two features)."""
import numpy as np

import mesh_ref as M

TIE_EPS, FD_STEP, FD_TOL = 1e-6, 1e-6, 1e-4  # scene_sdf_ref's


def closest(mesh, pts, signed=False):
    """For points [n, 3]: (d [n] the distance, signed where `signed`; c [n, 3] the closest point of the mesh; tri [n] the
    triangle it lies on, -1 without triangles; nrm [n, 3] the normal at c -- signed: the pseudonormal of the feature
    (face, edge or vertex) c lies on, not normalised; unsigned: the unit face normal of the triangle)."""
    return _closest(mesh, pts, signed)[:4]


def _closest(mesh, pts, signed):
    """`closest`, and e [n, 3] = p - c as it was formed (not as the difference of two rounded points)"""
    pts = np.asarray(pts, float).reshape(-1, 3)
    v, tr = mesh.verts, mesh.tris
    n = pts.shape[0]
    best, c, tri, nrm = np.full(n, np.inf), np.zeros((n, 3)), np.full(n, -1), np.zeros((n, 3))
    off = np.zeros((n, 3))
    if signed and tr.shape[0]:
        fn, en, vn = M._pseudonormals(mesh)
    with np.errstate(invalid="ignore"):
        for i, t in enumerate(tr):
            a, e1, e2 = v[t[0]], v[t[1]] - v[t[0]], v[t[2]] - v[t[0]]
            face = np.cross(e1, e2)
            face /= np.linalg.norm(face)
            G = np.array([[e1 @ e1, e1 @ e2], [e1 @ e2, e2 @ e2]])
            uv = np.linalg.solve(G, np.stack([(pts - a) @ e1, (pts - a) @ e2]))
            inside = (uv[0] >= 0) & (uv[1] >= 0) & (uv[0] + uv[1] <= 1)
            e = ((pts - a) @ face)[:, None] * face  # p - foot, along the normal
            q = pts - e
            d2 = np.where(inside, (e ** 2).sum(1), np.inf)
            feat = np.tile(face, (n, 1))
            for k in range(3):
                pa, pb = t[k], t[(k + 1) % 3]
                qs, s = M._segment(pts, v[pa], v[pb])
                ds = ((pts - qs) ** 2).sum(1)
                take = ~inside & (ds < d2)
                d2 = np.where(take, ds, d2)
                q = np.where(take[:, None], qs, q)
                e = np.where(take[:, None], pts - qs, e)
                if signed:
                    f = np.where((s == 0)[:, None], vn[pa], np.where((s == 1)[:, None], vn[pb], en[(min(pa, pb), max(pa, pb))]))
                    feat = np.where(take[:, None], f, feat)
            better = d2 < best  # strict: the lowest index keeps a tie
            best = np.where(better, d2, best)
            c = np.where(better[:, None], q, c)
            off = np.where(better[:, None], e, off)
            nrm = np.where(better[:, None], feat, nrm)
            tri = np.where(better, i, tri)
    d = np.sqrt(best)
    if signed:
        with np.errstate(invalid="ignore"):
            d = np.where((off * nrm).sum(1) < 0, -d, d)
    return d, c, tri, nrm, off


def dist_grad(mesh, pts, signed=False):
    """The untruncated distance [n] and its world gradient [n, 3] (zero without triangles or at a non-finite point)."""
    pts = np.asarray(pts, float).reshape(-1, 3)
    d, c, tri, nrm, e = _closest(mesh, pts, signed)
    r = np.abs(d)
    with np.errstate(divide="ignore", invalid="ignore"):
        away = e / r[:, None] * np.where(d < 0, -1.0, 1.0)[:, None]
        ln = np.linalg.norm(nrm, axis=1)
        on = nrm / np.where(ln > 0, ln, 1.0)[:, None]
    g = np.where((r > 0)[:, None], away, on)
    ok = (tri >= 0) & np.isfinite(pts).all(1)
    return np.where(ok, d, np.inf), np.where(ok[:, None], g, 0.0)


def sdf_rows(mesh, x, p, max_df, signed=False):
    """Column 2 of h [..., N+1] and of J_h [..., N+1, 10] for node positions x [..., N+1, >= 3] and parameters p
    [..., N+1, np] (the flag is p[..., 0])."""
    x, p = np.asarray(x, float), np.asarray(p, float)
    lead = x.shape[:-1]
    d, g = dist_grad(mesh, x[..., :3].reshape(-1, 3), signed)
    near = d < max_df
    df = np.where(near, d, max_df).reshape(lead)
    g = np.where(near[:, None], g, 0.0).reshape(lead + (3,))
    flag = p[..., 0]
    J = np.zeros(lead + (10,))
    J[..., :3] = flag[..., None] * g
    return flag * df + (1.0 - flag) * max_df, J


def decided(mesh, x, max_df, signed=False):
    """Rows [..., N+1] bool: |d - max_df| > TIE_EPS, |d| > TIE_EPS, and the analytic gradient within FD_TOL per component
    of the central difference (step FD_STEP) of mesh_ref.distance.  A row without a finite distance is not decided."""
    x = np.asarray(x, float)
    lead = x.shape[:-1]
    pts = x[..., :3].reshape(-1, 3)
    d, g = dist_grad(mesh, pts, signed)
    ok = np.isfinite(d) & (np.abs(d - max_df) > TIE_EPS) & (np.abs(d) > TIE_EPS)
    safe = np.where(np.isfinite(pts).all(1)[:, None], pts, 0.0)
    for i in range(3):
        e = np.zeros(3)
        e[i] = FD_STEP
        fd = (M.distance(mesh, safe + e, signed) - M.distance(mesh, safe - e, signed)) / (2.0 * FD_STEP)
        with np.errstate(invalid="ignore"):
            ok &= np.abs(fd - g[:, i]) <= FD_TOL
    return ok.reshape(lead)
