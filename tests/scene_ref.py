"""fp64 numpy reference for csrc/scene.hip, written from the geometry and not from the kernel: a ray caster that
tests every face of every primitive on its own (the kernel intersects parameter intervals), the closed-form signed
distances, the pixel-centre rays of ColChecker's pixel grid, and the `decided` mask of the GPU comparison.

Also the one fixed set of inputs every scene test uses (SCENE, SENSOR, POSES, SHAPES)."""
import numpy as np

# ---- the fixed inputs: (kind, values) as sdf_nmpc_amd.scene.Scene takes them
SCENE = [("sphere", [2.5, -0.8, 0.3, 0.5]),
         ("box", [3.5, 0.5, -1.0, 4.1, 1.5, 1.2]),
         ("cylinder", [3.0, 0.3, 0.4, -1.5, 1.5]),
         ("box", [-10.0, -10.0, -1.6, 10.0, 10.0, -1.5])]   # the floor
SENSOR = dict(hfov=0.7592, vfov=0.4903, dmax=5.0)           # pinhole
SPHERICAL = dict(hfov=1.2, vfov=0.6, dmax=5.0)
POSES = [((0.0, 0.0, 0.0), (0.0, 0.0, 0.0)),                # position, ZYX roll-pitch-yaw of the camera
         ((0.5, 0.4, 0.2), (0.0, 0.0, 0.3)),
         ((0.2, -0.3, -0.1), (0.15, -0.2, -0.25))]
SHAPES = [(27, 48), (18, 32)]                                # 27 x 48: five full 256-lane blocks and a 16-lane tail
DECIDE_EPS, DECIDE_TOL = 1e-5, 1e-3


def rpy2rot(roll, pitch, yaw):
    """R = Rz(yaw) Ry(pitch) Rx(roll): camera axes (x forward, y left, z up) in the world frame."""
    cr, sr, cp, sp, cy, sy = np.cos(roll), np.sin(roll), np.cos(pitch), np.sin(pitch), np.cos(yaw), np.sin(yaw)
    Rz = np.array([[cy, -sy, 0], [sy, cy, 0], [0, 0, 1.0]])
    Ry = np.array([[cp, 0, sp], [0, 1.0, 0], [-sp, 0, cp]])
    Rx = np.array([[1.0, 0, 0], [0, cr, -sr], [0, sr, cr]])
    return Rz @ Ry @ Rx


def camera_poses(poses=POSES):
    """-> W_p_C [B, 3], W_R_C [B, 3, 3]"""
    return np.array([p for p, _ in poses], float), np.stack([rpy2rot(*e) for _, e in poses])


def ray_dirs(h, w, hfov, vfov, is_spherical=False, du=0.0, dv=0.0):
    """Unit directions [h, w, 3] in the camera frame of the rays through the pixel centres, the horizontal / vertical
    pixel coordinate (tangent for a pinhole, angle for a spherical image) shifted by du / dv."""
    fu = 1.0 - (2.0 * np.arange(w) + 1.0) / w
    fv = 1.0 - (2.0 * np.arange(h) + 1.0) / h
    if is_spherical:
        az, el = np.meshgrid(hfov * fu + du, vfov * fv + dv, indexing="xy")
        return np.stack([np.cos(el) * np.cos(az), np.cos(el) * np.sin(az), np.sin(el)], -1)
    ty, tz = np.meshgrid(np.tan(hfov) * fu + du, np.tan(vfov) * fv + dv, indexing="xy")
    d = np.stack([np.ones_like(ty), ty, tz], -1)
    return d / np.linalg.norm(d, axis=-1, keepdims=True)


def _inside(kind, a, p):
    if kind == "sphere":
        return np.linalg.norm(p - a[:3]) <= a[3]
    if kind == "box":
        return bool(np.all(p >= a[:3]) and np.all(p <= a[3:6]))
    return bool(np.hypot(p[0] - a[0], p[1] - a[1]) <= a[2] and a[3] <= p[2] <= a[4])


def _hit_faces(kind, a, o, d):
    """Smallest t > 0 at which the rays o + t d [n, 3] cross a face of the primitive from anywhere (inf: none)."""
    n = d.shape[0]
    best = np.full(n, np.inf)

    def take(t, ok):
        nonlocal best
        t = np.where(ok & (t > 0), t, np.inf)
        best = np.minimum(best, t)

    with np.errstate(divide="ignore", invalid="ignore"):
        if kind == "sphere":
            oc = o - a[:3]
            b = d @ oc
            disc = b * b - (oc @ oc - a[3] ** 2)
            sq = np.sqrt(np.where(disc >= 0, disc, np.nan))
            for t in (-b - sq, -b + sq):
                take(t, disc >= 0)
        elif kind == "box":
            lo, hi = a[:3], a[3:6]
            for ax in range(3):
                o1, o2 = (ax + 1) % 3, (ax + 2) % 3
                for plane in (lo[ax], hi[ax]):
                    t = (plane - o[ax]) / d[:, ax]
                    q = o + t[:, None] * d
                    take(t, (q[:, o1] >= lo[o1]) & (q[:, o1] <= hi[o1]) & (q[:, o2] >= lo[o2]) & (q[:, o2] <= hi[o2]))
        else:
            cx, cy, r, z0, z1 = a[:5]
            ex, ey = o[0] - cx, o[1] - cy
            A = d[:, 0] ** 2 + d[:, 1] ** 2
            Bq = ex * d[:, 0] + ey * d[:, 1]
            disc = Bq * Bq - A * (ex * ex + ey * ey - r * r)
            sq = np.sqrt(np.where(disc >= 0, disc, np.nan))
            for t in ((-Bq - sq) / A, (-Bq + sq) / A):  # the side wall, between the caps
                z = o[2] + t * d[:, 2]
                take(t, (disc >= 0) & (A > 0) & (z >= z0) & (z <= z1))
            for zc in (z0, z1):                          # the cap discs
                t = (zc - o[2]) / d[:, 2]
                take(t, (o[0] + t * d[:, 0] - cx) ** 2 + (o[1] + t * d[:, 1] - cy) ** 2 <= r * r)
    return best


def cast(prims, o, d):
    """Range t >= 0 along unit rays d [n, 3] from o [3] to the union of the primitives: 0 when o lies inside one,
    else the nearest face crossing; inf for a miss."""
    o, d = np.asarray(o, float), np.asarray(d, float).reshape(-1, 3)
    best = np.full(d.shape[0], np.inf)
    for kind, a in prims:
        a = np.asarray(a, float)
        if _inside(kind, a, o):
            return np.zeros(d.shape[0])
        best = np.minimum(best, _hit_faces(kind, a, o, d))
    return best


def values(prims, W_p_C, W_R_C, h, w, hfov, vfov, dmax, is_depth=False, is_spherical=False, du=0.0, dv=0.0):
    """The pixel values in metres [B, h, w]: min(range or depth, dmax), dmax for a miss."""
    dc = ray_dirs(h, w, hfov, vfov, is_spherical, du, dv).reshape(-1, 3)
    out = []
    for p, R in zip(np.reshape(W_p_C, (-1, 3)), np.reshape(W_R_C, (-1, 3, 3))):
        t = cast(prims, p, dc @ R.T)
        val = t * dc[:, 0] if is_depth else t
        out.append(np.where(np.isfinite(t), np.minimum(val, dmax), dmax).reshape(h, w))
    return np.stack(out)


def render(prims, W_p_C, W_R_C, h, w, hfov, vfov, dmax, scale, **kw):
    return values(prims, W_p_C, W_R_C, h, w, hfov, vfov, dmax, **kw) * scale


def decided(prims, W_p_C, W_R_C, h, w, hfov, vfov, dmax, **kw):
    """Pixels whose value moves by at most DECIDE_TOL metres when both pixel coordinates (tangents; angles for a
    spherical image) are shifted by +-DECIDE_EPS, in the four sign combinations: away from silhouettes and edges,
    where a last-bit difference in the ray picks another surface."""
    v0 = values(prims, W_p_C, W_R_C, h, w, hfov, vfov, dmax, **kw)
    ok = np.ones(v0.shape, bool)
    for su in (-1.0, 1.0):
        for sv in (-1.0, 1.0):
            v = values(prims, W_p_C, W_R_C, h, w, hfov, vfov, dmax, du=su * DECIDE_EPS, dv=sv * DECIDE_EPS, **kw)
            ok &= np.abs(v - v0) <= DECIDE_TOL
    return ok


def distance(prims, pts):
    """Signed distance [n] from points [n, 3] to the union: the minimum over the primitives, negative inside."""
    pts = np.asarray(pts, float).reshape(-1, 3)
    best = np.full(pts.shape[0], np.inf)
    for kind, a in prims:
        a = np.asarray(a, float)
        if kind == "sphere":
            d = np.linalg.norm(pts - a[:3], axis=1) - a[3]
        else:
            if kind == "box":
                q = np.abs(pts - (a[:3] + a[3:6]) / 2) - (a[3:6] - a[:3]) / 2
            else:
                q = np.stack([np.hypot(pts[:, 0] - a[0], pts[:, 1] - a[1]) - a[2],
                              np.abs(pts[:, 2] - (a[3] + a[4]) / 2) - (a[4] - a[3]) / 2], 1)
            d = np.linalg.norm(np.maximum(q, 0.0), axis=1) + np.minimum(q.max(axis=1), 0.0)
        best = np.minimum(best, d)
    return best


def quat2rot(q):
    """[w, x, y, z] of any norm -> rotation matrix of q / |q|."""
    w, x, y, z = np.asarray(q, float) / np.linalg.norm(q)
    return np.array([[w * w + x * x - y * y - z * z, 2 * (x * y - w * z), 2 * (x * z + w * y)],
                     [2 * (x * y + w * z), w * w - x * x + y * y - z * z, 2 * (y * z - w * x)],
                     [2 * (x * z - w * y), 2 * (y * z + w * x), w * w - x * x - y * y + z * z]])
