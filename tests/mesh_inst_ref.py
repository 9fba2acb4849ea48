"""fp64 numpy reference for csrc/scene_inst.hip (instanced mesh scenes: Scene.instanced), built on tests/mesh_ref.py and
written from the geometry, not from the kernels: an instance is its part's *rounded* vertices taken to the world by the
instance's frame at t, c(t) = p + v t + amp sin(omega t + phase), R(t) = Rz(yaw_rate t) R(q) (scene_dyn_ref.frame); the
image is mesh_ref's ray cast of all instances' triangles merged, the distance the minimum over the instances of
mesh_ref.distance of each.

Where every point has a time of its own the transformed vertices would have to be formed once per point; the reference
then takes the point into the part's frame instead, x' = R(t)^T (x - c(t)), the same rigid map read the other way
(tests/test_mesh_inst_ref.py holds the two against each other).  The SDF row's gradient is R(t) g' with g' from
mesh_sdf_ref.dist_grad in the part's frame, the strictly smaller distance winning, so the lowest index keeps a tie.

The fixed scene: four parts, eight instances of which five move."""
import numpy as np

import mesh_ref as M
import mesh_sdf_ref as MS
import scene_dyn_ref as DR
import scene_ref as R
from sdf_nmpc_amd.mesh import Mesh

TIMES = (0.0, 0.7)


def parts():
    return [Mesh.box((-0.5, -0.5, -0.5), (0.5, 0.5, 0.5)), Mesh.icosphere((0.0, 0.0, 0.0), 0.5, 2),
            Mesh.box((-8.0, -8.0, -0.0625), (8.0, 8.0, 0.0625)), Mesh.cylinder((0.0, 0.0), 0.25, -1.0, 1.0, 24)]


Z = (0.0, 0.0, 0.0)
# (part, p, rpy, v, yaw_rate, amp, omega, phase)
SPEC = [(2, (0.0, 0.0, -1.5625), Z, Z, 0.0, Z, 0.0, 0.0),
        (0, (3.75, 1.0, 0.125), (0.3, -0.2, 0.5), (0.0, -0.5, 0.0), 0.4, Z, 0.0, 0.0),
        (0, (1.5, -1.625, 0.0), (0.0, 0.0, 0.785), Z, 0.0, (0.0, 0.0, 0.25), 2.0, 0.3),
        (1, (2.5, 0.5, 0.25), Z, (0.25, 0.5, 0.0), 0.0, Z, 0.0, 0.0),
        (1, (4.5, -1.0, -0.5), (0.1, 0.2, 0.3), Z, 1.0, Z, 0.0, 0.0),
        (3, (2.0, 2.0, -0.5), (0.0, 0.2, 0.0), (0.0, -0.25, 0.0), 0.5, Z, 0.0, 0.0),
        (3, (5.0, 0.0, -0.5), Z, Z, 0.0, Z, 0.0, 0.0),
        (0, (3.0, -0.5, 0.9), (0.7, 0.1, -0.4), Z, -0.8, (0.5, 0.0, 0.0), 1.5, 0.0)]


def instance(part, p, rpy=Z, v=Z, yaw_rate=0.0, amp=Z, omega=0.0, phase=0.0, q=None):
    """The reference's record of an instance: the part, the position and scene_dyn_ref's motion (R0 a matrix)."""
    R0 = R.quat2rot(q) if q is not None else R.rpy2rot(*rpy)
    return dict(part=int(part), p=np.asarray(p, float), R0=R0, v=np.asarray(v, float), amp=np.asarray(amp, float),
                yaw_rate=float(yaw_rate), omega=float(omega), phase=float(phase))


def fixed_instances():
    return [instance(*s) for s in SPEC]


def scene_instances(spec=SPEC):
    """SPEC as Scene.instanced takes it"""
    from sdf_nmpc_amd.scene import Scene
    return [Scene.instance(part, p, rpy=rpy, v=v, yaw_rate=yr, amp=amp, omega=om, phase=ph)
            for part, p, rpy, v, yr, amp, om, ph in spec]


def rounded_parts(ps):
    return [M.rounded(m) for m in ps]


def frame(inst, t):
    """c(t) [..., 3], R(t) [..., 3, 3]"""
    return DR.frame(inst["p"], inst, t)


def placed(ps, insts, t):
    """The instances at the scalar time t as world meshes, one each: the rounded part's vertices under the frame."""
    out = []
    for i in insts:
        c, Rt = frame(i, float(t))
        m = M.rounded(ps[i["part"]])
        out.append(Mesh(m.verts @ Rt.T + c, m.tris))
    return out


def merged(ps, insts, t):
    return Mesh.merge(*placed(ps, insts, t))


def values(ps, insts, t, *a, **kw):
    return M.values(merged(ps, insts, t), *a, **kw)


def decided(ps, insts, t, *a, **kw):
    return M.decided(merged(ps, insts, t), *a, **kw)


def _local(inst, pts, t):
    """x' = R(t)^T (x - c(t)) for points [n, 3] at times t (a scalar or [n]); also R(t) [n, 3, 3]"""
    pts = np.asarray(pts, float).reshape(-1, 3)
    c, Rt = frame(inst, np.broadcast_to(np.asarray(t, float), (pts.shape[0],)))
    return np.einsum("nji,nj->ni", Rt, pts - c), Rt


def distance(ps, insts, pts, t=0.0, signed=False):
    """min over the instances of mesh_ref.distance of each [n]; +inf without instances.  t a scalar: the transformed
    vertices; t [n]: the points in the parts' frames."""
    pts = np.asarray(pts, float).reshape(-1, 3)
    best = np.full(pts.shape[0], np.inf)
    if np.ndim(t) == 0:
        for m in placed(ps, insts, t):
            best = np.minimum(best, M.distance(m, pts, signed=signed))
        return best
    rp = rounded_parts(ps)
    for i in insts:
        best = np.minimum(best, M.distance(rp[i["part"]], _local(i, pts, t)[0], signed=signed))
    return best


def dist_grad(ps, insts, pts, t=0.0, signed=False):
    """(d [n], g [n, 3], which [n]): the untruncated distance, the world gradient R(t) g' of the minimising instance (the
    lowest index on a tie) and its index, -1 where there is none"""
    pts = np.asarray(pts, float).reshape(-1, 3)
    n = pts.shape[0]
    best, g, which = np.full(n, np.inf), np.zeros((n, 3)), np.full(n, -1)
    rp = rounded_parts(ps)
    for k, i in enumerate(insts):
        q, Rt = _local(i, pts, t)
        d, gl = MS.dist_grad(rp[i["part"]], q, signed)
        lower = d < best
        best = np.where(lower, d, best)
        g = np.where(lower[:, None], np.einsum("nij,nj->ni", Rt, gl), g)
        which = np.where(lower, k, which)
    return best, g, which


def speed_bound(ps, insts):
    """max over the instances of |v| + |omega| |amp| + |yaw_rate| rho, rho the largest |vertex| of the rounded part"""
    rho = [np.linalg.norm(m.verts, axis=1).max() if len(m.verts) else 0.0 for m in rounded_parts(ps)]
    return max([np.linalg.norm(i["v"]) + abs(i["omega"]) * np.linalg.norm(i["amp"]) + abs(i["yaw_rate"]) * rho[i["part"]]
                for i in insts], default=0.0)
