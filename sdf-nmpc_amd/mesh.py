"""Triangle meshes on the host: what ``Scene.mesh`` takes.  A ``Mesh`` is two arrays, ``verts`` [nv, 3] float64 and
``tris`` [nt, 3] int32 (indices into verts, counter-clockwise seen from outside where there is an outside), with a few
procedural generators -- each a pure function of its arguments -- and an OBJ reader.  Nothing here touches the device:
the library checks a mesh, rounds it to fp32 and builds its hierarchy when the scene is created (csrc/mesh_bvh.h).

    cave = Mesh.tunnel([(0, 0, 0), (4, 0.5, 0), (8, -0.5, 0.3)], radius=1.2, roughness=0.15, seed=3)
    scene = Scene.mesh(ctx, cave)                     # open surfaces: unsigned distance
    rocks = Mesh.merge(Mesh.icosphere((3, 0, 0), 0.5, 2), Mesh.box((4, -1, -1), (5, 1, 1)))
    scene = Scene.mesh(ctx, rocks, closed=True)       # closed manifolds: signed distance, negative inside
"""
from __future__ import annotations

import numpy as np


class Mesh:
    def __init__(self, verts, tris):
        self.verts = np.array(verts, dtype=np.float64).reshape(-1, 3)
        self.tris = np.array(tris, dtype=np.int32).reshape(-1, 3)

    # ---- combining and moving
    @staticmethod
    def merge(*meshes):
        """One mesh of all the triangles, the vertices of each kept apart (nothing is welded)."""
        verts, tris, off = [], [], 0
        for m in meshes:
            verts.append(m.verts)
            tris.append(m.tris + off)
            off += m.verts.shape[0]
        if not verts:
            return Mesh(np.zeros((0, 3)), np.zeros((0, 3), np.int32))
        return Mesh(np.concatenate(verts, 0), np.concatenate(tris, 0))

    def transformed(self, R=None, t=None, scale=1.0):
        """v -> scale R v + t: R a rotation [3, 3] (None: the identity), t a translation, scale > 0."""
        scale = float(scale)
        if not (np.isfinite(scale) and scale > 0.0):
            raise ValueError("Mesh.transformed: scale must be positive and finite")
        v = self.verts if R is None else self.verts @ np.asarray(R, dtype=np.float64).reshape(3, 3).T
        v = scale * v
        if t is not None:
            v = v + np.asarray(t, dtype=np.float64).reshape(3)
        return Mesh(v, self.tris)

    def is_closed(self):
        """Whether every edge is shared by exactly two triangles that traverse it in opposite directions: a closed,
        consistently oriented manifold, what ``Scene.mesh(closed=True)`` requires (the library checks it again)."""
        t = self.tris.astype(np.int64)
        if t.shape[0] == 0:
            return True
        a = np.concatenate([t[:, 0], t[:, 1], t[:, 2]])
        b = np.concatenate([t[:, 1], t[:, 2], t[:, 0]])
        fwd, rev = np.sort(a << 32 | b), np.sort(b << 32 | a)
        return bool(np.all(fwd[1:] != fwd[:-1]) and np.array_equal(fwd, rev))

    # ---- generators
    @staticmethod
    def box(lo, hi):
        """The axis-aligned box lo .. hi: 8 vertices, 12 triangles, outward orientation."""
        lo, hi = np.asarray(lo, dtype=np.float64).reshape(3), np.asarray(hi, dtype=np.float64).reshape(3)
        v = np.array([[(hi if i >> a & 1 else lo)[a] for a in range(3)] for i in range(8)])
        t = [(0, 2, 3), (0, 3, 1), (4, 5, 7), (4, 7, 6), (0, 1, 5), (0, 5, 4), (2, 7, 3), (2, 6, 7), (0, 4, 6), (0, 6, 2),
             (1, 3, 7), (1, 7, 5)]
        return Mesh(v, t)

    @staticmethod
    def icosphere(center, radius, subdiv):
        """An icosahedron subdivided subdiv times (20 * 4^subdiv triangles), every vertex on the sphere."""
        g = (1.0 + np.sqrt(5.0)) / 2.0
        v = [(-1, g, 0), (1, g, 0), (-1, -g, 0), (1, -g, 0), (0, -1, g), (0, 1, g), (0, -1, -g), (0, 1, -g), (g, 0, -1),
             (g, 0, 1), (-g, 0, -1), (-g, 0, 1)]
        v = [np.asarray(p, dtype=np.float64) / np.sqrt(1.0 + g * g) for p in v]
        t = [(0, 11, 5), (0, 5, 1), (0, 1, 7), (0, 7, 10), (0, 10, 11), (1, 5, 9), (5, 11, 4), (11, 10, 2), (10, 7, 6),
             (7, 1, 8), (3, 9, 4), (3, 4, 2), (3, 2, 6), (3, 6, 8), (3, 8, 9), (4, 9, 5), (2, 4, 11), (6, 2, 10), (8, 6, 7),
             (9, 8, 1)]
        for _ in range(int(subdiv)):
            mid, nt = {}, []

            def m(a, b):
                key = (min(a, b), max(a, b))
                if key not in mid:
                    p = v[a] + v[b]
                    v.append(p / np.linalg.norm(p))
                    mid[key] = len(v) - 1
                return mid[key]

            for a, b, c in t:
                ab, bc, ca = m(a, b), m(b, c), m(c, a)
                nt += [(a, ab, ca), (b, bc, ab), (c, ca, bc), (ab, bc, ca)]
            t = nt
        return Mesh(np.asarray(center, dtype=np.float64).reshape(3) + float(radius) * np.array(v), t)

    @staticmethod
    def cylinder(center_xy, radius, z0, z1, segments):
        """A capped cylinder along z, closed: `segments` side quads with their vertices on the circle, and a fan per
        cap.  The surface lies inside the true cylinder, within the sagitta radius (1 - cos(pi / segments)) of it."""
        n = int(segments)
        if n < 3:
            raise ValueError("Mesh.cylinder: at least 3 segments")
        cx, cy = (float(c) for c in center_xy)
        ang = 2.0 * np.pi * np.arange(n) / n
        ring = np.stack([cx + float(radius) * np.cos(ang), cy + float(radius) * np.sin(ang)], 1)
        v = np.concatenate([np.column_stack([ring, np.full(n, float(z0))]), np.column_stack([ring, np.full(n, float(z1))]),
                            [[cx, cy, float(z0)], [cx, cy, float(z1)]]], 0)
        t = []
        for i in range(n):
            j = (i + 1) % n
            t += [(i, j, n + j), (i, n + j, n + i), (2 * n, j, i), (2 * n + 1, n + i, n + j)]
        return Mesh(v, t)

    @staticmethod
    def heightfield(x0, y0, dx, dy, Z):
        """Open terrain: Z [nx, ny] is the height at (x0 + i dx, y0 + j dy); two triangles per cell, facing up."""
        Z = np.asarray(Z, dtype=np.float64)
        if Z.ndim != 2 or Z.shape[0] < 2 or Z.shape[1] < 2:
            raise ValueError("Mesh.heightfield: Z must be a 2-D array of at least 2 x 2")
        nx, ny = Z.shape
        i, j = np.meshgrid(np.arange(nx), np.arange(ny), indexing="ij")
        v = np.stack([float(x0) + float(dx) * i, float(y0) + float(dy) * j, Z], -1).reshape(-1, 3)
        a = (i[:-1, :-1] * ny + j[:-1, :-1]).ravel()
        t = np.concatenate([np.stack([a, a + ny, a + ny + 1], 1), np.stack([a, a + ny + 1, a + 1], 1)], 0)
        return Mesh(v, t)

    @staticmethod
    def tunnel(path, radius, segments=16, roughness=0.0, seed=0):
        """An open tube around the polyline `path` [n >= 2, 3]: one ring of `segments` vertices per path point, in the
        plane across the path there, of radius `radius` (1 + roughness u) with u uniform in [-1, 1) per ring through
        numpy.random.default_rng(seed).  No caps; the cave a vehicle flies inside."""
        p = np.asarray(path, dtype=np.float64).reshape(-1, 3)
        n, m = p.shape[0], int(segments)
        if n < 2 or m < 3 or not 0.0 <= float(roughness) < 1.0:
            raise ValueError("Mesh.tunnel: at least 2 path points, 3 segments and 0 <= roughness < 1")
        tan = np.gradient(p, axis=0)
        tan /= np.linalg.norm(tan, axis=1, keepdims=True)
        rad = float(radius) * (1.0 + float(roughness) * np.random.default_rng(seed).uniform(-1.0, 1.0, size=n))
        ang = 2.0 * np.pi * np.arange(m) / m
        v = np.empty((n, m, 3))
        for k in range(n):
            up = np.array([0.0, 0.0, 1.0]) if abs(tan[k, 2]) < 0.9 else np.array([1.0, 0.0, 0.0])
            e1 = np.cross(up, tan[k])
            e1 /= np.linalg.norm(e1)
            e2 = np.cross(tan[k], e1)
            v[k] = p[k] + rad[k] * (np.cos(ang)[:, None] * e1 + np.sin(ang)[:, None] * e2)
        t = []
        for k in range(n - 1):
            for i in range(m):
                j = (i + 1) % m
                a, b, c, d = k * m + i, k * m + j, (k + 1) * m + j, (k + 1) * m + i
                t += [(a, b, c), (a, c, d)]
        return Mesh(v.reshape(-1, 3), t)

    # ---- OBJ
    @staticmethod
    def from_obj(path):
        """Reads the `v` and `f` lines of a Wavefront OBJ file and nothing else; a polygon becomes a fan about its first
        vertex; `f` entries may carry texture / normal indices (v/vt/vn) and may be negative (relative)."""
        verts, tris = [], []
        with open(path) as f:
            for line in f:
                w = line.split()
                if not w:
                    continue
                if w[0] == "v":
                    verts.append([float(x) for x in w[1:4]])
                elif w[0] == "f":
                    idx = [int(x.split("/")[0]) for x in w[1:]]
                    idx = [i - 1 if i > 0 else len(verts) + i for i in idx]
                    tris += [(idx[0], idx[k], idx[k + 1]) for k in range(1, len(idx) - 1)]
        return Mesh(np.array(verts, dtype=np.float64).reshape(-1, 3), np.array(tris, dtype=np.int32).reshape(-1, 3))

    def to_obj(self, path):
        with open(path, "w") as f:
            for v in self.verts:
                f.write("v %r %r %r\n" % tuple(float(x) for x in v))
            for t in self.tris:
                f.write("f %d %d %d\n" % tuple(int(i) + 1 for i in t))
