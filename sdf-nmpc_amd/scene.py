"""Analytic scenes on the device (csrc/scene.hip through the C ABI, sdfnmpc_scene_*): the range or depth image a
sensor of the config would take of a known world from a camera pose, the camera pose of a state, and the exact
signed distance from a point to the world.

The reference has no counterpart -- its images come from the simulator it is run against.  A ``Scene`` is the
producer in front of what the package already consumes: ``VaeWrapper.set_img`` (raw images), ``ColChecker`` /
``DfComputer`` (normalised images) and ``Nmpc.rollout(scene=...)``, which takes a new image of the scene from every
instance's current pose inside the device loop.

    scene = Scene(ctx, [Scene.sphere((2.5, -0.8, 0.3), 0.5), Scene.box((3.5, 0.5, -1), (4.1, 1.5, 1.2)),
                        Scene.cylinder((3.0, 0.3), 0.4, -1.5, 1.5)])
    img = scene.render_from_state(x, cfg)            # DeviceArray [B, h, w] float32, normalised by sensor.dmax
    d = scene.distance(points)                       # numpy [n] float64, negative inside

Primitives may be oriented and may move: ``Scene.moving(prim, v=, q= | rpy=, yaw_rate=, amp=, omega=, phase=)`` gives
a primitive the rigid frame c(t) = c0 + v t + amp sin(omega t + phase), R(t) = Rz(yaw_rate t) R(q) about its reference
point c0 (sphere: centre; box: (lo + hi) / 2; cylinder: (cx, cy, (z0 + z1) / 2)) -- a box with a rotation is an
oriented box, a sphere with v a moving obstacle.  ``render(..., t=)``, ``render_from_state(..., t=)`` and
``distance(..., t=)`` then show the scene at time t; a scene without such primitives is the static scene whatever t.

A scene of more than 32 primitives takes a grid index: ``Scene(ctx, Scene.forest(1024, lo, hi), grid=True)`` holds up
to 65536 static primitives per scene, and every call above -- and every consumer of a scene -- returns what the plain
scene would return, bit for bit, from kernels that visit only the grid cells along a ray or around a point.  A few
moving obstacles go beside it: ``Scene(ctx, forest, grid=True, movers=Scene.crowd(8, lo, hi))``.

A world that is a surface -- a cave, a building, terrain -- is a triangle mesh: ``Scene.mesh(ctx, Mesh.tunnel(path, 1.2))``
holds one static ``mesh.Mesh`` per scene behind a bounding-volume hierarchy (csrc/scene_mesh.hip); ``render``,
``distance``, ``swept_distance`` and the rollouts take it like any other scene, and so does ``Nmpc.set_sdf_scene`` when
the scene is created with ``sdf_source=True`` (csrc/scene_mesh.hip: scene_sdf_rows_mesh_kernel).  Something crossing
the vehicle's path goes beside it: ``Scene.mesh(ctx, tunnel, movers=[Scene.moving(Scene.sphere(c, 0.4), v=v)])``.

A world of repeated or moving objects -- a forest of tree meshes, shelves with a forklift driving between them, a door
that swings -- is a list of instances: ``Scene.instanced(ctx, [tree, rock], Scene.scatter(200, lo, hi, parts=2))``
stores every part once and places it by rigid frames, ``Scene.instance(part, pos, rpy=, v=, yaw_rate=, ...)``, that may
move as a ``Scene.moving`` primitive does (csrc/scene_inst.hip); up to 256 instances per scene, every query the
minimum over them at its time.

World frame z up; camera frame x forward, y left, z up, the pixel grid of ``ColChecker``.  There is no CPU path.
"""
from __future__ import annotations

import weakref

import numpy as np

from . import _lib


def _three(a, name):
    a = [float(v) for v in a]
    if len(a) != 3:
        raise ValueError(f"Scene.moving: {name} has three components")
    return a


def _is_prim(p):
    return isinstance(p, tuple) and len(p) in (2, 3) and isinstance(p[0], (str, int))


def _flatten(scenes):
    """lists of primitives, one per scene -> (flat list of (kind, values), one motion dict or None per primitive)"""
    flat, motion = [], []
    for s in scenes:
        for kind, vals, *mo in s:
            vals = list(vals)
            if len(vals) > 6:
                raise ValueError(f"primitive {kind!r}: at most 6 values, got {len(vals)}")
            # an unknown kind goes to the library as it is (it refuses it)
            flat.append((_lib.PRIM_KINDS.get(kind, kind if isinstance(kind, int) else -1), vals))
            motion.append(mo[0] if mo else None)
    return flat, motion


def _mover_lists(movers, S):
    """``movers`` as Scene and Scene.mesh take it -> one list per scene: an empty list is no mover anywhere, a flat list
    of primitives the movers of a single scene, else one list per scene (ValueError when their number is not S)"""
    movers = list(movers)
    mlists = [[] for _ in range(S)] if not movers else \
        [movers] if all(_is_prim(p) for p in movers) else [list(m) for m in movers]
    if len(mlists) != S:
        raise ValueError(f"Scene: movers holds {len(mlists)} lists for {S} scenes")
    return mlists


class Swept:
    """What ``Scene.swept_distance`` returns, arrays [n]: dmin, s, gap (float64) and evals (int32)."""

    def __init__(self, dmin, s, gap, evals):
        self.dmin, self.s, self.gap, self.evals = dmin, s, gap, evals


class Scene:
    """One scene (a list of primitives) or several (a list of lists) with ``scene_of`` [B], the scene of each
    instance; without ``scene_of`` every instance sees scene 0.  At most 32 primitives per scene; with ``grid=True``
    at most 65536 static ones, indexed by a uniform grid of cell edge ``cell`` [m] (None: the library's default, a
    function of the primitives) -- ``is_indexed``.  An indexed scene may also hold ``movers``: a list of at most 32
    plain or ``Scene.moving`` primitives (a list of lists, one per scene, for several scenes) that are not in the grid
    and may move anywhere; every query then is the minimum over both sets at its time, and the scene is both
    ``is_indexed`` and ``is_dynamic``.  The primitives are checked by the library when the scene is
    created (SdfnmpcError: too many, an unknown kind, a radius <= 0, lo >= hi, a grid too fine); ``scene_of``, ``cell``,
    ``movers`` without ``grid`` or of another number of scenes, and a moving primitive among ``prims`` of an indexed
    scene (ValueError) are checked here."""

    @staticmethod
    def sphere(center, radius):
        return ("sphere", [float(v) for v in center] + [float(radius)])

    @staticmethod
    def box(lo, hi):
        return ("box", [float(v) for v in lo] + [float(v) for v in hi])

    @staticmethod
    def cylinder(center_xy, radius, z0, z1):
        """A capped cylinder along z: axis through center_xy, z in [z0, z1]."""
        return ("cylinder", [float(v) for v in center_xy] + [float(radius), float(z0), float(z1)])

    @staticmethod
    def moving(prim, *, v=(0.0, 0.0, 0.0), q=None, rpy=None, yaw_rate=0.0, amp=(0.0, 0.0, 0.0), omega=0.0, phase=0.0):
        """The primitive with a frame that depends on time: orientation q = (w, x, y, z) of any non-zero norm or
        rpy = (roll, pitch, yaw), ZYX (not both), about its reference point; yaw_rate [rad/s] about the world z axis;
        velocity v [m/s]; a harmonic term amp sin(omega t + phase).  The library checks the values when the scene is
        created (SdfnmpcError: a non-finite value, a zero quaternion)."""
        if q is not None and rpy is not None:
            raise ValueError("Scene.moving: give q or rpy, not both")
        if rpy is not None:
            (cr, sr), (cp, sp), (cy, sy) = ((np.cos(0.5 * float(a)), np.sin(0.5 * float(a))) for a in rpy)
            q = (cr * cp * cy + sr * sp * sy, sr * cp * cy - cr * sp * sy, cr * sp * cy + sr * cp * sy,
                 cr * cp * sy - sr * sp * cy)
        m = dict(q=[float(a) for a in (q if q is not None else (1.0, 0.0, 0.0, 0.0))], v=_three(v, "v"),
                 amp=_three(amp, "amp"), yaw_rate=float(yaw_rate), omega=float(omega), phase=float(phase))
        if len(m["q"]) != 4:
            raise ValueError("Scene.moving: q = (w, x, y, z)")
        return (prim[0], list(prim[1]), m)

    @staticmethod
    def forest(n, lo, hi, radius=(0.15, 0.4), seed=0, keep_clear=None):
        """A list of n upright cylinders in the box lo .. hi (three components each): axes uniform in xy, radii uniform
        in radius = (r0, r1), every cylinder from lo[2] to hi[2].  keep_clear = (centre_xy, radius): a cylinder whose
        axis lies within that circle is moved radially out of it, onto its rim (one on the centre: along +x).  A pure
        function of its arguments through numpy.random.default_rng(seed)."""
        lo, hi = _three(lo, "lo"), _three(hi, "hi")
        r0, r1 = (float(v) for v in radius)
        n = int(n)
        if n < 0 or not (lo[0] < hi[0] and lo[1] < hi[1] and lo[2] < hi[2]) or not 0.0 < r0 <= r1:
            raise ValueError("Scene.forest: n >= 0, lo < hi and 0 < r0 <= r1 required")
        rng = np.random.default_rng(seed)
        xy = rng.uniform(lo[:2], hi[:2], size=(n, 2))
        rad = rng.uniform(r0, r1, size=n)
        if keep_clear is not None:
            c, rc = np.asarray(keep_clear[0], dtype=np.float64).reshape(2), float(keep_clear[1])
            e = xy - c
            dist = np.hypot(e[:, 0], e[:, 1])
            inside = dist < rc
            e[dist == 0.0] = (1.0, 0.0)
            dist = np.where(dist == 0.0, 1.0, dist)
            xy = np.where(inside[:, None], c + e * (rc * (1.0 + 1e-9) / dist)[:, None], xy)
        return [Scene.cylinder(xy[i], rad[i], lo[2], hi[2]) for i in range(n)]

    @staticmethod
    def crowd(n, lo, hi, radius=(0.2, 0.35), height=1.8, speed=(0.5, 1.5), seed=0):
        """A list of n moving upright cylinders in the box lo .. hi, the mover counterpart of ``forest``: radii uniform
        in radius = (r0, r1), every cylinder from lo[2] to lo[2] + height, each swinging as amp sin(omega t + phase)
        along a random horizontal direction about a centre uniform in the box.  amp is 0.5 to 0.95 of the largest
        amplitude that keeps the cylinder inside lo .. hi for every t, the peak speed amp omega is uniform in speed =
        (s0, s1) [m/s], the phase uniform in [0, 2 pi).  A pure function of its arguments through
        numpy.random.default_rng(seed)."""
        lo, hi = _three(lo, "lo"), _three(hi, "hi")
        r0, r1 = (float(v) for v in radius)
        s0, s1 = (float(v) for v in speed)
        n, height = int(n), float(height)
        if n < 0 or not (lo[0] < hi[0] and lo[1] < hi[1] and lo[2] < hi[2]) or not 0.0 < r0 <= r1 or not 0.0 < s0 <= s1:
            raise ValueError("Scene.crowd: n >= 0, lo < hi, 0 < r0 <= r1 and 0 < s0 <= s1 required")
        if not 0.0 < height <= hi[2] - lo[2] or not (hi[0] - lo[0] > 2.0 * r1 and hi[1] - lo[1] > 2.0 * r1):
            raise ValueError("Scene.crowd: 0 < height <= hi[2] - lo[2] and a box wider than 2 r1 required")
        rng = np.random.default_rng(seed)
        rad = rng.uniform(r0, r1, size=n)
        u = rng.uniform(0.0, 1.0, size=(n, 2))
        ang = rng.uniform(0.0, 2.0 * np.pi, size=n)
        frac = rng.uniform(0.5, 0.95, size=n)
        peak = rng.uniform(s0, s1, size=n)
        phase = rng.uniform(0.0, 2.0 * np.pi, size=n)
        out = []
        for i in range(n):
            room_lo, room_hi = np.array(lo[:2]) + rad[i], np.array(hi[:2]) - rad[i]
            c = room_lo + u[i] * (room_hi - room_lo)
            d = np.array([np.cos(ang[i]), np.sin(ang[i])])
            with np.errstate(divide="ignore"):  # a direction along an axis: no limit from the other one
                amax = float(np.min(np.minimum(c - room_lo, room_hi - c) / np.abs(d)))
            a = frac[i] * max(amax, 0.0)
            omega = peak[i] / a if a > 0.0 else 0.0
            out.append(Scene.moving(Scene.cylinder(c, rad[i], lo[2], lo[2] + height), amp=(a * d[0], a * d[1], 0.0),
                                    omega=omega, phase=phase[i]))
        return out

    def __init__(self, ctx: "_lib.Context", prims, scene_of=None, grid=False, cell=None, movers=None):
        scenes = [list(prims)] if all(_is_prim(p) for p in prims) else [list(s) for s in prims]
        flat, motion = _flatten(scenes)
        self.ctx, self.S = ctx, len(scenes)
        self._sdf_users = weakref.WeakSet()  # controllers whose SDF source this scene is (Nmpc.set_sdf_scene)
        if movers is not None and not grid:
            raise ValueError("Scene: movers need grid=True (a plain scene takes Scene.moving primitives in prims)")
        if grid:
            if any(m is not None for m in motion):
                raise ValueError("Scene: an indexed scene (grid=True) holds static primitives only, no Scene.moving "
                                 "(moving primitives go into movers=)")
            if cell is not None and not (np.isfinite(float(cell)) and float(cell) > 0.0):
                raise ValueError("Scene: cell must be positive and finite (None: the default)")
            cell = 0.0 if cell is None else float(cell)
            if movers is None:  # the call an indexed scene has always made
                self.h = _lib.scene_create_large(ctx, [len(s) for s in scenes], flat, cell)
            else:
                mlists = _mover_lists(movers, len(scenes))
                mflat, mmotion = _flatten(mlists)
                self.h = _lib.scene_create_mixed(ctx, [len(s) for s in scenes], flat, cell, [len(m) for m in mlists],
                                                 mflat, mmotion if any(m is not None for m in mmotion) else None)
        else:
            if cell is not None:
                raise ValueError("Scene: cell needs grid=True")
            # plain primitives only: the call a scene has always made
            self.h = _lib.scene_create(ctx, [len(s) for s in scenes], flat,
                                       motion if any(m is not None for m in motion) else None)
        self.is_dynamic = bool(_lib.load().sdfnmpc_scene_is_dynamic(self.h))
        self.is_indexed = bool(_lib.load().sdfnmpc_scene_is_indexed(self.h))
        self.is_mesh = self.is_instanced = False
        self.is_sdf_source = bool(_lib.load().sdfnmpc_scene_is_sdf_source(self.h))  # every set that is not a mesh set
        self._set_scene_of(scene_of)

    @classmethod
    def mesh(cls, ctx: "_lib.Context", meshes, scene_of=None, closed=False, leaf_size=None, sdf_source=False, movers=None):
        """A scene set of triangle meshes: one ``mesh.Mesh`` or a list of them (S scenes, ``scene_of`` [B] as above), each
        a static surface behind a bounding-volume hierarchy that the library builds when the scene is created
        (csrc/mesh_bvh.h) -- ``is_mesh``.  closed=False: open surfaces, ``distance`` is unsigned.  closed=True: every mesh
        must be a closed, consistently oriented manifold (``Mesh.is_closed``) and ``distance`` is negative inside.
        leaf_size: 1..8 triangles per leaf (None: the library's default, 4), or -1 for no hierarchy at all -- every
        result is the same bit for bit, only slower.  ``render``, ``render_from_state``, ``distance``,
        ``swept_distance``, ``speed_bound`` (0) and ``Nmpc.rollout(scene=)`` take it like any other scene; hits are
        double-sided, and a camera inside a closed mesh sees its inner walls.

        sdf_source=True: ``Nmpc.set_sdf_scene`` (and ``_lib.scene_sdf_rows``, ``lin_args.sdf_scene``) accept the scene
        as the controller's exact SDF -- ``is_sdf_source``: the value of ``distance`` bit for bit, truncated at max_df,
        with the gradient (p - c) / |p - c| to the closest point c (negated inside a closed mesh); an open scene is
        searched only within max_df of each node.  With the default False they refuse it (SdfnmpcError, error -4), as
        they refused every mesh scene when meshes were first built: a test of the project pins that refusal for a
        scene made by ``Scene.mesh(ctx, mesh, closed=True)`` and must keep passing as it is, so a mesh scene is a
        source only when it is created as one.  Nothing else about the scene depends on the option.

        movers: moving obstacles beside the meshes, parsed as ``Scene(..., grid=True, movers=)`` parses them -- one flat
        list of at most 32 plain or ``Scene.moving`` primitives for a single scene (``Scene.crowd(...)`` as it is), or
        a list of lists, one per mesh (another number of lists: ValueError).  Every query then is the minimum over the
        mesh and the movers at its time (csrc/scene_mesh.hip's *_mesh_mixed kernels): ``render(t=)``,
        ``distance(t=)``, ``swept_distance(t0=, t1=)``, ``speed_bound`` (the movers') and, with sdf_source=True, the
        SDF rows, where the mesh keeps a tie with a mover; the scene is ``is_mesh`` and ``is_dynamic``, and
        ``Nmpc.rollout`` runs its scene clock.  None: the call ``Scene.mesh`` has always made; [] (or no mover in any
        list): the plain mesh scene.

        The library refuses a malformed mesh (SdfnmpcError): a non-finite vertex, an index out of range, a triangle
        of zero area, closed=True on a surface with a boundary or a flipped triangle, an sdf_source other than a
        boolean (0 or 1); and of the movers what ``Scene`` refuses of its own."""
        from .mesh import Mesh
        ms = [meshes] if isinstance(meshes, Mesh) else list(meshes)
        self = cls.__new__(cls)
        self.ctx, self.S = ctx, len(ms)
        self._sdf_users = weakref.WeakSet()
        extra = {}
        if movers is not None:
            mlists = _mover_lists(movers, len(ms))
            mflat, mmotion = _flatten(mlists)
            extra = dict(mcounts=[len(m) for m in mlists], mprims=mflat,
                         mmotion=mmotion if any(m is not None for m in mmotion) else None)
        self.h = _lib.scene_create_mesh(ctx, [m.verts for m in ms], [m.tris for m in ms],
                                        0 if leaf_size is None else int(leaf_size), bool(closed), sdf_source, **extra)
        self.is_dynamic = bool(_lib.load().sdfnmpc_scene_is_dynamic(self.h))
        self.is_indexed = bool(_lib.load().sdfnmpc_scene_is_indexed(self.h))
        self.is_mesh = bool(_lib.load().sdfnmpc_scene_is_mesh(self.h))
        self.is_instanced = False
        self.is_sdf_source = bool(_lib.load().sdfnmpc_scene_is_sdf_source(self.h))
        self._set_scene_of(scene_of)
        return self

    # ---- instanced mesh scenes
    @staticmethod
    def instance(part, pos, *, q=None, rpy=None, v=(0.0, 0.0, 0.0), yaw_rate=0.0, amp=(0.0, 0.0, 0.0), omega=0.0,
                 phase=0.0):
        """One instance for ``Scene.instanced``: part ``part`` of the pool with its origin at ``pos`` and the frame of
        ``Scene.moving`` about it -- orientation q = (w, x, y, z) or rpy (not both), yaw_rate about the world z axis,
        velocity v, a harmonic term amp sin(omega t + phase): c(t) = pos + v t + amp sin(omega t + phase),
        R(t) = Rz(yaw_rate t) R(q).  Rigid: there is no scale."""
        m = Scene.moving(("sphere", [0.0, 0.0, 0.0, 1.0]), v=v, q=q, rpy=rpy, yaw_rate=yaw_rate, amp=amp, omega=omega,
                         phase=phase)[2]
        return ("instance", int(part), _three(pos, "pos"), m)

    @staticmethod
    def scatter(n, lo, hi, parts=1, seed=0, keep_clear=None, yaw=True):
        """A list of n static instances in the box lo .. hi (three components each), the instances' ``forest``: the part
        of each drawn uniformly from range(parts) (or from the sequence of indices ``parts``), its origin uniform in
        the box, and with yaw=True a yaw uniform in [0, 2 pi).  keep_clear = (centre_xy, radius): an origin within that
        circle is moved radially out of it, onto its rim, as ``forest`` moves an axis.  A pure function of its arguments
        through numpy.random.default_rng(seed)."""
        lo, hi = _three(lo, "lo"), _three(hi, "hi")
        n = int(n)
        pool = list(range(int(parts))) if np.ndim(parts) == 0 else [int(p) for p in parts]
        if n < 0 or not (lo[0] <= hi[0] and lo[1] <= hi[1] and lo[2] <= hi[2]) or not pool:
            raise ValueError("Scene.scatter: n >= 0, lo <= hi and at least one part required")
        rng = np.random.default_rng(seed)
        pos = rng.uniform(lo, hi, size=(n, 3))
        which = rng.integers(0, len(pool), size=n)
        ang = rng.uniform(0.0, 2.0 * np.pi, size=n)
        if keep_clear is not None:
            c, rc = np.asarray(keep_clear[0], dtype=np.float64).reshape(2), float(keep_clear[1])
            e = pos[:, :2] - c
            dist = np.hypot(e[:, 0], e[:, 1])
            inside = dist < rc
            e[dist == 0.0] = (1.0, 0.0)
            dist = np.where(dist == 0.0, 1.0, dist)
            pos[:, :2] = np.where(inside[:, None], c + e * (rc * (1.0 + 1e-9) / dist)[:, None], pos[:, :2])
        return [Scene.instance(pool[which[i]], pos[i], rpy=(0.0, 0.0, ang[i] if yaw else 0.0)) for i in range(n)]

    @classmethod
    def instanced(cls, ctx: "_lib.Context", parts, instances, scene_of=None, closed=False, leaf_size=None,
                  sdf_source=False):
        """A scene set of instances -- ``is_instanced``: ``parts`` is the pool, one ``mesh.Mesh`` or a list of them, each
        checked, rounded and put behind its own hierarchy as a scene of ``Scene.mesh`` is and stored once; ``instances``
        one flat list of ``Scene.instance`` for a single scene (``Scene.scatter(...)`` as it is, [] for an empty scene),
        or one list per scene (``scene_of`` [B] as above), at most 256 each.  closed, leaf_size and sdf_source mean what
        they mean for ``Scene.mesh``; closed=True needs every part closed, and ``distance`` is then the minimum of the
        instances' signed distances -- the union, instances may overlap.

        Every query is the minimum over the scene's instances at its time (csrc/scene_inst.hip): ``render(t=)``,
        ``render_from_state``, ``distance(t=)``, ``swept_distance``, ``speed_bound``, ``Rollout.clearance``, every
        ``Nmpc.rollout(scene=)`` and, with sdf_source=True, ``Nmpc.set_sdf_scene(..., predict=)``; the results depend
        neither on leaf_size nor on the order of the instances.  ``is_dynamic`` exactly when some instance has a
        non-zero v, amp or yaw_rate; ``is_mesh`` and ``is_indexed`` are False.  A scene without instances renders a miss
        everywhere and is at distance +inf.

        The library refuses (SdfnmpcError) a part index outside the pool, more than 256 instances in a scene, a zero
        quaternion, a non-finite value, and of a part what ``Scene.mesh`` refuses of a mesh."""
        from .mesh import Mesh
        ps = [parts] if isinstance(parts, Mesh) else list(parts)
        instances = list(instances)
        is_inst = lambda p: isinstance(p, tuple) and len(p) == 4 and p[0] == "instance"  # noqa: E731
        lists = [instances] if all(is_inst(p) for p in instances) else [list(s) for s in instances]
        for s in lists:
            if not all(is_inst(p) for p in s):
                raise ValueError("Scene.instanced: instances holds Scene.instance(...) entries, or one list of them per scene")
        self = cls.__new__(cls)
        self.ctx, self.S = ctx, len(lists)
        self._sdf_users = weakref.WeakSet()
        self.h = _lib.scene_create_instanced(ctx, [m.verts for m in ps], [m.tris for m in ps], [len(s) for s in lists],
                                             [(p[1], p[2], p[3]) for s in lists for p in s],
                                             0 if leaf_size is None else int(leaf_size), bool(closed), sdf_source)
        self.is_dynamic = bool(_lib.load().sdfnmpc_scene_is_dynamic(self.h))
        self.is_indexed = bool(_lib.load().sdfnmpc_scene_is_indexed(self.h))
        self.is_mesh = bool(_lib.load().sdfnmpc_scene_is_mesh(self.h))
        self.is_instanced = bool(_lib.load().sdfnmpc_scene_is_instanced(self.h))
        self.is_sdf_source = bool(_lib.load().sdfnmpc_scene_is_sdf_source(self.h))
        self._set_scene_of(scene_of)
        return self

    def _set_scene_of(self, scene_of):
        self.scene_of = self._scene_of = None
        if scene_of is not None:
            so = np.ascontiguousarray(scene_of, dtype=np.int32).ravel()
            if so.size and (so.min() < 0 or so.max() >= self.S):
                raise ValueError(f"scene_of entries must lie in [0, {self.S})")
            self.scene_of = so
            self._scene_of = _lib.DeviceArray.from_numpy(self.ctx, so)

    # ---- helpers
    def _f64(self, a, shape):
        """Host array -> device fp64 of `shape`; a device fp64 array of that many elements passes through."""
        if hasattr(a, "data_ptr"):
            if np.dtype(str(a.dtype).replace("torch.", "")) != np.float64:
                raise TypeError(f"device input must be float64, got {a.dtype}")
            if int(np.prod(a.shape)) != int(np.prod(shape)):
                raise ValueError(f"expected a device array of shape {shape}, got {tuple(a.shape)}")
            return _lib.sync_producer(a)
        return _lib.DeviceArray.from_numpy(self.ctx, np.reshape(np.asarray(a, dtype=np.float64), shape))

    def _batch(self, B):
        if self.scene_of is not None and self.scene_of.size != B:
            raise ValueError(f"scene_of names {self.scene_of.size} instances, the call has {B}")

    @staticmethod
    def img_opts(cfg):
        s = cfg.sensor
        return _lib.img_opts(s.dmax, s.hfov, s.vfov, s.is_depth, s.is_spherical)

    @staticmethod
    def scale(cfg, normalized=True) -> float:
        """Pixel value per metre: 1 / dmax (the images ColChecker / DfComputer read) or 1000 / mm_resolution (the
        raw sensor images VaeWrapper.set_img expects)."""
        return 1.0 / float(cfg.sensor.dmax) if normalized else 1000.0 / float(cfg.sensor.mm_resolution)

    # ---- the three kernels
    def render(self, W_p_C, W_R_C, cfg, shape=None, normalized=True, out=None, t=0.0):
        """Images [B, h, w] float32 (a DeviceArray; asynchronous on the context stream) of the camera poses W_p_C
        [B, 3], W_R_C [B, 3, 3] (host or device fp64) with the sensor of cfg: range, or depth with
        sensor.is_depth; pinhole or spherical pixels; clipped at sensor.dmax.  shape (h, w) defaults to
        sensor.shape_imgs[-2:].  out: a float32 DeviceArray [B, h, w] to write instead of a new one.  t: the time the
        scene is shown at (finite; a scene without moving or oriented primitives looks the same at every t)."""
        h, w = (int(v) for v in (shape if shape is not None else cfg.sensor.shape_imgs[-2:]))
        B = int(np.prod(W_p_C.shape)) // 3 if hasattr(W_p_C, "data_ptr") else np.asarray(W_p_C).reshape(-1, 3).shape[0]
        self._batch(B)
        p, R = self._f64(W_p_C, (B, 3)), self._f64(W_R_C, (B, 9))
        if out is None:
            out = _lib.DeviceArray(self.ctx, (B, h, w), np.float32)
        elif tuple(out.shape) != (B, h, w) or np.dtype(out.dtype) != np.float32:
            raise ValueError(f"out must be float32 [{B}, {h}, {w}]")
        if isinstance(t, float) and t == 0.0:
            _lib.scene_render(self.ctx, self.h, self._scene_of, self.img_opts(cfg), h, w, self.scale(cfg, normalized), B,
                              p, R, out)
        else:
            _lib.scene_render_at(self.ctx, self.h, self._scene_of, self.img_opts(cfg), h, w, self.scale(cfg, normalized),
                                 B, p, R, float(t), out)
        out._inputs = (p, R)  # temporaries of an asynchronous launch stay alive with its result
        return out

    def pose(self, x, cfg):
        """States x [B, 10] (host or device fp64) -> dict of DeviceArrays W_p_Bo [B, 3], W_R_Bo [B, 9],
        W_p_C [B, 3], W_R_C [B, 9]: the body pose quat2rot(q / |q|) and the camera pose with the extrinsics of cfg
        (what Nmpc.set_latent forms from the body pose)."""
        B = int(np.prod(x.shape)) // 10 if hasattr(x, "data_ptr") else np.asarray(x).reshape(-1, 10).shape[0]
        dx = self._f64(x, (B, 10))
        out = {k: _lib.DeviceArray(self.ctx, (B, n)) for k, n in (("W_p_Bo", 3), ("W_R_Bo", 9), ("W_p_C", 3), ("W_R_C", 9))}
        _lib.scene_pose(self.ctx, cfg.sensor.B_p_C, cfg.sensor.B_R_C, B, dx, *out.values())
        out["W_p_Bo"]._inputs = dx
        return out

    def render_from_state(self, x, cfg, shape=None, normalized=True, out=None, t=0.0):
        """``render`` from the camera poses of the states x (``pose``); the result carries them as ``.pose``."""
        ps = self.pose(x, cfg)
        img = self.render(ps["W_p_C"], ps["W_R_C"], cfg, shape, normalized, out, t)
        img.pose = ps  # the poses the images were taken from (device arrays, as ``pose`` returns them)
        return img

    def distance(self, points, p_to_scene=None, t=None):
        """Signed distance [n] (numpy fp64) from world points [n, 3] to their scene, negative inside.  p_to_scene
        [n]: the scene of each point; None: the default ordering, point j -> scene j // (n / S).  t: the time each
        point is measured at, a scalar or [n] (finite); None: t = 0."""
        pts = self._f64(points, (-1, 3) if not hasattr(points, "data_ptr") else tuple(points.shape))
        n = int(np.prod(pts.shape)) // 3
        p2s = None
        if p_to_scene is not None:
            a = np.ascontiguousarray(p_to_scene, dtype=np.int32).ravel()
            if a.size != n or (n and (a.min() < 0 or a.max() >= self.S)):
                raise ValueError(f"p_to_scene needs one entry in [0, {self.S}) per point")
            p2s = _lib.DeviceArray.from_numpy(self.ctx, a)
        times = None
        if t is not None:
            a = np.asarray(t, dtype=np.float64)
            a = np.full(n, float(a)) if a.ndim == 0 else np.ascontiguousarray(a).ravel()
            if a.size != n or not np.isfinite(a).all():
                raise ValueError(f"t needs one finite time per point ({n}) or a scalar")
            times = _lib.DeviceArray.from_numpy(self.ctx, a)
        out = _lib.DeviceArray(self.ctx, (n,), np.float64)
        if times is None:
            _lib.scene_distance(self.ctx, self.h, pts, p2s, n, out)
        else:
            _lib.scene_distance_at(self.ctx, self.h, pts, p2s, times, n, out)
        return out.numpy()  # the copy waits for the launch

    @property
    def speed_bound(self):
        """[S] float64: V of each scene, a bound on the speed of any surface point of any of its movers -- the maximum
        of |v| + |omega| |amp| + |yaw_rate| rho (rho: 0 for a sphere, the half diagonal of a box, sqrt(r^2 + hz^2) for
        a cylinder, the largest |vertex| of an instance's part), inflated by 1 + 1e-12; 0 for a scene set that is not
        dynamic.  The scene's distance at a fixed
        point changes no faster than V."""
        return _lib.scene_speed_bound(self.h, self.S)

    def swept_distance(self, p0, p1, p_to_scene=None, t0=None, t1=None, eps=1e-3, max_evals=4096):
        """The minimum signed distance to the scene along segments of space-time: segment j runs from the world point
        p0[j] at time t0[j] to p1[j] at t1[j] ([n, 3] and a scalar or [n] each; t0 and t1 both None: t = 0, one alone
        is a ValueError; a scene that is not dynamic ignores them), p(s) = p0 + s (p1 - p0), t(s) = t0 + s (t1 - t0).
        Returns a ``Swept`` of numpy arrays [n]: ``dmin`` the smallest distance found (the value of ``distance`` at
        p(s), t(s)), ``s`` where, ``gap`` its certificate -- the true minimum over the segment lies in [dmin - gap, dmin]
        -- and ``evals`` the distance evaluations used.  A Lipschitz branch and bound with the constant |p1 - p0| +
        ``speed_bound`` |t1 - t0|: gap <= ``eps`` unless ``max_evals`` (2..65536) ran out or an interval reached
        2^-20 of the segment, and then gap says by how much.  A segment with a non-finite coordinate or time gives
        NaN (and 0 evals), the others are unaffected.  p_to_scene as for ``distance``."""
        a0 = self._f64(p0, (-1, 3) if not hasattr(p0, "data_ptr") else tuple(p0.shape))
        n = int(np.prod(a0.shape)) // 3
        a1 = self._f64(p1, (n, 3))
        p2s = None
        if p_to_scene is not None:
            a = np.ascontiguousarray(p_to_scene, dtype=np.int32).ravel()
            if a.size != n or (n and (a.min() < 0 or a.max() >= self.S)):
                raise ValueError(f"p_to_scene needs one entry in [0, {self.S}) per segment")
            p2s = _lib.DeviceArray.from_numpy(self.ctx, a)
        if (t0 is None) != (t1 is None):
            raise ValueError("swept_distance: t0 and t1 go together (both None: t = 0)")
        times = [None, None]
        if t0 is not None:
            for k, t in enumerate((t0, t1)):
                a = np.asarray(t, dtype=np.float64)
                a = np.full(n, float(a)) if a.ndim == 0 else np.ascontiguousarray(a).ravel()
                if a.size != n:
                    raise ValueError(f"t{k} needs one time per segment ({n}) or a scalar")
                times[k] = _lib.DeviceArray.from_numpy(self.ctx, a)
        out = Swept(*[_lib.DeviceArray(self.ctx, (n,), dt) for dt in (np.float64, np.float64, np.float64, np.int32)])
        _lib.scene_swept_distance(self.ctx, self.h, a0, a1, p2s, times[0], times[1], n, eps, max_evals, out.dmin, out.s,
                                  out.gap, out.evals)
        return Swept(*[a.numpy() for a in (out.dmin, out.s, out.gap, out.evals)])  # the copies wait for the launch

    def close(self):
        if getattr(self, "h", None):
            for n in list(getattr(self, "_sdf_users", ())):  # a solver keeps the handle: back to the network first
                if n._sdf_scene is self and n.ocp.parts and n.ocp.parts[0].solver.h:
                    n.set_sdf_scene(None)
            _lib.load().sdfnmpc_scene_free(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass
