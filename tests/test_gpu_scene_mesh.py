"""csrc/scene_mesh.hip (mesh sets: Scene.mesh) against tests/mesh_ref.py and against the merged primitive kernels: the
rendered images on decided pixels, the distance and its sign, the hierarchy's independence bit for bit, leak-freeness,
the set semantics, the refusals, and the swept clearance through a thin wall.

The image bar is tests/test_gpu_scene_render.py's IMG_ATOL = 1e-4 m on decided pixels.  The kernel forms t = n . (a - o)
/ (n . d) in fp32 from the rounded vertices and the unit normal: with coordinates of at most 10 m, so |a - o| <= 10 and
an error of about 8 eps (the subtraction, two three-term dot products, the normal's rounding, the division) on a
numerator of that size, and |n . d| >= 0.1 on a decided pixel, the error of t is about 8 eps 10 / 0.1 = 5e-5 m with
eps = 2^-24.  The vertices are rounded to fp32 by the library; the reference sees the rounded mesh (mesh_ref.rounded).

The distance is fp64 on both sides: 1e-12, as for the primitives."""
import ctypes as C

import numpy as np
import pytest

import mesh_ref as M
import scene_ref as R
from sdf_nmpc_amd import _lib
from sdf_nmpc_amd.config import Config
from sdf_nmpc_amd.mesh import Mesh
from sdf_nmpc_amd.scene import Scene

pytestmark = [pytest.mark.gpu, pytest.mark.filterwarnings("ignore:no SDF weights"),
              pytest.mark.filterwarnings("ignore:QP reached")]

IMG_ATOL = 1e-4  # metres: tests/test_gpu_scene_render.py
P, RM = R.camera_poses()
B = len(P)
LEAVES = (1, 4, 8)
OLD_NAMES = ["scene_render", "scene_render_grid", "scene_render_dyn", "scene_render_mixed", "scene_dist", "scene_dist_grid",
             "scene_dist_dyn", "scene_dist_mixed", "scene_swept", "scene_swept_grid", "scene_swept_dyn", "scene_swept_mixed"]
NEW_NAMES = ["scene_render_mesh", "scene_dist_mesh", "scene_swept_mesh"]


def _cfg(sensor="pinhole", is_depth=False, **over):
    s = R.SENSOR if sensor == "pinhole" else R.SPHERICAL
    return Config(sensor__hfov=s["hfov"], sensor__vfov=s["vfov"], sensor__dmax=s["dmax"], sensor__is_depth=is_depth,
                  sensor__is_spherical=sensor == "spherical", **over)


def _points():
    return np.random.default_rng(4).uniform([-1, -3, -2.5], [6, 3, 2.5], (700, 3))  # test_distance_matches_reference's


FIXED = M.fixed_scene()


@pytest.fixture(scope="module")
def fixed(gpu_ctx):
    return {closed: Scene.mesh(gpu_ctx, FIXED, closed=closed) for closed in (True, False)}


@pytest.fixture(scope="module")
def ref():
    """Reference values in metres and decided masks of the fixed scene, once per (sensor, shape, is_depth)."""
    cache, mesh = {}, M.rounded(FIXED)

    def get(sensor, shape, is_depth):
        key = (sensor, tuple(shape), bool(is_depth))
        if key not in cache:
            s = R.SENSOR if sensor == "pinhole" else R.SPHERICAL
            kw = dict(is_depth=is_depth, is_spherical=sensor == "spherical")
            v = M.values(mesh, P, RM, *shape, s["hfov"], s["vfov"], s["dmax"], **kw)
            ok = M.decided(mesh, P, RM, *shape, s["hfov"], s["vfov"], s["dmax"], **kw)
            v.setflags(write=False)
            ok.setflags(write=False)
            cache[key] = (v, ok)
        return cache[key]

    return get


@pytest.fixture(scope="module")
def ref_dist():
    pts = _points()
    want = M.distance(M.rounded(FIXED), pts, signed=True)
    pts.setflags(write=False)
    want.setflags(write=False)
    return pts, want


# ---- 1. render and distance against the reference
@pytest.mark.parametrize("shape", R.SHAPES)
@pytest.mark.parametrize("sensor", ["pinhole", "spherical"])
def test_render_matches_reference_on_decided_pixels(fixed, ref, sensor, shape):
    assert fixed[True].is_mesh and not fixed[True].is_dynamic and not fixed[True].is_indexed
    for is_depth in (False, True):
        cfg = _cfg(sensor, is_depth)
        want, ok = ref(sensor, shape, is_depth)
        assert ok.mean() >= 0.95
        imgs = []
        for closed in (True, False):
            img = fixed[closed].render(P, RM, cfg, shape).numpy()
            assert img.shape == (B,) + tuple(shape) and img.dtype == np.float32
            gap = np.abs(img.astype(np.float64) * 5.0 - want)
            print(f"\n{sensor} {shape} depth={is_depth} closed={closed}: worst gap on decided pixels {gap[ok].max():.3e} m, "
                  f"on all pixels {gap.max():.3e} m, decided {ok.mean():.4f}")
            assert gap[ok].max() <= IMG_ATOL
            assert img.max() <= np.float32(1.0) and (img == np.float32(5.0) * np.float32(0.2)).any() and (img < 0.9).any()
            imgs.append(img)
        np.testing.assert_array_equal(imgs[0], imgs[1])  # the render does not read what closed adds


def test_distance_matches_reference(fixed, ref_dist):
    pts, want = ref_dist
    assert (want < 0).sum() > 20 and (want > 0).sum() > 300
    got = fixed[True].distance(pts)
    print(f"\nclosed: max |got - want| {np.abs(got - want).max():.3e}")
    assert np.abs(got - want).max() <= 1e-12
    np.testing.assert_array_equal(fixed[False].distance(pts), np.abs(got))  # the open set: the same, unsigned
    np.testing.assert_array_equal(fixed[True].speed_bound, [0.0])


# ---- 2. against the merged primitive kernels
BOXES = [((3.5, 0.5, -1.0), (4.0, 1.5, 1.25)), ((-10.0, -10.0, -1.625), (10.0, 10.0, -1.5)),
         ((1.0, -2.0, -0.5), (1.75, -1.25, 0.5))]  # disjoint, every coordinate an fp32 number


def test_box_meshes_against_analytic_boxes(gpu_ctx):
    prims = [Scene.box(lo, hi) for lo, hi in BOXES]
    mesh = Mesh.merge(*[Mesh.box(lo, hi) for lo, hi in BOXES])
    analytic, meshed = Scene(gpu_ctx, prims), Scene.mesh(gpu_ctx, mesh, closed=True)
    pts = np.concatenate([_points()[:640], np.random.default_rng(8).uniform(BOXES[0][0], BOXES[0][1], (60, 3))])
    da, dm = analytic.distance(pts), meshed.distance(pts)
    assert (da < 0).sum() >= 60
    print(f"\nmesh boxes against analytic boxes: max distance gap {np.abs(da - dm).max():.3e}")
    assert np.abs(da - dm).max() <= 1e-12
    for sensor, s in (("pinhole", R.SENSOR), ("spherical", R.SPHERICAL)):
        for shape in R.SHAPES:
            kw = dict(is_spherical=sensor == "spherical")
            ok = R.decided(prims, P, RM, *shape, s["hfov"], s["vfov"], s["dmax"], **kw) & \
                M.decided(mesh, P, RM, *shape, s["hfov"], s["vfov"], s["dmax"], **kw)
            assert ok.mean() >= 0.95
            cfg = _cfg(sensor)
            ia, im = (sc.render(P, RM, cfg, shape).numpy().astype(np.float64) * 5.0 for sc in (analytic, meshed))
            print(f"{sensor} {shape}: worst image gap on pixels decided for both {np.abs(ia - im)[ok].max():.3e} m")
            assert np.abs(ia - im)[ok].max() <= IMG_ATOL and (im[ok] < 5.0).any()


# ---- 3. the hierarchy changes no bit
def _coplanar64():
    """64 coplanar triangles whose centroids coincide pairwise: every split of the hierarchy is degenerate somewhere."""
    v, t = [], []
    for k in range(32):
        x, y = 0.375 * (k % 8) - 1.5, 0.375 * (k // 8) - 0.75
        q = [(0, 0), (3, 0), (0, 3), (2, 2), (-1, 2), (2, -1)]  # two triangles about one centroid
        v += [(2.0, x + 0.125 * a, y + 0.125 * b) for a, b in q]
        t += [(6 * k, 6 * k + 1, 6 * k + 2), (6 * k + 3, 6 * k + 4, 6 * k + 5)]
    return Mesh(v, t)


def _hierarchy_cases():
    i, j = np.meshgrid(np.arange(24), np.arange(24), indexing="ij")
    terrain = Mesh.heightfield(-1.0, -3.0, 0.25, 0.25, -1.0 + 0.3 * np.sin(0.5 * i) * np.cos(0.4 * j))
    tunnel = Mesh.tunnel([(-1, 0, 0), (1, 0.4, 0.1), (3, -0.3, 0.3), (5, 0.2, 0.0), (7, 0, -0.2)], 1.2, segments=12,
                         roughness=0.15, seed=3)
    one = Mesh([(2.5, -1.0, -0.5), (2.5, 1.0, -0.5), (2.0, 0.0, 1.0)], [(0, 1, 2)])
    return dict(fixed=(FIXED, True), fixed_open=(FIXED, False), terrain=(terrain, False), tunnel=(tunnel, False),
                one=(one, False), coplanar=(_coplanar64(), False))


@pytest.mark.parametrize("name", ["fixed", "fixed_open", "terrain", "tunnel", "one", "coplanar"])
def test_hierarchy_changes_no_bit(gpu_ctx, name):
    mesh, closed = _hierarchy_cases()[name]
    v, t = mesh.verts.astype(np.float32).astype(np.float64), mesh.tris  # where the library puts the vertices
    rng = np.random.default_rng(11)
    pick = rng.permutation(t.shape[0])[:150]
    tv = v[t[pick]]                                                       # [k, 3, 3]
    lo, hi = v.min(0) - 1.0, v.max(0) + 1.0
    # exact ties: mesh vertices, edge midpoints, face centroids; then points all around
    pts = np.concatenate([tv.reshape(-1, 3), (0.5 * (tv + np.roll(tv, 1, axis=1))).reshape(-1, 3), tv.mean(1),
                          rng.uniform(lo, hi, (200, 3))])
    # chords between vertices, and random ones
    p0 = np.concatenate([tv[:, 0], rng.uniform(lo, hi, (60, 3))])
    p1 = np.concatenate([np.roll(tv[:, 1], 7, axis=0), rng.uniform(lo, hi, (60, 3))])
    # cameras: the fixed poses, one far outside looking back at the mesh, one touching a face
    c = 0.5 * (lo + hi)
    far = c + np.array([-30.0, 4.0, 2.5])
    yaw, pitch = np.arctan2(c[1] - far[1], c[0] - far[0]), -np.arctan2(c[2] - far[2], np.hypot(*(c - far)[:2]))
    cp = np.concatenate([P, [far], [v[t[0]].mean(0)]])
    cR = np.concatenate([RM, [R.rpy2rot(0.0, pitch, yaw)], [np.eye(3)]])
    s = R.SENSOR  # the pinhole images reach 1000 m, so the far camera's values are not clipped
    cfgs = [(Config(sensor__hfov=s["hfov"], sensor__vfov=s["vfov"], sensor__dmax=1000.0, sensor__is_depth=True), (27, 48)),
            (_cfg("spherical", False), (18, 32))]

    def run(leaf):
        sc = Scene.mesh(gpu_ctx, mesh, closed=closed, leaf_size=leaf)
        imgs = [sc.render(cp, cR, cfg, shape).numpy() for cfg, shape in cfgs]
        d = sc.distance(pts)
        sw = sc.swept_distance(p0, p1, eps=1e-3, max_evals=256)
        sc.close()
        return imgs, d, sw

    bi, bd, bs = run(-1)
    assert np.isfinite(bd).all() and (bd[:tv.shape[0] * 3] == 0).all()  # a vertex is at distance 0 exactly
    assert (np.abs(bd) < 1e-9).sum() >= 7 * pick.size                   # and the midpoints and centroids lie on the mesh
    assert all((im < 1.0).any() for im in bi)
    assert (bi[0][3] < 1.0).any() or name in ("one", "coplanar")         # the far camera sees the mesh, 30 m away
    for leaf in LEAVES:
        imgs, d, s = run(leaf)
        for a, b in zip(imgs, bi):
            np.testing.assert_array_equal(a.view(np.uint32), b.view(np.uint32), err_msg=f"render, leaf {leaf}")
        np.testing.assert_array_equal(d, bd, err_msg=f"distance, leaf {leaf}")
        for k in ("dmin", "s", "gap", "evals"):
            np.testing.assert_array_equal(getattr(s, k), getattr(bs, k), err_msg=f"swept {k}, leaf {leaf}")


# ---- 4. no leaks
@pytest.mark.parametrize("sensor", ["pinhole", "spherical"])
def test_no_ray_leaves_or_misses_a_closed_icosphere(gpu_ctx, sensor):
    r, c = 2.0, np.array([0.3, -0.2, 0.1])
    sc = Scene.mesh(gpu_ctx, Mesh.icosphere(c, r, 3), closed=True)
    cfg, s = _cfg(sensor), (R.SENSOR if sensor == "pinhole" else R.SPHERICAL)
    for shape in R.SHAPES:
        inside = sc.render(np.tile(c, (B, 1)), RM, cfg, shape).numpy().astype(np.float64) * 5.0
        assert inside.max() < 5.0 and inside.min() > 0.97 * r * 0.999 and inside.max() <= r + 1e-4  # its inner wall
        # from outside, aimed at it: every ray that passes within 0.9 r of the centre hits
        o = c - 4.5 * RM[:, :, 0]
        img = sc.render(o, RM, cfg, shape).numpy().astype(np.float64) * 5.0
        dc = R.ray_dirs(*shape, s["hfov"], s["vfov"], sensor == "spherical").reshape(-1, 3)
        for b in range(B):
            d = dc @ RM[b].T
            w = c - o[b]
            miss = np.linalg.norm(w - (d @ w)[:, None] * d, axis=1).reshape(shape)
            assert (miss <= 0.9 * r).sum() > 50
            assert (img[b][miss <= 0.9 * r] < 5.0).all()
            assert (img[b][miss > r] == 5.0).all()
    sc.close()


# ---- 5. set semantics
def test_two_scenes_permutation_and_empty(gpu_ctx, fixed):
    cfg, shape = _cfg("pinhole", True), (27, 48)
    other = Mesh.merge(Mesh.icosphere((2.0, 0.2, 0.0), 0.6, 2), Mesh.box((-10, -10, -1.6), (10, 10, -1.5)))
    empty = Mesh(np.zeros((0, 3)), np.zeros((0, 3), np.int32))
    both = Scene.mesh(gpu_ctx, [FIXED, other, empty], scene_of=[1, 0, 2], closed=True)
    assert both.S == 3 and both.is_mesh
    alone = Scene.mesh(gpu_ctx, other, closed=True)
    img = both.render(P, RM, cfg, shape).numpy()
    own = [fixed[True].render(P, RM, cfg, shape).numpy(), alone.render(P, RM, cfg, shape).numpy()]
    np.testing.assert_array_equal(img[0], own[1][0])
    np.testing.assert_array_equal(img[1], own[0][1])
    assert (img[2] == np.float32(5.0) * np.float32(0.2)).all()  # the empty scene: a miss everywhere
    assert np.abs(own[0] - own[1]).max() > 0.1
    perm = [2, 0, 1]
    np.testing.assert_array_equal(fixed[True].render(P[perm], RM[perm], cfg, shape).numpy(), own[0][perm])
    np.testing.assert_array_equal(fixed[True].render(P[1:2], RM[1:2], cfg, shape).numpy()[0], own[0][1])
    with pytest.raises(ValueError):
        Scene.mesh(gpu_ctx, [FIXED, other], scene_of=[0, 2, 1])
    with pytest.raises(ValueError):
        both.render(P[:2], RM[:2], cfg, shape)
    # distance: p_to_scene, and the default ordering (thirds)
    pts = _points()[:699]
    d0, d1 = fixed[True].distance(pts), alone.distance(pts)
    p2s = np.random.default_rng(9).integers(0, 3, 699)
    np.testing.assert_array_equal(both.distance(pts, p2s), np.where(p2s == 0, d0, np.where(p2s == 1, d1, np.inf)))
    third = np.arange(699) // 233
    np.testing.assert_array_equal(both.distance(pts), np.where(third == 0, d0, np.where(third == 1, d1, np.inf)))
    with pytest.raises(_lib.SdfnmpcError):
        both.distance(pts[:698])
    s = both.swept_distance(pts[:9], pts[9:18], p_to_scene=np.repeat([0, 1, 2], 3))
    assert np.isfinite(s.dmin[:6]).all() and (s.dmin[6:] == np.inf).all() and (s.gap[6:] == 0).all()
    np.testing.assert_array_equal(both.speed_bound, [0.0, 0.0, 0.0])
    # B == 0 and n == 0 are no-ops
    fill = np.full((B,) + shape, -7.0, np.float32)
    out = _lib.DeviceArray.from_numpy(gpu_ctx, fill)
    dp, dR = _lib.DeviceArray.from_numpy(gpu_ctx, P), _lib.DeviceArray.from_numpy(gpu_ctx, RM.reshape(B, 9))
    _lib.scene_render(gpu_ctx, fixed[True].h, None, Scene.img_opts(cfg), *shape, 0.2, 0, dp, dR, out)
    _lib.scene_distance(gpu_ctx, fixed[True].h, None, None, 0, None)
    gpu_ctx.synchronize()
    np.testing.assert_array_equal(out.numpy(), fill)
    for sc in (both, alone):
        sc.close()


def test_kernel_stats_land_on_the_new_names(gpu_ctx, fixed):
    pts = _points()[:64]
    gpu_ctx.enable_timing(True)
    gpu_ctx.reset_stats()
    fixed[True].render(P, RM, _cfg(), (18, 32)).numpy()
    fixed[True].distance(pts)
    fixed[False].swept_distance(pts[:32], pts[32:])
    counts = {k: gpu_ctx.kernel_stats(k)[1] for k in NEW_NAMES + OLD_NAMES}
    gpu_ctx.enable_timing(False)
    assert counts == {**{k: 1 for k in NEW_NAMES}, **{k: 0 for k in OLD_NAMES}}


# ---- 6. refusals
def _raw_create(ctx, S, nvert, verts, ntri, tris, opts=None):
    """sdfnmpc_scene_create_mesh as C sees it -> (return code, handle value, message)."""
    nv = (C.c_int * max(len(nvert), 1))(*nvert)
    nt = (C.c_int * max(len(ntri), 1))(*ntri)
    va = None if verts is None else np.ascontiguousarray(verts, np.float64)
    ta = None if tris is None else np.ascontiguousarray(tris, np.int32)
    h = C.c_void_p()
    rc = _lib.load().sdfnmpc_scene_create_mesh(
        ctx.h, S, nv, None if va is None else va.ctypes.data_as(C.POINTER(C.c_double)), nt,
        None if ta is None else ta.ctypes.data_as(C.POINTER(C.c_int)), None if opts is None else C.byref(_lib.MeshOptsC(*opts)),
        C.byref(h))
    return rc, h.value, _lib.load().sdfnmpc_last_error().decode()


def test_creation_refusals(gpu_ctx):
    box = Mesh.box((0, 0, 0), (1, 2, 3))
    v, t = box.verts, box.tris
    i, j = np.meshgrid(np.arange(4), np.arange(4), indexing="ij")
    terrain = Mesh.heightfield(0.0, 0.0, 1.0, 1.0, 0.1 * i * j)
    flipped = t.copy()
    flipped[3] = flipped[3][::-1]
    nan_v, inf_v = v.copy(), v.copy()
    nan_v[2, 1], inf_v[5, 0] = np.nan, np.inf
    tri = np.array([[0.0, 0, 0], [1, 0, 0], [0.5, 1e-50, 0]])  # a triangle in fp64, a segment in fp32
    bad = [
        ("S must be", (0, [8], v, [12], t)),
        ("negative count", (1, [-1], v, [12], t)),
        ("negative count", (1, [8], v, [-1], t)),
        ("2\\^21 vertices", (1, [(1 << 21) + 1], None, [0], None)),
        ("2\\^20 triangles", (1, [8], v, [(1 << 20) + 1], None)),
        ("2\\^24 triangles", (17, [0] * 17, None, [1 << 20] * 17, None)),
        ("non-finite vertex", (1, [8], nan_v, [12], t)),
        ("non-finite vertex", (1, [8], inf_v, [12], t)),
        ("index outside", (1, [8], v, [12], np.where(t == 7, 8, t))),
        ("index outside", (1, [8], v, [12], np.where(t == 0, -1, t))),
        ("index outside", (2, [8, 7], np.concatenate([v, v[:7]]), [12, 12], np.concatenate([t, t]))),  # local to the scene
        ("zero area", (1, [8], v, [1], [[0, 1, 1]])),
        ("zero area", (1, [3], [[0, 0, 0], [1, 1, 1], [2, 2, 2]], [1], [[0, 1, 2]])),
        ("zero area", (1, [3], tri, [1], [[0, 1, 2]])),
        ("leaf_size", (1, [8], v, [12], t, (9, 0))),
        ("leaf_size", (1, [8], v, [12], t, (-2, 0))),
        ("closed must be", (1, [8], v, [12], t, (0, 2))),
        ("closed.*manifold", (1, [8], v, [11], t[1:], (0, 1))),
        ("closed.*manifold", (1, [8], v, [12], flipped, (0, 1))),
        ("closed.*manifold", (1, [16], terrain.verts, [18], terrain.tris, (4, 1))),
        ("NULL", (1, [8], None, [12], t)),
    ]
    import re
    for pattern, args in bad:
        rc, h, msg = _raw_create(gpu_ctx, *args)
        assert rc == -1 and h is None and re.search(pattern, msg), (pattern, rc, h, msg)
    # what they refuse is accepted once mended: the same arrays with closed = 0, the default options, one leaf per triangle
    for args in ((1, [8], v, [11], t[1:], (0, 0)), (1, [8], v, [12], flipped, None), (1, [16], terrain.verts, [18], terrain.tris, (1, 0)),
                 (1, [8], v, [12], t, (8, 1)), (1, [8], v, [12], t, (-1, 1)), (2, [8, 0], v, [12, 0], t, (0, 1))):
        rc, h, msg = _raw_create(gpu_ctx, *args)
        assert rc == 0 and h, msg
        assert _lib.load().sdfnmpc_scene_is_mesh(h) == 1 and _lib.load().sdfnmpc_scene_is_dynamic(h) == 0 and \
            _lib.load().sdfnmpc_scene_is_indexed(h) == 0
        _lib.load().sdfnmpc_scene_free(h)
    with pytest.raises(_lib.SdfnmpcError, match="error -1.*manifold"):
        Scene.mesh(gpu_ctx, terrain, closed=True)
    with pytest.raises(_lib.SdfnmpcError, match="error -1.*manifold"):
        Scene.mesh(gpu_ctx, Mesh(v, flipped), closed=True)
    assert _lib.load().sdfnmpc_scene_is_mesh(Scene(gpu_ctx, R.SCENE).h) == 0


def test_refusals_leave_the_output_untouched(gpu_ctx, fixed):
    h, w = 18, 32
    fill = np.full((B, h, w), -7.0, np.float32)
    out = _lib.DeviceArray.from_numpy(gpu_ctx, fill)
    dp = _lib.DeviceArray.from_numpy(gpu_ctx, P)
    dR = _lib.DeviceArray.from_numpy(gpu_ctx, RM.reshape(B, 9))
    good = dict(dmax=5.0, hfov=0.7592, vfov=0.4903, is_depth=False, is_spherical=False)

    def call(opts=None, H=h, W=w, scale=0.2, nb=B, p=dp, Rm=dR, img=out):
        o = _lib.img_opts(**{**good, **(opts or {})})
        _lib.scene_render(gpu_ctx, fixed[False].h, None, o, H, W, scale, nb, p, Rm, img)

    for kw in [dict(opts=dict(hfov=np.pi / 2)), dict(opts=dict(dmax=0.0)), dict(opts=dict(dmax=float("nan"))), dict(scale=0.0),
               dict(H=0), dict(W=0), dict(nb=-1), dict(p=None), dict(Rm=None), dict(img=None)]:
        with pytest.raises(_lib.SdfnmpcError, match="error -1"):
            call(**kw)
        gpu_ctx.synchronize()
        np.testing.assert_array_equal(out.numpy(), fill)
    call()
    assert (out.numpy() >= 0).all()


def test_a_mesh_is_no_sdf_source(gpu_ctx, fixed):
    """sdfnmpc_scene_sdf_rows, lin_args.sdf_scene and set_sdf_scene refuse a mesh set with the unsupported code and a
    message that names meshes; nothing is launched, so the outputs keep what they held."""
    from test_gpu_rollout import _setup
    Bn, N, npar = 2, 10, 17 + 128
    x = _lib.DeviceArray.from_numpy(gpu_ctx, np.zeros((Bn, N + 1, 10)))
    p = _lib.DeviceArray.from_numpy(gpu_ctx, np.ones((Bn, N + 1, npar)))
    hh = _lib.DeviceArray.from_numpy(gpu_ctx, np.full((Bn, N + 1, 3), -7.0))
    Jh = _lib.DeviceArray.from_numpy(gpu_ctx, np.full((Bn, N + 1, 10, 3), -7.0))
    gpu_ctx.enable_timing(True)
    gpu_ctx.reset_stats()
    with pytest.raises(_lib.SdfnmpcError, match="error -4.*mesh"):
        _lib.scene_sdf_rows(gpu_ctx, fixed[True].h, Bn, N, npar, x, p, hh, Jh, 1.0)
    launched = [gpu_ctx.kernel_stats(k)[1] for k in ("scene_sdf_rows", "scene_sdf_rows_grid", "scene_sdf_rows_mixed")]
    gpu_ctx.enable_timing(False)
    assert launched == [0, 0, 0]
    assert (hh.numpy() == -7.0).all() and (Jh.numpy() == -7.0).all()
    n, x0 = _setup(Config(mpc__N=10), Bn, 21)
    scene = Scene.mesh(n.ocp.ctx, FIXED, closed=True)
    with pytest.raises(_lib.SdfnmpcError, match="error -4.*mesh"):
        n.set_sdf_scene(scene)
    assert n._sdf_scene is None
    n.set_x0(x0)
    r = n.rollout(2)  # the controller is as it was: the network is still the source
    assert r.clearance is None and np.isfinite(r.u).all()
    scene.close()
    n.ocp.close()


# ---- 7. swept sees the wall
def test_swept_sees_the_wall(gpu_ctx):
    wall = Mesh([(2, -1, -1), (2, 1, -1), (2, 1, 1), (2, -1, 1)], [(0, 1, 2), (0, 2, 3)])
    sc = Scene.mesh(gpu_ctx, wall)
    rng = np.random.default_rng(12)
    yz = rng.uniform(-0.8, 0.8, (40, 2))
    p0, p1 = np.column_stack([np.full(40, 1.0), yz]), np.column_stack([np.full(40, 3.0), yz])
    eps = 1e-3
    assert np.abs(sc.distance(p0) - 1.0).max() <= 1e-12 and np.abs(sc.distance(p1) - 1.0).max() <= 1e-12
    s = sc.swept_distance(p0, p1, eps=eps)
    print(f"\nthrough the wall: dmin <= {s.dmin.max():.2e}, gap <= {s.gap.max():.2e}, |s - 0.5| <= {np.abs(s.s - 0.5).max():.2e}, "
          f"evals <= {s.evals.max()}")
    assert (s.dmin >= 0).all() and (s.dmin <= eps).all() and (s.gap <= eps).all() and (np.abs(s.s - 0.5) <= 1e-3).all()
    # a chord parallel to the wall never comes nearer than its ends
    q0, q1 = np.column_stack([np.full(40, 1.0), yz]), np.column_stack([np.full(40, 1.0), -yz])
    par = sc.swept_distance(q0, q1, eps=eps)
    assert np.abs(par.dmin - 1.0).max() <= 1e-12 and (par.gap <= eps).all()
    sc.close()
