"""Scenes of many primitives behind a uniform grid (csrc/scene_grid.hip, sdfnmpc_scene_create_large): every query
bitwise against the brute-force kernels -- on the same primitives where they fit a plain scene, else on chunks of at
most 32 combined by the minimum (tests/scene_grid_ref.py) -- with no tolerance anywhere: the three queries are minima
over the primitives, and a minimum does not depend on how the primitives are visited.  Forests of 0 to 200 cylinders
beside spheres and boxes that span many cells; the default grid, a single cell, and cells below the smallest radius."""
import ctypes as C

import numpy as np
import pytest

import scene_grid_ref as G
import scene_ref as R
from sdf_nmpc_amd import _lib
from sdf_nmpc_amd.config import Config
from sdf_nmpc_amd.scene import Scene

pytestmark = [pytest.mark.gpu, pytest.mark.filterwarnings("ignore:no SDF weights")]

LO, HI = (-6.0, -6.0, -1.0), (6.0, 6.0, 2.0)
RADIUS = (0.1, 0.35)
EXTRA = [Scene.sphere((0.5, 1.0, 0.5), 1.2), Scene.box((-5.0, -5.5, -0.5), (4.0, -4.5, 0.5)),
         Scene.sphere((3.0, 3.0, 1.0), 0.3), Scene.box((-5.5, 2.0, -0.9), (-4.5, 5.0, 1.9))]
CELLS = [None, 1000.0, 0.08]  # the default; one single cell; cells smaller than the smallest radius
SHAPES = [(27, 48), (16, 24), (1, 1)]  # (1, 1): the one pixel whose ray is the camera's x axis exactly
SENSORS = dict(pinhole=dict(hfov=0.7592, vfov=0.4903), spherical=dict(hfov=1.2, vfov=0.6))
DMAX = 8.0
MAX_DF = 1.0
NP = 17
ROW_SHAPES = [(1, 10), (3, 10), (37, 6)]  # those of tests/test_gpu_scene_sdf.py


def _world(n, seed=None):
    return Scene.forest(n, LO, HI, radius=RADIUS, seed=n if seed is None else seed) + EXTRA


def _cfg(sensor, is_depth):
    s = SENSORS[sensor]
    return Config(sensor__hfov=s["hfov"], sensor__vfov=s["vfov"], sensor__dmax=DMAX, sensor__is_depth=is_depth,
                  sensor__is_spherical=sensor == "spherical")


def _poses(prims):
    """Inside the grid's box; outside it looking in; inside a primitive; on a cell corner of the default grid looking
    along +x (the centre row of the 27-row image has d_z = 0, the (1, 1) image's ray is +x itself); looking along -z,
    parallel to every cylinder's axis."""
    g = G.build(prims)
    corner = g["org"] + g["cell"] * np.minimum(g["n"], np.array([2, 3, 1]))  # exact in fp32, as the grid's planes are
    p = np.array([(-2.0, 0.4, 0.3), (-8.5, 0.8, 0.6), (0.4, 1.1, 0.4), tuple(corner), (1.7, -2.2, 6.0)])
    Rm = np.stack([R.rpy2rot(0.1, -0.05, 0.4), R.rpy2rot(0.0, 0.05, -0.1), R.rpy2rot(0.0, 0.0, 1.0), np.eye(3),
                   np.array([[0.0, 0.0, 1.0], [0.0, 1.0, 0.0], [-1.0, 0.0, 0.0]])])
    return p, Rm


@pytest.mark.parametrize("n", [0, 1, 33, 200])
def test_render_is_bitwise_the_chunked_brute_force(gpu_ctx, n):
    prims = _world(n)
    P, Rm = _poses(prims)
    plain = [Scene(gpu_ctx, ch) for ch in G.chunks(prims)]
    grids = [Scene(gpu_ctx, prims, grid=True, cell=c) for c in CELLS]
    assert all(s.is_indexed and not s.is_dynamic for s in grids) and not any(s.is_indexed for s in plain)
    seen_hit = False
    for sensor in SENSORS:
        for is_depth in (False, True):
            cfg = _cfg(sensor, is_depth)
            for shape in SHAPES:
                want = np.minimum.reduce([s.render(P, Rm, cfg, shape).numpy() for s in plain])
                for g in grids:
                    np.testing.assert_array_equal(g.render(P, Rm, cfg, shape).numpy(), want)
                assert not want[2].any()  # inside a primitive: the all-zero image
                if shape != (1, 1):
                    assert (want[:2] < 1.0).any() and (want[:2] == 1.0).any()  # hits and misses, inside and from outside
                    seen_hit = seen_hit or bool((want[1] < 1.0).any())
    assert seen_hit
    # the raw image (another scale) and a time: an indexed set is static
    cfg = _cfg("pinhole", True)
    want = np.minimum.reduce([s.render(P, Rm, cfg, (16, 24), normalized=False).numpy() for s in plain])
    np.testing.assert_array_equal(grids[0].render(P, Rm, cfg, (16, 24), normalized=False, t=1.7).numpy(), want)
    for s in plain + grids:
        s.close()


def _points(prims, n=259, seed=2):
    """259 points, a full block and a tail: free space, inside primitives, on cell faces of the default grid, 100 m
    outside it."""
    g = G.build(prims)
    rng = np.random.default_rng(seed)
    pts = rng.uniform(-7, 7, (n, 3)) * np.array([1.0, 1.0, 0.4])
    pts[:8] = rng.uniform(-1, 1, (8, 3)) * 5.0 + np.array([100.0, -100.0, 100.0]) * rng.integers(-1, 2, (8, 3))
    pts[0] = (106.0, 0.3, 0.2)
    pts[8] = (0.5, 1.0, 0.5)      # the centre of EXTRA's sphere
    pts[9] = (-1.0, -5.0, 0.0)    # inside EXTRA's box
    for j in range(10, 20):       # on cell faces and corners
        k = rng.integers(0, g["n"] + 1)
        pts[j] = g["org"] + g["cell"] * k
        pts[j, j % 3] = rng.uniform(-3, 1.5) if j < 16 else pts[j, j % 3]
    return pts


def _inputs(B, N, seed):
    rng = np.random.default_rng(seed)
    x = rng.normal(0, 1, (B, N + 1, 10))
    x[..., :3] = rng.uniform(-6.5, 6.5, (B, N + 1, 3)) * np.array([1.0, 1.0, 0.35])
    p = rng.normal(0, 1, (B, N + 1, NP))
    p[..., 0] = 1.0
    p[:, 2::3, 0] = 0.0
    return x, p


def _rows(ctx, scene, x, p, max_df=MAX_DF):
    """-> h [B, N+1], J [B, N+1, 10]: column 2 of a launch on NaN-filled outputs, whose other columns stay NaN"""
    B, N = x.shape[0], x.shape[1] - 1
    dx, dp = _lib.DeviceArray.from_numpy(ctx, x), _lib.DeviceArray.from_numpy(ctx, p)
    dh = _lib.DeviceArray.from_numpy(ctx, np.full((B, N + 1, 3), np.nan))
    dJ = _lib.DeviceArray.from_numpy(ctx, np.full((B, N + 1, 10, 3), np.nan))
    _lib.scene_sdf_rows(ctx, scene.h, B, N, p.shape[-1], dx, dp, dh, dJ, max_df, scene_of=scene._scene_of)
    h, J = dh.numpy(), dJ.numpy()
    assert np.isnan(h[..., :2]).all() and np.isnan(J[..., :2]).all()
    return h[..., 2], J[..., 2]


def _chunked_rows(ctx, prims, x, p, max_df=MAX_DF):
    """The smallest truncated h[:, 2] over the chunks, with the J_h of the first chunk that attains it."""
    h = J = None
    for ch in G.chunks(prims) or [[]]:
        sc = Scene(ctx, ch)
        hc, Jc = _rows(ctx, sc, x, p, max_df)
        sc.close()
        if h is None:
            h, J = hc, Jc
        else:
            lower = hc < h
            h, J = np.where(lower, hc, h), np.where(lower[..., None], Jc, J)
    return h, J


def test_up_to_32_primitives_give_the_bits_of_the_plain_scene(gpu_ctx):
    """The same primitives with and without the grid: the direct check of the shared per-primitive code."""
    prims = _world(20) + list(R.SCENE)
    assert len(prims) <= 32
    plain = Scene(gpu_ctx, prims)
    P, Rm = _poses(prims)
    pts = _points(prims)
    x, p = _inputs(37, 6, seed=4)
    want_d = plain.distance(pts)
    assert (want_d < 0).any() and (want_d > 50).any()
    for cell in CELLS:
        grid = Scene(gpu_ctx, prims, grid=True, cell=cell)
        for sensor in SENSORS:
            for is_depth in (False, True):
                cfg = _cfg(sensor, is_depth)
                for shape in SHAPES:
                    np.testing.assert_array_equal(grid.render(P, Rm, cfg, shape).numpy(), plain.render(P, Rm, cfg, shape).numpy())
        np.testing.assert_array_equal(grid.distance(pts), want_d)
        for max_df in (0.2, 3.0):
            for got, want in zip(_rows(gpu_ctx, grid, x, p, max_df), _rows(gpu_ctx, plain, x, p, max_df)):
                np.testing.assert_array_equal(got, want)
        grid.close()
    plain.close()


@pytest.mark.parametrize("cell", CELLS)
def test_distance_is_bitwise_the_chunked_brute_force(gpu_ctx, cell):
    """S = 3 scenes of different sizes, one of them empty, with p_to_scene; a point midway between two equal spheres."""
    twins = [Scene.sphere((1.0, 0.0, 0.0), 0.5)] + Scene.forest(40, (8.0, 8.0, -1.0), (14.0, 14.0, 2.0), seed=3) + \
            [Scene.sphere((-1.0, 0.0, 0.0), 0.5)]
    scenes = [_world(200), [], twins]
    pts = _points(scenes[0])
    pts[20] = (0.0, 0.0, 0.0)  # midway between the twins
    p2s = np.random.default_rng(6).integers(0, 3, len(pts)).astype(np.int32)
    p2s[20] = 2
    p2s[:3] = (0, 1, 2)
    grid = Scene(gpu_ctx, scenes, grid=True, cell=cell)
    got = grid.distance(pts, p_to_scene=p2s)
    want = np.full(len(pts), np.inf)
    for s, prims in enumerate(scenes):
        if prims:
            want[p2s == s] = G.chunked_distance(gpu_ctx, prims, pts[p2s == s])
    np.testing.assert_array_equal(got, want)
    assert np.isinf(got[p2s == 1]).all() and got[20] == 0.5  # an empty scene: +inf, as a plain one gives
    assert (got[p2s == 0] < 0).any() and (got[p2s == 0] > 50).any()
    # the default ordering, point j -> scene j // (n / S), and a time per point: ignored, the set is static
    three = np.concatenate([pts[:86]] * 3)
    want3 = np.concatenate([G.chunked_distance(gpu_ctx, scenes[0], pts[:86]), np.full(86, np.inf),
                            G.chunked_distance(gpu_ctx, twins, pts[:86])])
    np.testing.assert_array_equal(grid.distance(three), want3)
    np.testing.assert_array_equal(grid.distance(three, t=2.5), want3)
    grid.close()


@pytest.mark.parametrize("B,N", ROW_SHAPES)
def test_sdf_rows_are_bitwise_the_chunked_brute_force(gpu_ctx, B, N):
    prims = _world(200)
    x, p = _inputs(B, N, seed=50 + B)
    grids = [Scene(gpu_ctx, prims, grid=True, cell=c) for c in CELLS]
    for max_df in (0.2, 3.0):  # below and above the typical gap between the trees
        want_h, want_J = _chunked_rows(gpu_ctx, prims, x, p, max_df)
        for g in grids:
            h, J = _rows(gpu_ctx, g, x, p, max_df)
            np.testing.assert_array_equal(h, want_h)
            np.testing.assert_array_equal(J, want_J)
        off = p[..., 0] == 0.0
        assert (want_h[off] == max_df).all() and not want_J[off].any() and not want_J[..., 3:].any()
        if B == 37:
            on = ~off
            assert (want_h[on] < max_df).any() and (want_h[on] < 0).any()
            # on the reference alone: rows are truncated at the smaller max_df, none in this forest at the larger
            assert (want_h[on] == max_df).any() == (max_df == 0.2)
            assert np.abs(want_J[on]).max() > 0.9
    for g in grids:
        g.close()


def test_on_a_tie_the_lowest_index_of_the_scene_supplies_the_gradient(gpu_ctx):
    """Centres (+-1, 0, 0), equal radii, a node at the origin: the two spheres 33 indices apart (in different chunks
    of the brute force) and, with cell = 0.5, in different cells."""
    a, b = Scene.sphere((1.0, 0.0, 0.0), 0.5), Scene.sphere((-1.0, 0.0, 0.0), 0.5)
    fill = Scene.forest(32, (8.0, 8.0, -1.0), (14.0, 14.0, 2.0), seed=3)
    x, p = _inputs(1, 10, seed=1)
    x[0, 0, :3] = 0.0
    p[..., 0] = 1.0
    for first, second, gx in ((a, b, -1.0), (b, a, 1.0)):
        prims = [first] + fill + [second]
        for cell in (None, 0.5):
            g = Scene(gpu_ctx, prims, grid=True, cell=cell)
            h, J = _rows(gpu_ctx, g, x, p)
            g.close()
            assert h[0, 0] == 0.5
            np.testing.assert_array_equal(J[0, 0, :3], [gx, 0.0, 0.0])
            want_h, want_J = _chunked_rows(gpu_ctx, prims, x, p)
            np.testing.assert_array_equal(h, want_h)
            np.testing.assert_array_equal(J, want_J)


def test_two_scenes_and_permutation_are_bitwise(gpu_ctx):
    """scene_of over S = 2 and a permutation of the instances: an instance's image and rows depend on its own pose
    and scene only (tests/test_gpu_scene_render.py's test for the plain scene)."""
    worlds = [_world(33), _world(200)]
    B, N = 5, 6
    so = np.array([1, 0, 1, 1, 0])
    P, Rm = _poses(worlds[0])
    cfg = _cfg("pinhole", True)
    both = Scene(gpu_ctx, worlds, scene_of=so, grid=True)
    own = [Scene(gpu_ctx, w, grid=True) for w in worlds]
    img = both.render(P, Rm, cfg, (27, 48)).numpy()
    own_img = [s.render(P, Rm, cfg, (27, 48)).numpy() for s in own]
    x, p = _inputs(B, N, seed=8)
    h, J = _rows(gpu_ctx, both, x, p)
    own_rows = [_rows(gpu_ctx, s, x, p) for s in own]
    for b, s in enumerate(so):
        np.testing.assert_array_equal(img[b], own_img[s][b])
        np.testing.assert_array_equal(h[b], own_rows[s][0][b])
        np.testing.assert_array_equal(J[b], own_rows[s][1][b])
    assert np.abs(own_img[0] - own_img[1]).max() > 0.1
    perm = np.array([3, 0, 4, 2, 1])
    other = Scene(gpu_ctx, worlds, scene_of=so[perm], grid=True)
    np.testing.assert_array_equal(other.render(P[perm], Rm[perm], cfg, (27, 48)).numpy(), img[perm])
    hp, Jp = _rows(gpu_ctx, other, x[perm], p[perm])
    np.testing.assert_array_equal(hp, h[perm])
    np.testing.assert_array_equal(Jp, J[perm])
    np.testing.assert_array_equal(own[0].render(P[1:2], Rm[1:2], cfg, (27, 48)).numpy()[0], own_img[0][1])
    with pytest.raises(ValueError):
        Scene(gpu_ctx, worlds, scene_of=[0, 2, 1], grid=True)
    for s in [both, other] + own:
        s.close()


def test_refusals(gpu_ctx):
    ok = Scene.sphere((0.0, 0.0, 0.0), 0.5)
    kinds = _lib.PRIM_KINDS

    def raw(prims, cell=0.0, count=None):
        """the C entry point itself: -> (return code, the handle it left, the message)"""
        pr = (_lib.PrimC * max(len(prims), 1))()
        for k, (kind, vals) in enumerate(prims):
            pr[k].kind = kinds[kind]
            pr[k].a[:len(vals)] = vals
        h = C.c_void_p()
        rc = _lib.load().sdfnmpc_scene_create_large(gpu_ctx.h, 1, (C.c_int * 1)(len(prims) if count is None else count),
                                                    pr, cell, C.byref(h))
        return rc, h.value, _lib.load().sdfnmpc_last_error().decode()

    rc, h, msg = raw([ok] * 65537)
    assert rc != 0 and h is None and "65536" in msg
    rc, h, msg = raw([ok], count=-1)
    assert rc != 0 and h is None
    for bad in (np.nan, np.inf, -np.inf):
        rc, h, msg = raw([ok], cell=bad)
        assert rc != 0 and h is None and "finite" in msg
    for prim in (Scene.sphere((0.0, 0.0, 0.0), -0.5), Scene.box((0, 0, 0), (1, 0, 1)), Scene.cylinder((0, 0), 0.3, 1.0, 1.0),
                 Scene.sphere((np.nan, 0.0, 0.0), 0.5)):
        rc, h, msg = raw([ok, prim])
        assert rc != 0 and h is None and "primitive" in msg
    rc, h, msg = raw([ok, Scene.sphere((900.0, 0.0, 0.0), 0.5)], cell=1e-3)  # 900 000 cells along x
    assert rc != 0 and h is None and "grid is too large" in msg
    # through the package: the library's refusals arrive as SdfnmpcError, the package's own as ValueError
    with pytest.raises(_lib.SdfnmpcError, match="65536"):
        Scene(gpu_ctx, [ok] * 65537, grid=True)
    with pytest.raises(_lib.SdfnmpcError, match="unknown primitive kind"):
        Scene(gpu_ctx, [ok, ("cone", [0.0, 0.0, 0.0, 1.0])], grid=True)
    for bad in (np.nan, np.inf, 0.0, -1.0):
        with pytest.raises(ValueError, match="cell"):
            Scene(gpu_ctx, [ok], grid=True, cell=bad)
    with pytest.raises(ValueError, match="cell"):
        Scene(gpu_ctx, [ok], cell=0.5)
    with pytest.raises(ValueError, match="static"):
        Scene(gpu_ctx, [ok, Scene.moving(ok, v=(0.1, 0.0, 0.0))], grid=True)
    with pytest.raises(ValueError, match="static"):  # even a motion record without motion: a large set carries none
        Scene(gpu_ctx, [Scene.moving(ok)], grid=True)
    with pytest.raises(_lib.SdfnmpcError, match="at most 32"):  # without the grid nothing changes
        Scene(gpu_ctx, [ok] * 33)
    s = Scene(gpu_ctx, [ok] * 33, grid=True)
    assert s.is_indexed and s.distance(np.zeros((1, 3)))[0] == -0.5
    s.close()
    big = Scene(gpu_ctx, [[ok] * 65536, []], grid=True, cell=10.0)  # the limit itself, every sphere in the one cell
    assert big.S == 2 and big.distance(np.array([[2.0, 0.0, 0.0]] * 2))[0] == 1.5
    big.close()


def test_kernel_stats_name_the_kernels_that_ran():
    ctx = _lib.Context(0)  # its own context: the timing switch and the statistics are per context
    prims = _world(33)
    P, Rm = _poses(prims)
    cfg = _cfg("pinhole", True)
    x, p = _inputs(3, 10, seed=2)
    names = ("scene_render", "scene_dist", "scene_sdf_rows")
    ctx.enable_timing(True)
    for scene, suffix, other in ((Scene(ctx, prims, grid=True), "_grid", ""), (Scene(ctx, prims[:32]), "", "_grid")):
        ctx.reset_stats()
        scene.render(P, Rm, cfg, (16, 24))
        scene.render(P, Rm, cfg, (16, 24), t=0.5)
        scene.distance(np.zeros((4, 3)))
        _rows(ctx, scene, x, p)
        assert [ctx.kernel_stats(k + suffix)[1] for k in names] == [2, 1, 1]
        assert [ctx.kernel_stats(k + other)[1] for k in names] == [0, 0, 0]
        assert all(ctx.kernel_stats(k + suffix)[0] > 0.0 for k in names)
        scene.close()
    ctx.close()
