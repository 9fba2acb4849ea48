"""Mixed scenes (Scene(..., grid=True, movers=), sdfnmpc_scene_create_mixed, csrc/scene_grid.hip's *_mixed kernels): an
indexed static set plus up to 32 movers, every query bitwise against the two scenes that existing kernels answer --
G = Scene(statics, grid=True) and D = Scene(movers) -- combined by tests/scene_mixed_ref.py's rule, with no tolerance:
every query is a minimum over primitives, evaluated by the functions the existing kernels call.  The worlds, sensors,
shapes, cells, poses, points and row inputs are those of tests/test_gpu_scene_grid.py."""
import ctypes as C

import numpy as np
import pytest

import scene_mixed_ref as M
import scene_sdf_ref as S
from sdf_nmpc_amd import _lib
from sdf_nmpc_amd.scene import Scene
from test_gpu_scene_grid import CELLS, HI, LO, ROW_SHAPES, SENSORS, SHAPES, _cfg, _inputs, _points, _poses, _world

pytestmark = [pytest.mark.gpu, pytest.mark.filterwarnings("ignore:no SDF weights")]

TIMES = (0.0, 1.7)
# The movers, in the order the counts 1, 5, 32 cut them: a sphere high above the grid's box (the box ends at z = 2); a
# rotating oriented box in front of the last pose's camera; a tilted cylinder; a plain primitive (no motion record: it
# still takes the mover path); a swinging sphere; a crowd.
MOVERS = [Scene.moving(Scene.sphere((0.0, 0.0, 14.0), 1.5), v=(0.3, 0.0, 0.0)),
          Scene.moving(Scene.box((-3.55, -4.25, 0.1), (-3.35, -3.25, 0.9)), rpy=(0.1, 0.2, 0.3), yaw_rate=0.4),
          Scene.moving(Scene.cylinder((1.0, -1.0), 0.3, -0.5, 1.5), rpy=(0.5, 0.3, 0.0), v=(0.0, 0.2, 0.0)),
          Scene.sphere((-1.0, 2.0, 0.5), 0.4),
          Scene.moving(Scene.sphere((2.0, 2.5, 0.2), 0.5), amp=(1.5, 0.0, 0.3), omega=1.1, phase=0.4)] + \
    Scene.crowd(27, LO, HI, seed=7)
# cx > 0 for every pixel is what makes min(G-image, D-image) the image of the nearer hit (scene_mixed_ref): the
# half-fields of both sensors are below pi / 2
assert len(MOVERS) == 32 and all(max(s.values()) < np.pi / 2 for s in SENSORS.values())


def _mixed_poses(prims):
    """test_gpu_scene_grid's five poses, then: above the grid's box looking up, where every ray misses the box and
    MOVERS[0] hangs; and 0.8 m behind MOVERS[1] looking along +x at it, at a spot where no static primitive of the
    three worlds is within 0.5 m of the first metre of the optical axis -- the movers' hit ends the walk in its first
    cells, with the forest behind it."""
    P, Rm = _poses(prims)
    up = np.array([[0.0, 0.0, -1.0], [0.0, 1.0, 0.0], [1.0, 0.0, 0.0]])  # camera x -> world z
    return np.concatenate([P, [(0.0, 0.0, 9.0), (-4.25, -3.75, 0.5)]]), np.concatenate([Rm, [up, np.eye(3)]])


@pytest.mark.parametrize("n", [0, 33, 200])
def test_render_is_bitwise_the_minimum_of_the_two_scenes(gpu_ctx, n):
    statics = _world(n)
    P, Rm = _mixed_poses(statics)
    G = Scene(gpu_ctx, statics, grid=True)
    from_g = from_d = False
    for m in (1, 5, 32):
        D = Scene(gpu_ctx, MOVERS[:m])
        mixed = [Scene(gpu_ctx, statics, grid=True, cell=c, movers=MOVERS[:m]) for c in CELLS]
        assert D.is_dynamic and all(s.is_indexed and s.is_dynamic for s in mixed)
        for sensor in SENSORS:
            for is_depth in (False, True):
                cfg = _cfg(sensor, is_depth)
                for shape in SHAPES:
                    g = G.render(P, Rm, cfg, shape).numpy()
                    for t in TIMES:
                        d = D.render(P, Rm, cfg, shape, t=t).numpy()
                        want = M.render(g, d)
                        for s in mixed:
                            np.testing.assert_array_equal(s.render(P, Rm, cfg, shape, t=t).numpy(), want)
                        from_g = from_g or bool(((want == g) & (g != d)).any())
                        from_d = from_d or bool(((want == d) & (g != d)).any())
                        if shape != (1, 1):
                            assert (want < 1.0).any() and (want == 1.0).any()  # hits and misses
                            assert (g[5] == 1.0).all() and (want[5] < 1.0).any()  # past the grid's box, a mover is seen
                            if m >= 5:  # the mover in front of the last camera hides statics behind it
                                assert ((want[6] == d[6]) & (d[6] < g[6])).any()
        # the raw image: another scale
        cfg = _cfg("pinhole", True)
        want = M.render(G.render(P, Rm, cfg, (16, 24), normalized=False).numpy(),
                        D.render(P, Rm, cfg, (16, 24), normalized=False, t=1.7).numpy())
        np.testing.assert_array_equal(mixed[0].render(P, Rm, cfg, (16, 24), normalized=False, t=1.7).numpy(), want)
        assert want.max() > 1.0
        for s in mixed + [D]:
            s.close()
    G.close()
    assert from_g and from_d  # pixels of either set


def test_distance_is_bitwise_the_minimum_of_the_two_scenes(gpu_ctx):
    """S = 3: movers only, statics only, both; a time per point; p_to_scene and the default ordering."""
    statics = [[], _world(200), _world(33)]
    movers = [MOVERS[:5], [], MOVERS]
    mixed = Scene(gpu_ctx, statics, grid=True, movers=movers)
    G, D = Scene(gpu_ctx, statics, grid=True), Scene(gpu_ctx, movers)
    assert mixed.is_indexed and mixed.is_dynamic and mixed.S == 3 and not G.is_dynamic and D.is_dynamic
    pts = _points(statics[1])
    assert len(pts) == 259
    rng = np.random.default_rng(6)
    t = rng.uniform(0.0, 3.0, len(pts))
    p2s = rng.integers(0, 3, len(pts)).astype(np.int32)
    p2s[:3] = (0, 1, 2)
    g, d = G.distance(pts, p_to_scene=p2s), D.distance(pts, p_to_scene=p2s, t=t)
    want = M.distance(g, d)
    np.testing.assert_array_equal(mixed.distance(pts, p_to_scene=p2s, t=t), want)
    both = p2s == 2
    assert (want[both] == g[both]).any() and ((want[both] == d[both]) & (d[both] < g[both])).any()
    assert np.isinf(g[p2s == 0]).all() and np.isinf(d[p2s == 1]).all() and np.isfinite(want).all()
    assert (want < 0).any() and (want > 50).any()
    assert (mixed.distance(pts, p_to_scene=p2s) != want).any()  # t = 0 is another scene
    # the default ordering, point j -> scene j // (n / S)
    three, t3 = np.concatenate([pts[:86]] * 3), np.concatenate([t[:86]] * 3)
    np.testing.assert_array_equal(mixed.distance(three, t=t3), M.distance(G.distance(three), D.distance(three, t=t3)))
    np.testing.assert_array_equal(mixed.distance(three), M.distance(G.distance(three), D.distance(three)))
    for s in (mixed, G, D):
        s.close()


def _rows(ctx, scene, x, p, max_df, t0=0.0, tau=None):
    """-> h [B, N+1], J [B, N+1, 10]: column 2 of a launch on NaN-filled outputs, whose other columns stay NaN"""
    B, N = x.shape[0], x.shape[1] - 1
    dx, dp = _lib.DeviceArray.from_numpy(ctx, x), _lib.DeviceArray.from_numpy(ctx, p)
    dh = _lib.DeviceArray.from_numpy(ctx, np.full((B, N + 1, 3), np.nan))
    dJ = _lib.DeviceArray.from_numpy(ctx, np.full((B, N + 1, 10, 3), np.nan))
    dtau = None if tau is None else _lib.DeviceArray.from_numpy(ctx, np.asarray(tau, float))
    _lib.scene_sdf_rows(ctx, scene.h, B, N, p.shape[-1], dx, dp, dh, dJ, max_df, scene_of=scene._scene_of, t0=t0, tau=dtau)
    h, J = dh.numpy(), dJ.numpy()
    assert np.isnan(h[..., :2]).all() and np.isnan(J[..., :2]).all()
    return h[..., 2], J[..., 2]


@pytest.mark.parametrize("B,N", ROW_SHAPES)
def test_sdf_rows_are_bitwise_the_selection_of_the_two_scenes(gpu_ctx, B, N):
    statics, movers = [_world(200), _world(33)], [MOVERS, MOVERS[:5]]
    so = np.arange(B) % 2
    mixed = [Scene(gpu_ctx, statics, scene_of=so, grid=True, cell=c, movers=movers) for c in CELLS]
    G, D = Scene(gpu_ctx, statics, scene_of=so, grid=True), Scene(gpu_ctx, movers, scene_of=so)
    x, p = _inputs(B, N, seed=50 + B)  # the flag is 1, and 0 at every third node
    t0, tau = 0.7, 0.15 * np.arange(N + 1)
    for max_df in (0.2, 3.0):
        for tk in (None, tau):
            gh, gJ = _rows(gpu_ctx, G, x, p, max_df)
            dh, dJ = _rows(gpu_ctx, D, x, p, max_df, t0=t0, tau=tk)
            want_h, want_J = M.rows(gh, gJ, dh, dJ)
            for s in mixed:
                h, J = _rows(gpu_ctx, s, x, p, max_df, t0=t0, tau=tk)
                np.testing.assert_array_equal(h, want_h)
                np.testing.assert_array_equal(J, want_J)
            off = p[..., 0] == 0.0
            assert (want_h[off] == max_df).all() and not want_J[off].any() and not want_J[..., 3:].any()
            if B == 37 and max_df == 3.0:  # rows of either set, and the node times reach the movers
                assert (dh < gh).any() and ((gh < dh) & (gh < max_df)).any()
                if tk is not None:
                    assert (dh != _rows(gpu_ctx, D, x, p, max_df, t0=t0)[0]).any()
    for s in mixed + [G, D]:
        s.close()


@pytest.mark.parametrize("cell", [None, 0.5])
def test_on_a_tie_the_static_primitive_supplies_the_gradient(gpu_ctx, cell):
    """Static sphere at (-2, 0, 0), a mover of the same radius passing (2, 0, 0) at t = 0, a node at the origin."""
    scene = Scene(gpu_ctx, [M.TIE_STATIC], grid=True, cell=cell, movers=[M.TIE_MOVER])
    x, p = _inputs(1, 10, seed=1)
    x[0, 0, :3] = 0.0
    p[..., 0] = 1.0
    h, J = _rows(gpu_ctx, scene, x, p, 3.0, t0=0.0)
    assert h[0, 0] == 1.0
    np.testing.assert_array_equal(J[0, 0, :3], [1.0, 0.0, 0.0])
    h, J = _rows(gpu_ctx, scene, x, p, 3.0, t0=M.TIE_T_NEARER)  # the mover strictly nearer: its gradient
    assert h[0, 0] == 0.75
    np.testing.assert_array_equal(J[0, 0, :3], [-1.0, 0.0, 0.0])
    scene.close()


def test_fractional_flag_against_the_numpy_reference(gpu_ctx):
    """Flag 0.3 on every row, against scene_mixed_ref.sdf_rows from the geometry.  tests/tolerances.py names no bar for
    the scene rows; it holds fp64 entries of the linearisation to atol 1e-12 x scale (scale = max(1, max |want|)),
    which is the bar tests/test_gpu_scene_sdf.py already uses for these rows (ATOL = 1e-12 on decided rows): a row is
    a closed form of some 30 fp64 operations on coordinates below 16, an error below 30 x 16 x 2^-53 = 5e-14."""
    statics, movers = _world(33), MOVERS[:5]
    scene = Scene(gpu_ctx, statics, grid=True, movers=movers)
    B, N = 37, 6
    x, p = _inputs(B, N, seed=9)
    p[..., 0] = 0.3
    t0, tau, max_df = 0.7, 0.15 * np.arange(N + 1), 3.0
    h, J = _rows(gpu_ctx, scene, x, p, max_df, t0=t0, tau=tau)
    want_h, want_J = M.sdf_rows(statics, movers, x, p, max_df, t0=t0, tau=tau)
    ok = S.decided(M.to_ref(statics + movers), x, max_df, t0=t0, tau=tau)
    scale = max(1.0, np.abs(want_h).max(), np.abs(want_J).max())
    eh, eJ = np.abs(h - want_h)[ok].max(), np.abs(J - want_J)[ok].max()
    print(f"\nfractional flag: {ok.size - ok.sum()} of {ok.size} rows undecided; max error h {eh:.2e}, J_h {eJ:.2e}")
    assert ok.mean() >= 0.95
    assert eh <= 1e-12 * scale and eJ <= 1e-12 * scale
    assert ((want_h < max_df) & ok).any() and np.abs(want_J[ok]).max() > 0.25
    scene.close()


def test_without_movers_the_handle_is_the_indexed_scene():
    ctx = _lib.Context(0)  # its own context: the timing switch and the statistics are per context
    prims = _world(33)
    P, Rm = _mixed_poses(prims)
    cfg = _cfg("pinhole", True)
    x, p = _inputs(3, 10, seed=2)
    names = ("scene_render", "scene_dist", "scene_sdf_rows")
    ctx.enable_timing(True)
    plain = Scene(ctx, prims, grid=True)
    want = plain.render(P, Rm, cfg, (16, 24)).numpy()
    for scene, suffix, others in ((Scene(ctx, prims, grid=True, movers=[]), "_grid", ("_mixed", "_dyn")),
                                  (Scene(ctx, [prims, prims], grid=True, movers=[[], []]), "_grid", ("_mixed", "_dyn")),
                                  (Scene(ctx, prims, grid=True, movers=MOVERS[:5]), "_mixed", ("_grid", "_dyn"))):
        assert scene.is_indexed and scene.is_dynamic == (suffix == "_mixed")
        ctx.reset_stats()
        img = scene.render(P, Rm, cfg, (16, 24))
        scene.render(P, Rm, cfg, (16, 24), t=0.5)
        scene.distance(np.zeros((4, 3)))
        _rows(ctx, scene, x, p, 1.0)
        assert [ctx.kernel_stats(k + suffix)[1] for k in names] == [2, 1, 1]
        for other in others:
            assert [ctx.kernel_stats(k + other)[1] for k in names[:2]] == [0, 0]
        assert ctx.kernel_stats("scene_sdf_rows" + others[0])[1] == 0 and ctx.kernel_stats("scene_sdf_rows")[1] == 0
        if suffix == "_grid":
            np.testing.assert_array_equal(img.numpy(), want)
        scene.close()
    plain.close()
    ctx.close()


def test_refusals(gpu_ctx):
    ok = Scene.sphere((0.0, 0.0, 0.0), 0.5)
    with pytest.raises(_lib.SdfnmpcError, match="at most 32 movers"):
        Scene(gpu_ctx, [ok], grid=True, movers=[ok] * 33)
    with pytest.raises(ValueError, match="grid"):
        Scene(gpu_ctx, [ok], movers=[ok])
    with pytest.raises(ValueError, match="movers"):
        Scene(gpu_ctx, [[ok], [ok]], grid=True, movers=[[ok]])
    with pytest.raises(ValueError, match="movers"):
        Scene(gpu_ctx, [ok], grid=True, movers=[[ok], [ok]])
    with pytest.raises(ValueError, match="static"):  # a moving primitive among prims stays refused
        Scene(gpu_ctx, [Scene.moving(ok, v=(0.1, 0.0, 0.0))], grid=True, movers=[ok])
    with pytest.raises(_lib.SdfnmpcError, match="quaternion"):
        Scene(gpu_ctx, [ok], grid=True, movers=[Scene.moving(ok, q=(0.0, 0.0, 0.0, 0.0))])
    for kw in (dict(v=(np.nan, 0.0, 0.0)), dict(omega=np.inf), dict(amp=(0.0, -np.inf, 0.0)), dict(yaw_rate=np.nan)):
        with pytest.raises(_lib.SdfnmpcError, match="finite"):
            Scene(gpu_ctx, [ok], grid=True, movers=[ok, Scene.moving(ok, **kw)])
    with pytest.raises(_lib.SdfnmpcError, match="primitive"):  # the movers' shapes are checked as any primitive's
        Scene(gpu_ctx, [ok], grid=True, movers=[Scene.sphere((0.0, 0.0, 0.0), -1.0)])
    with pytest.raises(_lib.SdfnmpcError, match="65536"):  # and the static set as sdfnmpc_scene_create_large checks it
        Scene(gpu_ctx, [ok] * 65537, grid=True, movers=[ok])
    scene = Scene(gpu_ctx, [ok], grid=True, movers=[Scene.moving(ok, v=(1.0, 0.0, 0.0))])
    P, Rm = np.array([[-3.0, 0.0, 0.0]]), np.eye(3)[None]
    for bad in (np.nan, np.inf):
        with pytest.raises(_lib.SdfnmpcError, match="finite"):
            scene.render(P, Rm, _cfg("pinhole", True), (4, 6), t=bad)
    assert scene.distance(np.array([[3.0, 0.0, 0.0]]), t=2.0)[0] == 0.5  # the mover's centre at x = 2
    assert scene.distance(np.array([[3.0, 0.0, 0.0]]))[0] == 2.5
    scene.close()
    # movers alone, and only movers without a motion record: still the mover path
    alone = Scene(gpu_ctx, [], grid=True, movers=[ok])
    assert alone.is_indexed and alone.is_dynamic and alone.distance(np.array([[2.0, 0.0, 0.0]]))[0] == 1.5
    alone.close()


def test_raw_abi_refuses_bad_mover_counts(gpu_ctx):
    lib = _lib.load()
    pr = (_lib.PrimC * 1)()
    pr[0].kind = _lib.PRIM_KINDS["sphere"]
    pr[0].a[:4] = [0.0, 0.0, 0.0, 0.5]
    one = (C.c_int * 1)(1)
    for mcount in (None, (C.c_int * 1)(-1), (C.c_int * 1)(33)):
        h = C.c_void_p()
        rc = lib.sdfnmpc_scene_create_mixed(gpu_ctx.h, 1, one, pr, 0.0, mcount, pr, None, C.byref(h))
        assert rc != 0 and h.value is None
    h = C.c_void_p()
    assert lib.sdfnmpc_scene_create_mixed(gpu_ctx.h, 1, one, pr, 0.0, one, pr, None, C.byref(h)) == 0 and h.value
    assert lib.sdfnmpc_scene_is_indexed(h) == 1 and lib.sdfnmpc_scene_is_dynamic(h) == 1
    lib.sdfnmpc_scene_free(h)
