"""Mesh scenes with movers (Scene.mesh(..., movers=), sdfnmpc_scene_create_mesh_mixed, csrc/scene_mesh.hip's *_mesh_mixed
kernels and scene_swept.hip's fifth evaluator): a triangle mesh plus up to 32 movers per scene, every query bitwise
against the two scenes that kernels from before this feature answer -- M = Scene.mesh(meshes) and D = Scene(movers) --
combined by tests/scene_mixed_ref.py's rules, with no tolerance; on a tie the mesh comes before a mover.  The swept
clearance has no composition and is held to test_gpu_scene_swept.py's certificates against a dense sampler.

Every test here fails without the feature: Scene.mesh has no ``movers`` and the library no
sdfnmpc_scene_create_mesh_mixed."""
import ctypes as C

import numpy as np
import pytest

import mesh_ref as MR
import mesh_sdf_ref as MS
import scene_dyn_ref as DR
import scene_mixed_ref as X
import scene_ref as R
import scene_sdf_ref as S
from sdf_nmpc_amd import _lib
from sdf_nmpc_amd.config import Config
from sdf_nmpc_amd.mesh import Mesh
from sdf_nmpc_amd.scene import Scene
from test_gpu_scene_mesh import FIXED, LEAVES, _cfg, _hierarchy_cases
from test_gpu_scene_mixed import _rows
from test_gpu_scene_sdf import NP, SHAPES as ROW_SHAPES

pytestmark = [pytest.mark.gpu, pytest.mark.filterwarnings("ignore:no SDF weights"),
              pytest.mark.filterwarnings("ignore:QP reached")]

TIMES = (0.0, 1.7)
LO, HI = (-1.0, -3.0, -1.5), (6.0, 3.0, 2.5)
# The movers, in the order the counts 1, 5, 32 cut them: a sphere that crosses in front of the fixed scene's wall (the
# box face x = 3.5, y in 0.5 .. 1.5); a rotating oriented box; a tilted cylinder; a plain primitive (no motion record:
# it is still a mover); a swinging sphere; a crowd.
MOVERS = [Scene.moving(Scene.sphere((3.0, 1.0, 0.0), 0.3), v=(0.0, -0.4, 0.0)),
          Scene.moving(Scene.box((1.5, -2.0, -0.5), (2.1, -1.4, 0.3)), rpy=(0.1, 0.2, 0.3), yaw_rate=0.4),
          Scene.moving(Scene.cylinder((1.0, 1.8), 0.25, -0.5, 1.0), rpy=(0.5, 0.3, 0.0), v=(0.0, 0.2, 0.0)),
          Scene.sphere((0.5, -1.5, 0.5), 0.4),
          Scene.moving(Scene.sphere((4.5, -1.5, 0.2), 0.5), amp=(1.5, 0.0, 0.3), omega=1.1, phase=0.4)] + \
    Scene.crowd(27, LO, HI, seed=7)
COUNTS = (1, 5, 32)
EMPTY = Mesh([], [])
CASES = ["fixed", "fixed_open", "terrain", "tunnel", "one"]
assert len(MOVERS) == 32 and all(max(s[k] for k in ("hfov", "vfov")) < np.pi / 2 for s in (R.SENSOR, R.SPHERICAL))


def _three(ctx, mesh, closed, m, **kw):
    """S = 3 -- scene 0 the mesh alone, scene 1 movers alone (a mesh without triangles), scene 2 both -- as the scene
    under test and as the two scenes that compose it"""
    meshes, movers = [mesh, EMPTY, mesh], [[], MOVERS[:m], MOVERS[:m]]
    so = kw.pop("scene_of", None)
    return (Scene.mesh(ctx, meshes, closed=closed, movers=movers, scene_of=so, **kw),
            Scene.mesh(ctx, meshes, closed=closed, scene_of=so, **kw), Scene(ctx, movers, scene_of=so))


def _poses():
    """The fixed scene's three poses, then: inside mover 3 (a plain sphere: the pixel is 0 at every time); inside the
    closed box of the fixed scene; behind mover 3 looking along +x past the mesh at it; 2.5 m in front of the wall with
    mover 0 between the camera and the wall at t = 0.  One instance per scene of the set, cyclically."""
    P, Rm = R.camera_poses()
    P = np.concatenate([P, [(0.5, -1.5, 0.5), (3.8, 1.0, 0.0), (-3.0, -1.5, 0.5), (0.5, 1.0, 0.0)]])
    return P, np.concatenate([Rm, [np.eye(3)] * 4])


def _special_points(mesh, rng, k):
    """vertices, edge midpoints and centroids of up to k triangles of the mesh as the library sees it"""
    v = mesh.verts.astype(np.float32).astype(np.float64)
    tv = v[mesh.tris[rng.permutation(mesh.tris.shape[0])[:k]]]
    return np.concatenate([tv.reshape(-1, 3), (0.5 * (tv + np.roll(tv, 1, axis=1))).reshape(-1, 3), tv.mean(1)])


def _points(mesh, n=259, seed=3):
    """n points with a time each: on the mesh (exact ties within it), inside movers at the points' times, inside the fixed
    scene's closed box, and all around"""
    rng = np.random.default_rng(seed)
    sp = _special_points(mesh, rng, 15)
    t = rng.uniform(0.0, 3.0, n)
    pts = rng.uniform(LO, HI, (n, 3))
    pts[:len(sp)] = sp
    k = len(sp)
    ref = X.to_ref(MOVERS)
    for i in range(40):  # the centre of mover i % 32 at the point's time, nudged: inside it
        c0, _ = DR.canonical(ref[i % 32][0], ref[i % 32][1])
        mo = ref[i % 32][2] if len(ref[i % 32]) > 2 else None
        c = np.asarray(c0, float) if mo is None else \
            np.asarray(c0) + np.asarray(mo["v"]) * t[k + i] + np.asarray(mo["amp"]) * np.sin(mo["omega"] * t[k + i] + mo["phase"])
        pts[k + i] = c + rng.uniform(-0.05, 0.05, 3)
    pts[k + 40:k + 60] = rng.uniform((3.5, 0.5, -1.0), (4.1, 1.5, 1.2), (20, 3))
    p2s = rng.integers(0, 3, n).astype(np.int32)
    p2s[:3] = (0, 1, 2)
    p2s[k:k + 50:2] = 2  # scene 2, the mesh and the movers, holds points inside movers (mover 0 among them) and in the box
    return pts, t, p2s


# ---- 1. render
@pytest.mark.parametrize("name", CASES)
def test_render_is_bitwise_the_minimum_of_the_two_scenes(gpu_ctx, name):
    mesh, closed = _hierarchy_cases()[name]
    P, Rm = _poses()
    so = np.arange(len(P)) % 3
    so[3:] = 2  # the constructed poses see both sets
    from_m = from_d = False
    for m in COUNTS:
        sc, Ms, Ds = _three(gpu_ctx, mesh, closed, m, scene_of=so)
        assert sc.is_mesh and sc.is_dynamic and not sc.is_indexed and not Ms.is_dynamic and Ds.is_dynamic
        for sensor in ("pinhole", "spherical"):
            for is_depth in (False, True):
                cfg = _cfg(sensor, is_depth)
                for shape in ((18, 32), (7, 13)):
                    g = Ms.render(P, Rm, cfg, shape).numpy()
                    for t in TIMES:
                        d = Ds.render(P, Rm, cfg, shape, t=t).numpy()
                        want = X.render(g, d)
                        np.testing.assert_array_equal(sc.render(P, Rm, cfg, shape, t=t).numpy().view(np.uint32),
                                                      want.view(np.uint32))
                        from_m = from_m or bool(((want == g) & (g != d)).any())
                        from_d = from_d or bool(((want == d) & (g != d)).any())
                        if m >= 5:
                            assert (want[3] == 0.0).all()  # a camera inside a mover sees zero
                            assert (want[5] < 1.0).any()   # the mover past the mesh is seen
                        if name == "fixed" and m <= 5:  # (a swinging member of the crowd may reach this camera)
                            assert (want[4] > 0.0).all() and (want[4] < 1.0).any()  # inside the closed mesh: its inner walls
                            if t == 0.0:  # the mover in front of the wall hides part of it, the wall shows beside it
                                assert ((d[6] < g[6]) & (want[6] == d[6])).any() and ((g[6] < d[6]) & (want[6] == g[6])).any()
        cfg = _cfg("pinhole", True)  # the raw image: another scale
        want = X.render(Ms.render(P, Rm, cfg, (18, 32), normalized=False).numpy(),
                        Ds.render(P, Rm, cfg, (18, 32), normalized=False, t=1.7).numpy())
        np.testing.assert_array_equal(sc.render(P, Rm, cfg, (18, 32), normalized=False, t=1.7).numpy(), want)
        assert want.max() > 1.0
        for s in (sc, Ms, Ds):
            s.close()
    assert from_m and from_d  # pixels of either set


# ---- 2. distance
@pytest.mark.parametrize("name", CASES)
def test_distance_is_bitwise_the_minimum_of_the_two_scenes(gpu_ctx, name):
    mesh, closed = _hierarchy_cases()[name]
    pts, t, p2s = _points(mesh)
    assert len(pts) == 259
    for m in COUNTS:
        sc, Ms, Ds = _three(gpu_ctx, mesh, closed, m)
        g, d = Ms.distance(pts, p_to_scene=p2s), Ds.distance(pts, p_to_scene=p2s, t=t)
        want = X.distance(g, d)
        np.testing.assert_array_equal(sc.distance(pts, p_to_scene=p2s, t=t), want)
        both = p2s == 2
        assert (want[both] == g[both]).any() and ((want[both] == d[both]) & (d[both] < g[both])).any()
        assert np.isinf(g[p2s == 1]).all() and np.isinf(d[p2s == 0]).all() and np.isfinite(want).all()
        assert (g[both] == 0).any()  # points on the mesh
        if m == 32:
            assert (d[both] < 0).any()  # points inside movers
            assert (sc.distance(pts, p_to_scene=p2s) != want).any()  # t = 0 is another scene
        if name == "fixed":
            assert (g[both] < 0).any()  # points inside the closed mesh
        # the default ordering, point j -> scene j // (n / S)
        three, t3 = np.concatenate([pts[:86]] * 3), np.concatenate([t[:86]] * 3)
        np.testing.assert_array_equal(sc.distance(three, t=t3), X.distance(Ms.distance(three), Ds.distance(three, t=t3)))
        np.testing.assert_array_equal(sc.distance(three), X.distance(Ms.distance(three), Ds.distance(three)))
        for s in (sc, Ms, Ds):
            s.close()


# ---- 3. SDF rows
def _row_inputs(B, N, seed):
    """test_gpu_scene_sdf's inputs: the flag is 1, and 0 at every third node"""
    rng = np.random.default_rng(seed)
    x = rng.normal(0, 1, (B, N + 1, 10))
    x[..., :3] = S.draw(B * (N + 1), seed).reshape(B, N + 1, 3)
    p = rng.normal(0, 1, (B, N + 1, NP))
    p[..., 0] = 1.0
    p[:, 2::3, 0] = 0.0
    return x, p


@pytest.mark.parametrize("closed", [True, False])
@pytest.mark.parametrize("B,N", ROW_SHAPES)
def test_sdf_rows_are_bitwise_the_selection_of_the_two_scenes(gpu_ctx, B, N, closed):
    so = np.arange(B) % 3
    x, p = _row_inputs(B, N, seed=50 + B)
    t0, tau = 0.7, 0.15 * np.arange(N + 1)
    for m in (5, 32):
        sc, Ms, Ds = _three(gpu_ctx, FIXED, closed, m, scene_of=so, sdf_source=True)
        assert sc.is_sdf_source
        for max_df in (0.2, 3.0):
            for tk in (None, tau):
                gh, gJ = _rows(gpu_ctx, Ms, x, p, max_df)
                dh, dJ = _rows(gpu_ctx, Ds, x, p, max_df, t0=t0, tau=tk)
                want_h, want_J = X.rows(gh, gJ, dh, dJ)
                h, J = _rows(gpu_ctx, sc, x, p, max_df, t0=t0, tau=tk)
                np.testing.assert_array_equal(h, want_h)
                np.testing.assert_array_equal(J, want_J)
                off = p[..., 0] == 0.0
                assert (want_h[off] == max_df).all() and not want_J[off].any() and not want_J[..., 3:].any()
                if B == 37 and max_df == 3.0:  # rows of either set, and the node times reach the movers
                    assert (dh < gh).any() and ((gh < dh) & (gh < max_df)).any()
                    if tk is not None:
                        assert (dh != _rows(gpu_ctx, Ds, x, p, max_df, t0=t0)[0]).any()
        for s in (sc, Ms, Ds):
            s.close()


@pytest.mark.parametrize("closed", [True, False])
def test_fractional_flag_against_the_numpy_reference(gpu_ctx, closed):
    """Flag 0.3 on every row, against rows built in numpy from mesh_sdf_ref and scene_sdf_ref by the composition rule, on
    every row (none set aside as undecided) at 1e-12 x scale, scale = max(1, max |want|): the bar of
    tests/test_gpu_scene_mixed.py and tests/test_gpu_scene_sdf_mesh.py for these fp64 closed forms."""
    movers = MOVERS[:5]
    sc = Scene.mesh(gpu_ctx, FIXED, closed=closed, sdf_source=True, movers=movers)
    B, N = 37, 6
    x, p = _row_inputs(B, N, seed=9)
    p[..., 0] = 0.3
    t0, tau, max_df = 0.7, 0.15 * np.arange(N + 1), 3.0
    h, J = _rows(gpu_ctx, sc, x, p, max_df, t0=t0, tau=tau)
    pts = x[..., :3].reshape(-1, 3)
    gd, gg = MS.dist_grad(MR.rounded(FIXED), pts, closed)
    dd, dg, _ = S.dist_grad(X.to_ref(movers), pts, S._times((B, N + 1), t0, tau).ravel())
    lower = dd < gd  # strictly: the mesh keeps a tie
    d, g = np.where(lower, dd, gd), np.where(lower[:, None], dg, gg)
    near = d < max_df
    want_h = (0.3 * np.where(near, d, max_df) + 0.7 * max_df).reshape(B, N + 1)
    want_J = np.zeros((B, N + 1, 10))
    want_J[..., :3] = (0.3 * np.where(near[:, None], g, 0.0)).reshape(B, N + 1, 3)
    scale = max(1.0, np.abs(want_h).max(), np.abs(want_J).max())
    eh, eJ = np.abs(h - want_h).max(), np.abs(J - want_J).max()
    print(f"\nfractional flag, closed={closed}: max error h {eh:.2e}, J_h {eJ:.2e} over all {h.size} rows; "
          f"{int(lower.sum())} rows from a mover")
    assert eh <= 1e-12 * scale and eJ <= 1e-12 * scale
    assert lower.any() and (~lower & near).any() and np.abs(want_J).max() > 0.25
    sc.close()


@pytest.mark.parametrize("closed", [True, False])
def test_row_contract(gpu_ctx, closed):
    """A NaN row and an infinite row leave the rest of the batch alone, are finite, and are the composition of M's and
    D's rows like any other: the mesh has no winner there and gives (max_df, 0) by scene_sdf_rows_mesh_kernel's rule; the
    movers give what scene_sdf_rows_kernel gives for such a point (a box's closed form drops a NaN in fmax / fmin and
    answers 0).  Beside spheres alone, whose closed form keeps the NaN, the row is (max_df, 0).  Columns 0 and 1 are
    untouched (test_gpu_scene_mixed._rows asserts their NaN fill on every launch)."""
    B, N = 37, 6
    x, p = _row_inputs(B, N, seed=87)
    for movers, strict in ((MOVERS[:5], False), ([MOVERS[0], MOVERS[3], MOVERS[4]], True)):
        sc = Scene.mesh(gpu_ctx, FIXED, closed=closed, sdf_source=True, movers=movers)
        Ms, Ds = Scene.mesh(gpu_ctx, FIXED, closed=closed, sdf_source=True), Scene(gpu_ctx, movers)
        h, J = _rows(gpu_ctx, sc, x, p, 1.0, t0=0.7)
        assert np.isfinite(h).all() and np.isfinite(J).all()
        rows = [(b, 0) for b in range(B) if h[b, 0] < 1.0][:2]
        assert len(rows) == 2
        xb = x.copy()
        xb[rows[0]][1], xb[rows[1]][0] = np.nan, np.inf
        hb, Jb = _rows(gpu_ctx, sc, xb, p, 1.0, t0=0.7)
        assert np.isfinite(hb).all() and np.isfinite(Jb).all()
        want_h, want_J = X.rows(*_rows(gpu_ctx, Ms, xb, p, 1.0), *_rows(gpu_ctx, Ds, xb, p, 1.0, t0=0.7))
        np.testing.assert_array_equal(hb, want_h)
        np.testing.assert_array_equal(Jb, want_J)
        keep = np.ones((B, N + 1), bool)
        for r in rows:
            keep[r] = False
            assert _rows(gpu_ctx, Ms, xb, p, 1.0)[0][r] == 1.0  # the mesh's rule
            if strict:
                assert hb[r] == 1.0 and not Jb[r].any()
        np.testing.assert_array_equal(hb[keep], h[keep])
        np.testing.assert_array_equal(Jb[keep], J[keep])
        for s_ in (sc, Ms, Ds):
            s_.close()


# ---- 4. the tie, from exactly representable numbers
@pytest.mark.parametrize("leaf", [None, -1])
@pytest.mark.parametrize("closed", [True, False])
def test_on_a_tie_the_mesh_supplies_the_gradient(gpu_ctx, closed, leaf):
    """A box mesh with its face at x = -1, a mover sphere of radius 1 passing x = 2 at t = 0, a node at the origin."""
    sc = Scene.mesh(gpu_ctx, Mesh.box((-2.0, -1.0, -1.0), (-1.0, 1.0, 1.0)), closed=closed, leaf_size=leaf, sdf_source=True,
                    movers=[X.TIE_MOVER])
    x, p = _row_inputs(1, 10, seed=1)
    x[0, 0, :3] = 0.0
    p[..., 0] = 1.0
    h, J = _rows(gpu_ctx, sc, x, p, 3.0, t0=0.0)
    assert h[0, 0] == 1.0
    np.testing.assert_array_equal(J[0, 0, :3], [1.0, 0.0, 0.0])
    h, J = _rows(gpu_ctx, sc, x, p, 3.0, t0=X.TIE_T_NEARER)  # the mover strictly nearer: its gradient
    assert h[0, 0] == 0.75
    np.testing.assert_array_equal(J[0, 0, :3], [-1.0, 0.0, 0.0])
    assert sc.distance(np.zeros((1, 3)))[0] == 1.0 and sc.distance(np.zeros((1, 3)), t=X.TIE_T_NEARER)[0] == 0.75
    sc.close()


# ---- 5. the hierarchy changes no bit
@pytest.mark.parametrize("name", CASES)
def test_hierarchy_changes_no_bit(gpu_ctx, name):
    mesh, closed = _hierarchy_cases()[name]
    P, Rm = _poses()
    pts, t, _ = _points(mesh)
    rng = np.random.default_rng(11)
    p0 = rng.uniform(LO, HI, (60, 3))
    p1 = p0 + rng.uniform(-0.7, 0.7, (60, 3))
    c0 = rng.uniform(0.0, 2.0, 60)
    x, p = _row_inputs(37, 6, seed=12)
    cfgs = [(_cfg("pinhole", True), (18, 32)), (_cfg("spherical", False), (7, 13))]

    def run(leaf):
        sc = Scene.mesh(gpu_ctx, mesh, closed=closed, leaf_size=leaf, sdf_source=True, movers=MOVERS[:5])
        imgs = [sc.render(P, Rm, cfg, shape, t=1.7).numpy() for cfg, shape in cfgs]
        d = sc.distance(pts, t=t)
        sw = sc.swept_distance(p0, p1, t0=c0, t1=c0 + 0.2, eps=1e-3, max_evals=256)
        rows = [_rows(gpu_ctx, sc, x, p, max_df, t0=0.7, tau=0.15 * np.arange(7)) for max_df in (0.2, 3.0)]
        sc.close()
        return imgs, d, sw, rows

    bi, bd, bs, br = run(-1)
    assert np.isfinite(bd).all() and all((im < 1.0).any() for im in bi)
    for leaf in LEAVES:
        imgs, d, s, rows = run(leaf)
        for a, b in zip(imgs, bi):
            np.testing.assert_array_equal(a.view(np.uint32), b.view(np.uint32), err_msg=f"render, leaf {leaf}")
        np.testing.assert_array_equal(d, bd, err_msg=f"distance, leaf {leaf}")
        for k in ("dmin", "s", "gap", "evals"):
            np.testing.assert_array_equal(getattr(s, k), getattr(bs, k), err_msg=f"swept {k}, leaf {leaf}")
        for (h, J), (wh, wJ) in zip(rows, br):
            np.testing.assert_array_equal(h, wh, err_msg=f"rows h, leaf {leaf}")
            np.testing.assert_array_equal(J, wJ, err_msg=f"rows J, leaf {leaf}")


# ---- 6. swept clearance
M_DENSE, EPS, N_SEG = 64, 1e-3, 300
SWEPT_MOVERS = MOVERS[:5]


@pytest.fixture(scope="module")
def swept_ref():
    """300 chords with times, and the dense sampler's minimum of D(s) = min(mesh_ref.distance, scene_dyn_ref distance)
    over the M_DENSE + 1 uniform samples of each, open and closed: the unsigned distance is |signed|.  M_DENSE = 64
    keeps the brute-force mesh reference to a few seconds; both certificates hold for every M."""
    rng = np.random.default_rng(17)
    p0 = rng.uniform((-0.5, -3.0, -1.4), (6.0, 3.0, 2.0), (N_SEG, 3))
    e = rng.normal(size=(N_SEG, 3))
    p1 = p0 + e / np.linalg.norm(e, axis=1, keepdims=True) * rng.uniform(0.0, 1.0, (N_SEG, 1))
    t0 = rng.uniform(0.0, 2.0, N_SEG)
    t1 = t0 + rng.uniform(-0.2, 0.2, N_SEG)
    s = np.arange(M_DENSE + 1) / M_DENSE
    q = (p0[:, None] + s[None, :, None] * (p1 - p0)[:, None]).reshape(-1, 3)
    tq = (t0[:, None] + s[None] * (t1 - t0)[:, None]).ravel()
    prims = X.to_ref(SWEPT_MOVERS)
    dm = MR.distance(MR.rounded(FIXED), q, signed=True)
    dd = DR.distance(prims, q, tq)
    dense = {True: np.minimum(dm, dd).reshape(N_SEG, -1).min(1), False: np.minimum(np.abs(dm), dd).reshape(N_SEG, -1).min(1)}
    import swept_ref as W
    V = W.speed_bound(prims)
    out = (p0, p1, t0, t1, dense, V)
    for a in (p0, p1, t0, t1, dense[True], dense[False]):
        a.setflags(write=False)
    return out


@pytest.mark.parametrize("closed", [True, False])
def test_swept_certificate_against_dense_sampling(gpu_ctx, swept_ref, closed):
    p0, p1, t0, t1, dense, V = swept_ref
    sc = Scene.mesh(gpu_ctx, FIXED, closed=closed, movers=SWEPT_MOVERS)
    Ds = Scene(gpu_ctx, SWEPT_MOVERS)
    np.testing.assert_array_equal(sc.speed_bound, Ds.speed_bound)
    assert abs(sc.speed_bound[0] - V) <= 1e-12 * V and V > 0
    r = sc.swept_distance(p0, p1, t0=t0, t1=t1, eps=EPS)
    L = np.linalg.norm(p1 - p0, axis=1) + V * np.abs(t1 - t0)
    dn = dense[closed]
    lo, hi = r.dmin - (dn - L / (2 * M_DENSE)), (r.dmin - r.gap) - dn
    print(f"\nmesh with movers, closed={closed}: dmin - (dense - L / 2M) >= {lo.min():.2e}, (dmin - gap) - dense <= "
          f"{hi.max():.2e}, gap <= {r.gap.max():.2e}, evals median {int(np.median(r.evals))} max {r.evals.max()}")
    assert (lo >= -1e-9).all()
    assert (hi <= 1e-9).all()
    assert (r.evals <= 4096).all() and (r.evals >= 1).all() and (r.gap >= 0.0).all()
    assert (r.gap[r.evals < 4096] <= EPS + 1e-12).all()
    at = sc.distance(p0 + r.s[:, None] * (p1 - p0), t=t0 + r.s * (t1 - t0))
    assert np.abs(at - r.dmin).max() <= 1e-9
    sc.close()
    Ds.close()


@pytest.mark.parametrize("closed", [True, False])
def test_swept_sees_a_mover_cross_a_chord(gpu_ctx, closed):
    """A sphere crosses the chord between t0 and t1; at both ends of the chord, at their times, the scene is clear."""
    mover = Scene.moving(Scene.sphere((1.25, -6.0, 0.0), 0.3), v=(0.0, 20.0, 0.0))  # over the chord's midpoint at t = 0.3
    sc = Scene.mesh(gpu_ctx, FIXED, closed=closed, movers=[mover])
    p0, p1 = np.array([[1.0, 0.0, 0.0]]), np.array([[1.5, 0.0, 0.0]])
    assert sc.distance(p0, t=0.2)[0] > 0.3 and sc.distance(p1, t=0.4)[0] > 0.3
    r = sc.swept_distance(p0, p1, t0=0.2, t1=0.4)
    print(f"\ncrossing mover, closed={closed}: dmin {r.dmin[0]:.4f} at s = {r.s[0]:.4f}, gap {r.gap[0]:.1e}, {r.evals[0]} evals")
    assert r.dmin[0] < 0.0 and -0.3 - 1e-9 <= r.dmin[0] <= -0.3 + r.gap[0] + 1e-9  # the centre passes through the chord
    assert sc.swept_distance(p0, p1).dmin[0] > 0.3  # without times nothing moves
    sc.close()


# ---- 7. what the handle is
def test_set_semantics_and_kernel_names():
    ctx = _lib.Context(0)  # its own context: the timing switch and the statistics are per context
    P, Rm = _poses()
    cfg = _cfg("pinhole", True)
    x, p = _row_inputs(3, 10, seed=2)
    names = ("scene_render", "scene_dist", "scene_sdf_rows", "scene_swept")
    ctx.enable_timing(True)
    plain = Scene.mesh(ctx, FIXED, sdf_source=True)
    want = plain.render(P, Rm, cfg, (18, 32)).numpy()
    for scene, suffix, other in ((Scene.mesh(ctx, FIXED, sdf_source=True, movers=[]), "_mesh", "_mesh_mixed"),
                                 (Scene.mesh(ctx, [FIXED, FIXED], sdf_source=True, movers=[[], []]), "_mesh", "_mesh_mixed"),
                                 (Scene.mesh(ctx, FIXED, sdf_source=True, movers=MOVERS[:5]), "_mesh_mixed", "_mesh"),
                                 (Scene.mesh(ctx, FIXED, sdf_source=True, movers=[MOVERS[3]]), "_mesh_mixed", "_mesh")):
        assert scene.is_mesh and not scene.is_indexed and scene.is_dynamic == (suffix == "_mesh_mixed")
        assert scene.is_sdf_source
        ctx.reset_stats()
        img = scene.render(P, Rm, cfg, (18, 32))
        scene.render(P, Rm, cfg, (18, 32), t=0.5)
        scene.distance(np.zeros((4, 3)))
        scene.swept_distance(np.zeros((4, 3)), np.ones((4, 3)))
        _rows(ctx, scene, x, p, 1.0)
        assert [ctx.kernel_stats(k + suffix)[1] for k in names] == [2, 1, 1, 1]
        assert [ctx.kernel_stats(k + other)[1] for k in names] == [0, 0, 0, 0]
        for o in ("", "_dyn", "_grid", "_mixed"):
            assert [ctx.kernel_stats(k + o)[1] for k in names] == [0, 0, 0, 0]
        if suffix == "_mesh":
            np.testing.assert_array_equal(img.numpy(), want)
            assert (scene.speed_bound == 0).all()
        scene.close()
    plain.close()
    ctx.close()


# ---- 8. refusals
def _raw_create(ctx, S, nvert, verts, ntri, tris, opts, mcount, mprims, mmotion=None):
    """sdfnmpc_scene_create_mesh_mixed as C sees it -> (return code, handle value, message)."""
    nv = (C.c_int * max(len(nvert), 1))(*nvert)
    nt = (C.c_int * max(len(ntri), 1))(*ntri)
    va = None if verts is None else np.ascontiguousarray(verts, np.float64)
    ta = None if tris is None else np.ascontiguousarray(tris, np.int32)
    mc = None if mcount is None else (C.c_int * len(mcount))(*mcount)
    h = C.c_void_p()
    rc = _lib.load().sdfnmpc_scene_create_mesh_mixed(
        ctx.h, S, nv, None if va is None else va.ctypes.data_as(C.POINTER(C.c_double)), nt,
        None if ta is None else ta.ctypes.data_as(C.POINTER(C.c_int)), None if opts is None else C.byref(_lib.MeshOptsC(*opts)),
        mc, mprims, mmotion, C.byref(h))
    return rc, h.value, _lib.load().sdfnmpc_last_error().decode()


def test_raw_abi_refusals(gpu_ctx):
    import re
    lib = _lib.load()
    box = Mesh.box((0, 0, 0), (1, 2, 3))
    v, t = box.verts, box.tris
    pr = (_lib.PrimC * 1)()
    pr[0].kind = _lib.PRIM_KINDS["sphere"]
    pr[0].a[:4] = [0.0, 0.0, 5.0, 0.5]
    bad_pr = (_lib.PrimC * 1)()
    bad_pr[0].kind = _lib.PRIM_KINDS["sphere"]
    bad_pr[0].a[:4] = [0.0, 0.0, 5.0, -0.5]
    bad_mo = _lib._motion_c([dict(q=(0.0, 0.0, 0.0, 0.0))], 1)
    nan_mo = _lib._motion_c([dict(v=(np.nan, 0.0, 0.0))], 1)
    flipped = t.copy()
    flipped[3] = flipped[3][::-1]
    nan_v = v.copy()
    nan_v[2, 1] = np.nan
    mesh_ok = (1, [8], v, [12], t, None)
    bad = [
        ("NULL", mesh_ok + (None, pr)),
        ("32 movers", mesh_ok + ([33], pr)),
        ("32 movers", mesh_ok + ([-1], pr)),
        ("primitive", mesh_ok + ([1], bad_pr)),
        ("quaternion", mesh_ok + ([1], pr, bad_mo)),
        ("finite", mesh_ok + ([1], pr, nan_mo)),
        ("NULL movers", mesh_ok + ([1], None)),
        # the mesh refusals of sdfnmpc_scene_create_mesh, with a good mover beside them
        ("S must be", (0, [8], v, [12], t, None, [1], pr)),
        ("negative count", (1, [-1], v, [12], t, None, [1], pr)),
        ("2\\^20 triangles", (1, [8], v, [(1 << 20) + 1], None, None, [1], pr)),
        ("non-finite vertex", (1, [8], nan_v, [12], t, None, [1], pr)),
        ("index outside", (1, [8], v, [12], np.where(t == 7, 8, t), None, [1], pr)),
        ("zero area", (1, [8], v, [1], [[0, 1, 1]], None, [1], pr)),
        ("leaf_size", (1, [8], v, [12], t, (9, 0, 0), [1], pr)),
        ("closed must be", (1, [8], v, [12], t, (0, 2, 0), [1], pr)),
        ("closed.*manifold", (1, [8], v, [12], flipped, (0, 1, 0), [1], pr)),
        ("sdf_source", (1, [8], v, [12], t, (0, 0, 2), [1], pr)),
        ("NULL", (1, [8], None, [12], t, None, [1], pr)),
    ]
    for pattern, args in bad:
        rc, h, msg = _raw_create(gpu_ctx, *args)
        assert rc == -1 and h is None and re.search(pattern, msg), (pattern, rc, h, msg)
    # accepted: a mover and no motion records; no mover at all is the mesh set
    for mcount, dynamic in (([1], 1), ([0], 0)):
        rc, h, msg = _raw_create(gpu_ctx, 1, [8], v, [12], t, (0, 1, 0), mcount, pr)
        assert rc == 0 and h, msg
        assert lib.sdfnmpc_scene_is_mesh(h) == 1 and lib.sdfnmpc_scene_is_dynamic(h) == dynamic and \
            lib.sdfnmpc_scene_is_indexed(h) == 0 and lib.sdfnmpc_scene_is_sdf_source(h) == 0
        lib.sdfnmpc_scene_free(h)


def test_python_refusals(gpu_ctx):
    ok = Scene.sphere((0.0, 0.0, 5.0), 0.5)
    with pytest.raises(ValueError, match="movers"):
        Scene.mesh(gpu_ctx, [FIXED, FIXED], movers=[[ok]])
    with pytest.raises(ValueError, match="movers"):
        Scene.mesh(gpu_ctx, FIXED, movers=[[ok], [ok]])
    with pytest.raises(_lib.SdfnmpcError, match="at most 32 movers"):
        Scene.mesh(gpu_ctx, FIXED, movers=[ok] * 33)
    with pytest.raises(_lib.SdfnmpcError, match="quaternion"):
        Scene.mesh(gpu_ctx, FIXED, movers=[Scene.moving(ok, q=(0.0, 0.0, 0.0, 0.0))])
    crowd = Scene.mesh(gpu_ctx, FIXED, movers=Scene.crowd(4, LO, HI, seed=1))  # a crowd as it is
    assert crowd.is_dynamic and crowd.speed_bound[0] > 0
    crowd.close()
    alone = Scene.mesh(gpu_ctx, EMPTY, movers=[ok])  # movers alone, without a motion record: still the mover path
    assert alone.is_mesh and alone.is_dynamic and alone.distance(np.array([[2.0, 0.0, 5.0]]))[0] == 1.5
    alone.close()


def test_without_sdf_source_the_three_entry_points_refuse(gpu_ctx):
    from test_gpu_rollout import _setup
    from test_gpu_scene_sdf import _problem
    B, N = 3, 10
    sc = Scene.mesh(gpu_ctx, FIXED, closed=True, movers=MOVERS[:5])
    assert sc.is_dynamic and not sc.is_sdf_source
    x, p = _row_inputs(B, N, seed=2)
    d = {k: _lib.DeviceArray.from_numpy(gpu_ctx, v) for k, v in
         dict(x=x, p=p, h=np.full((B, N + 1, 3), -7.0), Jh=np.full((B, N + 1, 10, 3), -7.0)).items()}
    cfg, q, prob, prims, bufs = _problem(gpu_ctx, "default", B, N, seed=13)
    lin = bufs()
    names = ("scene_sdf_rows_mesh_mixed", "scene_sdf_rows_mesh", "scene_sdf_rows", "linearize")
    gpu_ctx.enable_timing(True)
    gpu_ctx.reset_stats()
    try:
        with pytest.raises(_lib.SdfnmpcError, match="error -4.*mesh"):
            _lib.scene_sdf_rows(gpu_ctx, sc.h, B, N, NP, d["x"], d["p"], d["h"], d["Jh"], 1.0)
        with pytest.raises(_lib.SdfnmpcError, match="error -4.*mesh"):
            _lib.linearize(gpu_ctx, None, _lib.quad_model(cfg, q), B, N, q.np, lin, nyN=q.nyN,
                           sdf_scene=_lib.scene_sdf_opts(sc.h, q.max_df))
        gpu_ctx.synchronize()
        assert [gpu_ctx.kernel_stats(k)[1] for k in names] == [0, 0, 0, 0]
        assert (d["h"].numpy() == -7.0).all() and (d["Jh"].numpy() == -7.0).all()
        assert all(np.isnan(lin[k].numpy()).all() for k in ("h", "Jh", "xn", "AB"))
    finally:
        gpu_ctx.enable_timing(False)
    sc.close()
    n, x0 = _setup(Config(mpc__N=10), 2, 21)
    refused = Scene.mesh(n.ocp.ctx, FIXED, movers=MOVERS[:5])
    with pytest.raises(_lib.SdfnmpcError, match="error -4.*mesh"):
        n.set_sdf_scene(refused)
    assert n._sdf_scene is None
    refused.close()
    n.ocp.close()
