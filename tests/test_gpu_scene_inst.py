"""Instanced mesh scenes (Scene.instanced, sdfnmpc_scene_create_instanced, csrc/scene_inst.hip and scene_swept.hip's
EvalInst): a pool of parts stored once, scenes of up to 256 rigid instances whose frames are functions of time.

Against tests/mesh_inst_ref.py: images on decided pixels at the project's IMG_ATOL = 1e-4 m (tests/test_gpu_scene_dyn.py
takes that bar for rotated frames, tests/test_gpu_scene_mesh.py for triangles: the frame is formed in fp64 and rounded
once, so the ray in the part's frame carries the fp32 error of a static mesh's ray), distances and rows at the project's
1e-12 (fp64 on both sides).  Against the library itself, with no tolerance: an identity instance is the mesh scene of its
part, a scene is the minimum of its instances as scenes of their own, and neither the parts' hierarchies nor the order of
the instances changes a bit.

Every test here fails without the feature: there is no Scene.instanced and no sdfnmpc_scene_create_instanced."""
import ctypes as C
import re

import numpy as np
import pytest

import mesh_inst_ref as I
import mesh_ref as MR
import scene_ref as R
from sdf_nmpc_amd import _lib
from sdf_nmpc_amd.config import Config
from sdf_nmpc_amd.mesh import Mesh
from sdf_nmpc_amd.scene import Scene
from test_gpu_scene_mesh import FIXED, IMG_ATOL, _cfg
from test_gpu_scene_mesh_mixed import _row_inputs
from test_gpu_scene_mixed import _rows
from test_gpu_scene_sdf import NP

pytestmark = [pytest.mark.gpu, pytest.mark.filterwarnings("ignore:no SDF weights"),
              pytest.mark.filterwarnings("ignore:QP reached")]

PARTS, INST, REF = I.parts(), I.scene_instances(), I.fixed_instances()
P, RM = R.camera_poses()
B = len(P)
NAMES = ["scene_render_inst", "scene_dist_inst", "scene_sdf_rows_inst", "scene_swept_inst"]
OLD = [k + s for k in ("scene_render", "scene_dist", "scene_sdf_rows", "scene_swept")
       for s in ("", "_dyn", "_grid", "_mixed", "_mesh", "_mesh_mixed")]
MISS = np.float32(5.0) * np.float32(0.2)


def _points():
    return np.random.default_rng(4).uniform([-1, -3, -2.5], [6, 3, 2.5], (700, 3))


def _chords(n, seed):
    rng = np.random.default_rng(seed)
    p0 = rng.uniform((-0.5, -3.0, -1.4), (6.0, 3.0, 2.0), (n, 3))
    e = rng.normal(size=(n, 3))
    p1 = p0 + e / np.linalg.norm(e, axis=1, keepdims=True) * rng.uniform(0.0, 1.0, (n, 1))
    t0 = rng.uniform(0.0, 1.0, n)
    return p0, p1, t0, t0 + rng.uniform(-0.2, 0.2, n)


@pytest.fixture(scope="module")
def fixed(gpu_ctx):
    out = {closed: Scene.instanced(gpu_ctx, PARTS, INST, closed=closed, sdf_source=True) for closed in (True, False)}
    yield out
    for s in out.values():
        s.close()


# ---- 1. render against the reference
@pytest.mark.parametrize("shape", R.SHAPES)
@pytest.mark.parametrize("sensor", ["pinhole", "spherical"])
def test_render_matches_reference_on_decided_pixels(fixed, sensor, shape):
    sc = fixed[True]
    assert sc.is_instanced and sc.is_dynamic and not sc.is_mesh and not sc.is_indexed and sc.is_sdf_source
    s = R.SENSOR if sensor == "pinhole" else R.SPHERICAL
    for t in I.TIMES:
        world = I.merged(PARTS, REF, t)
        for is_depth in (False, True):
            kw = dict(is_depth=is_depth, is_spherical=sensor == "spherical")
            want = MR.values(world, P, RM, *shape, s["hfov"], s["vfov"], s["dmax"], **kw)
            ok = MR.decided(world, P, RM, *shape, s["hfov"], s["vfov"], s["dmax"], **kw)
            assert ok.mean() >= 0.95
            img = sc.render(P, RM, _cfg(sensor, is_depth), shape, t=t).numpy()
            assert img.shape == (B,) + tuple(shape) and img.dtype == np.float32
            gap = np.abs(img.astype(np.float64) * 5.0 - want)
            print(f"\n{sensor} {shape} depth={is_depth} t={t}: worst gap on decided pixels {gap[ok].max():.3e} m, on all "
                  f"pixels {gap.max():.3e} m, decided {ok.mean():.4f}, hits {(want < 5.0).mean():.2f}")
            assert gap[ok].max() <= IMG_ATOL
            assert (img == MISS).any() and (img < 0.9).any()
            np.testing.assert_array_equal(img, fixed[False].render(P, RM, _cfg(sensor, is_depth), shape, t=t).numpy())
    a, b = (sc.render(P, RM, _cfg(sensor), shape, t=t).numpy() for t in I.TIMES)
    assert (a != b).any()  # the scene moves
    np.testing.assert_array_equal(a, sc.render(P, RM, _cfg(sensor), shape).numpy())  # render() is t = 0


# ---- 2. distance against the reference
def test_distance_matches_reference(fixed):
    pts = _points()
    times = np.random.default_rng(5).uniform(0.0, 1.5, len(pts))
    for t, name in ((0.7, "t = 0.7"), (times, "a time per point")):
        want = I.distance(PARTS, REF, pts, t, signed=True)
        if np.ndim(t) == 0:
            assert (want < 0).sum() >= 20 and (want > 0).sum() >= 600
        got = fixed[True].distance(pts, t=t)
        want_open = I.distance(PARTS, REF, pts, t, signed=False)  # not |signed|: inside one of two overlapping solids
        got_open = fixed[False].distance(pts, t=t)
        print(f"\n{name}: max |got - want| closed {np.abs(got - want).max():.3e}, open {np.abs(got_open - want_open).max():.3e}; "
              f"{int((want < 0).sum())} points inside")
        assert np.abs(got - want).max() <= 1e-12
        assert np.abs(got_open - want_open).max() <= 1e-12 and (got_open >= 0).all()
    assert (fixed[True].distance(pts) != fixed[True].distance(pts, t=0.7)).any()
    np.testing.assert_array_equal(fixed[True].distance(pts), fixed[True].distance(pts, t=0.0))


# ---- 3. the identity pin
@pytest.mark.parametrize("closed", [True, False])
def test_identity_instance_is_the_mesh_scene_bit_for_bit(gpu_ctx, closed):
    meshes = [FIXED, Mesh.box((1.0, -1.0, -0.5), (2.0, 0.5, 0.75))]
    so = np.arange(B) % 2
    inst = Scene.instanced(gpu_ctx, meshes, [[Scene.instance(0, (0, 0, 0))], [Scene.instance(1, (0, 0, 0))]], scene_of=so,
                           closed=closed, sdf_source=True)
    mesh = Scene.mesh(gpu_ctx, meshes, scene_of=so, closed=closed, sdf_source=True)
    assert inst.is_instanced and not inst.is_dynamic and not inst.is_mesh and (inst.speed_bound == 0).all()
    for sensor in ("pinhole", "spherical"):
        for is_depth in (False, True):
            for shape in R.SHAPES:
                cfg = _cfg(sensor, is_depth)
                want = mesh.render(P, RM, cfg, shape).numpy()
                for t in (0.0, 1.3):  # nothing moves: any time
                    np.testing.assert_array_equal(inst.render(P, RM, cfg, shape, t=t).numpy().view(np.uint32),
                                                  want.view(np.uint32))
                assert (want < 1.0).any()
    pts = np.concatenate([MR.rounded(FIXED).verts[::7], _points()])  # the first half belongs to scene 0, the fixed scene
    pts = pts[:len(pts) // 2 * 2]
    want = mesh.distance(pts)
    np.testing.assert_array_equal(inst.distance(pts), want)
    np.testing.assert_array_equal(inst.distance(pts, t=0.9), want)
    assert (want == 0).any() and ((want < 0).any() == closed)
    p0, p1, t0, t1 = _chords(64, 3)
    a, b = inst.swept_distance(p0, p1, t0=t0, t1=t1, max_evals=512), mesh.swept_distance(p0, p1, max_evals=512)
    for k in ("dmin", "s", "gap", "evals"):
        np.testing.assert_array_equal(getattr(a, k), getattr(b, k), err_msg=k)
    x, p = _row_inputs(B, 10, seed=31)
    for max_df in (0.2, 3.0):
        h, J = _rows(gpu_ctx, inst, x, p, max_df, t0=0.4, tau=0.1 * np.arange(11))
        wh, wJ = _rows(gpu_ctx, mesh, x, p, max_df)
        np.testing.assert_array_equal(h, wh)
        np.testing.assert_array_equal(J, wJ)
    assert (wh < 3.0).any() and np.abs(wJ).max() > 0.5
    inst.close()
    mesh.close()


# ---- 4. a scene is the minimum of its instances
@pytest.mark.parametrize("closed", [True, False])
def test_scene_is_the_composition_of_its_instances(gpu_ctx, fixed, closed):
    n = len(INST)
    singles = Scene.instanced(gpu_ctx, PARTS, [[i] for i in INST], scene_of=np.repeat(np.arange(n), B), closed=closed,
                              sdf_source=True)
    sc = fixed[closed]
    for sensor, is_depth, shape in (("pinhole", True, R.SHAPES[0]), ("spherical", False, R.SHAPES[1])):
        cfg = _cfg(sensor, is_depth)
        for t in I.TIMES:
            each = singles.render(np.tile(P, (n, 1)), np.tile(RM, (n, 1, 1)), cfg, shape, t=t).numpy().reshape(n, B, *shape)
            np.testing.assert_array_equal(sc.render(P, RM, cfg, shape, t=t).numpy().view(np.uint32),
                                          each.min(0).view(np.uint32))
            assert sum(bool((each[k] == each.min(0))[each.min(0) < MISS].any()) for k in range(n)) >= 3
    pts = _points()[:300]
    times = np.random.default_rng(6).uniform(0.0, 1.5, len(pts))
    each = singles.distance(np.tile(pts, (n, 1)), t=np.tile(times, n)).reshape(n, -1)
    np.testing.assert_array_equal(sc.distance(pts, t=times), each.min(0))
    assert len(set(each.argmin(0))) >= 6
    x, p = _row_inputs(B, 10, seed=32)
    tau = 0.15 * np.arange(11)
    for max_df in (0.3, 3.0):
        eh, eJ = _rows(gpu_ctx, singles, np.tile(x, (n, 1, 1)), np.tile(p, (n, 1, 1)), max_df, t0=0.2, tau=tau)
        eh, eJ = eh.reshape(n, B, 11), eJ.reshape(n, B, 11, 10)
        wh, wJ = eh[0].copy(), eJ[0].copy()
        for k in range(1, n):  # strictly smaller: the lowest index keeps a tie
            lower = eh[k] < wh
            wh, wJ = np.where(lower, eh[k], wh), np.where(lower[..., None], eJ[k], wJ)
        h, J = _rows(gpu_ctx, sc, x, p, max_df, t0=0.2, tau=tau)
        np.testing.assert_array_equal(h, wh)
        np.testing.assert_array_equal(J, wJ)
    assert (wh < 3.0).sum() >= 10
    singles.close()


# ---- 5. neither the hierarchies nor the order of the instances changes a bit
@pytest.mark.parametrize("closed", [True, False])
def test_hierarchy_and_order_change_no_bit(gpu_ctx, closed):
    pts = _points()[:300]
    times = np.random.default_rng(7).uniform(0.0, 1.5, len(pts))
    p0, p1, t0, t1 = _chords(48, 8)
    x, p = _row_inputs(B, 10, seed=33)
    cfgs = [(_cfg("pinhole", True), R.SHAPES[1]), (_cfg("spherical", False), R.SHAPES[0])]

    def run(leaf, order):
        sc = Scene.instanced(gpu_ctx, PARTS, [INST[k] for k in order], closed=closed, leaf_size=leaf, sdf_source=True)
        out = ([sc.render(P, RM, cfg, shape, t=0.7).numpy() for cfg, shape in cfgs], sc.distance(pts, t=times),
               sc.swept_distance(p0, p1, t0=t0, t1=t1, max_evals=256),
               [_rows(gpu_ctx, sc, x, p, max_df, t0=0.2, tau=0.15 * np.arange(11)) for max_df in (0.3, 3.0)])
        sc.close()
        return out

    ident = list(range(len(INST)))
    bi, bd, bs, br = run(-1, ident)
    assert np.isfinite(bd).all() and all((im < 1.0).any() for im in bi)
    for leaf, order in [(1, ident), (4, ident), (8, ident), (None, list(np.random.default_rng(9).permutation(len(INST)))),
                        (-1, ident[::-1])]:
        imgs, d, s, rows = run(leaf, order)
        what = f"leaf {leaf}, order {order}"
        for a, b in zip(imgs, bi):
            np.testing.assert_array_equal(a.view(np.uint32), b.view(np.uint32), err_msg="render, " + what)
        np.testing.assert_array_equal(d, bd, err_msg="distance, " + what)
        np.testing.assert_array_equal(s.dmin, bs.dmin, err_msg="swept dmin, " + what)
        for (h, J), (wh, wJ) in zip(rows, br):
            np.testing.assert_array_equal(h, wh, err_msg="rows h, " + what)
        if order == ident:  # the hierarchy alone: every output of every query
            for k in ("s", "gap", "evals"):
                np.testing.assert_array_equal(getattr(s, k), getattr(bs, k), err_msg=f"swept {k}, " + what)
            for (h, J), (wh, wJ) in zip(rows, br):
                np.testing.assert_array_equal(J, wJ, err_msg="rows J, " + what)


# ---- 6. one part in two scenes, and a scene without instances
def test_shared_part_scene_of_and_the_empty_scene(gpu_ctx):
    a = [Scene.instance(1, (2.5, 0.5, 0.25), v=(0.25, 0.5, 0.0)), Scene.instance(0, (3.5, -1.0, 0.0), rpy=(0.1, 0.2, 0.3))]
    b = [Scene.instance(1, (3.0, -0.5, -0.25), rpy=(0.3, 0.0, 0.2), yaw_rate=0.7), Scene.instance(1, (4.0, 1.0, 0.5))]
    so = np.array([2, 1, 0, 2, 0, 1])
    P6, R6 = np.tile(P, (2, 1)), np.tile(RM, (2, 1, 1))
    both = Scene.instanced(gpu_ctx, PARTS, [a, [], b], scene_of=so, closed=True)
    own = {0: Scene.instanced(gpu_ctx, PARTS, a, closed=True), 2: Scene.instanced(gpu_ctx, PARTS, b, closed=True)}
    cfg = _cfg("pinhole", False)
    img = both.render(P6, R6, cfg, R.SHAPES[1], t=0.7).numpy()
    for k, s in enumerate(so):
        if s == 1:
            assert (img[k] == MISS).all()
        else:
            np.testing.assert_array_equal(img[k], own[s].render(P6[k:k + 1], R6[k:k + 1], cfg, R.SHAPES[1], t=0.7).numpy()[0])
            assert (img[k] < MISS).any()
    pts = _points()[:240]
    p2s = np.random.default_rng(10).integers(0, 3, len(pts)).astype(np.int32)
    d = both.distance(pts, p_to_scene=p2s, t=0.7)
    assert np.isposinf(d[p2s == 1]).all()
    for s in (0, 2):
        np.testing.assert_array_equal(d[p2s == s], own[s].distance(pts[p2s == s], t=0.7))
    d3 = both.distance(pts)  # the default ordering: point j -> scene j // (n / S)
    np.testing.assert_array_equal(d3[:80], own[0].distance(pts[:80]))
    assert np.isposinf(d3[80:160]).all()
    sw = both.swept_distance(pts[:6], pts[6:12], p_to_scene=np.ones(6, np.int32), t0=0.0, t1=0.5)
    assert np.isposinf(sw.dmin).all() and (sw.gap == 0).all()
    np.testing.assert_array_equal(both.speed_bound[1], 0.0)
    empty = Scene.instanced(gpu_ctx, PARTS, [])
    assert empty.S == 1 and not empty.is_dynamic and np.isposinf(empty.distance(pts[:4])).all()
    assert (empty.render(P, RM, cfg, R.SHAPES[1]).numpy() == MISS).all()
    for s in (both, empty, *own.values()):
        s.close()


# ---- 7. the rows contract
@pytest.mark.parametrize("closed", [True, False])
def test_rows_contract_against_the_reference(gpu_ctx, fixed, closed):
    sc = fixed[closed]
    Bn, N = 8, 10
    x, p = _row_inputs(Bn, N, seed=34)
    t0, tau = 0.2, 0.15 * np.arange(N + 1)
    pts = x[..., :3].reshape(-1, 3)
    tk = np.tile(t0 + tau, Bn)
    d, g, which = I.dist_grad(PARTS, REF, pts, tk, signed=closed)
    p[..., 0] = 0.3  # a fractional flag on every row
    for max_df in (0.25, 3.0):
        near = d < max_df
        want_h = (0.3 * np.where(near, d, max_df) + 0.7 * max_df).reshape(Bn, N + 1)
        want_J = np.zeros((Bn, N + 1, 10))
        want_J[..., :3] = (0.3 * np.where(near[:, None], g, 0.0)).reshape(Bn, N + 1, 3)
        h, J = _rows(gpu_ctx, sc, x, p, max_df, t0=t0, tau=tau)  # asserts that columns 0 and 1 stay untouched
        eh, eJ = np.abs(h - want_h).max(), np.abs(J - want_J).max()
        print(f"\nclosed={closed} max_df={max_df}: max error h {eh:.2e}, J_h {eJ:.2e}; {int(near.sum())} of {near.size} rows near, "
              f"from {len(set(which[near]))} instances")
        assert eh <= 1e-12 and eJ <= 1e-12
        assert not J[..., 3:].any()
        far = ~near.reshape(Bn, N + 1)
        assert (h[far] == max_df).all() and not J[far].any() and near.any()
        assert far.any() or max_df == 3.0  # the floor is within 3 m of every row
    p[..., 0] = 1.0
    p[:, 2::3, 0] = 0.0
    h, J = _rows(gpu_ctx, sc, x, p, 3.0, t0=t0, tau=tau)
    on = (p[..., 0] == 1.0) & (h < 3.0)
    assert np.abs(np.linalg.norm(J[on][:, :3], axis=1) - 1.0).max() <= 1e-12  # a unit vector
    assert (h[p[..., 0] == 0.0] == 3.0).all() and not J[p[..., 0] == 0.0].any()
    # predict: node k at t0 + tau[k], the bits of distance(t=)
    dist = sc.distance(pts, t=tk).reshape(Bn, N + 1)
    np.testing.assert_array_equal(h[on], dist[on])
    h0, _ = _rows(gpu_ctx, sc, x, p, 3.0, t0=t0)  # without tau: every node at t0
    np.testing.assert_array_equal(h0[on & (h0 < 3.0)], sc.distance(pts, t=t0).reshape(Bn, N + 1)[on & (h0 < 3.0)])
    assert (h0 != h).any()


# ---- 8. swept clearance
M_DENSE, EPS, N_SEG = 32, 1e-3, 100


@pytest.mark.parametrize("closed", [True, False])
def test_swept_certificate_against_dense_sampling(fixed, closed):
    sc = fixed[closed]
    p0, p1, t0, t1 = _chords(N_SEG, 17)
    s = np.arange(M_DENSE + 1) / M_DENSE
    q = (p0[:, None] + s[None, :, None] * (p1 - p0)[:, None]).reshape(-1, 3)
    tq = (t0[:, None] + s[None] * (t1 - t0)[:, None]).ravel()
    dn = I.distance(PARTS, REF, q, tq, signed=closed).reshape(N_SEG, -1).min(1)
    V = I.speed_bound(PARTS, REF)
    assert abs(sc.speed_bound[0] - V * (1.0 + 1e-12)) <= 1e-14 * V and V > 1.0  # the formula, inflated
    r = sc.swept_distance(p0, p1, t0=t0, t1=t1, eps=EPS)
    L = np.linalg.norm(p1 - p0, axis=1) + V * np.abs(t1 - t0)
    lo, hi = r.dmin - (dn - L / (2 * M_DENSE)), (r.dmin - r.gap) - dn
    print(f"\nclosed={closed}: dmin - (dense - L / 2M) >= {lo.min():.2e}, (dmin - gap) - dense <= {hi.max():.2e}, gap <= "
          f"{r.gap.max():.2e}, evals median {int(np.median(r.evals))} max {r.evals.max()}")
    assert (lo >= -1e-9).all()
    assert (hi <= 1e-9).all()
    assert (r.evals <= 4096).all() and (r.evals >= 1).all() and (r.gap >= 0.0).all()
    assert (r.gap[r.evals < 4096] <= EPS + 1e-12).all()
    at = sc.distance(p0 + r.s[:, None] * (p1 - p0), t=t0 + r.s * (t1 - t0))
    assert np.abs(at - r.dmin).max() <= 1e-9  # the value of distance at (p(s), t(s))


def test_swept_sees_a_thin_quad_cross_a_chord(gpu_ctx):
    """An open unit quad in its own z = 0 plane rises at 8 m/s through the chord (1, 0, 0) -> (1.5, 0, 0): it is 0.8 m
    below the chord's start at t = 0.2, 0.8 m above its end at t = 0.4 and in the chord's plane at t = 0.3."""
    quad = Mesh([(-0.5, -0.5, 0.0), (0.5, -0.5, 0.0), (0.5, 0.5, 0.0), (-0.5, 0.5, 0.0)], [(0, 1, 2), (0, 2, 3)])
    sc = Scene.instanced(gpu_ctx, quad, [Scene.instance(0, (1.25, 0.0, -2.4), v=(0.0, 0.0, 8.0))])
    p0, p1 = np.array([[1.0, 0.0, 0.0]]), np.array([[1.5, 0.0, 0.0]])
    rows = (sc.distance(p0, t=0.2)[0], sc.distance(p1, t=0.4)[0])
    assert abs(rows[0] - 0.8) <= 1e-12 and abs(rows[1] - 0.8) <= 1e-12  # what Rollout.clearance would log
    np.testing.assert_array_equal(sc.speed_bound, [8.0 * (1.0 + 1e-12)])
    r = sc.swept_distance(p0, p1, t0=0.2, t1=0.4)
    print(f"\ncrossing quad: dmin {r.dmin[0]:.2e} at s = {r.s[0]:.4f}, gap {r.gap[0]:.1e}, {r.evals[0]} evals")
    assert 0.0 <= r.dmin[0] <= r.gap[0] + 1e-9 and r.gap[0] <= 1e-3 and abs(r.s[0] - 0.5) < 1e-2
    assert sc.swept_distance(p0, p1).dmin[0] > 2.0  # without times nothing moves
    sc.close()


# ---- 9. capacity: 256 instances
def test_256_instances_against_the_welded_mesh(gpu_ctx):
    """256 boxes of edge 0.25 from Scene.scatter.  Against the welded mesh the positions are snapped to multiples of
    2^-8 and the boxes are not yawed, so that the welded vertices p + v are exact in fp32 and both scenes hold the same
    triangles: the images within IMG_ATOL on decided pixels, the distance within 1e-12.  With the yaw, the distance
    against the reference at the same bar."""
    part = Mesh.box((-0.125, -0.125, -0.125), (0.125, 0.125, 0.125))
    lo, hi = (0.5, -3.0, -1.5), (6.0, 3.0, 1.5)
    raw = Scene.scatter(256, lo, hi, parts=1, seed=3, keep_clear=((0.0, 0.0), 1.0), yaw=False)
    snapped = [Scene.instance(0, np.round(np.array(i[2]) * 256.0) / 256.0) for i in raw]
    sc = Scene.instanced(gpu_ctx, part, snapped)
    welded_mesh = Mesh.merge(*[part.transformed(t=i[2]) for i in snapped])
    assert (welded_mesh.verts == welded_mesh.verts.astype(np.float32)).all()
    welded = Scene.mesh(gpu_ctx, welded_mesh)
    pts = np.random.default_rng(11).uniform(lo, hi, (500, 3))
    got, want = sc.distance(pts), welded.distance(pts)
    print(f"\n256 instances: distance, max |instanced - welded| {np.abs(got - want).max():.2e}")
    assert np.abs(got - want).max() <= 1e-12 and (want < 0.2).any()
    s = R.SENSOR
    shape = R.SHAPES[1]
    ok = MR.decided(welded_mesh, P, RM, *shape, s["hfov"], s["vfov"], s["dmax"])
    a, b = sc.render(P, RM, _cfg(), shape).numpy(), welded.render(P, RM, _cfg(), shape).numpy()
    gap = np.abs(a.astype(np.float64) - b) * 5.0
    print(f"256 instances: worst image gap on decided pixels {gap[ok].max():.2e} m, hits {(b < MISS).mean():.2f}")
    assert gap[ok].max() <= IMG_ATOL and (b < MISS).mean() > 0.2 and ok.mean() > 0.3
    sc.close()
    welded.close()
    yawed = Scene.scatter(256, lo, hi, parts=1, seed=3, keep_clear=((0.0, 0.0), 1.0))
    sc = Scene.instanced(gpu_ctx, part, yawed, closed=True)
    ref = [I.instance(0, i[2], q=i[3]["q"]) for i in yawed]
    want = I.distance([part], ref, pts[:120], 0.0, signed=True)
    got = sc.distance(pts[:120])
    print(f"256 yawed instances: max |got - reference| {np.abs(got - want).max():.2e}")
    assert np.abs(got - want).max() <= 1e-12
    sc.close()


# ---- 10. refusals, predicates, kernel names
def _raw_create(ctx, nparts, nvert, verts, ntri, tris, opts, S, icount, inst):
    """sdfnmpc_scene_create_instanced as C sees it -> (return code, handle value, message); inst: a list of
    (part, p, motion dict or None), or None for a NULL pointer."""
    nv = (C.c_int * max(len(nvert), 1))(*nvert)
    nt = (C.c_int * max(len(ntri), 1))(*ntri)
    va = None if verts is None else np.ascontiguousarray(verts, np.float64)
    ta = None if tris is None else np.ascontiguousarray(tris, np.int32)
    ic = None if icount is None else (C.c_int * max(len(icount), 1))(*icount)
    ins = None
    if inst is not None:
        ins = (_lib.MeshInstanceC * max(len(inst), 1))()
        mo = _lib._motion_c([m for _, _, m in inst], len(inst))
        for k, (part, pos, _) in enumerate(inst):
            ins[k].part = part
            ins[k].p[:] = pos
            ins[k].motion = mo[k]
    h = C.c_void_p()
    rc = _lib.load().sdfnmpc_scene_create_instanced(
        ctx.h, nparts, nv, None if va is None else va.ctypes.data_as(C.POINTER(C.c_double)), nt,
        None if ta is None else ta.ctypes.data_as(C.POINTER(C.c_int)), None if opts is None else C.byref(_lib.MeshOptsC(*opts)),
        S, ic, ins, C.byref(h))
    return rc, h.value, _lib.load().sdfnmpc_last_error().decode()


def test_raw_abi_refusals_and_predicates(gpu_ctx):
    lib = _lib.load()
    box = Mesh.box((0, 0, 0), (1, 2, 3))
    v, t = box.verts, box.tris
    z = (0.0, 0.0, 0.0)
    one = [(0, z, None)]
    flipped = t.copy()
    flipped[3] = flipped[3][::-1]
    nan_v = v.copy()
    nan_v[2, 1] = np.nan
    part_ok = (1, [8], v, [12], t, None)
    bad = [
        ("part index", part_ok + (1, [1], [(1, z, None)])),
        ("part index", part_ok + (1, [1], [(-1, z, None)])),
        ("256 instances", part_ok + (1, [257], one * 257)),
        ("256 instances", part_ok + (1, [-1], one)),
        ("quaternion", part_ok + (1, [1], [(0, z, dict(q=(0.0, 0.0, 0.0, 0.0)))])),
        ("finite", part_ok + (1, [1], [(0, z, dict(v=(np.nan, 0.0, 0.0)))])),
        ("finite", part_ok + (1, [1], [(0, z, dict(omega=np.inf))])),
        ("finite position", part_ok + (1, [1], [(0, (0.0, np.inf, 0.0), None)])),
        ("NULL instances", part_ok + (1, [1], None)),
        ("NULL", part_ok + (1, None, one)),
        ("S must be", part_ok + (0, [1], one)),
        ("nparts must be", (0, [8], v, [12], t, None, 1, [0], one)),
        # what sdfnmpc_scene_create_mesh refuses of a part
        ("negative count", (1, [-1], v, [12], t, None, 1, [1], one)),
        ("2\\^20 triangles", (1, [8], v, [(1 << 20) + 1], None, None, 1, [1], one)),
        ("non-finite vertex", (1, [8], nan_v, [12], t, None, 1, [1], one)),
        ("index outside", (1, [8], v, [12], np.where(t == 7, 8, t), None, 1, [1], one)),
        ("zero area", (1, [8], v, [1], [[0, 1, 1]], None, 1, [1], one)),
        ("leaf_size", (1, [8], v, [12], t, (9, 0, 0), 1, [1], one)),
        ("closed must be", (1, [8], v, [12], t, (0, 2, 0), 1, [1], one)),
        ("closed.*manifold", (1, [8], v, [12], flipped, (0, 1, 0), 1, [1], one)),
        ("closed.*manifold", (1, [8], v, [11], t[1:], (0, 1, 0), 1, [1], one)),
        ("sdf_source", (1, [8], v, [12], t, (0, 0, 2), 1, [1], one)),
        ("NULL", (1, [8], None, [12], t, None, 1, [1], one)),
    ]
    for pattern, args in bad:
        rc, h, msg = _raw_create(gpu_ctx, *args)
        assert rc == -1 and h is None and re.search(pattern, msg), (pattern, rc, h, msg)
    moves = dict(yaw_rate=0.1)
    for inst, dynamic, src in ((one, 0, 0), ([(0, z, dict(q=(0.5, 0.5, 0.5, 0.5)))], 0, 1), ([(0, z, moves)], 1, 0),
                               ([(0, z, dict(amp=(0.0, 0.1, 0.0)))], 1, 1), ([(0, z, dict(v=(0.0, 0.0, 1.0)))], 1, 0),
                               ([(0, z, dict(omega=2.0, phase=1.0))], 0, 0)):  # omega without amp moves nothing
        rc, h, msg = _raw_create(gpu_ctx, 1, [8], v, [12], t, (0, 1, src), 1, [1], inst)
        assert rc == 0 and h, msg
        assert lib.sdfnmpc_scene_is_instanced(h) == 1 and lib.sdfnmpc_scene_is_mesh(h) == 0 and \
            lib.sdfnmpc_scene_is_indexed(h) == 0 and lib.sdfnmpc_scene_is_dynamic(h) == dynamic and \
            lib.sdfnmpc_scene_is_sdf_source(h) == src
        lib.sdfnmpc_scene_free(h)
    rc, h, msg = _raw_create(gpu_ctx, 1, [8], v, [12], t, None, 2, [0, 0], None)  # no instance anywhere: no list needed
    assert rc == 0 and h and lib.sdfnmpc_scene_is_dynamic(h) == 0, msg
    lib.sdfnmpc_scene_free(h)
    assert lib.sdfnmpc_scene_is_instanced(None) == 0


def test_python_refusals(gpu_ctx):
    box = Mesh.box((0, 0, 0), (1, 2, 3))
    ok = Scene.instance(0, (0, 0, 0))
    with pytest.raises(_lib.SdfnmpcError, match="part index"):
        Scene.instanced(gpu_ctx, box, [Scene.instance(1, (0, 0, 0))])
    with pytest.raises(_lib.SdfnmpcError, match="256 instances"):
        Scene.instanced(gpu_ctx, box, [ok] * 257)
    with pytest.raises(_lib.SdfnmpcError, match="quaternion"):
        Scene.instanced(gpu_ctx, box, [Scene.instance(0, (0, 0, 0), q=(0.0, 0.0, 0.0, 0.0))])
    with pytest.raises(_lib.SdfnmpcError, match="finite"):
        Scene.instanced(gpu_ctx, box, [Scene.instance(0, (0, np.nan, 0))])
    with pytest.raises(_lib.SdfnmpcError, match="closed.*manifold"):
        Scene.instanced(gpu_ctx, [box, Mesh(box.verts, box.tris[1:])], [ok], closed=True)
    with pytest.raises(ValueError, match="not both"):
        Scene.instance(0, (0, 0, 0), q=(1.0, 0.0, 0.0, 0.0), rpy=(0.0, 0.0, 0.0))
    with pytest.raises(ValueError, match="Scene.instance"):
        Scene.instanced(gpu_ctx, box, [[ok], [Scene.sphere((0, 0, 0), 1.0)]])
    with pytest.raises(ValueError, match="scene_of"):
        Scene.instanced(gpu_ctx, box, [ok], scene_of=[0, 1])
    sc = Scene.instanced(gpu_ctx, box, [ok] * 256)
    with pytest.raises(ValueError, match="scene_of"):
        Scene.instanced(gpu_ctx, box, [[ok], [ok]], scene_of=[0, 1]).render(P, RM, _cfg(), (18, 32))
    out = _lib.DeviceArray.from_numpy(gpu_ctx, np.full((B, 18, 32), -7.0, np.float32))
    with pytest.raises(_lib.SdfnmpcError, match="finite"):
        sc.render(P, RM, _cfg(), (18, 32), out=out, t=np.inf)
    with pytest.raises(_lib.SdfnmpcError, match="instanced set"):  # 16 KB of frames beside the spherical tables
        sc.render(P[:1], RM[:1], _cfg("spherical"), (1, 4200), out=_lib.DeviceArray(gpu_ctx, (1, 1, 4200), np.float32))
    gpu_ctx.synchronize()
    assert (out.numpy() == -7.0).all()
    sc.close()


def test_without_sdf_source_the_three_entry_points_refuse(gpu_ctx):
    from test_gpu_rollout import _setup
    from test_gpu_scene_sdf import _problem
    Bn, N = 3, 10
    sc = Scene.instanced(gpu_ctx, PARTS, INST, closed=True)
    assert sc.is_dynamic and sc.is_instanced and not sc.is_sdf_source
    x, p = _row_inputs(Bn, N, seed=2)
    d = {k: _lib.DeviceArray.from_numpy(gpu_ctx, v) for k, v in
         dict(x=x, p=p, h=np.full((Bn, N + 1, 3), -7.0), Jh=np.full((Bn, N + 1, 10, 3), -7.0)).items()}
    cfg, q, prob, prims, bufs = _problem(gpu_ctx, "default", Bn, N, seed=13)
    lin = bufs()
    gpu_ctx.enable_timing(True)
    gpu_ctx.reset_stats()
    try:
        with pytest.raises(_lib.SdfnmpcError, match="error -4.*instanced"):
            _lib.scene_sdf_rows(gpu_ctx, sc.h, Bn, N, NP, d["x"], d["p"], d["h"], d["Jh"], 1.0)
        with pytest.raises(_lib.SdfnmpcError, match="error -4.*instanced"):
            _lib.linearize(gpu_ctx, None, _lib.quad_model(cfg, q), Bn, N, q.np, lin, nyN=q.nyN,
                           sdf_scene=_lib.scene_sdf_opts(sc.h, q.max_df))
        gpu_ctx.synchronize()
        assert [gpu_ctx.kernel_stats(k)[1] for k in ("scene_sdf_rows_inst", "scene_sdf_rows_mesh", "scene_sdf_rows", "linearize")] \
            == [0, 0, 0, 0]
        assert (d["h"].numpy() == -7.0).all() and (d["Jh"].numpy() == -7.0).all()
        assert all(np.isnan(lin[k].numpy()).all() for k in ("h", "Jh", "xn", "AB"))
    finally:
        gpu_ctx.enable_timing(False)
    sc.close()
    n, x0 = _setup(Config(mpc__N=10), 2, 21)
    refused = Scene.instanced(n.ocp.ctx, PARTS, INST)
    with pytest.raises(_lib.SdfnmpcError, match="error -4.*instanced"):
        n.set_sdf_scene(refused)
    assert n._sdf_scene is None
    accepted = Scene.instanced(n.ocp.ctx, PARTS, INST, sdf_source=True)
    n.set_sdf_scene(accepted, predict=True)
    n.set_sdf_scene(None)
    for s in (refused, accepted):
        s.close()
    n.ocp.close()


def test_kernel_stats_land_on_the_new_names():
    ctx = _lib.Context(0)  # its own context: the timing switch and the statistics are per context
    x, p = _row_inputs(3, 10, seed=2)
    ctx.enable_timing(True)
    for inst in (INST, INST[:1], []):  # moving, standing still, empty: one set of kernels
        sc = Scene.instanced(ctx, PARTS, inst, sdf_source=True)
        ctx.reset_stats()
        sc.render(P, RM, _cfg(), (18, 32))
        sc.render(P, RM, _cfg(), (18, 32), t=0.5)
        sc.distance(np.zeros((4, 3)))
        sc.distance(np.zeros((4, 3)), t=0.5)
        sc.swept_distance(np.zeros((4, 3)), np.ones((4, 3)), t0=0.0, t1=0.5)
        _rows(ctx, sc, x, p, 1.0)
        assert [ctx.kernel_stats(k)[1] for k in NAMES] == [2, 2, 1, 1]
        assert [ctx.kernel_stats(k)[1] for k in OLD] == [0] * len(OLD)
        sc.close()
    ctx.close()
