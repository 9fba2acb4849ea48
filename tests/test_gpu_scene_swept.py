"""Swept clearance on the device (Scene.swept_distance, sdfnmpc_scene_swept_distance, csrc/scene_swept.hip): the
minimum of the scene's distance over segments of space-time with its certificate, for the four kinds of scene set,
against dense sampling of tests/swept_ref.py (M = 4096 samples per segment), closed forms, and the API contract.

The two certificates bracket the same true minimum m of D over the segment:
    dense - L / (2 M) <= m <= dense      (D is L-Lipschitz in s and a sample lies within 1 / (2 M) of every s)
    dmin - gap        <= m <= dmin       (the kernel's certificate)
hence dense - L / (2 M) <= dmin and dmin - gap <= dense; the 1e-9 m added to either side is five orders above fp64
rounding at these coordinates and six below eps."""
import numpy as np
import pytest

import scene_dyn_ref as D
import scene_ref as R
import swept_ref as W
from sdf_nmpc_amd import _lib
from sdf_nmpc_amd.scene import Scene

pytestmark = pytest.mark.gpu

M, EPS, N_SEG = 4096, 1e-3, 300
FOREST_LO, FOREST_HI = (-8.0, -8.0, -1.0), (8.0, 8.0, 2.0)
MOVERS = [(("sphere", [0.0, -6.0, 0.5, 0.4]), dict(v=(0.5, 2.0, 0.0))),
          (("box", [-3.0, -0.3, -1.0, -1.0, 0.3, 1.5]), dict(yaw_rate=1.5, rpy=(0.0, 0.0, 0.4))),
          (("cylinder", [4.0, 3.0, 0.3, -1.0, 0.8]), dict(amp=(2.0, -1.0, 0.0), omega=1.2, phase=0.5))]


def _gpu_prims(spec):
    return [Scene.moving(p, **kw) if kw is not None else p for p, kw in spec]


def _sets(ctx):
    """name -> (Scene, the reference's primitives, the box segments start in)"""
    plain = R.SCENE + [("sphere", [1.0, 1.5, 0.5, 0.3])]
    forest = Scene.forest(200, FOREST_LO, FOREST_HI, seed=4)
    few = Scene.forest(50, FOREST_LO, FOREST_HI, seed=5)
    return {"plain": (Scene(ctx, plain), plain, (np.array([-0.5, -3.0, -1.4]), np.array([6.0, 3.0, 2.0]))),
            "dynamic": (Scene(ctx, _gpu_prims(D.SPEC)), D.scene(), (np.array([-0.5, -3.0, -1.4]), np.array([6.0, 3.0, 2.0]))),
            "grid": (Scene(ctx, forest, grid=True), forest, (np.array(FOREST_LO), np.array(FOREST_HI))),
            "mixed": (Scene(ctx, few, grid=True, movers=_gpu_prims(MOVERS)), few + D.scene(MOVERS),
                      (np.array(FOREST_LO), np.array(FOREST_HI)))}


def _segments(rng, n, lo, hi):
    """n segments: |p1 - p0| <= 1 m, |t1 - t0| <= 0.2 s, t0 in [0, 2]"""
    p0 = rng.uniform(lo, hi, (n, 3))
    e = rng.normal(size=(n, 3))
    p1 = p0 + e / np.linalg.norm(e, axis=1, keepdims=True) * rng.uniform(0.0, 1.0, (n, 1))
    t0 = rng.uniform(0.0, 2.0, n)
    return p0, p1, t0, t0 + rng.uniform(-0.2, 0.2, n)


def _lipschitz(V, p0, p1, t0, t1):
    return np.linalg.norm(p1 - p0, axis=1) + V * np.abs(t1 - t0)


def _check_certificate(r, prims, p0, p1, t0, t1, max_evals, label):
    dn, _ = W.dense(prims, p0, p1, t0, t1, M)
    L = _lipschitz(W.speed_bound(prims), p0, p1, t0, t1)
    lo, hi = r.dmin - (dn - L / (2 * M)), (r.dmin - r.gap) - dn
    print(f"\n{label}: dmin - (dense - L / 2M) >= {lo.min():.2e}, (dmin - gap) - dense <= {hi.max():.2e}, gap <= "
          f"{r.gap.max():.2e}, evals median {int(np.median(r.evals))} max {r.evals.max()}, dmin in [{r.dmin.min():.3f}, "
          f"{r.dmin.max():.3f}]")
    assert (lo >= -1e-9).all()
    assert (hi <= 1e-9).all()
    assert (r.evals <= max_evals).all() and (r.evals >= 1).all()
    assert (r.gap >= 0.0).all()
    return dn


@pytest.fixture(scope="module")
def sets(gpu_ctx):
    s = _sets(gpu_ctx)
    yield s
    for scene, _, _ in s.values():
        scene.close()


@pytest.mark.parametrize("kind", ["plain", "dynamic", "grid", "mixed"])
def test_certificate_against_dense_sampling(sets, gpu_ctx, kind):
    scene, prims, (lo, hi) = sets[kind]
    assert (scene.is_indexed, scene.is_dynamic) == (kind in ("grid", "mixed"), kind in ("dynamic", "mixed"))
    p0, p1, t0, t1 = _segments(np.random.default_rng(17), N_SEG, lo, hi)
    gpu_ctx.enable_timing(True)
    gpu_ctx.reset_stats()
    r = scene.swept_distance(p0, p1, t0=t0, t1=t1, eps=EPS)
    names = {"plain": "scene_swept", "dynamic": "scene_swept_dyn", "grid": "scene_swept_grid", "mixed": "scene_swept_mixed"}
    launches = {k: gpu_ctx.kernel_stats(v)[1] for k, v in names.items()}
    gpu_ctx.enable_timing(False)
    assert launches == {k: int(k == kind) for k in names}  # dispatched on the handle as scene_distance_at is
    assert r.dmin.shape == r.s.shape == r.gap.shape == r.evals.shape == (N_SEG,) and r.evals.dtype == np.int32
    _check_certificate(r, prims, p0, p1, t0, t1, 4096, kind)
    assert (r.gap[r.evals < 4096] <= EPS + 1e-12).all()
    assert ((r.s >= 0.0) & (r.s <= 1.0)).all()
    # dmin is the distance at an actual point: the one the call names
    at = scene.distance(p0 + r.s[:, None] * (p1 - p0), t=t0 + r.s * (t1 - t0))
    assert np.abs(at - r.dmin).max() <= 1e-9
    ends = np.minimum(scene.distance(p0, t=t0), scene.distance(p1, t=t1))
    assert (r.dmin <= ends).all()
    print(f"{kind}: {int((r.dmin < ends - EPS).sum())} of {N_SEG} segments dip more than eps below both ends")
    # the interior matters on these fixtures: swept_ref.dense alone finds 30 or more such segments on each of them
    assert (r.dmin < ends - EPS).sum() >= 10


def test_tunnelling_through_a_thin_wall(gpu_ctx):
    scene = Scene(gpu_ctx, [Scene.box((1.0, -5.0, -5.0), (1.05, 5.0, 5.0))])
    p0, p1 = np.array([[0.5, 0.2, -0.1]]), np.array([[1.55, 0.2, -0.1]])
    ends = scene.distance(np.concatenate([p0, p1]))
    assert (ends > 0.49).all()
    r = scene.swept_distance(p0, p1)
    print(f"\nwall: ends {ends}, dmin {r.dmin[0]:.4f} at s = {r.s[0]:.4f}, gap {r.gap[0]:.1e}, {r.evals[0]} evaluations")
    assert r.dmin[0] < 0.0 and -0.025 - 1e-9 <= r.dmin[0] <= -0.025 + r.gap[0] + 1e-9  # the wall's mid-plane
    scene.close()


def test_tunnelling_of_a_mover_over_a_point(gpu_ctx):
    scene = Scene(gpu_ctx, [Scene.moving(Scene.sphere((-2.0, 0.0, 0.0), 0.3), v=(20.0, 0.0, 0.0))])
    p = np.zeros((1, 3))
    assert scene.distance(p, t=0.0)[0] > 1.6 and scene.distance(p, t=0.2)[0] > 1.6
    r = scene.swept_distance(p, p, t0=0.0, t1=0.2)
    print(f"\nmover: dmin {r.dmin[0]:.4f} at s = {r.s[0]:.4f}, gap {r.gap[0]:.1e}, {r.evals[0]} evaluations")
    assert r.dmin[0] < 0.0 and -0.3 - 1e-9 <= r.dmin[0] <= -0.3 + r.gap[0] + 1e-9  # the centre passes through the point
    assert scene.swept_distance(p, p).evals[0] == 1  # without times nothing moves
    scene.close()


def _point_segment(c, a, b):
    e = b - a
    u = np.clip(np.einsum("ni,ni->n", c - a, e) / np.einsum("ni,ni->n", e, e), 0.0, 1.0)
    return np.linalg.norm(a + u[:, None] * e - c, axis=1)


def test_closed_forms_for_a_sphere(gpu_ctx):
    rng = np.random.default_rng(2)
    c, rad, v = np.array([0.3, -0.2, 0.4]), 0.45, np.array([0.8, -0.5, 0.3])
    n = 64
    p0, p1 = rng.uniform(-2.0, 2.0, (n, 3)), rng.uniform(-2.0, 2.0, (n, 3))
    t0, t1 = rng.uniform(0.0, 1.0, n), rng.uniform(0.0, 1.0, n)
    still, moving = Scene(gpu_ctx, [Scene.sphere(c, rad)]), Scene(gpu_ctx, [Scene.moving(Scene.sphere(c, rad), v=v)])
    for scene, true in ((still, _point_segment(c[None], p0, p1) - rad),
                        (moving, _point_segment(c[None], p0 - v * t0[:, None], p1 - v * t1[:, None]) - rad)):
        r = scene.swept_distance(p0, p1, t0=t0, t1=t1)
        err = r.dmin - true
        print(f"\nsphere (dynamic {scene.is_dynamic}): dmin - true in [{err.min():.2e}, {err.max():.2e}], gap <= {r.gap.max():.2e}")
        assert (err >= -1e-9).all() and (err <= r.gap + 1e-9).all()
        scene.close()


def test_small_budget_reports_a_larger_gap(gpu_ctx):
    """Segments parallel to a wall: D is constant, the bound cannot prove it in 4 evaluations, and says so."""
    wall = [("box", [-5.0, -5.0, -1.0, 5.0, 5.0, 0.0])]
    scene = Scene(gpu_ctx, wall)
    rng = np.random.default_rng(3)
    n = 40
    p0 = np.column_stack([rng.uniform(-3.0, 3.0, (n, 2)), rng.uniform(0.05, 0.3, n)])
    ang = rng.uniform(0.0, 2.0 * np.pi, n)
    p1 = p0 + np.column_stack([np.cos(ang), np.sin(ang), np.zeros(n)])  # 1 m along the wall
    r = scene.swept_distance(p0, p1, max_evals=4)
    _check_certificate(r, wall, p0, p1, 0.0, 0.0, 4, "budget of 4")
    assert (r.evals == 4).all() and (r.gap > EPS).all()
    assert np.abs(r.dmin - p0[:, 2]).max() <= 1e-12
    full = scene.swept_distance(p0, p1)
    assert (full.gap <= EPS + 1e-12).all() and (full.evals < 4096).all() and (full.evals > 4).all()
    scene.close()


def test_indexed_set_equals_plain_set(gpu_ctx):
    prims = Scene.forest(20, (-3.0, -3.0, -1.0), (3.0, 3.0, 2.0), seed=8)
    plain, grid = Scene(gpu_ctx, prims), Scene(gpu_ctx, prims, grid=True)
    p0, p1, _, _ = _segments(np.random.default_rng(4), 200, np.array([-3.0, -3.0, -1.0]), np.array([3.0, 3.0, 2.0]))
    a, b = plain.swept_distance(p0, p1), grid.swept_distance(p0, p1)
    print(f"\nindexed against plain: |dmin| differs by {np.abs(a.dmin - b.dmin).max():.1e}, s by {np.abs(a.s - b.s).max():.1e}")
    assert np.abs(a.dmin - b.dmin).max() <= 1e-9
    plain.close()
    grid.close()


def test_edges(gpu_ctx):
    scene = Scene(gpu_ctx, R.SCENE)
    p0, p1, t0, t1 = _segments(np.random.default_rng(6), 257, np.array([-0.5, -3.0, -1.4]), np.array([6.0, 3.0, 2.0]))
    whole = scene.swept_distance(p0, p1)  # n = 257: a partial second block
    one = scene.swept_distance(p0[200:201], p1[200:201])  # n = 1
    for k in ("dmin", "s", "gap", "evals"):
        assert getattr(one, k)[0] == getattr(whole, k)[200]
    np.testing.assert_array_equal(scene.swept_distance(p0[256:], p1[256:]).dmin, whole.dmin[256:])
    # a set that is not dynamic ignores the times, non-finite ones included
    timed = scene.swept_distance(p0, p1, t0=t0, t1=np.full(257, np.nan))
    for k in ("dmin", "s", "gap", "evals"):
        np.testing.assert_array_equal(getattr(timed, k), getattr(whole, k))
    # a zero-length segment: one evaluation, no gap
    z = scene.swept_distance(p0[:5], p0[:5])
    np.testing.assert_array_equal(z.dmin, scene.distance(p0[:5]))
    assert (z.evals == 1).all() and (z.gap == 0.0).all() and (z.s == 0.0).all()
    # one NaN coordinate among valid segments: NaN there, the neighbours as they were, and the call returns
    q1 = p1.copy()
    q1[100, 1] = np.nan
    bad = scene.swept_distance(p0, q1)
    assert np.isnan(bad.dmin[100]) and np.isnan(bad.gap[100]) and bad.evals[100] == 0
    keep = np.arange(257) != 100
    for k in ("dmin", "s", "gap", "evals"):
        np.testing.assert_array_equal(getattr(bad, k)[keep], getattr(whole, k)[keep])
    dyn = Scene(gpu_ctx, _gpu_prims(D.SPEC))
    inf_t = np.zeros(4)
    inf_t[2] = np.inf
    bad = dyn.swept_distance(p0[:4], p1[:4], t0=np.zeros(4), t1=inf_t)
    assert np.isnan(bad.dmin[2]) and np.isfinite(bad.dmin[[0, 1, 3]]).all()
    dyn.close()
    scene.close()
    # an empty scene: +inf, no gap
    for empty in (Scene(gpu_ctx, []), Scene(gpu_ctx, [], grid=True)):
        r = empty.swept_distance(p0[:3], p1[:3])
        assert (r.dmin == np.inf).all() and (r.gap == 0.0).all()
        empty.close()


def test_two_scenes(gpu_ctx):
    """S = 2: p_to_scene, and the default ordering (the first half of the segments to scene 0)."""
    other = [("sphere", [1.5, 0.5, 0.2, 0.5]), ("box", [-2.0, -2.5, -1.0, 2.0, -1.5, 1.0])]
    both = Scene(gpu_ctx, [R.SCENE, other])
    singles = [Scene(gpu_ctx, R.SCENE), Scene(gpu_ctx, other)]
    p0, p1, _, _ = _segments(np.random.default_rng(9), 60, np.array([-0.5, -3.0, -1.4]), np.array([6.0, 3.0, 2.0]))
    want = [s.swept_distance(p0, p1) for s in singles]
    default = both.swept_distance(p0, p1)
    np.testing.assert_array_equal(default.dmin, np.concatenate([want[0].dmin[:30], want[1].dmin[30:]]))
    p2s = np.random.default_rng(1).integers(0, 2, 60)
    mapped = both.swept_distance(p0, p1, p_to_scene=p2s)
    for k in ("dmin", "s", "gap", "evals"):
        np.testing.assert_array_equal(getattr(mapped, k), np.where(p2s == 0, getattr(want[0], k), getattr(want[1], k)))
    with pytest.raises(_lib.SdfnmpcError, match="error -1"):
        both.swept_distance(p0[:59], p1[:59])  # n % S != 0 without p_to_scene
    for s in singles + [both]:
        s.close()


def test_speed_bound(sets, gpu_ctx):
    for kind, (scene, prims, _) in sets.items():
        V = scene.speed_bound
        assert V.shape == (1,) and V.dtype == np.float64
        want = W.speed_bound(prims)
        assert abs(V[0] - want) <= 1e-12 * want, (kind, V, want)
        assert (V[0] > 0.0) == scene.is_dynamic
    two = Scene(gpu_ctx, [R.SCENE, _gpu_prims(D.SPEC)])  # per scene: the static one of a dynamic set has none
    V = two.speed_bound
    assert V[0] == 0.0 and abs(V[1] - W.speed_bound(D.scene())) <= 1e-12 * V[1]
    two.close()


def test_refusals_launch_nothing(gpu_ctx):
    ctx = gpu_ctx
    scene = Scene(ctx, [R.SCENE, R.SCENE[:2]])
    other_ctx = _lib.Context(ctx.device)
    elsewhere = Scene(other_ctx, R.SCENE)
    n = 8
    p0, p1 = (_lib.DeviceArray.from_numpy(ctx, np.random.default_rng(k).uniform(-1, 1, (n, 3))) for k in (0, 1))
    t = _lib.DeviceArray.from_numpy(ctx, np.zeros(n))
    out = [_lib.DeviceArray.from_numpy(ctx, np.full(n, np.nan)) for _ in range(3)]
    evals = _lib.DeviceArray.from_numpy(ctx, np.full(n, -7, np.int32))
    good = dict(ctx=ctx, scene_h=scene.h, p0=p0, p1=p1, p_to_scene=None, t0=None, t1=None, n=n, eps=1e-3, max_evals=64,
                dmin=out[0], s=out[1], gap=out[2], evals=evals)

    class NoCtx:
        h = None

    bad = [dict(ctx=NoCtx()), dict(scene_h=None), dict(p0=None), dict(p1=None), dict(dmin=None), dict(n=-1), dict(n=2 ** 31),
           dict(n=7), dict(t0=t), dict(t1=t), dict(eps=float("nan")), dict(eps=float("inf")), dict(eps=1e-7), dict(eps=-1.0),
           dict(max_evals=1), dict(max_evals=65537), dict(scene_h=elsewhere.h)]
    for kw in bad:
        with pytest.raises(_lib.SdfnmpcError, match="error -1"):
            _lib.scene_swept_distance(**{**good, **kw})
        ctx.synchronize()
        for a in out:
            assert np.isnan(a.numpy()).all(), kw
        assert (evals.numpy() == -7).all(), kw
    _lib.scene_swept_distance(**{**good, "n": 0})  # a no-op
    ctx.synchronize()
    assert np.isnan(out[0].numpy()).all()
    _lib.scene_swept_distance(**{**good, "s": None, "gap": None, "evals": None, "max_evals": 2, "eps": 1e-6})  # the limits
    ctx.synchronize()
    assert np.isfinite(out[0].numpy()).all() and np.isnan(out[1].numpy()).all() and (evals.numpy() == -7).all()
    with pytest.raises(ValueError):
        scene.swept_distance(np.zeros((2, 3)), np.ones((2, 3)), t0=0.0)
    assert _lib.load().sdfnmpc_scene_speed_bound(None, None) == -1
    elsewhere.close()
    other_ctx.close()
    scene.close()
