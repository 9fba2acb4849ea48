"""The grid of an indexed scene and its two stop rules, where they can be examined without a GPU: tests/scene_grid_ref.py
(the numpy restatement of sdfnmpc_scene_create_large's build and of csrc/scene_grid.hip's searches) against the brute
force of tests/scene_ref.py on random forests -- a search may skip primitives, never the one that decides -- and
Scene.forest itself."""
import numpy as np
import pytest

import scene_grid_ref as G
import scene_ref as R
from sdf_nmpc_amd.scene import Scene

LO, HI = (-6.0, -6.0, -1.0), (6.0, 6.0, 2.0)
EXTRA = [Scene.sphere((0.5, 1.0, 0.5), 1.2), Scene.box((-5.0, -5.5, -0.5), (4.0, -4.5, 0.5)), Scene.sphere((3.0, 3.0, 1.0), 0.3)]


def _world(n, seed):
    return Scene.forest(n, LO, HI, radius=(0.1, 0.35), seed=seed) + EXTRA


def _rays(seed, n):
    """Origins inside the grid's box, outside it, and on cell planes; directions random, axis-parallel and vertical."""
    rng = np.random.default_rng(seed)
    o = rng.uniform(-7, 7, (n, 3)) * np.array([1, 1, 0.3])
    o[::5] = rng.uniform(-30, 30, (len(o[::5]), 3))
    d = rng.normal(0, 1, (n, 3))
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    d[1::7] = (1.0, 0.0, 0.0)
    d[2::7] = (0.0, 0.0, -1.0)
    d[3::7] = (0.0, -1.0, 0.0)
    return o, d


@pytest.mark.parametrize("n,cell", [(0, None), (1, None), (40, None), (40, 100.0), (40, 0.25), (150, None)])
def test_every_ray_finds_the_brute_force_hit(n, cell):
    prims = _world(n, seed=n) if n else []
    g = G.build(prims, cell)
    assert (g["n"] >= 1).all() and g["start"][-1] == len(g["items"])
    if cell == 100.0:
        assert (g["n"] == 1).all()
    o, d = _rays(3, 60)
    o[0] = (g["org"][0] + 2 * g["cell"], 0.1, 0.2)  # on a cell plane, looking along +x
    d[0] = (1.0, 0.0, 0.0)
    skipped = 0
    for oo, dd in zip(o, d):
        hits = [R.cast([p], oo, dd[None])[0] for p in prims]
        for tstop in (np.inf, 5.0):
            best, seen, cells = G.ray_search(g, oo, dd, tstop, lambda i: hits[i])
            want = min(hits, default=np.inf)
            assert cells <= g["n"].sum() + 3
            if want < tstop:
                assert best == want
            else:  # beyond tstop a pixel is a miss whatever was found
                assert best >= tstop
            skipped += len(prims) - len(seen)
    if n >= 40 and cell != 100.0:
        assert skipped > 0  # the index skips something: the test is not the brute force in disguise


@pytest.mark.parametrize("n,cell", [(0, None), (1, None), (40, None), (40, 100.0), (40, 0.25), (150, None)])
def test_every_point_finds_the_brute_force_distance(n, cell):
    prims = _world(n, seed=n) if n else []
    g = G.build(prims, cell)
    rng = np.random.default_rng(5)
    pts = rng.uniform(-7, 7, (80, 3)) * np.array([1, 1, 0.4])
    pts[:5] = rng.uniform(-1, 1, (5, 3)) * 100.0 + 100.0                       # far outside the grid
    pts[5] = (0.5, 1.0, 0.5)                                                   # inside a primitive
    pts[6] = g["org"] + g["cell"] * np.minimum(np.array([1, 1, 1]), g["n"])    # on a cell corner
    want = R.distance(prims, pts) if prims else np.full(len(pts), np.inf)
    per = [R.distance([p], pts) for p in prims]
    skipped = 0
    for j, p in enumerate(pts):
        best, seen, rounds = G.point_search(g, p, lambda i: per[i][j])
        assert best == want[j] and rounds <= g["n"].max() + 1
        for cap in (0.3, 2.0):  # the rows kernel: exact below max_df, and at least max_df when nothing is nearer
            b2, s2, _ = G.point_search(g, p, lambda i: per[i][j], cap)
            assert (b2 == want[j]) if want[j] < cap else (b2 >= cap)
            assert len(s2) <= len(seen)
        skipped += len(prims) - len(seen)
    if n >= 40 and cell != 100.0:
        assert skipped > 0


def test_a_primitive_is_listed_wherever_its_inflated_box_reaches():
    prims = _world(25, seed=4)
    g = G.build(prims)
    n, c, org = g["n"], g["cell"], g["org"]
    assert g["infl"] > 0 and (n <= 256).all()
    for i, p in enumerate(prims):
        lo, hi = G.bbox(p)
        assert (lo - 2 * g["infl"] >= org).all() and (hi + 2 * g["infl"] <= org + n * c).all()
        for z in range(n[2]):
            for y in range(n[1]):
                for x in range(n[0]):
                    cid = (z * n[1] + y) * n[0] + x
                    a = org + np.array([x, y, z]) * c
                    overlaps = ((lo - g["infl"] <= a + c) & (hi + g["infl"] >= a)).all()
                    listed = i in g["items"][g["start"][cid]:g["start"][cid + 1]]
                    assert listed or not overlaps
    with pytest.raises(ValueError):
        G.build(prims, 1e-3)


def test_forest_is_reproducible_and_keeps_clear():
    a = Scene.forest(300, LO, HI, radius=(0.1, 0.4), seed=7, keep_clear=((1.0, -2.0), 2.5))
    b = Scene.forest(300, LO, HI, radius=(0.1, 0.4), seed=7, keep_clear=((1.0, -2.0), 2.5))
    assert a == b and len(a) == 300 and a != Scene.forest(300, LO, HI, radius=(0.1, 0.4), seed=8)
    free = Scene.forest(300, LO, HI, radius=(0.1, 0.4), seed=7)
    v, f = np.array([p[1] for p in a]), np.array([p[1] for p in free])
    assert all(p[0] == "cylinder" for p in a)
    assert (v[:, 2] >= 0.1).all() and (v[:, 2] <= 0.4).all() and (v[:, 3] == LO[2]).all() and (v[:, 4] == HI[2]).all()
    assert (f[:, :2] >= LO[:2]).all() and (f[:, :2] <= HI[:2]).all()
    d, d_free = np.hypot(v[:, 0] - 1.0, v[:, 1] + 2.0), np.hypot(f[:, 0] - 1.0, f[:, 1] + 2.0)
    assert (d_free < 2.5).sum() > 10 and (d >= 2.5).all()
    moved = d_free < 2.5
    np.testing.assert_array_equal(v[~moved], f[~moved])  # the others stay where the seed put them
    assert Scene.forest(0, LO, HI) == []
    with pytest.raises(ValueError):
        Scene.forest(3, LO, (6.0, -6.0, 2.0))
