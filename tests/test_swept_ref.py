"""The numpy restatement of the swept-clearance query (tests/swept_ref.py) against dense sampling, the time-Lipschitz
bound V against finite differences in time, and closed forms for one sphere.  No GPU."""
import numpy as np
import pytest

import scene_dyn_ref as D
import scene_ref as R
import swept_ref as W

M = 4096


def _random_scene(rng, moving):
    """Five primitives over the three kinds around the origin; with `moving` each gets a random motion."""
    prims = []
    for i in range(5):
        c = rng.uniform(-2.0, 2.0, 3)
        kind = ("sphere", "box", "cylinder")[i % 3]
        if kind == "sphere":
            p = ("sphere", [*c, rng.uniform(0.2, 0.6)])
        elif kind == "box":
            h = rng.uniform(0.1, 0.7, 3)
            p = ("box", [*(c - h), *(c + h)])
        else:
            p = ("cylinder", [c[0], c[1], rng.uniform(0.15, 0.5), c[2] - 0.8, c[2] + 0.8])
        if moving:
            p = D.moving(p, v=rng.uniform(-1.0, 1.0, 3), rpy=rng.uniform(-0.6, 0.6, 3), yaw_rate=rng.uniform(-2.0, 2.0),
                         amp=rng.uniform(-0.5, 0.5, 3), omega=rng.uniform(0.5, 3.0), phase=rng.uniform(0.0, 6.0))
        prims.append(p)
    return prims


def _segment(rng):
    p0 = rng.uniform(-3.0, 3.0, 3)
    e = rng.normal(size=3)
    p1 = p0 + e / np.linalg.norm(e) * rng.uniform(0.0, 1.0)
    t0 = rng.uniform(0.0, 2.0)
    return p0, p1, t0, t0 + rng.uniform(-0.2, 0.2)


@pytest.mark.parametrize("moving", [False, True])
def test_bnb_brackets_the_dense_minimum(moving):
    rng = np.random.default_rng(5 + moving)
    prims = _random_scene(rng, moving)
    for _ in range(25):
        p0, p1, t0, t1 = _segment(rng)
        dmin, s, gap, evals = W.bnb(prims, p0, p1, t0, t1, eps=1e-3)
        dn = W.dense(prims, p0, p1, t0, t1, M)[0][0]
        L = W.lipschitz(prims, p0, p1, t0, t1)
        assert dn - L / (2 * M) - 1e-9 <= dmin
        assert dmin - gap <= dn + 1e-9
        assert evals < 4096 and gap <= 1e-3 + 1e-12
        assert dmin == W.distance(prims, (p0 + s * (p1 - p0))[None], t0 + s * (t1 - t0))[0]  # a value at an actual point


def test_bnb_small_budget_reports_its_gap():
    rng = np.random.default_rng(7)
    prims = _random_scene(rng, True)
    for _ in range(10):
        p0, p1, t0, t1 = _segment(rng)
        dmin, s, gap, evals = W.bnb(prims, p0, p1, t0, t1, eps=1e-3, max_evals=4)
        dn = W.dense(prims, p0, p1, t0, t1, M)[0][0]
        assert evals <= 4
        assert dn - W.lipschitz(prims, p0, p1, t0, t1) / (2 * M) - 1e-9 <= dmin and dmin - gap <= dn + 1e-9


def test_bnb_edges():
    prims = _random_scene(np.random.default_rng(1), True)
    p = np.array([0.3, -0.2, 0.1])
    d, s, gap, evals = W.bnb(prims, p, p, 0.4, 0.4)  # a point: one evaluation
    assert (s, gap, evals) == (0.0, 0.0, 1) and d == W.distance(prims, p[None], 0.4)[0]
    assert W.bnb([], p, p + 1.0, 0.0, 0.1)[:3] == (np.inf, 0.0, 0.0)  # an empty scene
    bad = W.bnb(prims, np.array([np.nan, 0.0, 0.0]), p, 0.0, 0.1)
    assert np.isnan(bad[0]) and bad[3] == 0


def test_dense_cull_keeps_the_minimum():
    """`relevant` drops only primitives that cannot hold the minimum: the same samples' minimum with and without."""
    rng = np.random.default_rng(3)
    prims = [("cylinder", [*rng.uniform(-6, 6, 2), rng.uniform(0.15, 0.4), -1.0, 2.0]) for _ in range(60)]
    prims += [D.moving(("sphere", [0.0, 0.0, 0.5, 0.3]), v=(1.0, 0.5, 0.0))]
    p0, p1, t0, t1 = (np.array(a) for a in zip(*[_segment(rng) for _ in range(10)]))
    for a, b in zip(W.dense(prims, p0, p1, t0, t1, 256), W.dense(prims, p0, p1, t0, t1, 256, cull=False)):
        np.testing.assert_array_equal(a, b)
    keep = W.relevant(prims, p0, p1)
    assert keep[:, -1].all() and (keep.sum(axis=1) < len(prims) // 2).all()  # the mover stays, most cylinders go


def test_speed_bound_is_lipschitz_in_time():
    """|D(p, t + delta) - D(p, t)| <= V delta for random movers, points and steps."""
    rng = np.random.default_rng(11)
    for k in range(8):
        prims = _random_scene(rng, True)
        V = W.speed_bound(prims)
        n = 400
        pts = rng.uniform(-4.0, 4.0, (n, 3))
        t = rng.uniform(0.0, 3.0, n)
        delta = 10.0 ** rng.uniform(-4.0, -0.5, n)
        diff = np.abs(W.distance(prims, pts, t + delta) - W.distance(prims, pts, t))
        assert (diff <= V * delta * (1.0 + 1e-9)).all(), (k, (diff / (V * delta)).max())
    assert W.speed_bound(R.SCENE) == 0.0
    # the terms one by one: a translating sphere, a swinging sphere, a box turning about z
    assert W.speed_bound([D.moving(R.SCENE[0], v=(3.0, 4.0, 0.0))]) == pytest.approx(5.0, rel=1e-11)
    assert W.speed_bound([D.moving(R.SCENE[0], amp=(0.0, 2.0, 0.0), omega=-1.5)]) == pytest.approx(3.0, rel=1e-11)
    assert W.speed_bound([D.moving(("box", [-1, -2, -2, 1, 2, 2]), yaw_rate=2.0)]) == pytest.approx(6.0, rel=1e-11)
    assert W.speed_bound([D.moving(("cylinder", [0, 0, 3.0, -4, 4]), yaw_rate=1.0)]) == pytest.approx(5.0, rel=1e-11)


def _point_segment(c, a, b):
    """Distance from the point c to the segment a -> b."""
    e = b - a
    u = np.clip((c - a) @ e / (e @ e), 0.0, 1.0)
    return np.linalg.norm(a + u * e - c)


def test_closed_form_sphere():
    rng = np.random.default_rng(2)
    for _ in range(20):
        c, r = rng.uniform(-1.0, 1.0, 3), rng.uniform(0.2, 0.5)
        p0, p1 = rng.uniform(-2.0, 2.0, 3), rng.uniform(-2.0, 2.0, 3)
        true = _point_segment(c, p0, p1) - r
        dmin, _, gap, _ = W.bnb([("sphere", [*c, r])], p0, p1)
        assert -1e-9 <= dmin - true <= gap + 1e-9
        # the sphere at constant velocity: the segment relative to it runs from p0 - v t0 to p1 - v t1
        v, t0, t1 = rng.uniform(-1.0, 1.0, 3), rng.uniform(0.0, 1.0), rng.uniform(0.0, 1.0)
        true = _point_segment(c, p0 - v * t0, p1 - v * t1) - r
        dmin, _, gap, _ = W.bnb([D.moving(("sphere", [*c, r]), v=v)], p0, p1, t0, t1)
        assert -1e-9 <= dmin - true <= gap + 1e-9
