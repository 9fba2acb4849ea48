"""tests/scene_dyn_ref.py pinned to answers one can derive by hand, and the condition the GPU comparison rests on: the
decided mask covers at least 98 % of every image of the dynamic fixture."""
import numpy as np
import pytest

import scene_dyn_ref as D
import scene_ref as R

X = np.array([[1.0, 0.0, 0.0]])
O = np.zeros(3)
S2 = np.sqrt(2.0)
UNIT_BOX = ("box", [-0.5, -0.5, -0.5, 0.5, 0.5, 0.5])


def _unit_box_at(c):
    c = np.asarray(c, float)
    return ("box", list(np.concatenate([c - 0.5, c + 0.5])))


def test_yawed_box_on_the_optical_axis():
    """Half extent 0.5 at (3, 0, 0), yawed by pi / 4: the vertical edge points at the camera, 3 - 0.5 sqrt 2."""
    box = _unit_box_at((3, 0, 0))
    assert D.cast([D.moving(box, rpy=(0, 0, np.pi / 4))], O, X)[0] == pytest.approx(3 - 0.5 * S2, abs=1e-14)
    assert D.cast([D.moving(box, q=(np.cos(np.pi / 8), 0, 0, np.sin(np.pi / 8)))], O, X)[0] == pytest.approx(3 - 0.5 * S2, abs=1e-14)
    assert D.cast([D.moving(box, yaw_rate=np.pi / 8)], O, X, t=2.0)[0] == pytest.approx(3 - 0.5 * S2, abs=1e-14)
    assert D.cast([D.moving(box)], O, X)[0] == pytest.approx(2.5, abs=1e-14)
    # through the image: the centre column of a one-row image with an odd width looks along the optical axis
    v = D.values([D.moving(box, rpy=(0, 0, np.pi / 4))], O, np.eye(3), 1, 3, 0.5, 0.3, 5.0)
    assert v[0, 0, 1] == pytest.approx(3 - 0.5 * S2, abs=1e-14)


def test_sphere_with_a_velocity():
    """Centre (3, 0, 0), r = 0.5, v = (0, 0.4, 0): at t = 2 the centre is (3, 0.8, 0)."""
    sph = D.moving(("sphere", [3.0, 0.0, 0.0, 0.5]), v=(0, 0.4, 0))
    assert D.cast([sph], O, X, t=0.0)[0] == pytest.approx(2.5, abs=1e-14)
    assert np.isinf(D.cast([sph], O, X, t=2.0)[0])                     # 0.8 > r: the axis ray passes it
    c = np.array([3.0, 0.8, 0.0])
    assert D.cast([sph], O, c[None] / np.linalg.norm(c), t=2.0)[0] == pytest.approx(np.linalg.norm(c) - 0.5, abs=1e-14)
    assert D.distance([sph], [[3.0, 2.0, 0.0]], t=2.0)[0] == pytest.approx(0.7, abs=1e-14)
    assert D.distance([sph], [[3.0, 0.8, 0.1]], t=2.0)[0] == pytest.approx(-0.4, abs=1e-14)


def test_rolled_cylinder():
    """Rolled by pi / 2 its axis lies along y: a ray along x meets the wall at cx - r wherever it starts along the
    axis, and passes above it at a height the upright cylinder would have blocked."""
    cyl = D.moving(("cylinder", [3.0, 0.0, 0.4, -1.0, 1.0]), rpy=(np.pi / 2, 0, 0))
    assert D.cast([cyl], O, X)[0] == pytest.approx(2.6, abs=1e-14)
    assert D.cast([cyl], np.array([0.0, 0.9, 0.0]), X)[0] == pytest.approx(2.6, abs=1e-14)
    assert np.isinf(D.cast([cyl], np.array([0.0, 0.0, 0.9]), X)[0])
    assert np.isinf(D.cast([cyl], np.array([0.0, 1.1, 0.0]), X)[0])
    # R(t) = Rz(yaw_rate t) R(q): the yaw comes after the roll, so a quarter turn lays the axis along x -- the cap at 2
    spun = D.moving(("cylinder", [3.0, 0.0, 0.4, -1.0, 1.0]), rpy=(np.pi / 2, 0, 0), yaw_rate=np.pi / 2)
    assert D.cast([spun], O, X, t=1.0)[0] == pytest.approx(2.0, abs=1e-14)
    assert D.distance([spun], [[0.0, 0.0, 0.0]], t=1.0)[0] == pytest.approx(2.0, abs=1e-14)
    assert D.distance([cyl], [[3.0, 1.5, 0.0]])[0] == pytest.approx(0.5, abs=1e-14)     # beyond the cap, on the axis


def test_harmonic_term_at_a_quarter_period():
    """amp sin(omega t + phase): omega = pi / 2 puts the quarter period at t = 1; a phase of pi / 2 puts it at t = 0."""
    sph = D.moving(("sphere", [3.0, 0.0, 0.0, 0.5]), amp=(0, 0, 1.0), omega=np.pi / 2)
    up = np.array([[3.0, 0.0, 4.0]])
    assert D.distance([sph], up, t=0.0)[0] == pytest.approx(3.5, abs=1e-14)
    assert D.distance([sph], up, t=1.0)[0] == pytest.approx(2.5, abs=1e-14)
    assert D.distance([sph], up, t=3.0)[0] == pytest.approx(4.5, abs=1e-14)
    assert D.distance([sph], up, t=2.0)[0] == pytest.approx(3.5, abs=1e-14)
    ahead = D.moving(("sphere", [3.0, 0.0, 0.0, 0.5]), amp=(0, 0, 1.0), omega=np.pi / 2, phase=np.pi / 2)
    assert D.distance([ahead], up, t=0.0)[0] == pytest.approx(2.5, abs=1e-14)
    np.testing.assert_allclose(D.distance([sph], np.repeat(up, 3, 0), t=[0.0, 1.0, 3.0]), [3.5, 2.5, 4.5], atol=1e-14)


def test_distance_to_a_rotated_box():
    """The unit box about the origin, yawed by pi / 4: its vertical edges are at distance sqrt(2) / 2 on the x and y
    axes."""
    box = D.moving(UNIT_BOX, rpy=(0, 0, np.pi / 4))
    e = 0.5 * S2
    assert D.distance([box], [[2.0, 0.0, 0.0]])[0] == pytest.approx(2 - e, abs=1e-14)                       # the edge
    assert D.distance([box], [[2.0, 0.0, 1.0]])[0] == pytest.approx(np.hypot(2 - e, 0.5), abs=1e-14)        # the corner
    # inside the rotated box, at a place outside the unrotated one: the nearest faces are at 0.5 - 0.6 / sqrt 2
    assert D.distance([box], [[0.6, 0.0, 0.0]])[0] == pytest.approx(-(0.5 - 0.6 / S2), abs=1e-14)
    assert R.distance([UNIT_BOX], [[0.6, 0.0, 0.0]])[0] == pytest.approx(0.1, abs=1e-14)
    assert not D.cast([box], np.array([0.6, 0.0, 0.0]), X).any()        # a camera there sees 0
    assert D.cast([D.moving(UNIT_BOX)], np.array([0.6, 0.0, 0.0]), X)[0] == np.inf


def test_without_motion_it_is_scene_ref_exactly():
    P, RM = R.camera_poses()
    s = R.SENSOR
    for kw in (dict(), dict(is_depth=True), dict(is_spherical=True)):
        want = R.values(R.SCENE, P, RM, 18, 32, s["hfov"], s["vfov"], s["dmax"], **kw)
        for t in (0.0, 1.7):
            np.testing.assert_array_equal(D.values(R.SCENE, P, RM, 18, 32, s["hfov"], s["vfov"], s["dmax"], t, **kw), want)
    pts = np.random.default_rng(1).uniform(-3, 5, (50, 3))
    np.testing.assert_array_equal(D.distance(R.SCENE, pts, t=0.9), R.distance(R.SCENE, pts))
    # carried through an identity frame the answer is the same to rounding
    ident = [D.moving(p) for p in R.SCENE]
    got = D.values(ident, P, RM, 18, 32, s["hfov"], s["vfov"], s["dmax"], 1.7)
    ok = R.decided(R.SCENE, P, RM, 18, 32, s["hfov"], s["vfov"], s["dmax"])
    assert np.abs(got - R.values(R.SCENE, P, RM, 18, 32, s["hfov"], s["vfov"], s["dmax"]))[ok].max() <= 1e-12
    assert np.abs(D.distance(ident, pts, t=0.9) - R.distance(R.SCENE, pts)).max() <= 1e-14


def test_fixture_is_decided_and_moves():
    """At least 98 % of every image of the fixture is decided -- the condition of the GPU comparison -- over both
    sensors, both shapes, the three times, range and depth; and the scene does move."""
    P, RM = R.camera_poses()
    prims = D.scene()
    worst = 1.0
    for sensor, sph in ((R.SENSOR, False), (R.SPHERICAL, True)):
        for shape in R.SHAPES:
            for t in D.TIMES:
                for is_depth in (False, True):
                    ok = D.decided(prims, P, RM, *shape, sensor["hfov"], sensor["vfov"], sensor["dmax"], t,
                                   is_depth=is_depth, is_spherical=sph)
                    worst = min(worst, ok.reshape(len(P), -1).mean(1).min())
    print(f"\nworst single image: {100 * worst:.2f} % decided")
    assert worst >= 0.98
    s = R.SENSOR
    a, b = (D.values(prims, P, RM, 27, 48, s["hfov"], s["vfov"], s["dmax"], t) for t in (0.0, 2.3))
    moved = (np.abs(a - b) > 0.1).mean()
    print(f"{100 * moved:.0f} % of the pixels move by more than 0.1 m between t = 0 and t = 2.3")
    assert moved > 0.2
