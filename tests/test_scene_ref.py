"""tests/scene_ref.py, the fp64 reference of csrc/scene.hip, pinned to answers derivable by hand, and the condition
under which the GPU comparison is meaningful: almost every pixel of every test image is `decided`."""
import numpy as np
import pytest

import scene_ref as R
import sdf_nmpc_amd.scene  # noqa: F401  (the feature under test: these tests describe its reference)


def test_box_face_seen_from_the_origin():
    """A face at x = d0 filling the view: depth d0 everywhere, range d0 sqrt(1 + ty^2 + tz^2)."""
    d0, h, w = 2.0, 9, 12
    prims = [("box", [d0, -20.0, -20.0, d0 + 1.0, 20.0, 20.0])]
    p, Rm = np.zeros((1, 3)), np.eye(3)[None]
    depth = R.values(prims, p, Rm, h, w, R.SENSOR["hfov"], R.SENSOR["vfov"], 5.0, is_depth=True)
    np.testing.assert_allclose(depth, d0, rtol=0, atol=1e-14)
    ty = np.tan(R.SENSOR["hfov"]) * (1 - (2 * np.arange(w) + 1) / w)
    tz = np.tan(R.SENSOR["vfov"]) * (1 - (2 * np.arange(h) + 1) / h)
    rng = R.values(prims, p, Rm, h, w, R.SENSOR["hfov"], R.SENSOR["vfov"], 5.0)[0]
    np.testing.assert_allclose(rng, d0 * np.sqrt(1 + ty[None, :] ** 2 + tz[:, None] ** 2), rtol=0, atol=1e-14)
    assert ty[0] > 0 > ty[-1] and tz[0] > 0 > tz[-1]  # u = 0 is the left column (y left), v = 0 the top row (z up)
    # nearer than the clip: the scaled image; beyond it: dmax
    np.testing.assert_allclose(R.render(prims, p, Rm, h, w, 0.7592, 0.4903, 5.0, 0.2, is_depth=True), 0.4, atol=1e-14)
    assert (R.values(prims, p, Rm, h, w, 0.7592, 0.4903, 1.5) == 1.5).all()


def test_sphere_on_the_optical_axis():
    """An odd image has a pixel on the axis: its ray passes through the centre, range |c| - r; a camera turned by
    yaw sees the same sphere on its axis when the sphere is turned with it; a pixel far off the axis misses."""
    c, r = 3.0, 0.75
    for yaw in (0.0, 0.4):
        Rm = R.rpy2rot(0, 0, yaw)
        prims = [("sphere", list(Rm @ np.array([c, 0, 0])) + [r])]
        v = R.values(prims, np.zeros((1, 3)), Rm[None], 9, 9, 0.7, 0.5, 5.0)[0]
        assert abs(v[4, 4] - (c - r)) <= 1e-14
        assert v[0, 0] == 5.0 and v[4, 4] == v.min()
        np.testing.assert_allclose(v, v[::-1, ::-1], atol=1e-13)  # symmetric about the axis
    # spherical pixels: the centre pixel of an odd image is the axis too
    v = R.values([("sphere", [c, 0, 0, r])], np.zeros((1, 3)), np.eye(3)[None], 7, 11, 1.2, 0.6, 5.0, is_spherical=True)[0]
    assert abs(v[3, 5] - (c - r)) <= 1e-14
    # inside: every ray starts in the obstacle
    assert not R.values([("sphere", [0.1, 0, 0, r])], np.zeros((1, 3)), np.eye(3)[None], 5, 5, 0.7, 0.5, 5.0).any()


def test_cylinder_side_and_cap():
    cyl = [("cylinder", [2.0, 0.0, 0.5, -1.0, 1.0])]
    assert abs(R.cast(cyl, [0, 0, 0], [[1.0, 0, 0]])[0] - 1.5) <= 1e-15          # the wall
    assert abs(R.cast(cyl, [2.0, 0.2, 3.0], [[0, 0, -1.0]])[0] - 2.0) <= 1e-15   # the top cap from above
    assert R.cast(cyl, [0, 0, 2.0], [[1.0, 0, 0]])[0] == np.inf                  # over it
    s = np.sqrt(0.5)
    assert abs(R.cast(cyl, [1.0, 0, 2.0], [[s, 0, -s]])[0] - np.sqrt(2)) <= 1e-14  # down onto the cap at x = 2
    assert abs(R.cast(cyl, [0, 0, 2.0], [[s, 0, -s]])[0] - 1.5 / s) <= 1e-14     # past the rim, onto the wall at z = 0.5


def test_signed_distance_at_hand_picked_points():
    box = [("box", [0.0, 0.0, 0.0, 2.0, 4.0, 6.0])]
    cyl = [("cylinder", [0.0, 0.0, 1.0, -2.0, 2.0])]
    sph = [("sphere", [1.0, 2.0, 3.0, 0.5])]
    d = lambda prims, p: R.distance(prims, [p])[0]
    assert abs(d(box, [3.0, 5.0, 8.0]) - np.sqrt(1 + 1 + 4)) <= 1e-15   # off the corner (2, 4, 6)
    assert abs(d(box, [1.0, 2.0, 7.5]) - 1.5) <= 1e-15                  # over a face
    assert abs(d(box, [3.0, 5.0, 3.0]) - np.sqrt(2)) <= 1e-15           # off an edge
    assert abs(d(box, [1.0, 2.0, 3.0]) + 1.0) <= 1e-15                  # inside: the nearest face is 1 away
    assert d(box, [2.0, 1.0, 1.0]) == 0.0                               # on a face
    assert abs(d(cyl, [4.0, 0.0, 6.0]) - 5.0) <= 1e-15                  # off the rim: 3 out, 4 up
    assert abs(d(cyl, [0.0, 3.0, 0.0]) - 2.0) <= 1e-15                  # beside the wall
    assert abs(d(cyl, [0.2, 0.0, 5.0]) - 3.0) <= 1e-15                  # over the cap
    assert abs(d(cyl, [0.0, 0.5, 0.0]) + 0.5) <= 1e-15                  # inside, nearer the wall
    assert abs(d(cyl, [0.0, 0.0, 1.75]) + 0.25) <= 1e-15                # inside, nearer the cap
    assert abs(d(sph, [1.0, 2.0, 5.0]) - 1.5) <= 1e-15 and abs(d(sph, [1.0, 2.0, 3.0]) + 0.5) <= 1e-15
    # the union: the minimum
    assert abs(d(box + sph + cyl, [1.0, 2.0, 3.0]) + 1.0) <= 1e-15
    assert R.distance([], [[0.0, 0.0, 0.0]])[0] == np.inf


def test_quat2rot_normalises():
    np.testing.assert_allclose(R.quat2rot([2.0, 0, 0, 0]), np.eye(3), atol=1e-16)
    a = 0.6
    np.testing.assert_allclose(R.quat2rot([3 * np.cos(a / 2), 0, 0, 3 * np.sin(a / 2)]), R.rpy2rot(0, 0, a), atol=1e-15)


@pytest.mark.parametrize("shape", R.SHAPES)
@pytest.mark.parametrize("sensor", ["pinhole", "spherical"])
def test_test_images_are_almost_everywhere_decided(shape, sensor):
    """The condition of the GPU comparison: at most 2 % of the pixels of every test image are undecided."""
    s = R.SENSOR if sensor == "pinhole" else R.SPHERICAL
    p, Rm = R.camera_poses()
    for is_depth in (False, True):
        ok = R.decided(R.SCENE, p, Rm, *shape, s["hfov"], s["vfov"], s["dmax"], is_depth=is_depth,
                       is_spherical=sensor == "spherical")
        share = 1.0 - ok.reshape(len(p), -1).mean(axis=1)
        print(f"\n{sensor} {shape} depth={is_depth}: undecided share per image {share}, overall {1 - ok.mean():.4f}")
        assert (share <= 0.02).all(), share
        v = R.values(R.SCENE, p, Rm, *shape, s["hfov"], s["vfov"], s["dmax"], is_depth=is_depth,
                     is_spherical=sensor == "spherical")
        assert ((v < s["dmax"]).mean(axis=(1, 2)) > 0.2).all() and (v == s["dmax"]).any()  # hits and misses
