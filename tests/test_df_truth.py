"""The numpy restatement of the reference's image ground truth (tests/df_truth_ref.py) against scenes whose
answer can be derived by hand, and the host side of the ColChecker / DfComputer classes.

The reference's own kernels are NVIDIA Warp and cannot run here, so these cases are the only check that the
restatement -- the yardstick of tests/test_gpu_df_truth.py -- is right.
"""
import numpy as np
import pytest

import df_truth_ref as R

DMAX, HFOV, VFOV = 5.0, 0.7592, 0.4903  # config/default.yaml sensor
H, W = 30, 40
D0 = 2.5  # the wall (d0 / dmax = 0.5 is exact in fp32, so the threshold pixel * dmax is d0 itself)


def wall(d0=D0, n=1, h=H, w=W):
    return np.full((n, h, w), d0 / DMAX, np.float32)


def on_axis(xs):
    return np.stack([xs, np.zeros_like(xs), np.zeros_like(xs)], 1).astype(np.float32)


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_wall_collision_label_flips_at_the_wall(dtype):
    xs = np.array([0.5, 1.0, D0 - 0.1, np.nextafter(np.float32(D0), np.float32(0)), D0, np.nextafter(np.float32(D0), np.float32(9)), D0 + 0.5, 4.9])
    lab = R.colcheck(wall(), on_axis(xs), None, DMAX, HFOV, VFOV, R.OUTSIDE["free"], 0.0, True, False, dtype)
    assert lab.tolist() == [0, 0, 0, 0, 1, 1, 1, 1]  # val >= pixel * dmax: exactly at x = d0
    # off axis, inside the field of view: a depth image's wall is the plane x = d0
    pts = np.array([[2.4, 0.8, 0.3], [2.6, 0.8, 0.3], [2.4, -1.2, -0.6], [2.6, -1.2, -0.6]], np.float32)
    lab = R.colcheck(wall(), pts, None, DMAX, HFOV, VFOV, 0, 0.0, True, False, dtype)
    assert lab.tolist() == [0, 1, 0, 1]


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_wall_udf_is_distance_to_the_wall(dtype):
    """Constant pinhole depth image (is_depth, and the UDF's pinhole branch, which the reference selects with
    is_spherical): udf(x, 0, 0) = d0 - x to within one pooled-pixel pitch at depth d0."""
    xs = np.linspace(D0 - 0.9, D0 - 0.05, 18)
    udf, grad, idx = R.udf(wall(), on_axis(xs), None, DMAX, HFOV, VFOV, True, True, dtype=dtype)
    # pooled pixels sit at y = d0 tan(hfov) (1 - 2 i / w): the pitch is 2 d0 tan(hfov) / w (and likewise in z)
    pitch = max(2 * D0 * np.tan(HFOV) / (W // 5), 2 * D0 * np.tan(VFOV) / (H // 5))
    assert np.all(udf >= (D0 - xs) - 1e-6)
    assert np.all(udf <= np.hypot(D0 - xs, pitch) + 1e-6)
    assert np.abs(udf - (D0 - xs)).max() <= pitch
    # the pixel on the axis (i = w/2, j = h/2) is exactly ahead: it wins, and the gradient points away from it
    assert np.all(idx == (H // 5 // 2) * (W // 5) + W // 5 // 2)
    assert np.allclose(grad, [[-1, 0, 0]] * len(xs), atol=1e-6)
    assert np.allclose(udf, D0 - xs, atol=1e-6)
    # farther than max_df from everything: saturated, zero gradient
    udf, grad, _ = R.udf(wall(), on_axis(np.array([0.2, D0 - 1.1])), None, DMAX, HFOV, VFOV, True, True, dtype=dtype)
    assert np.all(udf == 1.0) and np.all(grad == 0)
    # beyond the wall the virtual wall at dmax takes over once it is closer than every pixel
    udf, grad, _ = R.udf(wall(), on_axis(np.array([4.8])), None, DMAX, HFOV, VFOV, True, True, dtype=dtype)
    assert abs(udf[0] - 0.2) < 1e-6
    assert np.allclose(grad[0], -np.array([DMAX, 0, 0]) / DMAX, atol=1e-6)  # the reference's (dmax, p.y, p.z)


def test_udf_angular_branch_range_image():
    """A constant range image in the angular branch (is_spherical False, sic) is a sphere of radius d0."""
    img = wall()
    pts = on_axis(np.array([D0 - 0.8, D0 - 0.3]))
    udf, grad, _ = R.udf(img, pts, None, DMAX, HFOV, VFOV, False, False)
    # the nearest pooled pixel is at angle (0, 0) (i = w/2, j = h/2): exactly d0 - x
    assert np.allclose(udf, [0.8, 0.3], atol=1e-9)
    assert np.allclose(grad, [[-1, 0, 0]] * 2, atol=1e-9)


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_wall_signed_field(dtype):
    """+(d0 - x) in front of the wall, negative behind, to within the local voxel step; saturates at -0.3 and 1
    with zero gradient."""
    dist, grid, _ = R.dist_grid()
    xs = D0 + np.array([-1.5, -0.5, -0.2, -0.07, -0.015, 0.015, 0.07, 0.2, 0.6])
    sdf, grad, idx = R.sdf(wall(), on_axis(xs), None, grid, dist, DMAX, HFOV, VFOV, True, False, dtype=dtype)

    def step(d):  # the voxel pitch of the shell a distance d falls in (GRID_PARAMS)
        return next(s for lo, hi, s in R.GRID_PARAMS if lo < d <= hi)

    assert sdf[0] == 1.0 and np.all(grad[0] == 0) and idx[0] == -1  # nothing within 1 m: max_df
    for k in (1, 2, 3, 4):  # in front: the nearest occupied voxel is the first grid plane at or past the wall
        d = D0 - xs[k]
        assert d - 1e-6 <= sdf[k] <= d + step(d + step(d)) + 1e-6, (xs[k], sdf[k])
        assert np.allclose(grad[k], [-1, 0, 0], atol=1e-6)  # -sign * (+x direction)
        assert np.allclose(grid[idx[k]], [sdf[k], 0, 0], atol=1e-6)
    for k in (5, 6, 7):  # behind: the nearest free voxel is the first grid plane strictly in front of the wall
        d = xs[k] - D0
        assert -(d + step(d + step(d))) - 1e-6 <= sdf[k] < -d + 1e-6, (xs[k], sdf[k])
        assert np.allclose(grad[k], [-1, 0, 0], atol=1e-6)  # -(-1) * (-x direction)
    assert sdf[8] == dtype(-0.3) and np.all(grad[8] == 0)  # 0.6 m inside: min_df


def test_minpool_skips_zeros():
    rng = np.random.default_rng(0)
    img = rng.uniform(0.2, 1.0, (2, 10, 15)).astype(np.float32)
    img[0, 0:5, 0:5] = 0           # an all-zero block stays 0
    img[0, 5:10, 5:10][1, 2] = 0   # a zero among valid pixels is skipped
    img[1, 0:5, 10:15] = 0
    img[1, 2, 12] = 0.7            # one valid pixel: it is the minimum
    out = R.minpool5(img, DMAX)
    assert out.shape == (2, 2, 3)
    assert out[0, 0, 0] == 0
    blk = img[0, 5:10, 5:10]
    assert out[0, 1, 1] == blk[blk != 0].min()
    assert out[1, 0, 2] == np.float32(0.7)
    assert out[1, 1, 0] == img[1, 5:10, 0:5].min()
    with pytest.raises(AssertionError):
        R.minpool5(np.zeros((1, 12, 15), np.float32), DMAX)


def test_outside_modes_and_safe_ball():
    img = wall()
    out_az = [1.0, 1.2, 0.0]    # azimuth 0.876 > hfov, in front of the wall
    out_el = [1.0, 0.0, -0.7]   # elevation -0.61 < -vfov
    inside = [1.0, 0.2, 0.1]
    behind_out = [3.0, 3.6, 0.0]  # outside the fov and past the wall's depth
    pts = np.array([out_az, out_el, inside, behind_out], np.float32)

    def lab(mode, ball=0.0):
        return R.colcheck(img, pts, None, DMAX, HFOV, VFOV, R.OUTSIDE[mode], ball, True, False).tolist()

    assert lab("free") == [0, 0, 0, 0]
    assert lab("col") == [1, 1, 0, 1]
    assert lab("extrapolate") == [0, 0, 0, 1]  # clamped to the border pixel: the wall's depth decides
    # the safe ball wins over everything, but only strictly inside or on it (|p| > safe_ball)
    ln = float(np.sqrt(np.sum(np.square(pts[0].astype(np.float64)))))
    assert lab("col", ball=ln + 0.01)[0] == 0 and lab("col", ball=ln - 0.01)[0] == 1
    on5 = np.array([[3.0, 0.0, 4.0]], np.float32)  # |p| == 5 exactly; the range image's sphere is at 4.8
    assert R.colcheck(wall(4.0), on5, None, 6.0, 1.5, 1.5, 1, 5.0, False, True)[0] == 0  # on the ball: free
    assert R.colcheck(wall(4.0), on5, None, 6.0, 1.5, 1.5, 1, 4.999, False, True)[0] == 1


def test_behind_camera_dmax_and_origin():
    img = wall()
    pts = np.array([[-1.0, 0.1, 0.0],    # behind the camera: azimuth ~ pi, outside every fov
                    [0.0, 0.0, 0.0],     # the origin: |p| = 0 is not > safe_ball = 0 -> free
                    [5.0, 0.0, 0.0],     # val == dmax -> collision
                    [6.0, 9.0, 0.0],     # depth past dmax, whatever the angles
                    [1.0, 0.0, 0.0]], np.float32)
    for depth in (True, False):
        assert R.colcheck(img, pts, None, DMAX, HFOV, VFOV, 0, 0.0, depth, False).tolist() == [0, 0, 1, 1, 0]
        assert R.colcheck(img, pts, None, DMAX, HFOV, VFOV, 1, 0.0, depth, False).tolist() == [1, 0, 1, 1, 0]
    # extrapolate: the point behind is clamped to a border pixel; as a depth image val = x < 0 is before the wall
    assert R.colcheck(img, pts, None, DMAX, HFOV, VFOV, 2, 0.0, True, False).tolist() == [0, 0, 1, 1, 0]
    far_behind = np.array([[-3.0, 0.1, 0.0]], np.float32)  # as a range image val = |p| = 3 > d0
    assert R.colcheck(img, far_behind, None, DMAX, HFOV, VFOV, 2, 0.0, False, False)[0] == 1
    # a zero pixel always collides
    z = wall()
    z[:] = 0
    assert R.colcheck(z, pts[4:], None, DMAX, HFOV, VFOV, 0, 0.0, True, False)[0] == 1
    # range vs depth: |p| past dmax while x is not
    p = np.array([[3.0, 3.0, 3.0]], np.float32)
    assert R.colcheck(wall(4.9), p, None, DMAX, 1.2, 1.2, 0, 0.0, False, True)[0] == 1
    assert R.colcheck(wall(4.9), p, None, DMAX, 1.2, 1.2, 0, 0.0, True, True)[0] == 0


def test_pixel_mapping_and_p_to_i():
    """Each half of a split image is hit from its side; the explicit and the default point-to-image maps."""
    img = wall(n=2)
    img[0, :, : W // 2] = 1.0 / DMAX  # left half (positive azimuth: u < w/2) near
    img[1, : H // 2, :] = 1.0 / DMAX  # upper half (positive elevation) near
    pts = np.array([[1.5, 0.5, 0.0], [1.5, -0.5, 0.0], [1.5, 0.0, 0.3], [1.5, 0.0, -0.3]], np.float32)
    for sph in (False, True):
        assert R.colcheck(img, pts, [0, 0, 1, 1], DMAX, HFOV, VFOV, 0, 0.0, True, sph).tolist() == [1, 0, 1, 0]
        assert R.colcheck(img, pts, None, DMAX, HFOV, VFOV, 0, 0.0, True, sph).tolist() == [1, 0, 1, 0]
        assert R.colcheck(img, pts, [1, 1, 0, 0], DMAX, HFOV, VFOV, 0, 0.0, True, sph).tolist() == [0, 0, 0, 0]
    # margins: a point well inside a pixel and far from every threshold is decided; one at the wall is not
    lab, und = R.colcheck(wall(), on_axis(np.array([1.0, D0])) + np.float32([0, 0.013, 0.017]), None, DMAX, HFOV,
                          VFOV, 0, 0.0, True, False, margins=True)
    assert und.tolist() == [False, True]


def test_grid_shells():
    dist, grid, shells = R.dist_grid()
    assert shells == [4168, 3654, 2932, 3244, 3654]
    assert grid.shape == (17652, 3) and dist.shape == (17652,)
    assert dist.min() > 0 and dist.max() <= 1.0
    assert np.array_equal(dist, np.sqrt((grid * grid).sum(1)).astype(np.float32))


def test_classes_host_side():
    """What of ColChecker / DfComputer runs without a device: the constructor checks, the grid, the image
    rank rule."""
    from sdf_nmpc_amd.collision_checker import ColChecker, as_image_batch
    from sdf_nmpc_amd.df_computer import DfComputer
    with pytest.raises(AssertionError):
        ColChecker(DMAX, HFOV, VFOV, 0.0, outside="occupied")
    c = ColChecker(DMAX, HFOV, VFOV, 0.1, outside="extrapolate")
    assert c.outside == 2 and ColChecker(DMAX, HFOV, VFOV, 0.1).outside == 0
    assert as_image_batch(np.zeros((H, W), np.float32)).shape == (1, H, W)
    assert as_image_batch(np.zeros((3, H, W), np.float32)).shape == (3, H, W)
    for bad in (np.zeros(7, np.float32), np.zeros((1, 1, H, W), np.float32)):
        with pytest.raises(AssertionError):
            as_image_batch(bad)
    d = DfComputer(True, DMAX, HFOV, VFOV, 2.5, batch_size=17)
    assert (d.min_df, d.max_df) == (-0.3, 1)  # whatever max_df is passed (df_computer.py:16-17)
    dist, grid, _ = R.dist_grid()
    assert d.grid.shape == (17652, 3)
    assert np.array_equal(d.grid.numpy(), grid)
    assert np.abs(d.distances.numpy() - dist).max() <= 2 ** -23  # torch's norm and sqrt(sum) differ by an ulp
    g, ds, orig = d._sorted
    assert np.all(np.diff(ds.numpy()) >= 0)
    assert np.array_equal(g.numpy(), grid[orig.numpy()])
    same = np.diff(ds.numpy()) == 0
    assert np.all(np.diff(orig.numpy().astype(np.int64))[same] > 0)  # stable: ties keep the original order
    assert not hasattr(DfComputer(False, DMAX, HFOV, VFOV, 1.0), "grid")
