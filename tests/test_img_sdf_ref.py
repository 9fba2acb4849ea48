"""The numpy restatement of the image field as the SDF row (tests/img_sdf_ref.py), the yardstick of
tests/test_gpu_img_sdf.py, on rows whose answer can be derived by hand: the wall of tests/test_df_truth.py at depth d0,
seen through a camera that is yawed by 90 degrees and translated, so that the camera's x axis is the world's y axis and a
world gradient is the camera gradient rotated."""
import numpy as np

import df_truth_ref as R
import img_sdf_ref as S

DMAX, HFOV, VFOV = 5.0, 0.7592, 0.4903  # config/default.yaml sensor
H, W = 30, 40
D0 = 2.5
NP = 17
SIGNED = (DMAX, HFOV, VFOV, True, False)    # the sensor of test_df_truth.test_wall_signed_field
UNSIGNED = (DMAX, HFOV, VFOV, True, True)   # and of test_wall_udf_is_distance_to_the_wall (the pinhole branch, sic)
W_P_CO = np.array([1.0, -2.0, 0.5])
W_R_CO = np.array([[0.0, -1.0, 0.0], [1.0, 0.0, 0.0], [0.0, 0.0, 1.0]])  # Rz(90 deg): camera x = world y


def wall(d0=D0, n=1):
    return np.full((n, H, W), d0 / DMAX, np.float32)


def rows(cam_pts, flags, B=1):
    """x, p [B, n, .] whose world positions are the camera-frame points cam_pts [n][3] seen through the pose; every other
    entry of x and p is noise the field must not read."""
    cam_pts = np.asarray(cam_pts, float)
    n = len(cam_pts)
    rng = np.random.default_rng(1)
    x = rng.normal(0, 1, (B, n, 10))
    p = rng.normal(0, 1, (B, n, NP))
    x[..., :3] = W_P_CO + cam_pts @ W_R_CO.T
    p[..., 0] = flags
    p[..., 1:4] = W_P_CO
    p[..., 4:13] = W_R_CO.ravel()
    return x, p


def step(d):  # the voxel pitch of the shell a distance d falls in
    return next(s for lo, hi, s in R.GRID_PARAMS if lo < d <= hi)


def test_camera_frame_point_undoes_the_pose():
    cam = np.array([[2.3, 0.1, -0.2], [0.5, -0.3, 0.4]])
    x, p = rows(cam, 1.0)
    pts, exact = S.cam_points(x, p)
    assert pts.dtype == np.float32 and np.abs(exact[0] - cam).max() < 1e-15
    assert np.array_equal(pts, exact.astype(np.float32))
    assert np.allclose(x[0, 0, :3], [1.0 - 0.1, -2.0 + 2.3, 0.5 - 0.2])  # camera x along world y, camera y along world -x


def test_signed_rows_against_the_wall():
    dist, grid, _ = R.dist_grid()
    #        free, 0.2 before   0.6 behind        1.5 before: nothing within max_df   flag 0          flag 0.5
    cam = [[D0 - 0.2, 0, 0], [D0 + 0.6, 0, 0], [D0 - 1.5, 0, 0], [D0 - 0.2, 0, 0], [D0 - 0.2, 0, 0]]
    x, p = rows(cam, [1.0, 1.0, 1.0, 0.0, 0.5])
    h2, J2, pts = S.sdf_rows(wall(), x, p, SIGNED, True, 1.0, grid=grid, dist=dist)
    assert np.allclose(pts[0], cam, atol=1e-6)
    d = 0.2
    assert d - 1e-6 <= h2[0, 0] <= d + step(d + step(d)) + 1e-6   # d0 - x to one voxel step
    assert np.allclose(J2[0, 0, :3], W_R_CO @ [-1.0, 0.0, 0.0], atol=1e-6)  # the rotated -x: world (0, -1, 0)
    assert np.allclose(J2[0, 0, :3], [0.0, -1.0, 0.0], atol=1e-6)
    assert h2[0, 1] == np.float64(np.float32(-0.3)) and not J2[0, 1].any()   # behind: clamped at min_df, gradient 0
    assert h2[0, 2] == 1.0 and not J2[0, 2].any()                            # beyond max_df
    assert h2[0, 3] == 1.0 and not J2[0, 3].any()                            # flag 0: max_df, no gradient
    assert h2[0, 4] == 0.5 * h2[0, 0] + 0.5 * 1.0                            # flag 0.5 blends value and max_df
    assert np.array_equal(J2[0, 4], 0.5 * J2[0, 0])
    assert not J2[..., 3:].any()                                             # only the position columns
    # the field in fp32, as the kernel evaluates it, gives the same rows here
    h32, J32, _ = S.sdf_rows(wall(), x, p, SIGNED, True, 1.0, grid=grid, dist=dist, dtype=np.float32)
    assert np.allclose(h32, h2, atol=1e-6) and np.allclose(J32, J2, atol=1e-6)
    # columns 0 and 1 of h and Jh are not written
    h, Jh = S.write_rows(np.full((1, 5, 3), np.nan), np.full((1, 5, 10, 3), np.nan), h2, J2)
    assert np.isnan(h[..., :2]).all() and np.isnan(Jh[..., :2]).all()
    assert np.isfinite(h[..., 2]).all() and np.isfinite(Jh[..., 2]).all()


def test_unsigned_rows_and_the_virtual_wall():
    cam = [[D0 - 0.4, 0, 0], [4.8, 0, 0], [0.2, 0, 0]]
    x, p = rows(cam, [1.0, 1.0, 1.0])
    h2, J2, _ = S.sdf_rows(wall(), x, p, UNSIGNED, False, 1.0)
    assert abs(h2[0, 0] - 0.4) < 1e-6 and np.allclose(J2[0, 0, :3], [0.0, -1.0, 0.0], atol=1e-6)
    # past the wall the virtual wall at dmax is closer than every pixel: dmax - x, the reference's direction (dmax, y, z)
    assert abs(h2[0, 1] - 0.2) < 1e-6 and np.allclose(J2[0, 1, :3], W_R_CO @ [-1.0, 0.0, 0.0], atol=1e-6)
    assert h2[0, 2] == 1.0 and not J2[0, 2].any()  # farther than max_df from everything
    assert S.decided(wall(), x, p, UNSIGNED, signed=False).all()


def test_two_instances_read_their_own_image_through_img_of():
    dist, grid, _ = R.dist_grid()
    imgs = np.concatenate([wall(D0), wall(3.5)])
    x, p = rows([[D0 - 0.2, 0, 0]], 1.0, B=2)
    a, _, _ = S.sdf_rows(imgs, x, p, SIGNED, True, 1.0, grid=grid, dist=dist)
    b, _, _ = S.sdf_rows(imgs, x, p, SIGNED, True, 1.0, img_of=[1, 0], grid=grid, dist=dist)
    assert 0.2 - 1e-6 <= a[0, 0] <= 0.2 + step(0.2 + step(0.2)) + 1e-6 and a[1, 0] == 1.0  # the far wall: 1.2 m away
    assert b[0, 0] == a[1, 0] and b[1, 0] == a[0, 0]


def frustum_rows(n, seed):
    """n world points uniform in the viewing frustum after the pose, as rows of one instance"""
    rng = np.random.default_rng(seed)
    xc = rng.uniform(0.2, 4.8, n)
    cam = np.stack([xc, xc * np.tan(HFOV) * rng.uniform(-1, 1, n), xc * np.tan(VFOV) * rng.uniform(-1, 1, n)], 1)
    return rows(cam, 1.0)


def pillar_image():
    """a wall at 4 m with a pillar at 1.5 m over a third of the columns: piecewise constant, as a rendered scene is"""
    img = wall(4.0)
    img[:, :, 14:25] = 1.5 / DMAX
    return img


def test_decided_share_of_the_reference():
    """The undecided share of the reference alone, capped at 1 % as in test_gpu_df_truth.py: 2,000 points by the point's
    rule, and the voxels of the first 48 of them by the same margins (measured 0.70 % and 0.35 %)."""
    dist, grid, _ = R.dist_grid()
    img = pillar_image()
    x, p = frustum_rows(2000, seed=5)
    dec = S.decided(img, x, p, SIGNED)
    share = 1.0 - dec.mean()
    pts, _ = S.cam_points(x[0, :48], p[0, :48])
    occ, occ_und, counting, vox_und = R.sdf_sets(img, pts, np.zeros(48, int), grid, *SIGNED)
    print(f"\nundecided: {share:.4%} of 2000 points, {vox_und.mean():.4%} of the voxels of 48; occupied {occ.mean():.2f}")
    assert share <= 0.01 and vox_und.mean() <= 0.01
    assert 0.05 < occ.mean() < 0.95 and counting.any(1).mean() > 0.2  # free and occupied points, and rows near a surface
