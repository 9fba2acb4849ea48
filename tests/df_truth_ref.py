"""numpy restatement of the reference's image ground truth (helper module of test_df_truth.py and
test_gpu_df_truth.py), callable in float32 or float64:

  colcheck   utils/collision_checker.py:47-90   with the decision margins of the GPU tests
  minpool5   utils/df_computer.py:154-162
  udf        utils/df_computer.py:102-149,177-180
  sdf        utils/df_computer.py:200-221       with the "counting voxel" sets
  dist_grid  utils/df_computer.py:33-57

Inputs are taken as the float32 numbers the kernels see (images, points, grid, and the scalars dmax, hfov,
vfov rounded to float32); ``dtype`` is the precision of the arithmetic on them.

Decision margins (colcheck(..., margins=True) returns (label, undecided)).  A label is a chain of
comparisons; it is *decided* when no comparison it went through is close enough to flip under fp32 rounding:
  * | |p| - safe_ball |, | val - dmax | and | val - thr | above 1e-5 dmax (fp32 rounding of lengths and of
    thr = pixel * dmax at this scale is ~1e-7 dmax: two orders of slack),
  * outside the extrapolate mode, each angle more than 1e-5 rad from its limit (atan2f: ~1e-7),
  * each unclamped pixel coordinate more than 1e-3 from the integers 1 .. size-1, the boundaries between
    two pixels (coordinates near 0 or >= size-1 land on the same border pixel after int() and the clamp on
    either side, so those integers decide nothing; w/2 (1 - tan az / tan hfov) carries ~1e-5 px of fp32 error
    at w = 480).
"""
import numpy as np

GRID_PARAMS = [(0, 0.1, 0.01), (0.1, 0.2, 0.02), (0.2, 0.3, 0.03), (0.3, 0.5, 0.05), (0.5, 1, 0.1)]  # df_computer.py:27
MIN_DF, MAX_DF = -0.3, 1.0  # df_computer.py:16-17
OUTSIDE = {"free": 0, "col": 1, "extrapolate": 2}


def _scalars(dtype, *vals):
    return [dtype(np.float32(v)) for v in vals]


def default_p_to_i(n, n_img):
    assert n % n_img == 0
    return np.arange(n) // (n // n_img)


def colcheck(img, points, p_to_i, dmax, hfov, vfov, outside, safe_ball, is_depth, is_spherical, dtype=np.float64,
             margins=False):
    """img [n_img][H][W], points [..., 3], p_to_i [...] (None: default ordering) -> uint8 labels [...]
    (and the undecided mask)."""
    img = np.asarray(img, np.float32)
    P = np.asarray(points, np.float32).astype(dtype)
    if p_to_i is None:
        p_to_i = default_p_to_i(P.shape[0], img.shape[0])
    p_to_i = np.asarray(p_to_i)
    dmax, hfov, vfov, safe_ball = _scalars(dtype, dmax, hfov, vfov, safe_ball)
    H, W = img.shape[1:]
    h, w, one, two = dtype(H), dtype(W), dtype(1), dtype(2)
    x, y, z = P[..., 0], P[..., 1], P[..., 2]
    with np.errstate(all="ignore"):
        ln = np.sqrt(x * x + y * y + z * z)
        val = x if is_depth else ln
        az = np.arctan2(y, x)
        el = np.arctan2(z, np.sqrt(x * x + y * y)) if is_spherical else np.arctan2(z, x)
        if outside == 2:
            az = np.clip(az, -hfov, hfov)
            el = np.clip(el, -vfov, vfov)
            out_fov = np.zeros(x.shape, bool)
        else:
            out_fov = (np.abs(az) >= hfov) | (np.abs(el) >= vfov)
        if is_spherical:
            fu = w / two * (one - az / hfov)
            fv = h / two * (one - el / vfov)
        else:
            fu = w / two * (one - np.tan(az) / np.tan(hfov))
            fv = h / two * (one - np.tan(el) / np.tan(vfov))
        u = np.clip(np.trunc(np.nan_to_num(fu, nan=0.0, posinf=1e9, neginf=-1e9)), 0, W - 1).astype(np.int64)
        v = np.clip(np.trunc(np.nan_to_num(fv, nan=0.0, posinf=1e9, neginf=-1e9)), 0, H - 1).astype(np.int64)
        thr = img[p_to_i, v, u].astype(dtype) * dmax
        in_ball = ~(ln > safe_ball)
        past = val >= dmax
        lab = np.where(in_ball, 0, np.where(past, 1, np.where(out_fov, int(outside == 1), val >= thr)))
        lab = lab.astype(np.uint8)
        if not margins:
            return lab
        eps = dtype(1e-5) * dmax
        und = np.abs(ln - safe_ball) <= eps
        s1 = ~in_ball  # reached the dmax test
        und |= s1 & (np.abs(val - dmax) <= eps)
        s2 = s1 & ~past  # reached the angles
        if outside != 2:
            und |= s2 & ((np.abs(np.abs(az) - hfov) <= 1e-5) | (np.abs(np.abs(el) - vfov) <= 1e-5))
        s3 = s2 & ~out_fov  # reached the pixel
        for f, size in ((fu, W), (fv, H)):
            r = np.rint(f)
            und |= s3 & (np.abs(f - r) <= 1e-3) & (r >= 1) & (r <= size - 1)
        und |= s3 & (np.abs(val - thr) <= eps)
    return lab, und


def minpool5(imgs, dmax):
    """[n_img][H][W] -> [n_img][H/5][W/5]: the minimum with zeros replaced by dmax (as written: the
    unnormalised dmax), 0 for an all-zero block."""
    imgs = np.asarray(imgs, np.float32)
    B, H, W = imgs.shape
    assert H % 5 == 0 and W % 5 == 0
    blk = imgs.reshape(B, H // 5, 5, W // 5, 5).transpose(0, 1, 3, 2, 4).reshape(B, H // 5, W // 5, 25)
    filled = np.where(blk == 0, np.float32(dmax), blk)
    return np.where((blk != 0).any(-1), filled.min(-1), np.float32(0)).astype(np.float32)


def udf_pixels(pooled, points, p_to_i, dmax, hfov, vfov, is_depth, is_spherical, dtype=np.float64):
    """Per point and pooled pixel: the distance [n][h w] and the direction [n][h w][3] (df_computer.py:102-149)."""
    pooled = np.asarray(pooled, np.float32)
    P = np.asarray(points, np.float32).astype(dtype)
    if p_to_i is None:
        p_to_i = default_p_to_i(P.shape[0], pooled.shape[0])
    dmax, hfov, vfov = _scalars(dtype, dmax, hfov, vfov)
    h_, w_ = pooled.shape[1:]
    h, w, one, two = dtype(h_), dtype(w_), dtype(1), dtype(2)
    fi = one - two * np.arange(w_).astype(dtype) / w
    fj = one - two * np.arange(h_).astype(dtype) / h
    if is_spherical:  # sic: the pinhole direction
        X = np.ones((h_, w_), dtype)
        Y = np.broadcast_to((np.tan(hfov) * fi)[None, :], (h_, w_))
        Z = np.broadcast_to((np.tan(vfov) * fj)[:, None], (h_, w_))
    else:
        az, el = hfov * fi, vfov * fj
        X = np.cos(el)[:, None] * np.cos(az)[None, :]
        Y = np.cos(el)[:, None] * np.sin(az)[None, :]
        Z = np.broadcast_to(np.sin(el)[:, None], (h_, w_))
    D = np.stack([X, Y, Z], -1).reshape(1, h_ * w_, 3).astype(dtype)
    s = pooled[np.asarray(p_to_i)].reshape(P.shape[0], h_ * w_, 1).astype(dtype)
    rel = D * s * dmax - P[:, None, :]
    d_p = np.sqrt((rel * rel).sum(-1))
    d_bg = dmax - (P[:, 0] if is_depth else np.sqrt((P * P).sum(-1)))
    wall = d_p > d_bg[:, None]
    dist = np.where(wall, d_bg[:, None], d_p)
    wall_dir = np.stack([np.full(P.shape[0], dmax, dtype), P[:, 1], P[:, 2]], -1)
    dirs = np.where(wall[..., None], wall_dir[:, None, :], rel)
    return dist, dirs


def udf_from_pixel(dist, dirs, idx, max_df=MAX_DF):
    """The epilogue (df_computer.py:177-180) for the pixel idx [n] of each point."""
    n = np.arange(dist.shape[0])
    dt = dist.dtype.type
    udf = np.clip(dist[n, idx], dt(0), dt(max_df))
    g = dirs[n, idx]
    with np.errstate(all="ignore"):
        grad = -np.where((udf == dt(max_df))[:, None], dt(0), g / np.sqrt((g * g).sum(-1))[:, None])
    return udf, grad


def udf(imgs, points, p_to_i, dmax, hfov, vfov, is_depth, is_spherical, max_df=MAX_DF, dtype=np.float64):
    """get_udf: (udf [n], grad [n][3], pixel index [n]); ties go to the lowest pixel index (np.argmin)."""
    dist, dirs = udf_pixels(minpool5(imgs, dmax), points, p_to_i, dmax, hfov, vfov, is_depth, is_spherical, dtype)
    idx = dist.argmin(1)
    return udf_from_pixel(dist, dirs, idx, max_df) + (idx,)


def dist_grid(grid_params=GRID_PARAMS, dtype=np.float32):
    """generate_dist_grid (df_computer.py:33-57): (distances [G], grid [G][3], shell sizes)."""
    dists, grids, shells = [], [], []
    for dmin, dmx, step in grid_params:
        nb = int(2.0 * dmx / step) + 1
        c = np.linspace(-dmx, dmx, nb).astype(dtype)
        g = np.stack([np.tile(c, nb * nb), np.tile(np.repeat(c, nb), nb), np.repeat(c, nb * nb)], 1)
        d = np.sqrt((g * g).sum(1)).astype(dtype)
        keep = (d > dtype(dmin)) & (d <= dtype(dmx))
        grids.append(g[keep])
        dists.append(d[keep])
        shells.append(int(keep.sum()))
    return np.concatenate(dists), np.concatenate(grids), shells


def sdf_sets(imgs, points, p_to_i, grid, dmax, hfov, vfov, is_depth, is_spherical, dtype=np.float64):
    """Per point: its collision label and whether it is undecided; per point and voxel: whether the voxel
    counts (its label differs from the point's) and whether the voxel's label is undecided.  The voxel point is
    fl32(p + grid[g]) in every precision; mode extrapolate, safe ball 0 (df_computer.py:22,188,213)."""
    imgs = np.asarray(imgs, np.float32)
    P = np.asarray(points, np.float32)
    grid = np.asarray(grid, np.float32)
    if p_to_i is None:
        p_to_i = default_p_to_i(P.shape[0], imgs.shape[0])
    p_to_i = np.asarray(p_to_i)
    occ, occ_und = colcheck(imgs, P, p_to_i, dmax, hfov, vfov, 2, 0.0, is_depth, is_spherical, dtype, margins=True)
    VP = (P[:, None, :] + grid[None, :, :]).astype(np.float32)
    vox, vox_und = colcheck(imgs, VP, np.broadcast_to(p_to_i[:, None], VP.shape[:2]), dmax, hfov, vfov, 2, 0.0,
                            is_depth, is_spherical, dtype, margins=True)
    return occ, occ_und, vox != occ[:, None], vox_und


def sdf_from_voxel(occ, found, dist_at, grid_at, min_df=MIN_DF, max_df=MAX_DF, dtype=np.float64):
    """The epilogue (df_computer.py:217-219) given each point's voxel: its distance and offset (ignored where
    not found)."""
    sign = (1 - 2 * occ.astype(np.int64)).astype(dtype)
    mind = np.where(found, np.asarray(dist_at).astype(dtype), dtype(max_df))
    sdf = np.clip(sign * mind, dtype(min_df), dtype(max_df))
    g = np.asarray(grid_at).astype(dtype)
    with np.errstate(all="ignore"):
        gd = g / np.sqrt((g * g).sum(-1))[:, None]
    sat = ~found | (sdf == dtype(min_df)) | (sdf == dtype(max_df))
    grad = -sign[:, None] * np.where(sat[:, None], dtype(0), gd)
    return sdf, grad + dtype(0)


def sdf(imgs, points, p_to_i, grid, dist, dmax, hfov, vfov, is_depth, is_spherical, min_df=MIN_DF, max_df=MAX_DF,
        dtype=np.float64):
    """get_sdf by its definition: (sdf [n], grad [n][3], voxel index [n], -1 where no voxel counts); ties go to
    the lowest voxel index."""
    occ, _, counting, _ = sdf_sets(imgs, points, p_to_i, grid, dmax, hfov, vfov, is_depth, is_spherical, dtype)
    dist = np.asarray(dist, np.float32)
    d = np.where(counting, dist[None, :], np.float32(np.inf))
    idx = d.argmin(1)
    found = counting.any(1)
    out = sdf_from_voxel(occ, found, dist[idx], np.asarray(grid, np.float32)[idx], min_df, max_df, dtype)
    return out + (np.where(found, idx, -1),)
