"""numpy restatement of the image field as the SDF row (csrc/df_truth.hip: img_sdf_rows_kernel; helper module of
test_img_sdf_ref.py and test_gpu_img_sdf.py), built on df_truth_ref.py:

  cam_points   Co_p_B = W_R_Co^T (x[0:3] - W_p_Co) in fp64 from each row's own parameters, in the association of the
               network kernels ((e0 R0j + e1 R1j) + e2 R2j), rounded to fp32
  field        df_truth_ref.sdf / udf per row with p_to_i = the instance's image
  epilogue     h2 = flag df + (1 - flag) max_df, J2[j] = flag ((R[j][0] g0 + R[j][1] g1) + R[j][2] g2) (j < 3), 0 (j = 3..9)
               in fp64 on the widened fp32 values (numpy never fuses a multiply-add)
  decided      df_truth_ref's decided rule for the point: the collision label that gives the signed field its sign
               went through no comparison that fp32 rounding could flip (the unsigned field has no such label)
"""
import numpy as np

import df_truth_ref as R

MIN_DF = R.MIN_DF
CHUNK = 64  # rows per df_truth_ref.sdf call: its points x voxels arrays stay under ~30 MB each


def cam_points(x, p):
    """x [..., 10], p [..., np] -> (pts float32 [..., 3], the same before rounding, float64)"""
    x, p = np.asarray(x, np.float64), np.asarray(p, np.float64)
    e = x[..., :3] - p[..., 1:4]
    Rm = p[..., 4:13].reshape(p.shape[:-1] + (3, 3))
    c = np.stack([(e[..., 0] * Rm[..., 0, j] + e[..., 1] * Rm[..., 1, j]) + e[..., 2] * Rm[..., 2, j] for j in range(3)], -1)
    return c.astype(np.float32), c


def epilogue(flag, df, g, Rm, max_df):
    """flag [...], df [...] and g [..., 3] float32, Rm [..., 3, 3] = W_R_Co -> h2 [...], J2 [..., 10] float64"""
    flag, d, g = np.asarray(flag, np.float64), np.asarray(df, np.float32).astype(np.float64), np.asarray(g, np.float32).astype(np.float64)
    h2 = flag * d + (1.0 - flag) * np.float64(np.float32(max_df))
    J = np.zeros(flag.shape + (10,))
    for j in range(3):
        J[..., j] = flag * ((Rm[..., j, 0] * g[..., 0] + Rm[..., j, 1] * g[..., 1]) + Rm[..., j, 2] * g[..., 2])
    return h2, J


def _img_index(B, N1, img_of):
    return np.repeat(np.arange(B) if img_of is None else np.asarray(img_of), N1)


def field(imgs, pts, p_to_i, sensor, signed, max_df, grid=None, dist=None, dtype=np.float64):
    """(df [n], grad [n][3]) of df_truth_ref for points pts [n][3] float32; sensor = (dmax, hfov, vfov, is_depth,
    is_spherical)."""
    dmax, hfov, vfov, depth, sph = sensor
    if not signed:
        return R.udf(imgs, pts, p_to_i, dmax, hfov, vfov, depth, sph, max_df, dtype)[:2]
    out = [R.sdf(imgs, pts[i:i + CHUNK], p_to_i[i:i + CHUNK], grid, dist, dmax, hfov, vfov, depth, sph, MIN_DF, max_df, dtype)
           for i in range(0, len(pts), CHUNK)]
    return np.concatenate([o[0] for o in out]), np.concatenate([o[1] for o in out])


def sdf_rows(imgs, x, p, sensor, signed=True, max_df=R.MAX_DF, img_of=None, grid=None, dist=None, dtype=np.float64):
    """x [B, N+1, 10], p [B, N+1, np] -> h2 [B, N+1], J2 [B, N+1, 10], pts float32 [B, N+1, 3].  The field is evaluated in
    ``dtype`` and rounded to fp32 before the epilogue, as the kernel hands it over."""
    x, p = np.asarray(x, np.float64), np.asarray(p, np.float64)
    B, N1 = x.shape[:2]
    pts, _ = cam_points(x, p)
    df, g = field(imgs, pts.reshape(-1, 3), _img_index(B, N1, img_of), sensor, signed, max_df, grid, dist, dtype)
    Rm = p[..., 4:13].reshape(B, N1, 3, 3)
    h2, J = epilogue(p[..., 0], df.astype(np.float32).reshape(B, N1), g.astype(np.float32).reshape(B, N1, 3), Rm, max_df)
    return h2, J, pts


def decided(imgs, x, p, sensor, signed=True, img_of=None):
    """[B, N+1] bool: the row's point is decided (df_truth_ref.colcheck's margins in mode extrapolate with safe ball 0,
    the label sdf takes its sign from); every row of the unsigned field is."""
    x = np.asarray(x, np.float64)
    B, N1 = x.shape[:2]
    if not signed:
        return np.ones((B, N1), bool)
    dmax, hfov, vfov, depth, sph = sensor
    pts, _ = cam_points(x, p)
    _, und = R.colcheck(imgs, pts.reshape(-1, 3), _img_index(B, N1, img_of), dmax, hfov, vfov, 2, 0.0, depth, sph,
                        np.float64, margins=True)
    return ~und.reshape(B, N1)


def write_rows(h, Jh, h2, J2):
    """What the kernel writes: column 2 of h [B, N+1, 3] and of Jh [B, N+1, 10, 3], nothing else."""
    h[..., 2] = h2
    Jh[..., 2] = J2
    return h, Jh
