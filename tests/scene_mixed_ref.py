"""The composition rule of a mixed scene (sdfnmpc_scene_create_mixed, csrc/scene_grid.hip's *_mixed kernels) in numpy:
a mixed scene M = (statics, movers) answers every query with the minimum over both sets at the query's time, so it is
specified by two scenes that existing kernels answer -- G, the indexed static set, and D, the movers as a dynamic set
of their own -- and by how their answers combine:

  render     min(G-image, D-image) pixel by pixel.  A pixel is fmin(hit cx, dmax) scale (depth) or fmin(hit, dmax) scale
             (range) with cx > 0 for half-fields below pi / 2: non-decreasing in the hit, so the image of the nearer
             hit is the smaller image.
  distance   min(G-distance, D-distance at the point's time)
  rows       D's (h, J_h) where D's h is strictly below G's, else G's: on a tie a static primitive comes before a mover
             (within each set the kernels' own rule holds, the lowest index)

`sdf_rows` is the same rule from the geometry (tests/scene_sdf_ref.py), for flags that are neither 0 nor 1."""
import numpy as np

import scene_dyn_ref as D
import scene_sdf_ref as S


def to_ref(prims):
    """Primitives as sdf_nmpc_amd.scene.Scene takes them (plain, or Scene.moving's with q as a list) -> as the
    references take them (scene_dyn_ref.moving's, with the orientation as a matrix)"""
    return [D.moving((pr[0], pr[1]), v=pr[2]["v"], q=pr[2]["q"], yaw_rate=pr[2]["yaw_rate"], amp=pr[2]["amp"],
                     omega=pr[2]["omega"], phase=pr[2]["phase"]) if len(pr) > 2 else (pr[0], list(pr[1])) for pr in prims]


def render(g_img, d_img):
    return np.minimum(g_img, d_img)


def distance(g_dist, d_dist):
    return np.minimum(g_dist, d_dist)


def rows(g_h, g_J, d_h, d_J):
    """h [...], J [..., 10] of the mixed scene from those of G and D"""
    lower = d_h < g_h  # strictly: the static set keeps a tie
    return np.where(lower, d_h, g_h), np.where(lower[..., None], d_J, g_J)


def dist_grad(statics, movers, pts, t=0.0):
    """Untruncated distance [n] and world gradient [n, 3] of the mixed scene, point j at time t or t[j]; statics and
    movers as Scene takes them"""
    gs, gg, _ = S.dist_grad(to_ref(statics), pts)
    ds, dg, _ = S.dist_grad(to_ref(movers), pts, t)
    lower = ds < gs
    return np.where(lower, ds, gs), np.where(lower[:, None], dg, gg)


def sdf_rows(statics, movers, x, p, max_df, t0=0.0, tau=None):
    """scene_sdf_ref.sdf_rows for the mixed scene: column 2 of h [..., N+1] and of J_h [..., N+1, 10]"""
    x, p = np.asarray(x, float), np.asarray(p, float)
    lead = x.shape[:-1]
    d, g = dist_grad(statics, movers, x[..., :3].reshape(-1, 3), S._times(lead, t0, tau).ravel())
    near = d < max_df
    df = np.where(near, d, max_df).reshape(lead)
    g = np.where(near[:, None], g, 0.0).reshape(lead + (3,))
    flag = p[..., 0]
    J = np.zeros(lead + (10,))
    J[..., :3] = flag[..., None] * g
    return flag * df + (1.0 - flag) * max_df, J


# the constructed tie of the tests: a node at the origin between a static sphere and a mover that passes x = 2 at t = 0
TIE_STATIC = ("sphere", [-2.0, 0.0, 0.0, 1.0])
TIE_MOVER = ("sphere", [2.0, 0.0, 0.0, 1.0], dict(q=[1.0, 0.0, 0.0, 0.0], v=[-0.5, 0.0, 0.0], amp=[0.0, 0.0, 0.0],
                                                  yaw_rate=0.0, omega=0.0, phase=0.0))
TIE_T_NEARER = 0.5  # the mover's centre at x = 1.75: 0.75 from the origin
