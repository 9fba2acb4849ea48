"""tests/scene_sdf_ref.py, the reference of csrc/scene_sdf.hip, pinned on the CPU: to answers derivable by hand, to the
distances of scene_ref / scene_dyn_ref (1e-12, DESIGN §3.15's bar for scene_distance), and its `decided` mask to the cap
the GPU tests rely on (at most 1 % of a test's rows undecided)."""
import numpy as np
import pytest

import scene_dyn_ref as D
import scene_ref as R
import scene_sdf_ref as S

BOX = ("box", [1.0, -1.0, -1.0, 2.0, 1.0, 1.0])
SPHERE = ("sphere", [0.0, 0.0, 0.0, 1.0])
CYL = ("cylinder", [0.0, 0.0, 1.0, -1.0, 1.0])
MAX_DF = 1.0


def row(prims, pt, flag=1.0, max_df=MAX_DF, **kw):
    """h2 and J_h2 of one node row at the point pt"""
    x = np.zeros((1, 1, 10))
    x[0, 0, :3] = pt
    p = np.zeros((1, 1, 17))
    p[..., 0] = flag
    h, J = S.sdf_rows(prims, x, p, max_df, **kw)
    assert h.shape == (1, 1) and J.shape == (1, 1, 10)
    return h[0, 0], J[0, 0]


@pytest.mark.parametrize("prims, pt, d, g", [
    ([BOX], (0.5, 0.0, 0.0), 0.5, (-1.0, 0.0, 0.0)),          # 0.5 m in front of the face x = 1
    ([BOX], (0.7, -1.4, 0.0), 0.5, (-0.6, -0.8, 0.0)),        # on the diagonal of the edge x = 1, y = -1: (0.3, 0.4)
    ([SPHERE], (0.0, 0.25, 0.0), -0.75, (0.0, 1.0, 0.0)),     # inside a sphere
    ([CYL], (1.3, 0.0, 1.4), 0.5, (0.6, 0.0, 0.8)),           # off the rim rho = 1, z = 1: (0.3, 0.4)
    ([BOX], (1.5, 0.2, 0.9), -0.1, (0.0, 0.0, 1.0)),          # inside a box: the nearest face is z = 1
    ([CYL], (0.0, 0.0, 0.0), -1.0, (1.0, 0.0, 0.0)),          # on the axis at mid height: the tie goes to e_rho
    ([SPHERE], (0.0, 0.0, 0.0), -1.0, (0.0, 0.0, 1.0)),       # the centre of a sphere
])
def test_hand_derived_rows(prims, pt, d, g):
    h, J = row(prims, pt)  # 1e-15: a few ulp of coordinates of size 1 that are not binary fractions (0.7, 1.4)
    assert abs(h - d) <= 1e-15
    np.testing.assert_allclose(J[:3], g, rtol=0, atol=1e-15)
    assert not J[3:].any()


def test_truncation_and_flag():
    h, J = row([BOX], (-0.5, 0.0, 0.0))             # 1.5 m away: beyond max_df
    assert h == MAX_DF and not J.any()
    h, J = row([], (0.0, 0.0, 0.0))                 # an empty scene
    assert h == MAX_DF and not J.any()
    h, J = row([BOX], (0.5, 0.0, 0.0), flag=0.0)    # flag 0: the row is switched off
    assert h == MAX_DF and not J.any()
    h, J = row([BOX], (0.5, 0.0, 0.0), flag=0.5)
    assert h == 0.5 * 0.5 + 0.5 * MAX_DF
    np.testing.assert_array_equal(J, [-0.5, 0, 0, 0, 0, 0, 0, 0, 0, 0])
    h, J = row([BOX, SPHERE], (0.5, 0.0, 0.0))      # the minimum over the primitives: the sphere is at -0.5
    assert h == -0.5 and tuple(J[:3]) == (1.0, 0.0, 0.0)


def test_moving_primitive_and_node_times():
    """A sphere moving along y: node k sees it at t0 + tau[k]; the gradient turns with an oriented box."""
    prims = [D.moving(SPHERE, v=(0.0, 1.0, 0.0))]
    x = np.zeros((1, 3, 10))
    x[..., 0] = 1.5
    p = np.ones((1, 3, 17))
    h, J = S.sdf_rows(prims, x, p, 5.0, t0=0.0, tau=np.array([0.0, 2.0, -2.0]))
    np.testing.assert_allclose(h[0], [0.5, 1.5, 1.5], rtol=0, atol=1e-15)
    np.testing.assert_allclose(J[0, :, :3], [[1, 0, 0], [0.6, -0.8, 0], [0.6, 0.8, 0]], rtol=0, atol=1e-15)
    h0, _ = S.sdf_rows(prims, x, p, 5.0, t0=2.0)    # without tau every node at t0
    np.testing.assert_allclose(h0[0], 1.5, rtol=0, atol=1e-15)
    box = [D.moving(("box", [-1.0, -1.0, -1.0, 1.0, 1.0, 1.0]), rpy=(0.0, 0.0, np.pi / 4))]
    c = np.sqrt(0.5)
    h, J = row(box, (2.0 * c, 2.0 * c, 0.0), max_df=5.0)  # on the rotated x axis, 1 m off the face
    assert abs(h - 1.0) <= 1e-15
    np.testing.assert_allclose(J[:3], [c, c, 0.0], rtol=0, atol=1e-15)


CASES = [("static", R.SCENE, 0.0), ("dyn 0.7", D.scene(), 0.7), ("dyn 2.3", D.scene(), 2.3)]


@pytest.mark.parametrize("name, prims, t", CASES, ids=[c[0] for c in CASES])
def test_pinned_to_scene_distance_and_decided_cap(name, prims, t):
    pts = S.draw(4000, seed=5)
    x = np.zeros((4000, 1, 10))
    x[:, 0, :3] = pts
    p = np.ones((4000, 1, 17))
    want = D.distance(prims, pts, t) if t else R.distance(prims, pts)
    d, g, _ = S.dist_grad(prims, pts, t)
    assert np.abs(d - want).max() <= 1e-12
    assert np.isfinite(g).all() and np.linalg.norm(g, axis=1).max() <= 1.0 + 1e-12
    h, J = S.sdf_rows(prims, x, p, MAX_DF, t0=t)
    assert np.abs(h[:, 0] - np.minimum(want, MAX_DF)).max() <= 1e-12
    assert not J[:, 0][want >= MAX_DF].any()
    # the fixture covers what the GPU tests need: points inside a primitive, near one and beyond the truncation
    assert (want < 0).mean() > 0.005 and 0.2 < (want < MAX_DF).mean() < 0.8
    und = 1.0 - S.decided(prims, x, MAX_DF, t0=t).mean()
    print(f"{name}: {100 * und:.3f} % of 4000 rows undecided, {100 * (want < 0).mean():.1f} % inside")
    assert und <= 0.01
