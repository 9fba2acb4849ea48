"""What the mesh-with-movers kernels (csrc/scene_mesh.hip's *_mesh_mixed) rest on, in numpy and without a GPU: the
composition rule of tests/scene_mixed_ref.py applied to a mesh (mesh_ref, mesh_sdf_ref) and a set of movers
(scene_dyn_ref, scene_sdf_ref) with its tie rule -- the mesh comes before a mover -- and the arithmetic of the pruning
bound b = fl(fl(d_m d_m) (1 + 2^-50)) that an open set's distance walk starts from (mesh_dev.h: mesh_mixed_distance)."""
import numpy as np

import mesh_ref as MR
import mesh_sdf_ref as MS
import scene_dyn_ref as D
import scene_mixed_ref as X
import scene_sdf_ref as S
from sdf_nmpc_amd.mesh import Mesh

BOX = Mesh.box((-2.0, -1.0, -1.0), (-1.0, 1.0, 1.0))  # its face at x = -1: the origin is at distance 1 exactly


def _rows(mesh, movers, pts, t, signed):
    """(h, J) of the mesh, of the movers, and their selection, untruncated"""
    gd, gg = MS.dist_grad(mesh, pts, signed)
    dd, dg, _ = S.dist_grad(X.to_ref(movers), pts, t)
    return (gd, gg), (dd, dg), X.rows(gd, gg, dd, dg)


def test_the_tie_goes_to_the_mesh():
    o = np.zeros((1, 3))
    for signed in (False, True):
        (gd, gg), (dd, dg), (h, J) = _rows(BOX, [X.TIE_MOVER], o, 0.0, signed)
        assert gd[0] == 1.0 and dd[0] == 1.0  # exactly representable: a tie
        np.testing.assert_array_equal(gg[0], [1.0, 0.0, 0.0])
        np.testing.assert_array_equal(dg[0], [-1.0, 0.0, 0.0])
        assert h[0] == 1.0
        np.testing.assert_array_equal(J[0], [1.0, 0.0, 0.0])  # the mesh's gradient
        (gd, gg), (dd, dg), (h, J) = _rows(BOX, [X.TIE_MOVER], o, X.TIE_T_NEARER, signed)
        assert dd[0] == 0.75 and h[0] == 0.75
        np.testing.assert_array_equal(J[0], [-1.0, 0.0, 0.0])  # the mover strictly nearer: its gradient


def test_the_minimum_is_the_union():
    """A closed mesh gives a signed value, a point inside a mover a negative one; distance and rows agree on the value."""
    mover = ("sphere", [0.5, 0.0, 0.0, 0.5], dict(q=[1.0, 0.0, 0.0, 0.0], v=[1.0, 0.0, 0.0], amp=[0.0] * 3, yaw_rate=0.0,
                                                  omega=0.0, phase=0.0))
    pts = np.array([[-1.5, 0.0, 0.0], [0.5, 0.0, 0.0], [1.5, 0.0, 0.0], [-0.5, 0.0, 0.0]])
    t = np.array([0.0, 0.0, 1.0, 0.0])
    m = MR.distance(BOX, pts, signed=True)
    d = D.distance(X.to_ref([mover]), pts, t)
    want = X.distance(m, d)
    np.testing.assert_array_equal(want, [-0.5, -0.5, -0.5, 0.5])  # inside the mesh; inside the mover at t = 0 and at t = 1
    assert m[0] == -0.5 and d[1] == -0.5 and d[2] == -0.5 and m[3] == 0.5 and d[3] == 0.5
    _, _, (h, J) = _rows(BOX, [mover], pts, t, True)
    np.testing.assert_array_equal(h, want)
    np.testing.assert_array_equal(J[3], [1.0, 0.0, 0.0])  # the tie at (-0.5, 0, 0): the mesh's gradient again
    np.testing.assert_array_equal(X.render(np.float32([0.25, 1.0]), np.float32([0.5, 0.0])), np.float32([0.25, 0.0]))


def test_pruning_bound_arithmetic():
    """d_m over 1e-6 .. 1e3.  A triangle whose squared distance d2 lies above b = fl(fl(d_m d_m) (1 + 2^-50)) has a
    correctly rounded root strictly above d_m: pruning it can neither change the minimum nor take a tie from the mesh.
    And every d2 whose root rounds to d_m (or below) is at or below b: it is searched as in the full walk."""
    rng = np.random.default_rng(0)
    dm = 10.0 ** rng.uniform(-6.0, 3.0, 200000)
    dm = np.concatenate([dm, 2.0 ** np.arange(-19, 10), np.nextafter(2.0 ** np.arange(-19, 10), 0.0),
                         np.nextafter(2.0 ** np.arange(-19, 10), np.inf)])
    b = (dm * dm) * (1.0 + 2.0 ** -50)
    assert (b > dm * dm).all()
    d2 = b
    for _ in range(4):  # the first doubles above the bound
        d2 = np.nextafter(d2, np.inf)
        assert (np.sqrt(d2) > dm).all()
    # the roots that round to d_m come from a band of relative width ulp(d_m) / d_m <= 2^-52 about d_m^2, at most a
    # few doubles; b lies 2^-50 above: every one of them is at or below the bound, with room to spare
    d2 = dm * dm
    for _ in range(3):
        d2 = np.nextafter(d2, 0.0)
    seen = np.zeros(dm.shape, bool)
    for _ in range(16):
        tie = np.sqrt(d2) == dm
        seen |= tie
        assert (d2[tie] <= b[tie]).all()
        d2 = np.nextafter(d2, np.inf)
    assert seen.all() and (np.sqrt(d2) > dm).all()  # the walk met every d_m's band and left it
