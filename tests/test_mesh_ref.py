"""tests/mesh_ref.py and the host-side ``Mesh`` (sdf_nmpc_amd/mesh.py) on the CPU: the reference distance to the meshed
box and cylinder against the closed forms of tests/scene_ref.py, ``is_closed``, the OBJ reader, and the generators'
purity.  No device."""
import numpy as np

import mesh_ref as M
import scene_ref as R
from sdf_nmpc_amd.mesh import Mesh


def _points(n=300):
    return np.random.default_rng(4).uniform([-1, -3, -2.5], [6, 3, 2.5], (n, 3))


def _terrain():
    i, j = np.meshgrid(np.arange(6), np.arange(5), indexing="ij")
    return Mesh.heightfield(-1.0, -2.0, 0.5, 0.75, 0.2 * np.sin(i) + 0.1 * np.cos(2.0 * j))


def _tunnel():
    return Mesh.tunnel([(0, 0, 0), (1.5, 0.3, 0), (3, -0.2, 0.4), (4.5, 0, 0.2)], 1.0, segments=8, roughness=0.2, seed=3)


def test_box_distance_is_the_closed_form():
    lo, hi = (3.5, 0.5, -1.0), (4.1, 1.5, 1.2)
    pts = np.concatenate([_points(), np.random.default_rng(5).uniform(lo, hi, (60, 3))])  # 60 inside
    want = R.distance([("box", list(lo) + list(hi))], pts)
    got = M.distance(Mesh.box(lo, hi), pts, signed=True)
    assert (want < 0).sum() >= 60
    assert np.abs(got - want).max() <= 1e-12
    assert np.abs(M.distance(Mesh.box(lo, hi), pts) - np.abs(want)).max() <= 1e-12


def test_cylinder_distance_is_within_the_sagitta():
    """The meshed cylinder lies inside the true one, its surface within r (1 - cos(pi / 64)) of it: its signed
    distance is not below the closed form and not more than that above it."""
    c, r, z0, z1 = (3.0, 0.3), 0.4, -1.5, 1.5
    pts = np.concatenate([_points(), np.random.default_rng(6).uniform([2.6, -0.1, z0], [3.4, 0.7, z1], (60, 3))])
    want = R.distance([("cylinder", [*c, r, z0, z1])], pts)
    got = M.distance(Mesh.cylinder(c, r, z0, z1, 64), pts, signed=True)
    assert (want < 0).sum() > 20
    gap = got - want
    assert gap.min() >= -1e-12 and gap.max() <= r * (1.0 - np.cos(np.pi / 64)) + 1e-12


def test_is_closed():
    box = Mesh.box((0, 0, 0), (1, 2, 3))
    for m in (box, Mesh.icosphere((0, 0, 0), 1.0, 2), Mesh.cylinder((0, 0), 1.0, -1.0, 1.0, 12),
              Mesh.merge(box, Mesh.icosphere((5, 0, 0), 1.0, 1)), M.fixed_scene()):
        assert m.is_closed()
    flipped = box.tris.copy()
    flipped[3] = flipped[3][::-1]
    for m in (_terrain(), _tunnel(), Mesh(box.verts, box.tris[1:]), Mesh(box.verts, flipped)):
        assert not m.is_closed()
    # outward orientation: the centre is inside by the pseudonormal sign
    assert M.distance(box, [[0.5, 1.0, 1.5]], signed=True)[0] == -0.5
    assert abs(M.distance(Mesh.icosphere((1, 2, 3), 2.0, 2), [[1, 2, 3]], signed=True)[0] + 2.0) < 0.05
    assert M.distance(Mesh.cylinder((0, 0), 1.0, -1.0, 1.0, 12), [[0, 0, 0.5]], signed=True)[0] == -0.5


def test_counts_and_transform():
    assert Mesh.box((0, 0, 0), (1, 1, 1)).tris.shape == (12, 3)
    assert Mesh.icosphere((0, 0, 0), 1.0, 2).tris.shape == (320, 3)
    assert np.abs(np.linalg.norm(Mesh.icosphere((1, 2, 3), 0.5, 3).verts - (1, 2, 3), axis=1) - 0.5).max() < 1e-15
    assert Mesh.cylinder((0, 0), 1.0, 0.0, 1.0, 24).tris.shape == (96, 3)
    assert _terrain().tris.shape == (2 * 5 * 4, 3) and _tunnel().tris.shape == (2 * 3 * 8, 3)
    m = Mesh.box((0, 0, 0), (1, 1, 1)).transformed(R=R.rpy2rot(0.0, 0.0, np.pi / 2), t=(1, 0, 0), scale=2.0)
    assert m.is_closed() and np.abs(m.verts.min(0) - (-1, 0, 0)).max() < 1e-15 and np.abs(m.verts.max(0) - (1, 2, 2)).max() < 1e-15
    both = Mesh.merge(_terrain(), _tunnel())
    assert both.tris.shape[0] == 40 + 48 and both.tris.max() == both.verts.shape[0] - 1


def test_obj_round_trip_with_a_quad(tmp_path):
    path = tmp_path / "quad.obj"
    path.write_text("# a unit square and a triangle on top\nv 0 0 0\nv 1 0 0\nv 1 1 0\nv 0 1 0\nvn 0 0 1\nv 0.5 0.5 1\n"
                    "f 1/1/1 2/2/1 3/3/1 4/4/1\nf -1 1 2\n")
    m = Mesh.from_obj(str(path))
    assert m.verts.shape == (5, 3) and m.tris.tolist() == [[0, 1, 2], [0, 2, 3], [4, 0, 1]]
    out = tmp_path / "again.obj"
    m.to_obj(str(out))
    again = Mesh.from_obj(str(out))
    np.testing.assert_array_equal(again.verts, m.verts)
    np.testing.assert_array_equal(again.tris, m.tris)


def test_generators_are_pure():
    for make in (lambda: Mesh.box((0, 0, 0), (1, 2, 3)), lambda: Mesh.icosphere((0, 1, 0), 0.7, 2),
                 lambda: Mesh.cylinder((1, 1), 0.5, 0.0, 2.0, 16), _terrain, _tunnel, M.fixed_scene):
        a, b = make(), make()
        np.testing.assert_array_equal(a.verts, b.verts)
        np.testing.assert_array_equal(a.tris, b.tris)
        assert a.verts.dtype == np.float64 and a.tris.dtype == np.int32
    assert (Mesh.tunnel([(0, 0, 0), (1, 0, 0)], 1.0, roughness=0.2, seed=1).verts !=
            Mesh.tunnel([(0, 0, 0), (1, 0, 0)], 1.0, roughness=0.2, seed=2).verts).any()
