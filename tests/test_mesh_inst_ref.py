"""tests/mesh_inst_ref.py on the CPU: against analytic oriented boxes and a moving sphere (scene_dyn_ref's closed forms),
its two ways of forming a distance against each other, and the conditions the GPU tests put on the fixed scene's inputs
(tests/test_gpu_scene_inst.py) -- all from the reference alone."""
import numpy as np

import mesh_inst_ref as I
import scene_dyn_ref as DR
import scene_ref as R
from sdf_nmpc_amd.mesh import Mesh
from sdf_nmpc_amd.scene import Scene

PTS = np.random.default_rng(4).uniform([-1, -3, -2.5], [6, 3, 2.5], (700, 3))


def test_box_instances_against_analytic_oriented_boxes():
    """Two instances of one box part, one tilted and yawing, one sliding: the signed distance and the range image of
    the same boxes as scene_dyn_ref's primitives, whose distance is exact for a box."""
    part = Mesh.box((-0.5, -0.25, -0.75), (0.5, 0.25, 0.75))
    kw = [dict(rpy=(0.3, -0.2, 0.5), yaw_rate=0.4, v=(0.0, -0.5, 0.0)), dict(amp=(0.0, 0.0, 0.25), omega=2.0, phase=0.3)]
    pos = [(3.0, 1.0, 0.125), (2.0, -1.5, 0.0)]
    insts = [I.instance(0, p, **k) for p, k in zip(pos, kw)]
    prims = [DR.moving(("box", [p[0] - 0.5, p[1] - 0.25, p[2] - 0.75, p[0] + 0.5, p[1] + 0.25, p[2] + 0.75]), **k)
             for p, k in zip(pos, kw)]
    for t in (0.0, 0.7):
        want = DR.distance(prims, PTS, t)
        assert np.abs(I.distance([part], insts, PTS, t, signed=True) - want).max() <= 1e-12
        assert np.abs(I.distance([part], insts, PTS, np.full(len(PTS), t), signed=True) - want).max() <= 1e-12
        assert np.abs(I.distance([part], insts, PTS, t) - np.abs(want)).max() <= 1e-12
        assert (want < 0).sum() >= 5
        P, RM = R.camera_poses()
        s = R.SENSOR
        got = I.values([part], insts, t, P, RM, 18, 32, s["hfov"], s["vfov"], s["dmax"])
        ok = DR.decided(prims, P, RM, 18, 32, s["hfov"], s["vfov"], s["dmax"], t)
        assert np.abs(got - DR.values(prims, P, RM, 18, 32, s["hfov"], s["vfov"], s["dmax"], t))[ok].max() <= 1e-9
        assert (got[ok] < s["dmax"]).any()


def test_sphere_instance_against_the_analytic_sphere():
    """An icosphere of subdivision 4 lies within r (1 - cos(edge angle / 2)) inside its sphere, 3e-3 r here."""
    part = Mesh.icosphere((0.0, 0.0, 0.0), 0.5, 4)
    inst = [I.instance(0, (2.5, 0.5, 0.25), v=(0.25, 0.5, 0.0), rpy=(0.1, 0.2, 0.3))]
    t = np.random.default_rng(1).uniform(0.0, 2.0, 60)
    pts = PTS[:60]
    want = np.linalg.norm(pts - (np.array([2.5, 0.5, 0.25]) + np.outer(t, [0.25, 0.5, 0.0])), axis=1) - 0.5
    got = I.distance([part], inst, pts, t, signed=True)
    assert (got >= want - 1e-12).all() and (got - want).max() <= 3e-3


def test_the_two_ways_agree_and_the_gradient_is_the_distances():
    ps, insts = I.parts(), I.fixed_instances()
    pts = PTS[:120]
    for signed in (True, False):
        a = I.distance(ps, insts, pts, 0.7, signed=signed)
        b = I.distance(ps, insts, pts, np.full(len(pts), 0.7), signed=signed)
        d, g, which = I.dist_grad(ps, insts, pts, 0.7, signed=signed)
        assert np.abs(a - b).max() <= 1e-13 and np.abs(a - d).max() <= 1e-13
        assert np.abs(np.linalg.norm(g, axis=1) - 1.0).max() <= 1e-12 and len(set(which)) >= 5
    e = 1e-6  # the gradient is the central difference of the distance away from the kinks
    fd = np.stack([(I.distance(ps, insts, pts + e * np.eye(3)[k], 0.7, signed=True) -
                    I.distance(ps, insts, pts - e * np.eye(3)[k], 0.7, signed=True)) / (2 * e) for k in range(3)], 1)
    d, g, _ = I.dist_grad(ps, insts, pts, 0.7, signed=True)
    assert np.median(np.abs(fd - g).max(1)) <= 1e-8 and (np.abs(fd - g).max(1) <= 1e-6).mean() >= 0.9


def test_fixed_scene_meets_the_conditions_on_the_gpu_tests_inputs():
    ps, insts = I.parts(), I.fixed_instances()
    assert len(ps) == 4 and len(insts) == 8 and all(m.is_closed() for m in ps)
    d = I.distance(ps, insts, PTS, 0.7, signed=True)
    assert (d < 0).sum() >= 20 and (d > 0).sum() >= 600
    P, RM = R.camera_poses()
    for sensor, s in (("pinhole", R.SENSOR), ("spherical", R.SPHERICAL)):
        for t in I.TIMES:
            kw = dict(is_spherical=sensor == "spherical")
            ok = I.decided(ps, insts, t, P, RM, 18, 32, s["hfov"], s["vfov"], s["dmax"], **kw)
            v = I.values(ps, insts, t, P, RM, 18, 32, s["hfov"], s["vfov"], s["dmax"], **kw)
            assert ok.mean() >= 0.95 and 0.3 <= (v < s["dmax"]).mean() <= 0.7
    assert (I.values(ps, insts, 0.0, P, RM, 18, 32, 0.75, 0.49, 5.0) != I.values(ps, insts, 0.7, P, RM, 18, 32, 0.75, 0.49, 5.0)).any()


def test_speed_bound_and_the_python_side_of_the_fixed_scene():
    ps, insts = I.parts(), I.fixed_instances()
    V = I.speed_bound(ps, insts)
    # instance 7: |omega| |amp| + |yaw_rate| rho = 1.5 * 0.5 + 0.8 * sqrt(0.75) is the largest
    assert abs(V - (0.75 + 0.8 * np.sqrt(0.75))) <= 1e-15
    assert I.speed_bound(ps, insts[:1]) == 0.0 and I.speed_bound(ps, []) == 0.0
    si = I.scene_instances()
    assert len(si) == 8 and all(a[0] == "instance" and a[1] == s[0] for a, s in zip(si, I.SPEC))
    for a, b in zip(si, insts):  # Scene.instance's quaternion is the reference's matrix
        assert np.abs(R.quat2rot(a[3]["q"]) - b["R0"]).max() <= 1e-15


def test_scatter_is_a_pure_function_of_its_arguments():
    a = Scene.scatter(50, (-1, -2, 0), (3, 2, 0), parts=3, seed=5, keep_clear=((0.0, 0.0), 1.0))
    b = Scene.scatter(50, (-1, -2, 0), (3, 2, 0), parts=3, seed=5, keep_clear=((0.0, 0.0), 1.0))
    assert a == b and len(a) == 50 and {i[1] for i in a} == {0, 1, 2}
    pos = np.array([i[2] for i in a])
    assert (np.hypot(pos[:, 0], pos[:, 1]) >= 1.0).all() and (pos[:, 2] == 0).all()
    assert (pos >= (-1, -2, 0)).all() and (pos[:, 0] <= 3).all()
    assert all(i[3]["v"] == [0.0, 0.0, 0.0] and i[3]["yaw_rate"] == 0.0 for i in a)
    assert len({tuple(i[3]["q"]) for i in a}) == 50
    flat = Scene.scatter(4, (0, 0, 0), (1, 1, 1), parts=[2], yaw=False)
    assert all(i[1] == 2 and i[3]["q"] == [1.0, 0.0, 0.0, 0.0] for i in flat)
    assert Scene.scatter(50, (-1, -2, 0), (3, 2, 0), parts=3, seed=6) != a
