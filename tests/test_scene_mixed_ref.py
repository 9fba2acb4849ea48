"""The composition rule of a mixed scene (tests/scene_mixed_ref.py) on its own, and Scene.crowd, the generator of
moving cylinders: no GPU."""
import numpy as np
import pytest

import scene_dyn_ref as D
import scene_mixed_ref as M
import scene_sdf_ref as S
from sdf_nmpc_amd.scene import Scene

LO, HI = (-6.0, -5.0, -1.0), (6.0, 4.0, 2.0)


def test_composition_takes_the_movers_only_where_strictly_lower():
    g_h, d_h = np.array([0.5, 0.5, 0.2, 1.0]), np.array([0.4, 0.5, 0.3, 1.0])
    g_J, d_J = np.full((4, 10), 1.0), np.full((4, 10), 2.0)
    h, J = M.rows(g_h, g_J, d_h, d_J)
    np.testing.assert_array_equal(h, [0.4, 0.5, 0.2, 1.0])
    np.testing.assert_array_equal(J[:, 0], [2.0, 1.0, 1.0, 1.0])
    np.testing.assert_array_equal(M.render(g_h, d_h), [0.4, 0.5, 0.2, 1.0])
    np.testing.assert_array_equal(M.distance(g_h, d_h), [0.4, 0.5, 0.2, 1.0])


def test_constructed_tie_goes_to_the_static_primitive():
    x = np.zeros((1, 10))
    p = np.ones((1, 17))
    h, J = M.sdf_rows([M.TIE_STATIC], [M.TIE_MOVER], x, p, 3.0, t0=0.0)
    assert h[0] == 1.0
    np.testing.assert_array_equal(J[0, :3], [1.0, 0.0, 0.0])  # away from the static sphere at x = -2
    h, J = M.sdf_rows([M.TIE_STATIC], [M.TIE_MOVER], x, p, 3.0, t0=M.TIE_T_NEARER)
    assert h[0] == 0.75
    np.testing.assert_array_equal(J[0, :3], [-1.0, 0.0, 0.0])  # away from the mover, now at x = 1.75
    assert not J[0, 3:].any()
    # the same rule from the two scenes' own rows
    gh, gJ = S.sdf_rows([M.TIE_STATIC], x, p, 3.0)
    for t0 in (0.0, M.TIE_T_NEARER):
        dh, dJ = S.sdf_rows(M.to_ref([M.TIE_MOVER]), x, p, 3.0, t0=t0)
        for got, want in zip(M.rows(gh, gJ, dh, dJ), M.sdf_rows([M.TIE_STATIC], [M.TIE_MOVER], x, p, 3.0, t0=t0)):
            np.testing.assert_array_equal(got, want)


def test_mixed_rows_are_the_rows_of_the_union_away_from_ties():
    """Away from ties the order of the primitives does not matter: the mixed rows are scene_sdf_ref's rows of the one
    list statics + movers, with a fractional flag and node times."""
    statics = Scene.forest(12, LO, HI, seed=4)
    movers = Scene.crowd(5, LO, HI, seed=4)
    rng = np.random.default_rng(0)
    x = rng.normal(0, 1, (3, 7, 10))
    x[..., :3] = rng.uniform(-6, 6, (3, 7, 3)) * np.array([1.0, 1.0, 0.3])
    p = rng.normal(0, 1, (3, 7, 17))
    p[..., 0] = 0.3
    tau = np.arange(7) * 0.2
    h, J = M.sdf_rows(statics, movers, x, p, 3.0, t0=0.4, tau=tau)
    want_h, want_J = S.sdf_rows(M.to_ref(statics + movers), x, p, 3.0, t0=0.4, tau=tau)
    np.testing.assert_array_equal(h, want_h)
    np.testing.assert_array_equal(J, want_J)
    assert (h < 3.0).any() and np.abs(J[..., :3]).max() > 0.1


def test_crowd_is_a_pure_function_of_its_arguments():
    a, b = Scene.crowd(9, LO, HI, seed=3), Scene.crowd(9, LO, HI, seed=3)
    assert a == b and len(a) == 9
    assert Scene.crowd(9, LO, HI, seed=4) != a
    assert Scene.crowd(0, LO, HI) == []
    for kind, vals, mo in a:
        assert kind == "cylinder" and len(vals) == 5 and set(mo) == {"q", "v", "amp", "yaw_rate", "omega", "phase"}
        assert mo["q"] == [1.0, 0.0, 0.0, 0.0] and mo["v"] == [0.0, 0.0, 0.0] and mo["yaw_rate"] == 0.0
        assert mo["amp"][2] == 0.0 and vals[3] == LO[2] and vals[4] == LO[2] + 1.8


def test_crowd_stays_in_its_box_and_moves_at_the_speed_asked_for():
    radius, speed = (0.2, 0.35), (0.5, 1.5)
    prims = Scene.crowd(40, LO, HI, radius=radius, speed=speed, seed=1)
    t = np.linspace(-50.0, 50.0, 1000)
    for kind, vals, mo in prims:
        c0, shape = D.canonical(kind, vals)
        c, _ = D.frame(c0, M.to_ref([(kind, vals, mo)])[0][2], t)  # [1000, 3]
        r = vals[2]
        assert radius[0] <= r <= radius[1]
        assert (c[:, 0] - r >= LO[0]).all() and (c[:, 0] + r <= HI[0]).all()
        assert (c[:, 1] - r >= LO[1]).all() and (c[:, 1] + r <= HI[1]).all()
        assert (c[:, 2] == c0[2]).all() and vals[3] >= LO[2] and vals[4] <= HI[2]
        peak = np.hypot(mo["amp"][0], mo["amp"][1]) * mo["omega"]
        assert speed[0] - 1e-12 <= peak <= speed[1] + 1e-12
        assert np.ptp(c[:, 0]) + np.ptp(c[:, 1]) > 0.0  # it does move


@pytest.mark.parametrize("kw", [dict(n=-1), dict(lo=(1.0, 0.0, 0.0), hi=(1.0, 1.0, 1.0)), dict(radius=(0.0, 0.3)),
                                dict(radius=(0.4, 0.3)), dict(speed=(0.0, 1.0)), dict(speed=(2.0, 1.0)), dict(height=0.0),
                                dict(height=3.5), dict(radius=(0.2, 6.0)), dict(lo=(0.0, 0.0)),
                                dict(speed=(0.5, float("nan")))])
def test_crowd_refuses_bad_arguments(kw):
    args = dict(n=3, lo=LO, hi=HI)
    args.update(kw)
    with pytest.raises(ValueError):
        Scene.crowd(**args)
