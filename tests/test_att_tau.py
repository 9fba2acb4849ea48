"""The 'att_tau' model (mpc.model: att_tau; first-order roll / pitch lag) on the host side: model.Quad accepts it
with the 'att' dimensions and bounds and refuses it with recursive feasibility; the command maps follow the
reference's formulas; the binding carries the kind; and the CPU truth of the GPU tests (att_tau_ref.py) equals the
fixtures recorded from the reference's helpers (tests/golden/tau_golden.npz, make_tau_golden.py)."""
import os

import numpy as np
import pytest

import att_tau_ref as T
from sdf_nmpc_amd import _lib
from sdf_nmpc_amd.config import Config
from sdf_nmpc_amd.model import Quad, UnsupportedConfig

HERE = os.path.dirname(os.path.abspath(__file__))


@pytest.fixture(scope="module")
def tau_golden():
    return np.load(os.path.join(HERE, "golden", "tau_golden.npz"))


def test_quad_accepts_att_tau_with_the_att_dimensions_and_bounds():
    a, t = Quad(Config()), Quad(Config(mpc__model="att_tau"))
    assert t.kind == "att_tau" and a.kind == "att"
    assert (t.tau_roll, t.tau_pitch) == (0.12, 0.12)
    assert (t.nx, t.nu, t.ny, t.nyN, t.np) == (10, 4, 11, 4, a.np)
    for k in ("lbu", "ubu", "u_hover", "lh", "uh", "zl", "Zl", "lhN", "uhN", "zlN", "ZlN"):
        assert np.array_equal(getattr(t, k), getattr(a, k)), k
    assert (t.h_cols, t.nh, t.nhs, t.nhN, t.nsN, t.term_rows) == (a.h_cols, a.nh, a.nhs, a.nhN, a.nsN, a.term_rows)
    assert np.array_equal(t.lbu, [0, -1, -1, -1]) and np.array_equal(t.ubu, [1, 1, 1, 1])
    assert np.array_equal(t.u_hover, [9.81 / t.cfg.robot.limits.gamma, 0, 0, 0])


def test_att_tau_with_recursive_feasibility_is_refused():
    with pytest.raises(UnsupportedConfig, match="att_tau"):
        Quad(Config(mpc__model="att_tau", flags__recursive_feasibility=True), braking_coeffs=np.zeros(35))
    with pytest.raises(UnsupportedConfig, match="att_tau"):
        Quad(Config(mpc__model="att_tau", flags__recursive_feasibility=True, flags__stability=True),
             braking_coeffs=np.zeros(35))
    for name in ("acc", "props", "rates", "wrench"):
        with pytest.raises(UnsupportedConfig):
            Quad(Config(mpc__model=name))
        with pytest.raises(UnsupportedConfig):
            _lib.quad_model(Config(mpc__model=name))


def test_binding_carries_the_kind():
    m0 = _lib.quad_model(Config())
    assert (m0.kind, m0.tau_roll, m0.tau_pitch) == (0, 0.0, 0.0)
    cfg = Config(mpc__model="att_tau")
    for m in (_lib.quad_model(cfg), _lib.quad_model(cfg, Quad(cfg))):
        assert (m.kind, m.tau_roll, m.tau_pitch) == (1, 0.12, 0.12)
        assert (m.rec_feas, m.stability) == (0, 0)
    # appended at the end: the earlier fields keep their offsets (include/sdfnmpc.h)
    names = [f[0] for f in _lib.QuadModelC._fields_]
    assert names[-3:] == ["kind", "tau_roll", "tau_pitch"] and names[-4] == "poly"
    assert _lib.QuadModelC.kind.offset == _lib.QuadModelC.poly.offset + 8 * _lib.POLY_MAX


def test_command_maps_match_the_reference_formulas():
    """u_to_TRPYr = [gamma m, roll_des, pitch_des, wz] and u_to_acc = [W_R_B^T W_a, wz] with W_R_B =
    quat2rot(q), W_a = W_R_B e_z gamma - g e_z (quad_rollpitchyawrate_tau.py:33-34,47-48)."""
    cfg = Config(mpc__model="att_tau")
    q, lim = Quad(cfg), cfg.robot.limits
    rng = np.random.default_rng(5)
    x = rng.normal(size=(6, 10))
    u = rng.uniform([0, -1, -1, -1], [1, 1, 1, 1], (6, 4))
    want_t = np.stack([u[:, 0] * lim.gamma * cfg.robot.mass, u[:, 1] * lim.roll, u[:, 2] * lim.pitch, u[:, 3] * lim.wz], -1)
    np.testing.assert_allclose(q.u_to_TRPYr(x, u), want_t, rtol=0, atol=1e-15)
    got = q.u_to_acc(x, u)
    for i in range(6):
        w, a, b, c = x[i, 3:7] / np.linalg.norm(x[i, 3:7])
        R = np.array([[w * w + a * a - b * b - c * c, 2 * (a * b - w * c), 2 * (a * c + w * b)],
                      [2 * (a * b + w * c), w * w - a * a + b * b - c * c, 2 * (b * c - w * a)],
                      [2 * (a * c - w * b), 2 * (b * c + w * a), w * w - a * a - b * b + c * c]])
        W_a = R @ np.array([0, 0, u[i, 0] * lim.gamma]) + np.array([0, 0, -9.81])
        np.testing.assert_allclose(got[i], np.concatenate([R.T @ W_a, [u[i, 3] * lim.wz]]), rtol=0, atol=1e-13)
    # the 'att' map reads roll and pitch from the input, this one from the state: they differ
    assert np.abs(got - Quad(Config()).u_to_acc(x, u)).max() > 1e-2


def test_helper_equals_the_golden_file(tau_golden):
    L = tau_golden
    xn, AB, y, Jy = T.dynamics(Config(), L["x"], L["u"], L["p"], L["dt"])
    np.testing.assert_allclose(xn, L["xn"], rtol=0, atol=1e-13)
    np.testing.assert_allclose(AB.transpose(0, 2, 1), np.concatenate([L["A"], L["B"]], 2), rtol=0, atol=1e-12)
    np.testing.assert_allclose(y, L["y"], rtol=0, atol=1e-13)
    np.testing.assert_allclose(Jy.transpose(0, 2, 1), L["Jy"], rtol=0, atol=1e-12)
    # the structure linearize_kernel's lane mapping rests on: the p and v columns of [A|B] are constants
    dt = L["dt"]
    for j in range(3):
        e = np.zeros((len(dt), 10)); e[:, j] = 1.0
        assert np.abs(AB[:, j] - e).max() <= 1e-15
        e = np.zeros((len(dt), 10)); e[:, 7 + j] = 1.0; e[:, j] = dt
        assert np.abs(AB[:, 7 + j] - e).max() <= 1e-15


def test_roll_follows_its_command_with_the_lag():
    """12 steps of dt = 0.01 from level hover with roll_des = 0.3: one time constant, roll = 0.3 (1 - 1/e) up to
    the pitch / yaw coupling and RK4's error (measured 0.189636119 against 0.189636168)."""
    cfg = Config(mpc__model="att_tau")
    lim = cfg.robot.limits
    x = np.zeros((1, 10)); x[0, 3] = 1.0
    u = np.array([[9.81 / lim.gamma, 0.3 / lim.roll, 0.0, 0.0]])
    for _ in range(12):
        x = T.step(cfg, x, u, 0.01)
    q0, q1, q2, q3 = x[0, 3:7] / np.linalg.norm(x[0, 3:7])
    roll = np.arctan2(2 * (q0 * q1 + q2 * q3), 1 - 2 * (q1 * q1 + q2 * q2))
    assert abs(roll - 0.3 * (1 - np.exp(-1.0))) <= 1e-6, roll
