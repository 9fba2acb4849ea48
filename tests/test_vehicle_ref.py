"""The CPU truth of the vehicle model (tests/vehicle_ref.py) against what its equations imply: the neutral model is
the plant, the delay ring, the thrust lag's analytic solution, the gust's stationary variance, the Philox counter
layout, and a yaw error that is a rotation about world z."""
import numpy as np
import pytest

import plant_ref
import sensor_ref
import vehicle_ref as V
from sdf_nmpc_amd.config import Config

DT = 0.15


@pytest.fixture(scope="module")
def cfg():
    return Config()


@pytest.mark.parametrize("kind", ["att", "att_tau"])
@pytest.mark.parametrize("substeps", [1, 4])
def test_everything_off_is_the_plant_exactly(cfg, kind, substeps):
    rng = np.random.default_rng(3)
    B = 37
    x, u = plant_ref.states(rng, B)
    acc, gs = rng.normal(0, 0.5, (B, 3)), rng.uniform(0.8, 1.2, B)
    for a, g in ((None, None), (acc, gs)):
        v = V.Vehicle(cfg, B, seed=9)
        np.testing.assert_array_equal(v.begin(x, 5), x)
        est = v.step(kind, u, 5, DT, substeps, acc_dist=a, gamma_scale=g)
        want = plant_ref.step(cfg, kind, x, u, DT, substeps, acc_dist=a, gamma_scale=g)
        np.testing.assert_array_equal(v.x_true, want)
        np.testing.assert_array_equal(est, want)
        np.testing.assert_array_equal(v.u_app, u)


@pytest.mark.parametrize("d", [1, 3, 8])
def test_delay_ring_delivers_frame_f_at_f_plus_d(cfg, d):
    """From any starting frame: hover for the first d calls, then the command given d calls earlier."""
    rng = np.random.default_rng(4)
    B, F, f0 = 5, 12, 7
    x, _ = plant_ref.states(rng, B)
    cmds = rng.uniform(0.2, 0.8, (F, B, 4))
    v = V.Vehicle(cfg, B, delay=d)
    v.begin(x, f0)
    hover = np.tile([plant_ref.G / plant_ref.limits(cfg)[0], 0.0, 0.0, 0.0], (B, 1))
    for k in range(F):
        v.step("att", cmds[k], f0 + k, DT)
        np.testing.assert_array_equal(v.u_app, hover if k < d else cmds[k - d])


def test_thrust_lag_follows_the_first_order_response(cfg):
    """A constant command: gamma_act(t) = g + (gamma_cmd - g)(1 - exp(-t / tau_m)).  RK4 on a linear equation has
    the local error (h / tau)^5 / 120 per step, so the error after T / h steps is at most (T / tau)(h / tau)^4 / 120 of
    the step |gamma_cmd - g|, and halving h divides it by about 16."""
    tau, K = 0.08, 6
    lim = plant_ref.limits(cfg)
    x, _ = plant_ref.states(np.random.default_rng(5), 3)
    u = np.tile([0.75, 0.1, -0.1, 0.2], (3, 1))
    gamma_cmd = 0.75 * lim[0]
    errs = []
    for substeps in (4, 8):
        v = V.Vehicle(cfg, 3, thrust_tau=tau)
        v.begin(x, 0)
        np.testing.assert_array_equal(v.gamma_act, plant_ref.G)
        err = 0.0
        for k in range(K):
            v.step("att_tau", u, k, DT, substeps)
            want = plant_ref.G + (gamma_cmd - plant_ref.G) * (1.0 - np.exp(-(k + 1) * DT / tau))
            err = max(err, np.abs(v.gamma_act - want).max())
        h = DT / substeps
        assert err <= (K * DT / tau) * (h / tau) ** 4 / 120 * abs(gamma_cmd - plant_ref.G), (substeps, err)
        errs.append(err)
    assert 10.0 < errs[0] / errs[1] < 24.0, errs  # fourth order


@pytest.mark.parametrize("tau_g", [0.0, 0.5])
def test_gust_has_the_configured_stationary_variance(cfg, tau_g):
    sigma, F = 0.7, 4096
    v = V.Vehicle(cfg, 1, seed=11, gust_std=sigma, gust_tau=tau_g)
    x, u = plant_ref.states(np.random.default_rng(6), 1)
    v.begin(x, 0)
    w = np.empty((F, 3))
    for f in range(F):
        v.step("att", u, f, 0.1)
        w[f] = v.w[0]
        v.x_true = x.copy()  # the gust does not depend on the state: keep it in the box
    ratio = w.var() / sigma**2
    print(f"\ntau_g {tau_g}: sample variance / sigma^2 = {ratio:.4f} (per axis {w.var(0) / sigma**2})")
    assert abs(ratio - 1.0) <= 0.10


def test_counter_layout_is_pinned(cfg):
    """(j, frame, stream, 1) under the key (seed low, seed high): three word sets from sensor_ref.philox4x32_10."""
    lit = [((0, 0, 0, 0), (0x2dce73e5, 0x1348e23f, 0xfcf8e0ec, 0xa287aadb)),
           ((0x123456789abcdef0, 3, 11, 37), (0x5513f47c, 0x952a1b0b, 0xaac40468, 0x4ce38869)),
           ((7, 4, 2147483647, -1), (0x746cc5a0, 0x5463e750, 0x61d1e3b2, 0xf6b88cd9))]
    for (seed, j, frame, stream), want in lit:
        got = tuple(int(w[0]) for w in V.words(seed, j, frame, np.array([stream])))
        assert got == want
        direct = sensor_ref.philox4x32_10(j, frame, stream & 0xffffffff, 1, seed & 0xffffffff, seed >> 32)
        assert tuple(int(w) for w in direct) == want
    # the sensor's words (last counter word 0) are others
    assert tuple(int(w) for w in sensor_ref.philox4x32_10(0, 0, 0, 0, 0, 0)) != lit[0][1]
    # call j fills n[2j] and n[2j + 1]
    n = V.normals(0x123456789abcdef0, 11, np.array([37]))
    w = V.words(0x123456789abcdef0, 3, 11, np.array([37]))
    assert n[0, 6] == sensor_ref.normal(w[0], w[1])[0] and n[0, 7] == sensor_ref.normal(w[2], w[3])[0]


def test_yaw_error_keeps_norm_roll_and_pitch(cfg):
    rng = np.random.default_rng(7)
    B = 256
    x, _ = plant_ref.states(rng, B)
    x[:, 3:7] /= np.linalg.norm(x[:, 3:7], axis=-1, keepdims=True)
    n = V.normals(5, 3, np.arange(B))
    xe = V.estimate(x, n, std_yaw=0.3, bias=np.r_[np.zeros(6), 0.5])

    def angles(s):
        q0, q1, q2, q3 = (s[:, 3:7] / np.linalg.norm(s[:, 3:7], axis=-1, keepdims=True)).T
        return (np.arctan2(2 * (q0 * q1 + q2 * q3), 1 - 2 * (q1 * q1 + q2 * q2)), np.arcsin(2 * (q0 * q2 - q3 * q1)),
                np.arctan2(2 * (q0 * q3 + q1 * q2), 1 - 2 * (q2 * q2 + q3 * q3)))

    r0, p0, y0 = angles(x)
    r1, p1, y1 = angles(xe)
    assert np.abs(np.linalg.norm(xe[:, 3:7], axis=-1) - 1.0).max() <= 1e-15
    assert np.abs(r1 - r0).max() <= 1e-15 and np.abs(p1 - p0).max() <= 1e-15
    delta = 0.5 + 0.3 * n[:, 9]
    dy = (y1 - y0 - delta + np.pi) % (2 * np.pi) - np.pi
    assert np.abs(dy).max() <= 1e-14 and np.abs(delta).max() > 0.5  # and it is the yaw that turned
    np.testing.assert_array_equal(xe[:, :3], x[:, :3])
    np.testing.assert_array_equal(xe[:, 7:], x[:, 7:])
