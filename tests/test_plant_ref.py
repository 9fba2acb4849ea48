"""tests/plant_ref.py, the CPU truth of the plant kernel, pinned to the project's two independent integrators at
substeps = 1 without mismatch -- the C oracle's RK4 ('att', as tests/scene_setup.plant uses it) and
tests/att_tau_ref.py's torch plant ('att_tau') -- and checked for the order of its substep refinement."""
import numpy as np
import pytest

import att_tau_ref
import plant_ref
from sdf_nmpc_amd import weights as W
from sdf_nmpc_amd.config import Config
from tolerances import lin_close

DT = 0.075  # Config().mpc.T / N at the default horizon: the control period the closed-loop tests run at


@pytest.fixture(scope="module")
def cases():
    return plant_ref.states(np.random.default_rng(7), 64)


def test_att_matches_oracle_integrator(oracle_lib, cfg, cases):
    O = oracle_lib
    x, u = cases
    B = x.shape[0]
    onet = O.Net(W.DEFAULT_SPEC, W.siren_weights(W.DEFAULT_SPEC, seed=0))
    lin = O.linearize_batch(O.quad_model(cfg), onet, np.stack([x, x], 1), u[:, None], np.zeros((B, 2, 145)),
                            np.array([DT]))
    got = plant_ref.step(cfg, "att", x, u, DT)
    print(f"\nplant_ref att vs oracle: max abs {np.abs(got - lin['xn'][:, 0]).max():.2e}")
    assert lin_close(got, lin["xn"][:, 0], rtol=1e-13)


def test_att_tau_matches_att_tau_ref(cfg, cases):
    x, u = cases
    want = att_tau_ref.step(cfg, x, u, DT)
    got = plant_ref.step(cfg, "att_tau", x, u, DT)
    print(f"\nplant_ref att_tau vs att_tau_ref: max abs {np.abs(got - want).max():.2e}")
    assert lin_close(got, want, rtol=1e-13)


@pytest.mark.parametrize("kind", ["att", "att_tau"])
def test_substeps_refine_at_fifth_order(cfg, cases, kind):
    """RK4's local error over one period is C dt^5, so four substeps leave C dt^5 / 4^4 and the two results differ by
    (1 - 4^-4) C dt^5: halving dt divides the difference by 2^5 = 32 up to the next order (bounds 24..40).  The
    asymptotic regime needs L dt << 1 for the fastest rate L of the model, the 'att_tau' lag's 1 / tau = 8.3 / s, so
    the check runs at dt = 0.02 (L dt = 0.17), where C dt^5 ~ (L dt)^5 / 120 x rates of O(10) ~ 1e-5: the
    difference stays below 1e-4, while a helper that dropped a stage weight or stepped with the wrong
    dt / substeps would differ at O(dt^2) ~ 1e-3 and scale by 4."""
    x, u = cases
    d = []
    for dt in (0.02, 0.01):
        d.append(np.abs(plant_ref.step(cfg, kind, x, u, dt, 4) - plant_ref.step(cfg, kind, x, u, dt, 1)).max())
    print(f"\n{kind}: |substeps 4 - substeps 1| = {d[0]:.3e} at dt, {d[1]:.3e} at dt / 2, ratio {d[0] / d[1]:.1f}")
    assert 1e-12 < d[0] < 1e-4
    assert 24.0 < d[0] / d[1] < 40.0


@pytest.mark.parametrize("kind", ["att", "att_tau"])
def test_mismatch_terms(cfg, cases, kind):
    """acc_dist adds a constant acceleration: with everything else equal the velocity gains exactly dt a and the
    position dt^2 a / 2 (the dynamics are affine in it and the attitude does not see it); gamma_scale = s equals
    the thrust input scaled by s."""
    x, u = cases
    a = np.tile([0.3, -0.2, -1.0], (x.shape[0], 1))
    base = plant_ref.step(cfg, kind, x, u, DT, 2)
    got = plant_ref.step(cfg, kind, x, u, DT, 2, acc_dist=a)
    np.testing.assert_allclose(got[:, 7:] - base[:, 7:], DT * a, atol=1e-13)
    np.testing.assert_allclose(got[:, :3] - base[:, :3], DT * DT / 2 * a, atol=1e-13)
    np.testing.assert_array_equal(got[:, 3:7], base[:, 3:7])
    s = np.linspace(0.8, 1.2, x.shape[0])
    us = u.copy()
    us[:, 0] *= s
    np.testing.assert_allclose(plant_ref.step(cfg, kind, x, u, DT, 1, gamma_scale=s), plant_ref.step(cfg, kind, x, us, DT, 1),
                               rtol=0, atol=1e-13)
