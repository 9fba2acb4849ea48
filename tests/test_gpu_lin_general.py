"""The preparation kernel (csrc/linearize.hip) on general inputs.

1. The braking polynomial of flags.recursive_feasibility with every monomial live: the reference-pinned dense
   coefficients of degrees 0..6 (flag_sets.dense_braking) against the checker, and the physical law plus noise on
   every monomial (flag_sets.noisy_braking) through the QP kernels, the phase split and the controller.  Every other
   test takes the four-term polynomial of flag_sets.braking (a constant and one value on x^2, y^2, z^2), which
   cannot tell the x exponent from the y exponent, a mixed term's index or gradient, or any degree but 0 and 2.
2. The 'att' instantiation (KIND == 0: drsqrt from the hardware estimate, yaw from (x3, x6) / |(x3, x6)|, the
   lane-pair sincos) away from synth.make_problem's hover-ish iterate (test_flags.att_wide_problem), and its
   s03 == 0 branch.

tests/test_flags.py holds each reference on the CPU first (test_terminal_extras_oracle_dense_polynomial,
test_noisy_braking_is_seen_and_converges, test_att_wide_problem_referees, test_s03_zero_point_in_the_checker)."""
import numpy as np
import pytest

import flag_sets as F
import test_gpu_flags as G
from sdf_nmpc_amd import _lib, synth, weights as W
from sdf_nmpc_amd.model import poly_eval
from test_flags import ATT_WIDE_SHAPES, FLAG_VALUES, LIN_GEN_ATOL, LIN_GEN_RTOL, att_wide_problem, s03_zero_problem
from test_gpu_controller import eval_sdf_ref
from test_gpu_linearize import OUTS, check_vs_oracle, run_gpu
from tolerances import lin_close, sdf_df_ok

pytestmark = [pytest.mark.gpu, pytest.mark.filterwarnings("ignore:no SDF weights")]

# (B, N): the terminal node at row 1 of a block; at every third row across two blocks (33 rows, 32 per block); the
# shape of test_gpu_flags.test_linearisation_per_flag_set
DENSE_SHAPES = [(1, 1), (11, 2), (6, 20)]


def _close(got, ref, what):
    """test_linearisation_per_flag_set's bar: rtol 1e-9, atol 1e-11 max(1, |ref|.max()); returns the worst error
    in units of the bar's absolute part."""
    scale = max(1.0, float(np.abs(ref).max()))
    np.testing.assert_allclose(got, ref, rtol=LIN_GEN_RTOL, atol=LIN_GEN_ATOL * scale, err_msg=what)
    return float(np.abs(got - ref).max()) / scale


@pytest.mark.parametrize("deg", range(7))
@pytest.mark.parametrize("name", ["rec_feas", "stability"])
def test_dense_polynomial_linearise_vs_checker(gpu_ctx, oracle_lib, name, deg):
    """sdfnmpc_linearize with the dense polynomial of degree 0..6 (degree 6 fills poly[84] and pw[.][6] to the last
    element), terminal flags from {0, 1, 0.3} (each value at every shape with B > 1), velocities along the view:
    every fp64 output against oracle.linearize_batch at rtol 1e-9, atol 1e-11 max(1, |ref|.max()); the sdf column
    at test_linearisation_per_flag_set's network bars.  With flag 0: hE[:3], JhE[..., :3] and the stability yN,
    JyN are exactly 0 and hE[3:6] is v bit for bit.  Measured worst, relative to max(1, |ref|.max()): hE 2.1e-16,
    JhE 1.5e-15, y 1.5e-15 (with the wrong builds that turn this test red)."""
    import torch
    coeffs = F.dense_braking(deg)
    worst = {}
    for B, N in DENSE_SHAPES:
        cfg, q, prob, x0, t = G._setup(gpu_ctx, name, B, N, seed=11, coeffs=coeffs)
        assert q.poly_deg == deg and np.array_equal(q.poly, coeffs)
        flag = np.array([FLAG_VALUES[(b + deg) % 3] for b in range(B)])
        assert B == 1 or set(flag) == set(FLAG_VALUES)
        prob["p"][:, N, 0] = flag
        t["p"].copy_(torch.from_numpy(np.ascontiguousarray(prob["p"])))
        torch.cuda.synchronize()
        _lib.linearize(gpu_ctx, G._net(gpu_ctx, q), _lib.quad_model(cfg, q), B, N, q.np, t, nyN=q.nyN, no_sdf=not q.need_sdf)
        gpu_ctx.synchronize()
        got = G._np(t, G.LIN)
        ref = oracle_lib.linearize_batch(oracle_lib.quad_model(cfg), G._onet(oracle_lib, q), prob["x"], prob["u"], prob["p"],
                                         prob["dt"], model=q)
        for k in ("xn", "AB", "y", "Jy", "yN", "JyN", "hE", "JhE"):
            worst[k] = max(worst.get(k, 0.0), _close(got[k], ref[k], f"{k} at {(B, N)}"))
        for c in (0, 1):
            _close(got["h"][..., c], ref["h"][..., c], f"h[{c}] at {(B, N)}")
            _close(got["Jh"][..., c], ref["Jh"][..., c], f"Jh[{c}] at {(B, N)}")
        np.testing.assert_allclose(got["h"][..., 2], ref["h"][..., 2], rtol=0, atol=1e-5 * max(1.0, np.abs(ref["h"][..., 2]).max()))
        np.testing.assert_allclose(got["Jh"][..., 2], ref["Jh"][..., 2], rtol=0, atol=1e-4 * max(1.0, np.abs(ref["Jh"][..., 2]).max()))
        v = prob["x"][:, N, 7:]
        pv, _ = poly_eval(coeffs, deg, v)
        # the reference is the polynomial, not a constant: hE[0] = -flag poly(v) (exactly the checker's convention)
        np.testing.assert_allclose(ref["hE"][:, 0], -flag * pv, rtol=1e-12, atol=1e-12 * max(1.0, np.abs(pv).max()))
        off = flag == 0
        assert (got["hE"][off, :3] == 0).all() and (got["JhE"][off][..., :3] == 0).all()
        assert np.array_equal(got["hE"][:, 3:], v)  # at every flag
        np.testing.assert_array_equal(got["JhE"][..., 3:], np.broadcast_to(np.eye(10)[:, 7:], (B, 10, 3)))
        if q.stability:
            assert (got["yN"][off] == 0).all() and (got["JyN"][off] == 0).all()
    print(f"\ndense polynomial {name} deg {deg}: worst |gpu - checker| / max(1, |ref|.max()) " +
          ", ".join(f"{k} {e:.1e}" for k, e in worst.items()))


@pytest.mark.parametrize("name,deg,B,N,kernel", [pytest.param(*r, id=f"{r[0]}-deg{r[1]}-N{r[3]}-{r[4]}") for r in F.NOISY_QP_RUNS])
def test_qp_with_noisy_braking(gpu_ctx, oracle_lib, name, deg, B, N, kernel):
    """test_gpu_flags._check_qp (the C IPM on the GPU's linearisation, the exact solution) with the noisy
    polynomial: a misplaced mixed term moves hE by 0.14 and du by 0.02 (0.18 with stability) at degree 4, far above
    every bar.  Problem seed 11; the exact solution on the first four instances (two at N = 40) and on every one
    off the C IPM.  (Whether a hard stage row binds is the problem's property: not asked here.)"""
    coeffs = F.noisy_braking(F.config(name), deg, F.NOISY_SEEDS.get((name, deg, N), 1))
    seg = kernel == "segmented"
    w = G._check_qp(gpu_ctx, oracle_lib, name, B, N, kernel, need_active=False, iters_frac=0.9 if seg else 1.0,
                    n_exact=2 if seg else 4, seed=11, coeffs=coeffs)
    q = w["q"]
    assert q.poly_deg == deg and np.array_equal(q.poly, coeffs)
    # the linearisation the QP ran on is the checker's, terminal extras included
    ref = oracle_lib.linearize_batch(oracle_lib.quad_model(w["cfg"]), G._onet(oracle_lib, q), w["prob"]["x"], w["prob"]["u"],
                                     w["prob"]["p"], w["prob"]["dt"], model=q)
    for k in ("hE", "JhE", "yN", "JyN"):
        _close(w["lin"][k], ref[k], k)


def test_phase_split_bitwise_with_noisy_braking(gpu_ctx):
    """rti_prepare + qp_feedback == linearize + qp_solve bit for bit (test_phase_split_bitwise_per_flag_set's body)
    on stability with the noisy polynomial of degree 6: the model struct's poly[84] reaches both entry points."""
    coeffs = F.noisy_braking(F.config("stability"), 6, F.NOISY_SEEDS.get(("stability", 6, 20), 1))
    G._phase_split(gpu_ctx, "stability", 8, 20, "auto", 11, coeffs=coeffs)


NMPC_COEFF_SEED = 1  # the first coefficient seed at which Nmpc.solve returns 0 on every instance


def test_controller_step_and_eval_with_noisy_braking(oracle_lib):
    """One Nmpc.solve step of rec_feas_soft_brake with the noisy polynomial of degree 6 (coefficients through the
    controller's braking_coeffs argument into the solver object's model struct) under
    test_controller_rti_step_per_flag_set's assertions; the solver's hE and JhE against the checker at the
    linearisation bar; and Nmpc.eval(N) by value: column 0 the network's df (the checker's fp64 evaluation at the
    same fp32 input, SDF bar of tolerances.py), column 1 poly_eval(v_N), column 2 their difference, exactly."""
    name, deg, N = "rec_feas_soft_brake", 6, 20
    coeffs = F.noisy_braking(F.config(name), deg, NMPC_COEFF_SEED)

    def check(n, q, x0, xbar, glin, lin, onet):
        assert n.model.poly_deg == deg and np.array_equal(n.model.poly, coeffs)
        e = {k: _close(glin[k], lin[k], k) for k in ("hE", "JhE")}
        ev = n.eval(N)
        xN = n.ocp.download("x")[:, N]
        bd, _ = poly_eval(coeffs, deg, xN[:, 7:10])
        df = eval_sdf_ref(onet, n, N)
        print(f"\ncontroller, noisy degree 6: |hE - checker| {e['hE']:.1e}, |JhE - checker| {e['JhE']:.1e}, "
              f"|eval[0] - df| max {np.abs(ev[:, 0] - df).max():.1e}, poly(v_N) in [{bd.min():.3f}, {bd.max():.3f}]")
        assert ev.shape == (n.B, 3)
        assert sdf_df_ok(ev[:, 0], df)
        np.testing.assert_array_equal(ev[:, 1], bd)
        np.testing.assert_array_equal(ev[:, 2], ev[:, 0] - ev[:, 1])
        assert np.abs(bd - poly_eval(F.braking(n.cfg), deg, xN[:, 7:10])[0]).max() > 1e-4  # the noise is live

    G._controller_step(oracle_lib, name, N, coeffs=coeffs, check=check)


# ---- the 'att' dynamics on the widened problem
def _att_run(gpu_ctx, cfg, prob):
    return run_gpu(gpu_ctx, _lib.Net.siren(gpu_ctx, 0), cfg, prob)


@pytest.mark.parametrize("B,N,uniform", ATT_WIDE_SHAPES)
def test_att_wide_linearise_vs_checker(gpu_ctx, oracle_lib, cfg, B, N, uniform):
    """linearize_kernel<0> on att_wide_problem (roll and pitch to +-1.2 rad, quaternion norms 0.5..2 and both signs,
    commands at the box, flag 0 at every third node; (7, 40) on the non-uniform grid) against
    oracle.linearize_batch, at test_linearize_vs_oracle's bars.  At (7, 40) also: a second run agrees bit for bit,
    and permuting the instances permutes the outputs bit for bit."""
    _, dt = oracle_lib.shooting_grid(N, float(cfg.mpc.T), uniform)
    prob = att_wide_problem(cfg, B, N, seed=B * 100 + N, dt=dt)
    got = _att_run(gpu_ctx, cfg, prob)
    onet = oracle_lib.Net(W.DEFAULT_SPEC, W.siren_weights(W.DEFAULT_SPEC, 0))
    ref = oracle_lib.linearize_batch(oracle_lib.quad_model(cfg), onet, prob["x"], prob["u"], prob["p"], prob["dt"], 4)
    for k in OUTS:
        assert np.isfinite(got[k]).all(), k
    print(f"\natt wide ({B}, {N}): |gpu - checker| / max(1, |ref|.max()) " + ", ".join(
        f"{k} {np.abs(got[k] - ref[k]).max() / max(1.0, np.abs(ref[k]).max()):.1e}" for k in ("xn", "AB", "y", "Jy", "yN", "JyN")))
    check_vs_oracle(got, ref, prob, oracle_lib)
    if B > 1 and not uniform:
        again = _att_run(gpu_ctx, cfg, prob)
        perm = np.random.default_rng(0).permutation(B)
        assert not np.array_equal(perm, np.arange(B))
        moved = _att_run(gpu_ctx, cfg, {k: (prob[k][perm] if k in ("x", "u", "p") else prob[k]) for k in ("x", "u", "p", "dt")})
        for k in OUTS:
            assert np.array_equal(got[k], again[k]), k
            assert np.array_equal(got[k][perm], moved[k]), k


def test_att_s03_zero_branch(gpu_ctx, oracle_lib, cfg):
    """quad_f's s03 == 0 branch (x3 = x6 = 0: yaw 0 with a zero tangent), unit and non-unit quaternions
    (test_flags.s03_zero_problem): x+ against synth.rk4 and the checker, y against the checker, to lin_close; the
    constant columns of [A | B] (p and v) exact; every output finite.  No claim about the q and u columns of
    [A | B] and J_y there: the checker has none (the derivative of atan2 at (0, 0) is 0 / 0, its columns are not
    finite), and the kernel's choice -- the yaw held at 0 -- is a convention, not a derivative."""
    prob = s03_zero_problem(cfg)
    B, N = prob["u"].shape[:2]
    got = _att_run(gpu_ctx, cfg, prob)
    for k in OUTS:
        assert np.isfinite(got[k]).all(), k
    m, lim = oracle_lib.quad_model(cfg), cfg.robot.limits
    want = np.stack([synth.rk4(prob["x"][:, k], prob["u"][:, k], prob["dt"][k], lim) for k in range(N)], 1)
    assert lin_close(got["xn"], want), np.abs(got["xn"] - want).max()
    xc, yc = np.empty((B, N, 10)), np.empty((B, N, 11))
    for b in range(B):
        for k in range(N):
            xc[b, k] = oracle_lib.rk4(m, prob["x"][b, k], prob["u"][b, k], prob["dt"][k])[0]
            yc[b, k] = oracle_lib.cost(m, prob["x"][b, k], prob["u"][b, k], prob["p"][b, k])[0]
    assert lin_close(got["xn"], xc) and lin_close(got["y"], yc), (np.abs(got["xn"] - xc).max(), np.abs(got["y"] - yc).max())
    assert (got["xn"][..., 3] == 0).all() and (got["xn"][..., 6] == 0).all()  # the whole step stayed on the branch
    AB = got["AB"]  # [B, N, 14 columns, 10 rows]
    for k in range(N):
        dt = prob["dt"][k]
        hs = ((dt / 6 + dt / 3) + dt / 3) + dt / 6  # the RK4 accumulation's order
        for j in range(3):
            e = np.zeros(10); e[j] = 1.0
            assert (AB[:, k, j] == e).all()
            e = np.zeros(10); e[j], e[7 + j] = hs, 1.0
            assert (AB[:, k, 7 + j] == e).all()
