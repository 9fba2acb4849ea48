"""The controller mirror end to end on the GPU: Nmpc.set_x0 / set_latent / set_ref / solve (one
SQP-RTI iteration per instance) against the CPU pipeline oracle.linearize_batch + qp_oracle
(dense Mehrotra IPM) from the same iterate; Ocp.init / shift semantics (ocp.py:144-156)."""
import os

import numpy as np
import pytest

from sdf_nmpc_amd import weights as W
from sdf_nmpc_amd.config import Config
from sdf_nmpc_amd.controller import Nmpc
from sdf_nmpc_amd.reference import Ref, yaw2quat
from tolerances import sdf_df_ok

pytestmark = [pytest.mark.gpu, pytest.mark.filterwarnings("ignore:no SDF weights")]

U0_ATOL = 2e-5   # fp32 SDF rows differ from the oracle's by ~1e-7 rel; the QP solutions agree to ~1e-6
# flags.sdf_cost puts the fp32 SDF gradient (parity bar 1e-5 rel) into the Hessian
# with weight 20 through J = -2 (1 - s/2)^3 ds/dx; the GPU-vs-oracle QP parity on IDENTICAL
# linearisations stays at 1e-5 (tests/test_gpu_qp.py::test_qp_sdf_cost_matches_riccati_oracle)
U0_ATOL_SDF_COST = 1e-4


def scenario(n, rng):
    """Random but feasible-looking control problems through the reference API."""
    B, N = max(n.B, 1), n.N
    x0 = np.zeros((B, 10))
    x0[:, :3] = rng.uniform(-1, 1, (B, 3))
    x0[:, 3:7] = np.stack([yaw2quat(y) for y in rng.uniform(-np.pi, np.pi, B)])
    x0[:, 7:] = rng.normal(0, 0.3, (B, 3))
    lat = rng.normal(0, 1, (B, 128))
    pos = x0[:, :3] + rng.normal(0, 0.2, (B, 3))
    R = np.stack([np.eye(3)] * B)
    goal = x0[:, :3] + rng.uniform(-3, 3, (B, 3))
    sq = (lambda a: a[0]) if n.B == 1 else (lambda a: a)
    n.set_sdf_flag(1.0)
    n.set_latent(sq(lat), sq(pos), sq(R))
    for b in range(B):
        for k in range(N + 1):
            r = Ref(n.cfg)
            r.p, r.q = goal[b], yaw2quat(0.3 * b)
            r.use_weights(r.W_on)
            n.set_ref(r, k, b=None if n.B == 1 else b)
    return sq(x0)


def eval_sdf_ref(onet, n, k):
    """What column 0 of Nmpc.eval(k) is: the checker's network (fp64 evaluation of the fp32 weights) at node k of the
    controller's iterate, at the fp32 input the device kernel reads -- the camera-frame position W_R_Co^T (p_k -
    W_p_Co) and the latent of node k's parameters (gen_model.py:64, flag = 1)."""
    idx = n.cfg.mpc.p_idx
    x = n.ocp.download("x")[:, k]
    pk = (n.p if n.B > 1 else n.p[None])[:, k]
    Co_p_B = np.einsum("bji,bj->bi", pk[:, idx.W_R_Co].reshape(-1, 3, 3), x[:, :3] - pk[:, idx.W_p_Co])
    inp = np.concatenate([Co_p_B.astype(np.float32).astype(np.float64), pk[:, idx.latent:].astype(np.float32)], 1)
    return onet.f64(inp)[0]


def oracle_u0(n, x0, oracle_lib):
    import qp_oracle
    O = oracle_lib
    B, N = max(n.B, 1), n.N
    x0 = np.atleast_2d(x0)
    xbar = np.repeat(x0[:, None], N + 1, axis=1)
    ubar = np.broadcast_to(n.model.u_hover, (B, N, 4)).copy()
    p = n.p if n.B > 1 else n.p[None]
    y, Wt, yN, WN = (a if n.B > 1 else a[None] for a in (n.y, n.W, n.yN, n.WN))
    onet = O.Net(W.DEFAULT_SPEC, W.siren_weights(W.DEFAULT_SPEC, seed=0))
    lin = O.linearize_batch(O.quad_model(n.cfg), onet, xbar, ubar, p, n.ocp.dt)
    u0 = []
    for b in range(B):
        q = qp_oracle.stage_qp({k: v[b] for k, v in lin.items() if k != "sdf"}, xbar[b], ubar[b], x0[b], y[b], Wt[b],
                               yN[b], WN[b], n.ocp.dt, n.model, float(n.cfg.mpc.lm_reg))
        u0.append(ubar[b, 0] + qp_oracle.solve_dense(q)["du"][0])
    return np.array(u0)


@pytest.mark.parametrize("B,sdf_cost", [(1, False), (3, False), (3, True)])
def test_nmpc_rti_step_matches_oracle(oracle_lib, B, sdf_cost):
    n = Nmpc(Config(flags__sdf_cost=sdf_cost), batch=B)
    assert n.model.ny == (12 if sdf_cost else 11) and n.W.shape[-1] == n.model.ny
    x0 = scenario(n, np.random.default_rng(10 + B))
    n.set_x0(x0)
    assert n.solve() == 0
    assert (n.ocp.status == 0).all()
    u = np.atleast_2d(n.get_u())
    np.testing.assert_allclose(u, oracle_u0(n, x0, oracle_lib), rtol=0, atol=U0_ATOL_SDF_COST if sdf_cost else U0_ATOL)
    assert (u >= n.model.lbu - 1e-9).all() and (u <= n.model.ubu + 1e-9).all()
    x, uu = n.get_matrices()
    np.testing.assert_array_equal(np.atleast_2d(u), np.atleast_2d(uu[..., 0, :]))
    np.testing.assert_allclose(x[..., 0, :], x0, atol=1e-12)
    ev = np.atleast_1d(n.eval(3))
    assert ev.shape == ((1,) if B == 1 else (B, 1))
    onet = oracle_lib.Net(W.DEFAULT_SPEC, W.siren_weights(W.DEFAULT_SPEC, seed=0))
    assert sdf_df_ok(ev.reshape(-1), eval_sdf_ref(onet, n, 3))  # by value: the network's df at node 3, flag = 1
    n.ocp.close()


def test_batch_equals_single_instances():
    rng = np.random.default_rng(5)
    nb = Nmpc(Config(), batch=3)
    x0 = scenario(nb, rng)
    nb.set_x0(x0)
    nb.solve()
    ub = nb.get_u()
    for b in range(3):
        n1 = Nmpc(Config(), batch=1)
        n1.p, n1.y, n1.W, n1.yN, n1.WN = (a[b].copy() for a in (nb.p, nb.y, nb.W, nb.yN, nb.WN))
        n1.set_x0(x0[b])
        n1.solve()
        np.testing.assert_allclose(n1.get_u(), ub[b], rtol=0, atol=1e-12)
        n1.ocp.close()
    nb.ocp.close()


def test_ocp_init_and_shift():
    n = Nmpc(Config(mpc__shift=2), batch=2)
    x0 = np.arange(20.0).reshape(2, 10)
    n.set_x0(x0)
    o = n.ocp
    np.testing.assert_array_equal(o.download("x"), np.repeat(x0[:, None], n.N + 1, 1))
    np.testing.assert_array_equal(o.download("u"), np.broadcast_to(n.model.u_hover, (2, n.N, 4)))
    rng = np.random.default_rng(0)
    xs, us = rng.normal(size=(2, n.N + 1, 10)), rng.normal(size=(2, n.N, 4))
    o.upload("x", xs)
    o.upload("u", us)
    o.shift(2)
    X, U = o.download("x"), o.download("u")
    assert np.array_equal(X[:, : n.N - 2], xs[:, 2: n.N]) and np.array_equal(X[:, n.N - 2:], xs[:, n.N - 2:])
    assert np.array_equal(U[:, : n.N - 2], us[:, 2:]) and np.array_equal(U[:, n.N - 2:], us[:, n.N - 2:])
    o.solver.set(4, "u", [0.1, 0.2, 0.3, 0.4])
    np.testing.assert_array_equal(o.solver.get(4, "u"), np.broadcast_to([0.1, 0.2, 0.3, 0.4], (2, 4)))
    np.testing.assert_array_equal(np.delete(o.download("u"), 4, axis=1), np.delete(U, 4, axis=1))
    o.close()


def test_controller_path_is_torch_free():
    """the Nmpc.solve path needs no tensor library -- run it in a fresh process where
    importing torch fails."""
    import subprocess
    import sys
    import textwrap
    code = textwrap.dedent("""
        import sys, warnings
        sys.modules["torch"] = None  # any import of torch raises ImportError
        sys.path.insert(0, %r)
        warnings.simplefilter("ignore")
        import numpy as np
        import sdf_nmpc_amd
        from sdf_nmpc_amd.config import Config
        from sdf_nmpc_amd.controller import Nmpc
        from sdf_nmpc_amd.reference import Ref
        n = Nmpc(Config(mpc__N=20), batch=3)
        n.set_sdf_flag(1.0)
        n.set_latent(np.zeros((3, 128)), np.zeros((3, 3)), np.stack([np.eye(3)] * 3))
        for k in range(21):
            r = Ref(n.cfg); r.p = np.array([1.0, 0, 1]); r.use_weights(r.W_on); n.set_ref(r, k)
        x0 = np.zeros((3, 10)); x0[:, 3] = 1.0
        n.set_x0(x0)
        for _ in range(3):
            assert n.solve() == 0
        n.gen_refs_device("hover")
        assert n.solve() == 0
        u = n.get_u(); assert u.shape == (3, 4) and np.isfinite(u).all()
        print("torch-free ok", "torch" in sys.modules and sys.modules["torch"] is not None)
    """) % os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-3000:]
    assert "torch-free ok False" in r.stdout


def test_host_set_ref_after_device_refs_keeps_device_regions(oracle_lib):
    """gen_refs_device / set_latent_device write the device; a later host set_ref at one node
    uploads only that node's rows, so the device-written latents and the other nodes survive."""
    rng = np.random.default_rng(3)
    B = 2
    na, nb = Nmpc(Config(mpc__N=20), batch=B), Nmpc(Config(mpc__N=20), batch=B)
    x0 = scenario(na, rng)
    lat = rng.normal(size=(B, 128))
    pos, R = rng.normal(size=(B, 3)), np.stack([np.eye(3)] * B)
    for n in (na, nb):
        n.set_x0(x0)
        n.set_latent_device(lat, pos, R, flag=1.0)  # device-side latent + flag
        n.gen_refs_device("hover")                  # device-side references at every node
    r = Ref(na.cfg)
    r.p, r.q = np.array([0.5, -0.5, 1.0]), yaw2quat(0.2)
    r.use_weights(r.W_on)
    na.set_ref(r, 7)                                # host override of node 7 only
    na.solve()
    # the same state built by hand: download the device buffers of nb and apply node 7 on the host
    p = nb.ocp.download("p")
    y, Wt = nb.ocp.download("yref"), nb.ocp.download("W")
    yr, wr = nb.model.formate_ref(r)
    p[:, 7, 13:17], y[:, 7], Wt[:, 7] = r.q, yr, wr
    nb.ocp.solve(x0, y, nb.ocp.download("yNref")[:, 0], Wt, nb.ocp.download("WN")[:, 0], p)
    np.testing.assert_array_equal(na.get_u(), nb.get_u())
    np.testing.assert_array_equal(na.ocp.download("p")[..., 17:], np.broadcast_to(lat[:, None], (B, 21, 128)))
    na.ocp.close()
    nb.ocp.close()
