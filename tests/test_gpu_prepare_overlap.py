"""The preparation phase's schedule: sdfnmpc_rti_prepare forks linearize and the QP record pack
onto the auxiliary stream before the latent hoist, so they run beside sdf_hoist / sdf_mlp.  Only launch order,
streams and priorities differ from the serial preparation (SDFNMPC_SERIAL_PREP=1 at context creation: every
kernel on the one stream, the whole pack after the SDF kernel), so every output is bitwise the same; and an
early-forked linearize or pack must not touch what the previous step's QP still reads.

Shapes: more than 64 rows (at or below it the few-row path runs serially whatever the context).  B = 5, N = 13
is 70 nodes: 17.5 pack workgroups of four nodes (the last one partial) and 2.2 SDF tiles of 32 rows; B = 2,
N = 40 is the flagship horizon (82 rows, the segmented QP kernel)."""
import os

import numpy as np
import pytest

import flag_sets as F
from sdf_nmpc_amd import _lib

pytestmark = pytest.mark.gpu

OUT = ("xn", "AB", "y", "Jy", "yN", "JyN", "h", "Jh", "sdf", "dx", "du", "status", "iters")
SEED = 13


@pytest.fixture(scope="module")
def serial_ctx(gpu_ctx):
    """A context with the serial preparation on the same stream (the variable is read at creation only)."""
    import torch
    prev = os.environ.get("SDFNMPC_SERIAL_PREP")
    os.environ["SDFNMPC_SERIAL_PREP"] = "1"
    try:
        ctx = _lib.Context(gpu_ctx.device, stream=torch.cuda.current_stream().cuda_stream)
    finally:
        if prev is None:
            del os.environ["SDFNMPC_SERIAL_PREP"]
        else:
            os.environ["SDFNMPC_SERIAL_PREP"] = prev
    yield ctx
    ctx.close()


def _problem(name, B, N):
    cfg = F.config(name, mpc__N=N)
    q = F.quad(name, cfg)
    prob = F.problem(cfg, q, B, N, SEED)
    x0 = prob["x"][:, 0] + np.random.default_rng(SEED).normal(0, 0.05, (B, 10))
    return cfg, q, prob, x0


def _bufs(ctx, q, prob, x0, B, N):
    import torch
    dev = torch.device("cuda", ctx.device)
    t = {k: torch.from_numpy(np.ascontiguousarray(v)).to(dev) for k, v in
         dict(x=prob["x"], u=prob["u"], p=prob["p"], dt=prob["dt"], x0=x0, yref=prob["yref"], W=prob["W"],
              yNref=prob["yN"], WN=prob["WN"]).items()}
    sh = dict(xn=(B, N, 10), AB=(B, N, 14, 10), y=(B, N, 11), Jy=(B, N, 14, 11), yN=(B, q.nyN), JyN=(B, 10, q.nyN),
              h=(B, N + 1, 3), Jh=(B, N + 1, 10, 3), hE=(B, 6), JhE=(B, 10, 6), dx=(B, N + 1, 10), du=(B, N, 4),
              slack=(B, N + 1, 3, 2), res=(B, 2))
    for k, s in sh.items():
        t[k] = torch.full(s, float("nan"), dtype=torch.float64, device=dev)
    t["sdf"] = torch.full((B, N + 1, 4), float("nan"), dtype=torch.float32, device=dev)
    t["status"] = torch.full((B,), -1, dtype=torch.int32, device=dev)
    t["iters"] = torch.full((B,), -1, dtype=torch.int32, device=dev)
    return t


def _net(ctx, q):
    if F.uses_scene(q):
        import scene_setup as S
        return _lib.Net.from_file(ctx, S.SCENE)
    return _lib.Net.siren(ctx, 0)


def _np(t, keys):
    return {k: t[k].cpu().numpy() for k in keys}


# default: the split pack beside the SDF kernel, the sdf row of C^T patched by the QP kernel; sdf_cost_only:
# ny = 12, the whole pack follows the join; rec_feas_no_sdf_row: the network read by the terminal braking row
# only, sdf_row == -1 (split pack, nothing to patch)
@pytest.mark.parametrize("name,B,N", [("default", 5, 13), ("default", 2, 40), ("sdf_cost_only", 5, 13),
                                      ("rec_feas_no_sdf_row", 5, 13)])
def test_forked_preparation_bitwise_equals_serial(gpu_ctx, serial_ctx, name, B, N):
    import torch
    cfg, q, prob, x0 = _problem(name, B, N)
    assert B * (N + 1) > 64 and q.need_sdf
    assert (q.ny == 12) == (name == "sdf_cost_only")
    opts, qm = _lib.qp_opts(q), _lib.quad_model(cfg, q)
    if name == "rec_feas_no_sdf_row":
        assert 2 not in list(opts.h_col)[:opts.nh]  # no stage row reads J_h's sdf column
    got = {}
    for key, ctx in (("forked", gpu_ctx), ("serial", serial_ctx)):
        t = _bufs(ctx, q, prob, x0, B, N)
        _lib.rti_prepare(ctx, _net(ctx, q), qm, opts, B, N, q.np, t)
        _lib.qp_feedback(ctx, opts, B, N, t)
        torch.cuda.synchronize()
        got[key] = _np(t, OUT)
    assert (got["serial"]["iters"] >= 1).all() and (got["serial"]["status"] >= 0).all()  # the QP ran
    for k in OUT:
        np.testing.assert_array_equal(got["forked"][k], got["serial"][k], err_msg=k)


def test_back_to_back_steps_equal_one_step_alone(gpu_ctx):
    """Three steps queued with no host synchronisation between them, each from the restored iterate as
    bench.py's step(): the next step's early fork (linearize, pack) must wait for the previous step's QP and
    update, which still read the linearisation and the stage records."""
    import torch
    B, N = 5, 13
    cfg, q, prob, x0 = _problem("default", B, N)
    opts, qm = _lib.qp_opts(q), _lib.quad_model(cfg, q)
    net = _net(gpu_ctx, q)
    keys = OUT + ("x", "u", "u0")

    def run(steps):
        t = _bufs(gpu_ctx, q, prob, x0, B, N)
        t["u0"] = torch.full((B, 4), float("nan"), dtype=torch.float64, device=t["x"].device)
        x_init, u_init = t["x"].clone(), t["u"].clone()
        x_init[:, 0].copy_(t["x0"])
        torch.cuda.synchronize()
        for _ in range(steps):
            t["x"].copy_(x_init)
            t["u"].copy_(u_init)
            _lib.rti_prepare(gpu_ctx, net, qm, opts, B, N, q.np, t)
            _lib.qp_feedback(gpu_ctx, opts, B, N, t)
            _lib.rti_apply(gpu_ctx, B, N, t["x"], t["u"], t["dx"], t["du"], t["u0"])
        torch.cuda.synchronize()
        return _np(t, keys)

    one, three = run(1), run(3)
    assert (one["iters"] >= 1).all() and np.isfinite(one["u0"]).all()
    for k in keys:
        np.testing.assert_array_equal(three[k], one[k], err_msg=k)
