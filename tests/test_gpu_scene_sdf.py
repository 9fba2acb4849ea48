"""The exact scene distance as the SDF row (csrc/scene_sdf.hip, sdfnmpc_scene_sdf_rows): the rows kernel against
tests/scene_sdf_ref.py (1e-12 on decided rows, the bar of scene_distance), a dynamic set with and without per-node
times, batch independence, the static set under any clock, the refusals, the phase split with lin_args.sdf_scene
(bitwise linearize + scene_sdf_rows + qp_solve) and Nmpc.set_pose_device (bitwise set_latent_device's pose columns)."""
import numpy as np
import pytest

import flag_sets as F
import scene_dyn_ref as D
import scene_ref as R
import scene_sdf_ref as S
import scene_setup
from sdf_nmpc_amd import _lib
from sdf_nmpc_amd.config import Config
from sdf_nmpc_amd.scene import Scene

pytestmark = [pytest.mark.gpu, pytest.mark.filterwarnings("ignore:no SDF weights")]

MAX_DF = 1.0
NP = 17
ATOL = 1e-12
# a second static scene beside scene_ref.SCENE: instances alternate between the two
OTHER = [("sphere", [1.0, 1.0, 0.0, 0.6]), ("cylinder", [4.0, -1.0, 0.5, -1.0, 1.0]), ("box", [1.5, -2.5, -1.0, 2.5, -1.5, 0.5])]
SHAPES = [(1, 10), (3, 10), (37, 6)]  # 11 rows; 33 rows, one partial block; 259 rows, a full 256-lane block and a tail


def _dyn_prims():
    return [Scene.moving(p, **kw) if kw is not None else p for p, kw in D.SPEC]


def _inputs(B, N, seed):
    """Node positions from scene_sdf_ref's box (the other state entries are noise the kernel must not read), the flag
    off at every third node, the rest of p noise."""
    rng = np.random.default_rng(seed)
    x = rng.normal(0, 1, (B, N + 1, 10))
    x[..., :3] = S.draw(B * (N + 1), seed).reshape(B, N + 1, 3)
    p = rng.normal(0, 1, (B, N + 1, NP))
    p[..., 0] = 1.0
    p[:, 2::3, 0] = 0.0
    return x, p


def _run(ctx, scene, B, N, x, p, **kw):
    """-> h [B, N+1, 3], Jh [B, N+1, 10, 3] of a launch on NaN-filled outputs"""
    dx, dp = _lib.DeviceArray.from_numpy(ctx, x), _lib.DeviceArray.from_numpy(ctx, p)
    dh = _lib.DeviceArray.from_numpy(ctx, np.full((B, N + 1, 3), np.nan))
    dJ = _lib.DeviceArray.from_numpy(ctx, np.full((B, N + 1, 10, 3), np.nan))
    tau = kw.pop("tau", None)
    dtau = None if tau is None else _lib.DeviceArray.from_numpy(ctx, np.asarray(tau, float))
    _lib.scene_sdf_rows(ctx, scene.h, B, N, p.shape[-1], dx, dp, dh, dJ, kw.pop("max_df", MAX_DF),
                        scene_of=scene._scene_of, tau=dtau, **kw)
    return dh.numpy(), dJ.numpy()


def _check_layout(h, J):
    """Column 2 finite everywhere (the seven zero columns too), columns 0 and 1 untouched."""
    assert np.isfinite(h[..., 2]).all() and np.isfinite(J[..., 2]).all()
    assert not J[:, :, 3:, 2].any()
    assert np.isnan(h[..., :2]).all() and np.isnan(J[..., :2]).all()


def _compare(h, J, want_h, want_J, ok, what):
    eh, eJ = np.abs(h[..., 2] - want_h)[ok], np.abs(J[..., 2] - want_J)[ok]
    print(f"\n{what}: {ok.size - ok.sum()} of {ok.size} rows undecided; max error h {eh.max():.2e}, J_h {eJ.max():.2e}")
    assert ok.mean() >= 0.99
    assert eh.max() <= ATOL and eJ.max() <= ATOL


@pytest.mark.parametrize("B,N", SHAPES)
def test_rows_kernel_vs_reference(gpu_ctx, B, N):
    scenes = [R.SCENE, OTHER]
    so = np.arange(B) % 2
    scene = Scene(gpu_ctx, scenes, scene_of=so)
    assert not scene.is_dynamic
    x, p = _inputs(B, N, seed=100 + B)
    h, J = _run(gpu_ctx, scene, B, N, x, p)
    _check_layout(h, J)
    want = [S.sdf_rows(scenes[s], x[b], p[b], MAX_DF) for b, s in enumerate(so)]
    ok = np.stack([S.decided(scenes[s], x[b], MAX_DF) for b, s in enumerate(so)])
    _compare(h, J, np.stack([w[0] for w in want]), np.stack([w[1] for w in want]), ok, f"static B={B} N={N}")
    off = p[..., 0] == 0.0
    assert off.any() and (h[..., 2][off] == MAX_DF).all() and not J[..., 2][off].any()
    if B == 37:  # on the reference alone: the case holds an inside row, a truncated row and an untruncated one
        d = np.stack([S.dist_grad(scenes[s], x[b, :, :3])[0] for b, s in enumerate(so)])
        on = ~off
        assert (d[on] < 0).any() and (d[on] >= MAX_DF).any() and ((d[on] > 0) & (d[on] < MAX_DF)).any()
    scene.close()


@pytest.mark.parametrize("t0", D.TIMES)
def test_dynamic_set_with_and_without_node_times(gpu_ctx, t0):
    B, N = 5, 10
    prims = D.scene()
    scene = Scene(gpu_ctx, _dyn_prims())
    assert scene.is_dynamic
    x, p = _inputs(B, N, seed=7)
    x[:, 1:, :3] = x[:, :1, :3] + 0.05 * np.arange(1, N + 1)[None, :, None]  # a short path: the scene moves under it
    tau = np.concatenate([[0.0], np.cumsum(np.full(N, 0.15))])
    h0, J0 = _run(gpu_ctx, scene, B, N, x, p, t0=t0)
    h1, J1 = _run(gpu_ctx, scene, B, N, x, p, t0=t0, tau=tau)
    for (h, J), tk, what in (((h0, J0), None, "frozen"), ((h1, J1), tau, "tau")):
        _check_layout(h, J)
        want_h, want_J = S.sdf_rows(prims, x, p, MAX_DF, t0=t0, tau=tk)
        _compare(h, J, want_h, want_J, S.decided(prims, x, MAX_DF, t0=t0, tau=tk), f"dynamic t0={t0} {what}")
    np.testing.assert_array_equal(h0[:, 0, 2], h1[:, 0, 2])  # tau[0] = 0: node 0 is the same row
    np.testing.assert_array_equal(J0[:, 0, :, 2], J1[:, 0, :, 2])
    assert (h0[:, 1:, 2] != h1[:, 1:, 2]).any()              # and a later node sees another scene
    scene.close()


def test_rows_do_not_depend_on_their_place_in_the_batch(gpu_ctx):
    B, N = 37, 6
    x, p = _inputs(B, N, seed=3)
    so = np.arange(B) % 2
    perm = np.random.default_rng(1).permutation(B)
    tau = 0.1 * np.arange(N + 1)
    for prims, kw in (([R.SCENE, OTHER], {}), ([_dyn_prims(), OTHER], dict(t0=0.7, tau=tau))):
        a = Scene(gpu_ctx, prims, scene_of=so)
        b = Scene(gpu_ctx, prims, scene_of=so[perm])
        ha, Ja = _run(gpu_ctx, a, B, N, x, p, **dict(kw))
        hb, Jb = _run(gpu_ctx, b, B, N, x[perm], p[perm], **dict(kw))
        np.testing.assert_array_equal(ha[perm][..., 2], hb[..., 2])
        np.testing.assert_array_equal(Ja[perm][..., 2], Jb[..., 2])
        a.close()
        b.close()


def test_static_set_gives_the_same_bits_at_any_time(gpu_ctx):
    B, N = 3, 10
    # a motion record without motion: the set is not dynamic and takes the static kernel
    scene = Scene(gpu_ctx, [Scene.moving(R.SCENE[0])] + list(R.SCENE[1:]))
    assert not scene.is_dynamic
    x, p = _inputs(B, N, seed=9)
    h0, J0 = _run(gpu_ctx, scene, B, N, x, p)
    for kw in (dict(t0=1.7), dict(t0=-3.0, tau=0.2 * np.arange(N + 1))):
        h, J = _run(gpu_ctx, scene, B, N, x, p, **kw)
        np.testing.assert_array_equal(h[..., 2], h0[..., 2])
        np.testing.assert_array_equal(J[..., 2], J0[..., 2])
    scene.close()


def test_refusals_leave_the_outputs_untouched(gpu_ctx):
    B, N = 3, 10
    scene = Scene(gpu_ctx, R.SCENE)
    other_ctx = _lib.Context(gpu_ctx.device)
    elsewhere = Scene(other_ctx, R.SCENE)
    x, p = _inputs(B, N, seed=2)
    d = {k: _lib.DeviceArray.from_numpy(gpu_ctx, v) for k, v in
         dict(x=x, p=p, h=np.full((B, N + 1, 3), -7.0), Jh=np.full((B, N + 1, 10, 3), -7.0)).items()}

    def call(scene_h=scene.h, B=B, N=N, np_=NP, max_df=MAX_DF, t0=0.0, **null):
        a = {k: (None if k in null else v) for k, v in d.items()}
        _lib.scene_sdf_rows(gpu_ctx, scene_h, B, N, np_, a["x"], a["p"], a["h"], a["Jh"], max_df, t0=t0)

    for kw in (dict(scene_h=None), dict(B=-1), dict(N=0), dict(np_=16), dict(max_df=0.0), dict(max_df=-1.0),
               dict(max_df=float("inf")), dict(max_df=float("nan")), dict(t0=float("nan")), dict(t0=float("inf")),
               dict(scene_h=elsewhere.h), dict(x=1), dict(p=1), dict(h=1), dict(Jh=1)):
        with pytest.raises(_lib.SdfnmpcError, match="error -1"):
            call(**kw)
        gpu_ctx.synchronize()
        assert (d["h"].numpy() == -7.0).all() and (d["Jh"].numpy() == -7.0).all()
    call(B=0)  # a no-op
    gpu_ctx.synchronize()
    assert (d["h"].numpy() == -7.0).all() and (d["Jh"].numpy() == -7.0).all()
    call()     # and the same arguments unrefused do write
    assert (d["h"].numpy()[..., 2] != -7.0).all()
    elsewhere.close()
    other_ctx.close()
    scene.close()


# ---- the phase split with the scene source
OUT = ("xn", "AB", "y", "Jy", "yN", "JyN", "h", "Jh", "dx", "du", "slack", "status", "iters", "res")


def _problem(gpu_ctx, name, B, N, seed):
    """flag_sets' synthetic problem of a set on the device (outputs NaN-filled), and a scene placed on its iterate: a
    sphere 0.6 m off every instance's node 5 (up to 16 of them), so that SDF rows are untruncated."""
    cfg = F.config(name, mpc__N=N)
    q = F.quad(name, cfg)
    prob = F.problem(cfg, q, B, N, seed)
    x0 = prob["x"][:, 0] + np.random.default_rng(seed).normal(0, 0.05, (B, 10))
    prims = [("sphere", list(prob["x"][b, 5, :3] + np.array([0.6, 0.0, 0.0])) + [0.3]) for b in range(min(B, 16))]

    def bufs():
        t = {k: _lib.DeviceArray.from_numpy(gpu_ctx, v) for k, v in
             dict(x=prob["x"], u=prob["u"], p=prob["p"], dt=prob["dt"], x0=x0, yref=prob["yref"], W=prob["W"],
                  yNref=prob["yN"], WN=prob["WN"]).items()}
        sh = dict(xn=(B, N, 10), AB=(B, N, 14, 10), y=(B, N, 11), Jy=(B, N, 14, 11), yN=(B, q.nyN), JyN=(B, 10, q.nyN),
                  h=(B, N + 1, 3), Jh=(B, N + 1, 10, 3), hE=(B, 6), JhE=(B, 10, 6), dx=(B, N + 1, 10), du=(B, N, 4),
                  slack=(B, N + 1, 3, 2), res=(B, 2))
        for k, s in sh.items():
            t[k] = _lib.DeviceArray.from_numpy(gpu_ctx, np.full(s, np.nan))
        for k in ("status", "iters"):
            t[k] = _lib.DeviceArray.from_numpy(gpu_ctx, np.full(B, -1, np.int32))
        return t

    return cfg, q, prob, prims, bufs


@pytest.mark.parametrize("name", ["default", "sdf_cost_only", "rec_feas_no_sdf_row"])
@pytest.mark.parametrize("B,N,kernel", [(24, 20, "auto"), (3, 40, "segmented")])
def test_phase_split_with_scene_source_bitwise(gpu_ctx, name, B, N, kernel):
    """rti_prepare(lin_args.sdf_scene) + qp_feedback == linearize(net) ; scene_sdf_rows ; qp_solve on the same buffers,
    bit for bit, also with net == NULL -- on the serial QP kernel and with the segmented one forced; the default rows,
    the sdf cost (H and g read h[2]) and the set whose only SDF row is the terminal braking row (no stage row to patch:
    the split-pack case)."""
    cfg, q, prob, prims, bufs = _problem(gpu_ctx, name, B, N, seed=13)
    scene = Scene(gpu_ctx, prims)
    net = _lib.Net.from_file(gpu_ctx, scene_setup.SCENE) if F.uses_scene(q) else _lib.Net.siren(gpu_ctx, 0)
    qm, opts = _lib.quad_model(cfg, q), _lib.qp_opts(q)
    src = _lib.scene_sdf_opts(scene.h, q.max_df, t0=0.4)
    ta, tb, tc = bufs(), bufs(), bufs()
    gpu_ctx.set_qp_kernel(kernel)
    try:
        assert gpu_ctx.qp_kernel(N, B, opts) == ("segmented" if kernel == "segmented" else "serial")
        _lib.linearize(gpu_ctx, net, qm, B, N, q.np, ta, nyN=q.nyN)
        _lib.scene_sdf_rows(gpu_ctx, scene.h, B, N, q.np, ta["x"], ta["p"], ta["h"], ta["Jh"], q.max_df, t0=0.4)
        _lib.qp_solve(gpu_ctx, opts, B, N, ta)
        _lib.rti_prepare(gpu_ctx, net, qm, opts, B, N, q.np, tb, sdf_scene=src)
        _lib.qp_feedback(gpu_ctx, opts, B, N, tb)
        _lib.rti_prepare(gpu_ctx, None, qm, opts, B, N, q.np, tc, sdf_scene=src)  # no network at all
        _lib.qp_feedback(gpu_ctx, opts, B, N, tc)
        # linearize alone takes the source too, and refuses it beside no_sdf; a captured step refuses it
        td = bufs()
        _lib.linearize(gpu_ctx, None, qm, B, N, q.np, td, nyN=q.nyN, sdf_scene=src)
        with pytest.raises(_lib.SdfnmpcError, match="error -1"):
            _lib.linearize(gpu_ctx, None, qm, B, N, q.np, td, nyN=q.nyN, no_sdf=True, sdf_scene=src)
        with pytest.raises(_lib.SdfnmpcError, match="error -4"):
            _lib.RtiStep(gpu_ctx, net, qm, opts, B, N, q.np, bufs(), graph=True, sdf_scene=src)
        gpu_ctx.synchronize()
    finally:
        gpu_ctx.set_qp_kernel("auto")
    a = {k: ta[k].numpy() for k in OUT}
    h2 = a["h"][..., 2]
    print(f"\n{name} B={B} N={N} {kernel}: status {a['status'].tolist()}, {int((h2 < q.max_df).sum())} of {h2.size} rows "
          f"untruncated, min h2 {h2.min():.3f}")
    assert np.isfinite(h2).all() and (h2 < q.max_df).any()  # the scene reached the rows
    for t in (tb, tc):
        for k in OUT:
            np.testing.assert_array_equal(a[k], t[k].numpy(), err_msg=k)
    for k in ("h", "Jh", "xn", "AB"):
        np.testing.assert_array_equal(a[k], td[k].numpy(), err_msg=k)
    net.close()
    scene.close()


# ---- the pose-only parameter update
@pytest.mark.parametrize("device_arrays", [False, True])
def test_set_pose_device_writes_set_latent_device_s_pose_bits(gpu_ctx, device_arrays):
    from sdf_nmpc_amd.controller import Nmpc
    B = 3
    n = Nmpc(Config(mpc__N=10), batch=B)
    ctx = n.ocp.ctx
    rng = np.random.default_rng(4)
    lat = rng.normal(0, 1, (B, 128))
    pose = []
    for _ in range(2):
        q = rng.normal(0, 1, (B, 4))
        pose.append((rng.normal(0, 2, (B, 3)), np.stack([R.quat2rot(v) for v in q]).reshape(B, 9)))
    dev = (lambda a: _lib.DeviceArray.from_numpy(ctx, a)) if device_arrays else (lambda a: a)
    n.set_latent_device(lat, *pose[0], flag=np.array([1.0, 0.0, 0.5]))
    p0 = n.ocp.download("p")
    n.set_pose_device(dev(pose[1][0]), dev(pose[1][1]))
    p1 = n.ocp.download("p")
    n.set_latent_device(lat, *pose[1])
    p2 = n.ocp.download("p")
    np.testing.assert_array_equal(p1[..., 1:13], p2[..., 1:13])   # the pose columns: the same bits
    assert (p1[..., 1:13] != p0[..., 1:13]).any()
    np.testing.assert_array_equal(p1[..., 0], p0[..., 0])         # flag and latent (and q_d): untouched
    np.testing.assert_array_equal(p1[..., 13:], p0[..., 13:])
    assert (p0[..., 0] == np.array([1.0, 0.0, 0.5])[:, None]).all() and np.abs(p0[..., 17:]).max() > 0
    n.ocp.close()
