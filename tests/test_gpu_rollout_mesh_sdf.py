"""Closed-loop rollouts of a controller whose SDF is the exact distance of the triangle mesh it flies in
(Scene.mesh(sdf_source=True), Nmpc.set_sdf_scene): bitwise against the host-driven loop, against tests/mesh_sdf_ref.py on
the last step's rows, with and without the hierarchy, in chunks, against the CPU oracle pipeline with the SDF row from
mesh_sdf_ref past the pillar of tests/scene_setup.py restated as a mesh, and the API contract.  N = 10, B = 3, K <= 12.
The helpers are tests/test_gpu_rollout_scene_sdf.py's."""
import numpy as np
import pytest

import mesh_ref as M
import mesh_sdf_ref as MS
import test_gpu_rollout_scene_sdf as T
from sdf_nmpc_amd import _lib
from sdf_nmpc_amd import weights as W
from sdf_nmpc_amd.config import Config
from sdf_nmpc_amd.controller import Nmpc
from sdf_nmpc_amd.mesh import Mesh
from sdf_nmpc_amd.reference import Ref, yaw2quat
from sdf_nmpc_amd.scene import Scene
from sdf_nmpc_amd.vehicle import VehicleModel
from test_gpu_closed_loop import U0_ATOL
from test_gpu_rollout import _setup
from test_gpu_rollout_scene_sdf import B, K, K_ORACLE, SCENE_OF, T0, _host_loop, _start, _wps, oracle_loop

pytestmark = [pytest.mark.gpu, pytest.mark.filterwarnings("ignore:no SDF weights"),
              pytest.mark.filterwarnings("ignore:QP reached")]

# test_gpu_rollout_scene_sdf's two scenes restated as meshes: instances 0 and 2 see the fixed scene
OTHER = Mesh.merge(Mesh.icosphere((1.5, 0.5, 0.2), 0.5, 2), Mesh.box((-2.0, -2.5, -1.0), (2.0, -1.5, 1.0)))
MESHES = [OTHER, M.fixed_scene()]
PILLAR = Mesh.cylinder((3.0, 0.3), 0.4, -3.0, 3.0, 24)  # scene_setup's pillar as a closed 24-segment prism
BITES = dict(delay=2, gust_std=1.0, gust_tau=0.3, est_std_pos=0.05, est_std_vel=0.02, est_std_yaw=0.01)  # ..._vehicle.py's


@pytest.fixture(scope="module", autouse=True)
def _torch_first(gpu_ctx):
    """torch opens the device before the first controller of this module does, as in tests/test_gpu_rollout.py."""


def _make(cfg, closed=True, leaf=None, seed=21):
    n, x0 = _setup(cfg, B, seed)
    scene = Scene.mesh(n.ocp.ctx, MESHES, scene_of=SCENE_OF, closed=closed, leaf_size=leaf, sdf_source=True)
    n.set_sdf_scene(scene)
    return n, x0, scene


@pytest.mark.parametrize("closed,every", [(True, 1), (False, 3)])
def test_rollout_with_mesh_source_equals_host_driven_loop_bitwise(closed, every):
    cfg = Config(mpc__N=10)
    wps = _wps()
    na, x0, sa = _make(cfg, closed)
    nb, _, sb = _make(cfg, closed)
    assert sa.is_mesh and sa.is_sdf_source
    na.set_x0(x0)
    r = na.rollout(K, refs="wps", wps=wps, perceive_every=every, scene_t0=T0)
    x, u, status, iters = _host_loop(nb, sb, x0, K, every, wps, T0)
    np.testing.assert_array_equal(r.x, x)
    np.testing.assert_array_equal(r.u, u)
    np.testing.assert_array_equal(r.status, status)
    np.testing.assert_array_equal(r.iters, iters)
    pa, pb = na.ocp.download("p"), nb.ocp.download("p")
    np.testing.assert_array_equal(pa, pb)
    assert (r.iters > 0).all() and np.ptp(r.u[:, :, 0]) > 1e-3
    # the source reached the rows: h[2] is the reference's distance of the last linearisation point, x - dx
    h = na.ocp.download("h")
    xi = na.ocp.download("x") - na.ocp.download("dx")
    rounded = [M.rounded(m) for m in MESHES]
    want = np.stack([MS.sdf_rows(rounded[s], xi[b], pa[b], na.model.max_df, closed)[0] for b, s in enumerate(SCENE_OF)])
    ok = (r.status[:, -1] < 2)[:, None] & np.stack([MS.decided(rounded[s], xi[b], na.model.max_df, closed)
                                                     for b, s in enumerate(SCENE_OF)])
    print(f"\nlast step's h[2] against the reference on {ok.sum()} rows: {np.abs(h[..., 2] - want)[ok].max():.2e}; "
          f"{int((want < na.model.max_df).sum())} untruncated")
    # x - dx is the linearisation point up to one rounding of a coordinate (1e-15 m) and |grad| <= 1: the rows' bar
    assert ok.sum() >= 20 and (want < na.model.max_df).any() and np.abs(h[..., 2] - want)[ok].max() <= 1e-12
    # the clearance: the source scene's distance at the logged positions
    want_c = np.stack([M.distance(rounded[s], r.x[b, :, :3], signed=closed) for b, s in enumerate(SCENE_OF)])
    assert r.clearance.shape == (B, K + 1) and np.abs(r.clearance - want_c).max() <= 1e-12
    for m in (na, nb):
        m.ocp.close()


@pytest.mark.parametrize("vehicle", [False, True], ids=["plain", "vehicle"])
def test_rollout_with_the_hierarchy_equals_the_rollout_without_bitwise(vehicle):
    cfg = Config(mpc__N=10)
    out = []
    for leaf in (None, -1):
        n, x0, scene = _make(cfg, True, leaf)
        kw = dict(vehicle=VehicleModel(cfg, n.ocp.ctx, B, seed=17, **BITES)) if vehicle else {}
        n.set_x0(x0)
        out.append((n, scene, n.rollout(K, refs="wps", wps=_wps(), perceive_every=2, scene_t0=T0, swept=True, **kw)))
    (na, sa, ra), (nb, sb, rb) = out
    fields = ("x", "u", "status", "iters", "t", "clearance", "swept_clearance", "swept_gap", "swept_s") + \
        (("xhat", "u_applied") if vehicle else ())
    for f in fields:
        np.testing.assert_array_equal(getattr(ra, f), getattr(rb, f), err_msg=f)
    for k in ("p", "h", "Jh", "x", "u"):
        np.testing.assert_array_equal(na.ocp.download(k), nb.ocp.download(k), err_msg=k)
    assert (na.ocp.download("h")[..., 2] < na.model.max_df).any() and (ra.iters > 0).all()
    p2s = np.repeat(SCENE_OF, K + 1)
    np.testing.assert_array_equal(ra.clearance, sb.distance(ra.x[:, :, :3].reshape(-1, 3), p2s).reshape(B, K + 1))
    assert (ra.swept_clearance <= np.minimum(ra.clearance[:, :-1], ra.clearance[:, 1:]) + 1e-9).all()
    for m in (na, nb):
        m.ocp.close()


def test_chunks_with_phase_are_the_uncut_rollout():
    cfg = Config(mpc__N=10)
    wps = _wps()
    n, x0, _ = _make(cfg, False)
    n.set_x0(x0)
    xs, us, cl = [np.reshape(x0, (B, 10))], [], []
    for k in range(K):
        r = n.rollout(1, refs="wps", wps=wps, perceive_every=2, perceive_phase=k, scene_t0=T0)
        xs.append(r.x[:, 1])
        us.append(r.u[:, 0])
        cl.append(r.clearance)
    m, _, _ = _make(cfg, False)
    m.set_x0(x0)
    whole = m.rollout(K, refs="wps", wps=wps, perceive_every=2, scene_t0=T0)
    np.testing.assert_array_equal(whole.x, np.stack(xs, 1))
    np.testing.assert_array_equal(whole.u, np.stack(us, 1))
    np.testing.assert_array_equal(m.ocp.download("p"), n.ocp.download("p"))
    for k in range(K):
        np.testing.assert_array_equal(cl[k], whole.clearance[:, k:k + 2])
    n.ocp.close()
    m.ocp.close()


def test_rollout_with_mesh_source_matches_oracle_pipeline(oracle_lib, monkeypatch):
    """Past the pillar of scene_setup's world as a closed 24-segment prism, with its exact distance: u_0 of every step of
    every instance within U0_ATOL of the CPU loop -- test_gpu_rollout_scene_sdf.oracle_loop with the SDF row from
    mesh_sdf_ref.sdf_rows.  K_ORACLE = 12 steps from 1.1 m in front of the pillar at 1.5 m/s.  The CPU loop run alone, on a
    machine without a GPU: every QP converged; the SDF row is active at 4, 3 and 1 steps of the three instances and
    released at the last step; h2min per step 1.0, 0.076, 0.383, 0.414, 0.42, 0.32, 0.372, 0.608, 0.882, 1.0, 1.0, 1.0;
    minimum clearance 0.320 m.  Measured on the MI355X: max |u0 - u0_oracle| per step 1.6e-11 at the first step, 6.4e-8 at the
    last."""
    O = oracle_lib
    cfg = Config(mpc__N=10)
    n = Nmpc(cfg, batch=B)
    x0 = _start(n)
    scene = Scene.mesh(n.ocp.ctx, PILLAR, closed=True, sdf_source=True)
    n.set_sdf_scene(scene)
    mesh = M.rounded(PILLAR)
    monkeypatch.setattr(T.SR, "sdf_rows", lambda prims, xs, p, max_df: MS.sdf_rows(mesh, xs, p, max_df, True))
    onet = O.Net(W.DEFAULT_SPEC, W.siren_weights(W.DEFAULT_SPEC, seed=0))
    hist, x_end = oracle_loop(O, onet, n, cfg, None, x0, K_ORACLE, n.model.max_df)
    bound = n.model.lh[n.model.h_cols.index(2)]
    active = np.array([(h["sdf_slack"] > 1e-6) | (h["h2min"] <= bound + 1e-6) for h in hist])  # [K, B]
    xo = np.stack([h["x0"] for h in hist] + [x_end], 1)
    clear = np.stack([M.distance(mesh, xo[b, :, :3], signed=True) for b in range(B)])
    print(f"\nCPU loop: SDF row active at steps {[int(a.sum()) for a in active.T]} per instance, h2min per step "
          f"{np.round([h['h2min'].min() for h in hist], 3).tolist()}, min clearance {clear.min():.3f} m, final x {x_end[:, 0]}")
    assert active.any() and not active[-1].any()
    assert clear.min() > 0
    n.set_x0(x0)
    r = n.rollout(K_ORACLE)
    uo = np.stack([h["u0"] for h in hist], 1)
    d = np.abs(r.u - uo).max(axis=(0, 2))
    print(f"max |u0 - u0_oracle| per step {d}")
    assert (r.status == 0).all()
    assert d.max() <= U0_ATOL, d
    np.testing.assert_allclose(r.clearance, np.stack([M.distance(mesh, r.x[b, :, :3], signed=True) for b in range(B)]),
                               rtol=0, atol=1e-12)
    n.ocp.close()


def test_api_contract(monkeypatch):
    """set_sdf_scene(None) restores the network bitwise; the scene can be closed under the controller; scene= beside a
    source is a ValueError; a batch split over two parts is refused with its state untouched."""
    cfg = Config(mpc__N=10, mpc__shift=1)
    n, x0 = _setup(cfg, B, 21)
    n.set_x0(x0)
    before = n.rollout(3, refs="hover")
    m, _ = _setup(cfg, B, 21)
    scene = Scene.mesh(m.ocp.ctx, M.fixed_scene(), closed=True, sdf_source=True)
    m.set_sdf_scene(scene, max_df=0.75, predict=True)  # predict: accepted, a mesh set is static
    m.set_x0(x0)
    with_src = m.rollout(3, refs="hover")
    with pytest.raises(ValueError):
        m.rollout(2, refs="hover", scene=scene, vae=object())
    m.set_sdf_scene(None)
    m.reset()  # as test_set_sdf_scene_none_restores_the_network: every host region is uploaded again
    m.p[...], m.y[...], m.W[...], m.yN[...], m.WN[...] = n.p, n.y, n.W, n.yN, n.WN
    m.set_x0(x0)
    after = m.rollout(3, refs="hover")
    for k in ("x", "u", "status", "iters"):
        np.testing.assert_array_equal(getattr(before, k), getattr(after, k))
    np.testing.assert_array_equal(n.ocp.download("p"), m.ocp.download("p"))
    assert before.clearance is None and after.clearance is None and with_src.clearance is not None
    assert (with_src.u != before.u).any()
    # closing the scene while it is the source returns to the network first
    m.set_sdf_scene(scene)
    assert m._sdf_scene is scene
    scene.close()
    assert m._sdf_scene is None
    plant = _lib.plant_opts(cfg, dt=float(m.ocp.dt[0]))
    xl, ul = _lib.DeviceArray(m.ocp.ctx, (B, 3, 10)), _lib.DeviceArray(m.ocp.ctx, (B, 2, 4))
    with pytest.raises(_lib.SdfnmpcError, match="no scene source"):
        m.ocp.parts[0].solver.rollout_scene_sdf(2, plant, xl, ul)
    r = m.rollout(2, refs="hover")
    assert r.clearance is None and np.isfinite(r.u).all()
    n.ocp.close()
    m.ocp.close()
    # a batch split over two parts (test_gpu_rollout_scene_sdf's way to one on a single device)
    from sdf_nmpc_amd import ocp as ocp_mod
    from sdf_nmpc_amd import shard
    from sdf_nmpc_amd.model import Quad
    cfg = Config(mpc__N=10)
    plan = shard.plan
    monkeypatch.setattr(shard, "plan", lambda total, capacity, n_dev: plan(total, 2, n_dev))
    o = ocp_mod.Ocp(Quad(cfg), batch=4, devices=[0, 0])
    assert len(o.parts) == 2
    s = Nmpc(cfg, batch=4, ocp=o)
    x4 = np.zeros((4, 10))
    x4[:, :3] = np.random.default_rng(2).uniform(-1, 1, (4, 3))
    x4[:, 3] = 1.0
    s.set_sdf_flag(1.0)
    s.set_latent(np.random.default_rng(3).normal(0, 1, (4, 128)), x4[:, :3], np.stack([np.eye(3)] * 4))
    ref = Ref(cfg)
    ref.p, ref.q = np.array([0.5, -0.4, 0.3]), yaw2quat(0.4)
    ref.use_weights(ref.W_on)
    for k in range(s.N + 1):
        s.set_ref(ref, k)
    s.set_x0(x4)
    s.solve()  # flush the host setters, so that the device fields are settled
    state = {k: o.download(k) for k in ("x", "u", "p", "x0")}
    for part in o.parts:
        sc = Scene.mesh(part.ctx, M.fixed_scene(), closed=True, sdf_source=True)
        with pytest.raises(ValueError, match="split"):
            s.set_sdf_scene(sc)
        part.ctx.synchronize()
        np.testing.assert_array_equal(s.x0, x4)
        for k, v in state.items():
            np.testing.assert_array_equal(o.download(k), v)
        sc.close()
    assert s._sdf_scene is None
    o.close()
