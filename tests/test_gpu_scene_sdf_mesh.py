"""A mesh set as the exact SDF source (csrc/scene_mesh.hip: scene_sdf_rows_mesh_kernel, Scene.mesh(sdf_source=True)):
the rows against tests/mesh_sdf_ref.py, against Scene.distance bit for bit, against the hierarchy bit for bit, against the
primitive rows kernel on a box, the row and entry-point contracts, and the phase split with lin_args.sdf_scene.

The bar against the references is 1e-12, the project's tolerance for the fp64 scene rows (tests/test_gpu_scene_sdf.py),
on the rows mesh_sdf_ref.decided keeps.  Measured on an MI355X, worst gap on decided rows: h 3.3e-16, J_h 9.2e-13 (B = 37; a
row 1.3 mm off a face: the rounding of the closest point, about 1e-15 m, divided by the distance), 1.3e-14 at B = 3."""
import numpy as np
import pytest

import mesh_ref as M
import mesh_sdf_ref as MS
import scene_sdf_ref as S
from sdf_nmpc_amd import _lib
from sdf_nmpc_amd.config import Config
from sdf_nmpc_amd.mesh import Mesh
from sdf_nmpc_amd.scene import Scene
from test_gpu_scene_mesh import FIXED, LEAVES, _hierarchy_cases
from test_gpu_scene_sdf import NP, OUT, SHAPES, _check_layout, _problem, _run

pytestmark = [pytest.mark.gpu, pytest.mark.filterwarnings("ignore:no SDF weights"),
              pytest.mark.filterwarnings("ignore:QP reached")]

ATOL = 1e-12
NAME = "scene_sdf_rows_mesh"
OTHER = Mesh.merge(Mesh.icosphere((2.0, 0.2, 0.0), 0.6, 2), Mesh.box((-10, -10, -1.6), (10, 10, -1.5)))
MESHES = [FIXED, OTHER]
BOX8 = ((1.0, -0.5, -0.25), (1.75, 0.5, 0.5))  # every coordinate a multiple of 1/8: exact in fp32


def _inputs(B, N, seed):
    """test_gpu_scene_sdf's inputs: positions from scene_sdf_ref's box, the flag off at every third node, the rest noise"""
    rng = np.random.default_rng(seed)
    x = rng.normal(0, 1, (B, N + 1, 10))
    x[..., :3] = S.draw(B * (N + 1), seed).reshape(B, N + 1, 3)
    p = rng.normal(0, 1, (B, N + 1, NP))
    p[..., 0] = 1.0
    p[:, 2::3, 0] = 0.0
    return x, p


def _ref_rows(so, x, p, max_df, closed):
    """mesh_sdf_ref's (h2, J_h2, decided) of every instance's scene: each scene evaluated once over all the rows"""
    per = [MS.sdf_rows(m, x, p, max_df, closed) + (MS.decided(m, x, max_df, closed),) for m in map(M.rounded, MESHES)]
    return tuple(np.stack([per[s][k][b] for b, s in enumerate(so)]) for k in range(3))


@pytest.fixture(scope="module")
def ref():
    """mesh_sdf_ref's rows and decided masks of the two-scene set, once per (B, N, closed, max_df)"""
    cache = {}

    def get(B, N, closed, max_df=1.0):
        key = (B, N, closed, max_df)
        if key not in cache:
            x, p = _inputs(B, N, seed=100 + B)
            so = np.arange(B) % 2
            h, J, ok = _ref_rows(so, x, p, max_df, closed)
            for a in (x, p, so, h, J, ok):
                a.setflags(write=False)
            cache[key] = (x, p, so, h, J, ok)
        return cache[key]

    return get


@pytest.fixture(scope="module")
def sets(gpu_ctx):
    made = {}

    def get(B, closed, leaf=None):
        key = (B, closed, leaf)
        if key not in made:
            made[key] = Scene.mesh(gpu_ctx, MESHES, scene_of=np.arange(B) % 2, closed=closed, leaf_size=leaf, sdf_source=True)
        return made[key]

    yield get
    for sc in made.values():
        sc.close()


# ---- 1. against the reference
@pytest.mark.parametrize("closed", [True, False])
@pytest.mark.parametrize("B,N", SHAPES)
def test_rows_match_the_reference_on_decided_rows(gpu_ctx, ref, sets, B, N, closed):
    x, p, so, want_h, want_J, ok = ref(B, N, closed)
    scene = sets(B, closed)
    assert scene.is_mesh and scene.is_sdf_source and not scene.is_dynamic
    h, J = _run(gpu_ctx, scene, B, N, x, p)
    _check_layout(h, J)
    eh, eJ = np.abs(h[..., 2] - want_h)[ok], np.abs(J[..., 2] - want_J)[ok]
    print(f"\nmesh rows B={B} N={N} closed={closed}: {ok.size - ok.sum()} of {ok.size} rows undecided; max error h "
          f"{eh.max():.2e}, J_h {eJ.max():.2e}")
    assert ok.mean() >= 0.99
    assert eh.max() <= ATOL and eJ.max() <= ATOL
    off = p[..., 0] == 0.0
    assert off.any() and (h[..., 2][off] == 1.0).all() and not J[..., 2][off].any()
    if B == 37:  # the case holds a truncated row, an untruncated one and (closed) an inside row
        on = ~off
        assert (want_h[on] == 1.0).any() and ((want_h[on] > 0) & (want_h[on] < 1.0)).any()
        assert closed or not (want_h[on] < 0).any()


# ---- 2. against Scene.distance, bit for bit
def _special_points(mesh, rng, k):
    """vertices, edge midpoints and centroids of k triangles of the mesh as the library sees it"""
    v = mesh.verts.astype(np.float32).astype(np.float64)
    tv = v[mesh.tris[rng.permutation(mesh.tris.shape[0])[:k]]]
    return np.concatenate([tv.reshape(-1, 3), (0.5 * (tv + np.roll(tv, 1, axis=1))).reshape(-1, 3), tv.mean(1)])


@pytest.mark.parametrize("closed", [True, False])
@pytest.mark.parametrize("max_df", [1.0, 0.5])
def test_h_is_scene_distance_bit_for_bit(gpu_ctx, closed, max_df):
    N, rng = 10, np.random.default_rng(21)
    lo, hi = np.array(BOX8[0]), np.array(BOX8[1])
    box = Mesh.box(lo, hi)
    # exactly max_df (and 1.0, 0.5, 0.25) from a face, over both triangles of it and on its diagonal; all in fp32
    exact = []
    for a in range(3):
        for side, sgn in ((lo, -1.0), (hi, 1.0)):
            for off in (max_df, 1.0, 0.5, 0.25):
                for uv in ((0.25, 0.125), (0.125, 0.25), (0.25, 0.25)):
                    q = lo + np.array([0.25, 0.25, 0.25])
                    q[(a + 1) % 3] = lo[(a + 1) % 3] + uv[0]
                    q[(a + 2) % 3] = lo[(a + 2) % 3] + uv[1]
                    q[a] = side[a] + sgn * off
                    exact.append(q)
    exact = np.array(exact)
    inside = rng.uniform(lo, hi, (20, 3))
    pts = [np.concatenate([exact, _special_points(box, rng, 12), inside, rng.uniform(lo - 1.5, hi + 1.5, (300, 3))]),
           np.concatenate([_special_points(FIXED, rng, 40), S.draw(300, 5)])]
    per = [-(-q.shape[0] // (N + 1)) for q in pts]           # instances per scene, the tail padded with random rows
    pts = [np.concatenate([q, S.draw(k * (N + 1) - q.shape[0], 6)]) for q, k in zip(pts, per)]
    so = np.repeat([0, 1], per)
    B = so.size
    x = rng.normal(0, 1, (B, N + 1, 10))
    x[..., :3] = np.concatenate(pts).reshape(B, N + 1, 3)
    p = rng.normal(0, 1, (B, N + 1, NP))
    p[..., 0] = 1.0
    scene = Scene.mesh(gpu_ctx, [box, FIXED], scene_of=so, closed=closed, sdf_source=True)
    h, J = _run(gpu_ctx, scene, B, N, x, p, max_df=max_df)
    _check_layout(h, J)
    d = scene.distance(x[..., :3].reshape(-1, 3), np.repeat(so, N + 1)).reshape(B, N + 1)
    np.testing.assert_array_equal(h[..., 2], np.where(d < max_df, d, max_df))
    at = d == max_df
    assert at.sum() >= 18 and (h[..., 2][at] == max_df).all() and not J[..., 2][at].any()  # exactly max_df: not near
    assert (d == 0).sum() >= 6 * 12 and (np.abs(d) < 1e-9).sum() >= 7 * 12 + 6 * 40  # vertices; midpoints and centroids
    assert ((d > 0) & (d < max_df)).any() and (d > max_df).any() and (d < 0).any() == closed
    on = d == 0  # on the surface: a unit normal, finite
    assert (np.abs(np.linalg.norm(J[..., :3, 2][on], axis=1) - 1.0) <= ATOL).all()
    scene.close()


# ---- 3. against the hierarchy, bit for bit
@pytest.mark.parametrize("name", ["fixed", "fixed_open", "terrain", "tunnel", "one", "coplanar"])
def test_hierarchy_changes_no_bit(gpu_ctx, name):
    mesh, closed = _hierarchy_cases()[name]
    v, t = mesh.verts.astype(np.float32).astype(np.float64), mesh.tris
    rng = np.random.default_rng(11)
    tv = v[t[rng.permutation(t.shape[0])[:150]]]
    lo, hi = v.min(0) - 1.0, v.max(0) + 1.0
    pts = np.concatenate([tv.reshape(-1, 3), (0.5 * (tv + np.roll(tv, 1, axis=1))).reshape(-1, 3), tv.mean(1),
                          rng.uniform(lo, hi, (200, 3))])  # test_gpu_scene_mesh's points
    N = 9
    B = pts.shape[0] // (N + 1)
    x = rng.normal(0, 1, (B, N + 1, 10))
    x[..., :3] = pts[:B * (N + 1)].reshape(B, N + 1, 3)
    p = rng.normal(0, 1, (B, N + 1, NP))
    p[..., 0] = 1.0
    p[:, 2::3, 0] = 0.0

    def run(leaf):
        sc = Scene.mesh(gpu_ctx, mesh, closed=closed, leaf_size=leaf, sdf_source=True)
        out = _run(gpu_ctx, sc, B, N, x, p)
        sc.close()
        return out

    bh, bJ = run(-1)
    _check_layout(bh, bJ)
    on = p[..., 0] == 1.0
    assert (bh[..., 2][on] < 1.0).any() and (bh[..., 2][on] == 0.0).any()  # near rows, and rows on a vertex
    for leaf in LEAVES:
        h, J = run(leaf)
        np.testing.assert_array_equal(h[..., 2], bh[..., 2], err_msg=f"h, leaf {leaf}")
        np.testing.assert_array_equal(J[..., 2], bJ[..., 2], err_msg=f"Jh, leaf {leaf}")


# ---- 4. against the primitive rows kernel
def test_box_mesh_against_the_primitive_rows_kernel(gpu_ctx):
    B, N = 37, 6
    lo, hi = (3.5, 0.5, -1.0), (4.0, 1.5, 1.25)  # test_gpu_scene_mesh's first box: every coordinate an fp32 number
    prim, mesh = [Scene.box(lo, hi)], Mesh.box(lo, hi)
    x, p = _inputs(B, N, seed=8)
    x[:8, :, :3] = np.random.default_rng(8).uniform(np.array(lo) - 0.8, np.array(hi) + 0.8, (8, N + 1, 3))  # around and inside
    analytic, meshed = Scene(gpu_ctx, prim), Scene.mesh(gpu_ctx, mesh, closed=True, sdf_source=True)
    assert analytic.is_sdf_source
    ha, Ja = _run(gpu_ctx, analytic, B, N, x, p)
    hm, Jm = _run(gpu_ctx, meshed, B, N, x, p)
    ok = S.decided(prim, x, 1.0) & MS.decided(mesh, x, 1.0, True)
    near = (ha[..., 2] < 1.0) & (p[..., 0] == 1.0)
    print(f"\nbox mesh against the box primitive: h gap {np.abs(ha[..., 2] - hm[..., 2]).max():.2e} on all rows, J_h gap "
          f"{np.abs(Ja[..., 2] - Jm[..., 2])[ok].max():.2e} on {ok.sum()} of {ok.size} rows decided by both; {near.sum()} near")
    assert near.sum() >= 40 and (ha[..., 2] < 0).any() and ok.mean() >= 0.95
    assert np.abs(ha[..., 2] - hm[..., 2]).max() <= ATOL
    assert np.abs(Ja[..., 2] - Jm[..., 2])[ok].max() <= ATOL
    analytic.close()
    meshed.close()


# ---- 5. the row contract
@pytest.mark.parametrize("closed", [True, False])
def test_row_contract(gpu_ctx, ref, sets, closed):
    B, N = 37, 6
    x, p, so, want_h, _, _ = ref(B, N, closed)
    scene = sets(B, closed)
    h, J = _run(gpu_ctx, scene, B, N, x, p)
    _check_layout(h, J)  # columns 0 and 1 keep their NaN fill
    d = scene.distance(x[..., :3].reshape(-1, 3), np.repeat(so, N + 1)).reshape(B, N + 1)
    on = p[..., 0] == 1.0
    near, g = on & (d < 1.0), np.linalg.norm(J[..., :3, 2], axis=-1)
    assert (near & (np.abs(d) > 1e-6)).sum() > 20
    assert np.abs(g[near & (np.abs(d) > 1e-6)] - 1.0).max() <= ATOL
    assert (on & ~near).sum() > 20 and (g[~near] == 0.0).all() and (h[..., 2][~near] == 1.0).all()
    # a permuted batch gives permuted rows
    perm = np.random.default_rng(1).permutation(B)
    other = Scene.mesh(gpu_ctx, MESHES, scene_of=so[perm], closed=closed, sdf_source=True)
    hp, Jp = _run(gpu_ctx, other, B, N, x[perm], p[perm])
    np.testing.assert_array_equal(h[perm][..., 2], hp[..., 2])
    np.testing.assert_array_equal(J[perm][..., 2], Jp[..., 2])
    other.close()
    # a mesh set is static: the clock changes no bit
    for kw in (dict(t0=1.7), dict(t0=-3.0, tau=0.2 * np.arange(N + 1))):
        ht, Jt = _run(gpu_ctx, scene, B, N, x, p, **kw)
        np.testing.assert_array_equal(ht[..., 2], h[..., 2])
        np.testing.assert_array_equal(Jt[..., 2], J[..., 2])
    # a NaN and an infinite position: (max_df, 0) in their rows, the rest of the batch unchanged
    xb = x.copy()
    rows = [(k, 0) for k in range(B) if near[k, 0]][:2]
    assert len(rows) == 2
    xb[rows[0]][1], xb[rows[1]][0] = np.nan, np.inf
    hb, Jb = _run(gpu_ctx, scene, B, N, xb, p)
    _check_layout(hb, Jb)
    keep = np.ones((B, N + 1), bool)
    for r in rows:
        keep[r] = False
        assert hb[r][2] == 1.0 and not Jb[r][:, 2].any() and h[r][2] < 1.0
    np.testing.assert_array_equal(hb[..., 2][keep], h[..., 2][keep])
    np.testing.assert_array_equal(Jb[..., 2][keep], J[..., 2][keep])


# ---- 6. the entry points
def test_entry_point_contract(gpu_ctx):
    from test_gpu_rollout import _setup
    B, N = 3, 10
    good = Scene.mesh(gpu_ctx, FIXED, closed=True, sdf_source=True)
    plain = {closed: Scene.mesh(gpu_ctx, FIXED, closed=closed, sdf_source=False) for closed in (True, False)}
    assert good.is_sdf_source and not plain[True].is_sdf_source and not plain[False].is_sdf_source
    assert Scene.mesh(gpu_ctx, FIXED).is_sdf_source is False
    x, p = _inputs(B, N, seed=2)
    d = {k: _lib.DeviceArray.from_numpy(gpu_ctx, v) for k, v in
         dict(x=x, p=p, h=np.full((B, N + 1, 3), -7.0), Jh=np.full((B, N + 1, 10, 3), -7.0)).items()}
    untouched = lambda: (d["h"].numpy() == -7.0).all() and (d["Jh"].numpy() == -7.0).all()
    cfg, q, prob, prims, bufs = _problem(gpu_ctx, "default", B, N, seed=13)
    lin = bufs()
    gpu_ctx.enable_timing(True)
    gpu_ctx.reset_stats()
    try:
        _lib.scene_sdf_rows(gpu_ctx, good.h, 0, N, NP, d["x"], d["p"], d["h"], d["Jh"], 1.0)  # B = 0: a no-op
        gpu_ctx.synchronize()
        assert untouched() and gpu_ctx.kernel_stats(NAME)[1] == 0
        for sc in plain.values():
            with pytest.raises(_lib.SdfnmpcError, match="error -4.*mesh"):
                _lib.scene_sdf_rows(gpu_ctx, sc.h, B, N, NP, d["x"], d["p"], d["h"], d["Jh"], 1.0)
            with pytest.raises(_lib.SdfnmpcError, match="error -4.*mesh"):
                _lib.linearize(gpu_ctx, None, _lib.quad_model(cfg, q), B, N, q.np, lin, nyN=q.nyN,
                               sdf_scene=_lib.scene_sdf_opts(sc.h, q.max_df))
            with pytest.raises(_lib.SdfnmpcError, match="error -4.*mesh"):
                _lib.rti_prepare(gpu_ctx, None, _lib.quad_model(cfg, q), _lib.qp_opts(q), B, N, q.np, lin,
                                 sdf_scene=_lib.scene_sdf_opts(sc.h, q.max_df))
        gpu_ctx.synchronize()
        launched = [gpu_ctx.kernel_stats(k)[1] for k in (NAME, "scene_sdf_rows", "linearize")]
        assert launched == [0, 0, 0] and untouched()
        assert all(np.isnan(lin[k].numpy()).all() for k in ("h", "Jh", "xn", "AB"))
        _lib.scene_sdf_rows(gpu_ctx, good.h, B, N, NP, d["x"], d["p"], d["h"], d["Jh"], 1.0)  # and unrefused it does write
        gpu_ctx.synchronize()
        assert gpu_ctx.kernel_stats(NAME)[1] == 1 and gpu_ctx.kernel_stats("scene_sdf_rows")[1] == 0
        assert (d["h"].numpy()[..., 2] != -7.0).all()
    finally:
        gpu_ctx.enable_timing(False)
    for bad in (2, -1):
        with pytest.raises(_lib.SdfnmpcError, match="error -1.*sdf_source"):
            Scene.mesh(gpu_ctx, FIXED, sdf_source=bad)
    # the third entry point: a controller
    n, x0 = _setup(Config(mpc__N=10), 2, 21)
    refused = Scene.mesh(n.ocp.ctx, FIXED, closed=False, sdf_source=False)
    with pytest.raises(_lib.SdfnmpcError, match="error -4.*mesh"):
        n.set_sdf_scene(refused)
    assert n._sdf_scene is None
    accepted = Scene.mesh(n.ocp.ctx, FIXED, closed=False, sdf_source=True)
    n.set_sdf_scene(accepted)
    assert n._sdf_scene is accepted
    n.set_sdf_scene(None)
    for sc in (refused, accepted, good, *plain.values()):
        sc.close()
    n.ocp.close()


# ---- 7. the phase split with the mesh source
@pytest.mark.parametrize("name", ["default", "sdf_cost_only"])
@pytest.mark.parametrize("B,N,kernel", [(24, 20, "auto"), (3, 40, "segmented")])
def test_phase_split_with_mesh_source_bitwise(gpu_ctx, name, B, N, kernel):
    """test_gpu_scene_sdf's phase split with the spheres restated as closed icospheres: rti_prepare(lin_args.sdf_scene) +
    qp_feedback == linearize(net) ; scene_sdf_rows ; qp_solve bit for bit, also with net == NULL."""
    import flag_sets as F
    import scene_setup
    cfg, q, prob, prims, bufs = _problem(gpu_ctx, name, B, N, seed=13)
    scene = Scene.mesh(gpu_ctx, Mesh.merge(*[Mesh.icosphere(a[:3], a[3], 1) for _, a in prims]), closed=True, sdf_source=True)
    net = _lib.Net.from_file(gpu_ctx, scene_setup.SCENE) if F.uses_scene(q) else _lib.Net.siren(gpu_ctx, 0)
    qm, opts = _lib.quad_model(cfg, q), _lib.qp_opts(q)
    src = _lib.scene_sdf_opts(scene.h, q.max_df, t0=0.4)
    ta, tb, tc, td = bufs(), bufs(), bufs(), bufs()
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
        _lib.linearize(gpu_ctx, None, qm, B, N, q.np, td, nyN=q.nyN, sdf_scene=src)
        with pytest.raises(_lib.SdfnmpcError, match="error -4"):  # a captured step still refuses a scene source
            _lib.RtiStep(gpu_ctx, net, qm, opts, B, N, q.np, bufs(), graph=True, sdf_scene=src)
        gpu_ctx.synchronize()
    finally:
        gpu_ctx.set_qp_kernel("auto")
    a = {k: ta[k].numpy() for k in OUT}
    h2 = a["h"][..., 2]
    print(f"\n{name} B={B} N={N} {kernel}: status {a['status'].tolist()}, {int((h2 < q.max_df).sum())} of {h2.size} rows "
          f"untruncated, min h2 {h2.min():.3f}")
    assert np.isfinite(h2).all() and (h2 < q.max_df).any()  # the mesh reached the rows
    for t in (tb, tc):
        for k in OUT:
            np.testing.assert_array_equal(a[k], t[k].numpy(), err_msg=k)
    for k in ("h", "Jh", "xn", "AB"):
        np.testing.assert_array_equal(a[k], td[k].numpy(), err_msg=k)
    net.close()
    scene.close()
