"""csrc/ref_pack.hip at general horizons, batches, paths, yaw modes and layouts, against tests/ref_gen_ref.py (the
numpy restatement that tests/test_ref_gen_ref.py holds to the reference's recorded RefGen outputs bit for bit).

Bars: positions, velocities, wz, weights and every yref / yNref / W / WN entry are bitwise (NaN in the same entries
for a first waypoint on x0, where the reference divides 0 by 0); every entry the kernel does not own keeps the
sentinel; quaternion entries that pass through atan2 / sin / cos stay within the bound ref_gen_ref derives per entry
(Q_K ulp of each function: 2.2e-16 to 8.9e-16), all others bitwise.

Measured on the MI355X (printed by every test): the largest quaternion difference over all cases is 2.2e-16,
at most 0.40 of its entry's bound; the pose of modes -1 / -2 came out bit for bit.
"""
import numpy as np
import pytest

import make_refgen_wide_golden as G
import ref_gen_ref as R
from sdf_nmpc_amd import _lib
from sdf_nmpc_amd.config import Config
from sdf_nmpc_amd.model import Quad
from test_gpu_ref_pack import POSE_RTOL, SENTINEL, _check, _pack
from test_ref_gen_ref import same_bits

pytestmark = [pytest.mark.gpu, pytest.mark.filterwarnings("ignore:no SDF weights")]

B = 37
NS = (1, 2, 63, 64, 65, 130)  # 64, 65, 66 nodes cross the 64-lane wrap; 131 take three passes
N_WP = (1, 2, 7, 32)
STRIDES = (7, 10, 13)
KINDS = ("long", "short", "zero", "grid", "dup", "first")
WS = dict(Wp=[30.0, 31.0, 32.0], Wq=[3.0, 4.0, 5.0], Wv=[6.0, 7.0, 8.0], Ww=[0.5, 0.6, 0.7], Wa=0.9)


@pytest.fixture(scope="module")
def model():
    return Quad(Config())


def _dyadic_T(N):
    """T in [1, 2) with T / N a power of two: with vref in {0.5, 1, 2} the samples of a 0.25 m grid path fall on
    its waypoints."""
    return N / 2.0 ** int(np.floor(np.log2(N)))


def _quat(rng, yaw):
    """A slightly tilted attitude of the given yaw (Z-Y-X Euler angles 0.1, -0.1, yaw)."""
    cr, sr, cp, sp, cy, sy = np.cos(0.05), np.sin(0.05), np.cos(-0.05), np.sin(-0.05), np.cos(yaw / 2), np.sin(yaw / 2)
    return np.array([cr * cp * cy + sr * sp * sy, sr * cp * cy - cr * sp * sy, cr * sp * cy + sr * cp * sy,
                     cr * cp * sy - sr * sp * cy])


def _state(rng, stride, yaw=None):
    x0 = rng.normal(0, 1, 13)
    x0[:3] = rng.integers(-8, 9, 3) * 0.25
    x0[3:7] = _quat(rng, rng.uniform(-np.pi, np.pi) if yaw is None else yaw)
    return x0[:stride]


def _config(kn, N, T):
    cfg = Config(mpc__N=int(N), mpc__T=float(T))
    cfg.ref.yaw_mode = kn["yaw_mode"]
    cfg.ref.stop_and_turn.enable = kn["st_enable"]
    cfg.ref.stop_and_turn.dang_min = kn["dang_min"]
    cfg.ref.align_yaw_offset = kn["align_off"]
    cfg.ref.vref, cfg.ref.yaw_align_dmin, cfg.ref.wzref = kn["vref"], kn["dmin"], kn["wzref"]
    return cfg


def _wps_batch(seed, N, n_wp, mode, st_on, stride, nb=B):
    """One launch: shared knobs, instances that differ in x0, waypoints and path kind; with stop-and-turn on in a
    mode that can stop, every other instance starts near the target yaw, so stops and sampled paths share a grid."""
    rng = np.random.default_rng(seed)
    dyadic = (R.MODES.index(mode) + int(st_on)) % 2 == 0
    T = _dyadic_T(N) if dyadic else float(rng.uniform(1.0, 2.5))
    kn = R.knobs(mode, st_on, rng.uniform(0.3, 1.5), float(rng.choice([0.0, 0.2])), float(rng.choice([0.5, 1.0, 2.0])),
                 0.1, 1.0)
    cases = []
    for b in range(nb):
        kind = KINDS[b % len(KINDS)]
        while True:
            x0 = _state(rng, stride)
            wp_p = G.path(rng, kind, x0, n_wp, kn["vref"] * T)
            wp_q = np.array([_quat(rng, y) for y in rng.uniform(-np.pi, np.pi, n_wp)])
            if st_on and mode in ("align", "topic") and b % 2:
                tgt = R._stop_target(x0, wp_p, wp_q, kn)[1] if mode == "topic" else \
                    np.arctan2(wp_p[0][1] - x0[1], wp_p[0][0] - x0[0]) + kn["align_off"]
                x0[3:7] = _quat(rng, tgt + 0.1)
            case = dict(kind="wps", path=kind, x0=x0, wp_p=wp_p, wp_q=wp_q, knobs=kn)
            if R.decisive(case):
                break
        cases.append(case)
    return kn, T, cases


class Worst:
    """The largest quaternion difference seen, and the largest share of its entry's bound."""

    def __init__(self):
        self.diff, self.share = 0.0, 0.0

    def see(self, got_q, want_q, tol):
        d = np.abs(got_q - want_q)
        self.diff = max(self.diff, float(d.max(initial=0.0)))
        on = tol > 0
        self.share = max(self.share, float((d[on] / tol[on]).max(initial=0.0)))


def _compare(got, b, exp, qtol, count, worst, what):
    """Instance b of a launch against packed(): the quaternion columns within their per-entry bound (bitwise where
    it is 0), everything else bit for bit, untouched entries at the sentinel (packed() leaves them there)."""
    gq, wq = got["p"][b][:, 13:17], exp["p"][:, 13:17]
    exact = np.ones_like(wq, dtype=bool)
    exact[:count] = qtol[:count] == 0
    assert same_bits(gq[exact], wq[exact]), what
    assert (np.abs(gq[:count] - wq[:count]) <= qtol[:count]).all(), (what, np.abs(gq[:count] - wq[:count]).max())
    worst.see(gq[:count], wq[:count], qtol[:count])
    rest = np.ones(exp["p"].shape[1], dtype=bool)
    rest[13:17] = False
    assert same_bits(got["p"][b][:, rest], exp["p"][:, rest]), what
    for k in ("yref", "W", "yNref", "WN"):
        assert same_bits(got[k][b], exp[k]), (what, k)


def _same_launch(a, b, ia=slice(None), ib=slice(None)):
    return all(same_bits(a[k][ia], b[k][ib]) for k in ("p", "yref", "W", "yNref", "WN"))


@pytest.mark.parametrize("N", NS)
def test_waypoints_batched_vs_restatement(gpu_ctx, model, N):
    """gen_ref_list_wps: all six yaw modes with stop-and-turn off and on, n_wp in {1, 2, 7, 32}, x0 strides 7 / 10 /
    13, B = 37 path kinds per launch; instances alone equal the batched ones and a second launch the first, bitwise."""
    wrow = R.weight_row(WS)
    worst, on_wp, seen = Worst(), 0, set()
    j = NS.index(N)
    for mi, mode in enumerate(R.MODES):
        for st_on in (False, True):
            n_wp, stride = N_WP[(j + mi + st_on) % 4], STRIDES[(j + 2 * mi + st_on) % 3]
            kn, T, cases = _wps_batch(1000 * N + 10 * mi + st_on, N, n_wp, mode, st_on, stride)
            cfg = _config(kn, N, T)
            x0, wp_p, wp_q = (np.stack([c[k] for c in cases]) for k in ("x0", "wp_p", "wp_q"))
            got = _pack(gpu_ctx, cfg, model, 0, x0, wp_p, wp_q, wrow=wrow)
            stops = 0
            for b, c in enumerate(cases):
                rows, count, qtol, info = R.wps_full(c["x0"], c["wp_p"], c["wp_q"], N, T, kn)
                exp = R.packed(rows, count, wrow, model.np, sentinel=SENTINEL)
                what = (mode, st_on, n_wp, stride, b, c["path"])
                _compare(got, b, exp, qtol, count, worst, what)
                yN, WN = exp["yNref"], exp["WN"]
                _check(got, b, model, (got["p"][b][:, 13:17], exp["yref"], exp["W"], yN, WN))  # the fixture test's own check
                stops += info["stop"]
                on_wp += info["on_waypoint"] > 0 and b > 0
                seen.add("nan" if np.isnan(rows[:count]).any() else "stop" if info["stop"] else
                         "empty" if not info["n_even"] else "padded" if info["n_even"] <= N else "full")
            if st_on and mode in ("align", "topic"):
                assert 5 <= stops <= B - 5, (mode, stops)  # stops and sampled paths side by side in one grid
            else:
                assert stops == 0
            assert _same_launch(got, _pack(gpu_ctx, cfg, model, 0, x0, wp_p, wp_q, wrow=wrow))
            for b in (0, 17, B - 1):
                alone = _pack(gpu_ctx, cfg, model, 0, x0[b:b + 1], wp_p[b:b + 1], wp_q[b:b + 1], wrow=wrow)
                assert _same_launch(got, alone, slice(b, b + 1)), (mode, st_on, b)
    assert seen == {"nan", "stop", "empty", "padded", "full"}, seen
    assert on_wp >= 3  # batched instances with a sample exactly on a waypoint (the searchsorted tie)
    print(f"\nref_pack waypoints N={N}: quaternion max diff {worst.diff:.2e}, {worst.share:.2f} of the entry's bound")


@pytest.mark.parametrize("N", NS)
def test_joystick_and_from_x0_batched_vs_restatement(gpu_ctx, model, N):
    """gen_ref_joystick over all six modes (|v_xy| above and below dmin, zero commands; position weights zeroed as
    ref_gen.py:122 does) and from_x0 (N references: node N untouched), B = 37."""
    worst = Worst()
    wrow = R.weight_row(WS)
    wjoy = wrow.copy()
    wjoy[:3] = 0.0
    for mi, mode in enumerate(R.MODES):
        rng = np.random.default_rng(7000 + 10 * N + mi)
        stride, T = STRIDES[(mi + N) % 3], float(rng.uniform(1.0, 2.5))
        kn = R.knobs(mode, bool(mi % 2), 0.5, 0.2, float(rng.choice([1.0, 3.0])), 0.1, float(rng.choice([1.0, 0.7])))
        x0s, vws = [], []
        for b in range(B):
            while True:
                vw = rng.uniform(-1, 1, 4)
                if b % 3 == 1:
                    vw[:2] *= 0.5 * kn["dmin"] / kn["vref"]
                elif b % 3 == 2:
                    vw[:3] = 0.0
                x0 = _state(rng, stride)
                if R.decisive(dict(kind="joystick", x0=x0, vw=vw, knobs=kn)):
                    break
            x0s.append(x0)
            vws.append(vw)
        x0s, vws = np.stack(x0s), np.stack(vws)
        cfg = _config(kn, N, T)
        got = _pack(gpu_ctx, cfg, model, 1, x0s, vw=vws, wrow=wjoy)
        for b in range(B):
            rows, count, qtol = R.joystick_full(x0s[b], vws[b], N, T, kn)
            _compare(got, b, R.packed(rows, count, wjoy, model.np, sentinel=SENTINEL), qtol, count, worst, (mode, b))
        assert _same_launch(got, _pack(gpu_ctx, cfg, model, 1, x0s, vw=vws, wrow=wjoy))
        alone = _pack(gpu_ctx, cfg, model, 1, x0s[B - 1:], vw=vws[B - 1:], wrow=wjoy)
        assert _same_launch(got, alone, slice(B - 1, B)), mode
        got = _pack(gpu_ctx, cfg, model, 2, x0s, wrow=wrow)  # from_x0 under the same knobs: none of them matters
        for b in range(B):
            rows, count, qtol = R.from_x0_full(x0s[b], N)
            exp = R.packed(rows, count, wrow, model.np, sentinel=SENTINEL)
            assert count == N and (exp["yNref"] == SENTINEL).all() and (exp["p"][N] == SENTINEL).all()
            _compare(got, b, exp, qtol, count, worst, ("from_x0", mode, b))
    print(f"\nref_pack joystick / from_x0 N={N}: quaternion max diff {worst.diff:.2e}, {worst.share:.2f} of the bound")


def _launch(ctx, opts, nb, N, np_, ny, nyN, host, n_wp=0, L=0, drop=(), alloc=None):
    """sdfnmpc_pack_refs on sentinel-filled outputs of the given layout (sized for max(nb, 1, alloc) instances);
    host: the inputs by name; drop: names passed as NULL.  Returns the outputs (the refusal raises before)."""
    D = lambda a: _lib.DeviceArray.from_numpy(ctx, np.asarray(a, dtype=np.float64))  # noqa: E731
    n = max(nb, 1, alloc or 0)
    bufs = {k: D(v) for k, v in host.items()}
    outs = dict(p=(n, N + 1, np_), yref=(n, N, ny), W=(n, N, ny), yNref=(n, nyN or 4), WN=(n, nyN or 4))
    for k, s in outs.items():
        bufs[k] = D(np.full([max(v, 1) for v in s], SENTINEL))
    args = {k: v for k, v in bufs.items() if k not in drop}
    try:
        _lib.pack_refs(ctx, opts, nb, N, np_, ny, args, n_wp=n_wp, L=L, nyN=nyN)
    finally:
        ctx.synchronize()
        res = {k: bufs[k].numpy() for k in outs}
        _launch.last = res
    return res


@pytest.mark.parametrize("np_", [17, 17 + 64, 17 + 200])
@pytest.mark.parametrize("ny,nyN", [(12, 4), (11, 5), (12, 5)])
def test_layouts(gpu_ctx, np_, ny, nyN):
    """ny = 12 (yref[11] = 0, W[11] = wrow[11]), nyN = 5 and parameter rows other than the deployed 17 + 128, on a
    waypoint launch with stops (topic), a joystick launch and from_x0, at N = 3 and 65."""
    wrow = R.weight_row(WS, [20.0] * (ny - 11))
    worst = Worst()
    for N in (3, 65):
        kn, T, cases = _wps_batch(99 + N + np_ + ny + nyN, N, 7, "topic", True, 10)
        opts = _lib.ref_opts(_config(kn, N, T), 0)
        host = dict(x0=np.stack([c["x0"] for c in cases]), wp_p=np.stack([c["wp_p"] for c in cases]),
                    wp_q=np.stack([c["wp_q"] for c in cases]), wrow=wrow)
        got = _launch(gpu_ctx, opts, B, N, np_, ny, nyN, host, n_wp=7)
        stops = 0
        for b, c in enumerate(cases):
            rows, count, qtol, info = R.wps_full(c["x0"], c["wp_p"], c["wp_q"], N, T, kn)
            exp = R.packed(rows, count, wrow, np_, ny=ny, nyN=nyN, sentinel=SENTINEL)
            _compare(got, b, exp, qtol, count, worst, ("wps", N, b))
            stops += info["stop"]
            if info["stop"]:
                assert (got["yNref"][b] == SENTINEL).all() and (got["WN"][b] == SENTINEL).all()
                assert (got["p"][b][N] == SENTINEL).all()
            elif ny == 12:
                assert (got["yref"][b][:, 11] == 0.0).all() and (got["W"][b][:, 11] == 20.0).all()
        assert 5 <= stops <= B - 5
        vw = np.random.default_rng(N).uniform(-1, 1, (B, 4))
        got = _launch(gpu_ctx, _lib.ref_opts(_config(kn, N, T), 1), B, N, np_, ny, nyN, dict(x0=host["x0"], vw=vw, wrow=wrow))
        for b in range(B):
            rows, count, qtol = R.joystick_full(host["x0"][b], vw[b], N, T, kn)
            _compare(got, b, R.packed(rows, count, wrow, np_, ny=ny, nyN=nyN, sentinel=SENTINEL), qtol, count, worst, ("joy", N, b))
        got = _launch(gpu_ctx, _lib.ref_opts(_config(kn, N, T), 2), B, N, np_, ny, nyN, dict(x0=host["x0"], wrow=wrow))
        for b in range(B):
            rows, count, qtol = R.from_x0_full(host["x0"][b], N)
            _compare(got, b, R.packed(rows, count, wrow, np_, ny=ny, nyN=nyN, sentinel=SENTINEL), qtol, count, worst, ("x0", N, b))
            assert (got["yNref"][b] == SENTINEL).all() and (got["WN"][b] == SENTINEL).all()
    print(f"\nref_pack layouts np={np_} ny={ny} nyN={nyN}: quaternion max diff {worst.diff:.2e}, {worst.share:.2f} of the bound")


@pytest.mark.parametrize("N", [1, 64, 130])
@pytest.mark.parametrize("L", [1, 64, 128, 200])
def test_latent_pose_flag_modes(gpu_ctx, L, N):
    """Modes -1 and -2, B = 5: flag only, latent + pose, latent + pose + flag, pose only (mode -2 with the latent and
    flag pointers passed all the same).  Latent and flag bitwise, pose within POSE_RTOL, columns 13..16 and every
    column past the latent untouched."""
    nb, np_ = 5, 17 + L + (2 if L != 128 else 0)
    rng = np.random.default_rng(31 * L + N)
    cfg = Config()
    lat, pos = rng.normal(0, 1, (nb, L)), rng.uniform(-3, 3, (nb, 3))
    Rm = np.stack([np.linalg.qr(rng.normal(size=(3, 3)))[0] for _ in range(nb)])
    flag = (np.arange(nb) % 2).astype(float)
    full = dict(latent=lat, W_p_Bo=pos, W_R_Bo=Rm.reshape(nb, 9), flag=flag)
    worst = 0.0
    for mode, names in ((-1, ("flag",)), (-1, ("latent", "W_p_Bo", "W_R_Bo")), (-1, tuple(full)), (-2, tuple(full)),
                        (-2, ("W_p_Bo", "W_R_Bo"))):
        host = {k: full[k] for k in names}
        got = _launch(gpu_ctx, _lib.ref_opts(cfg, mode), nb, N, np_, 11, 4, host, L=L)
        for k in ("yref", "W", "yNref", "WN"):
            assert (got[k] == SENTINEL).all()
        for b in range(nb):
            exp = R.pose_latent_flag(mode, N, np_, cfg.sensor.B_p_C, cfg.sensor.B_R_C, W_p_Bo=host.get("W_p_Bo", [None] * nb)[b],
                                     W_R_Bo=host.get("W_R_Bo", [None] * nb)[b], latent=host["latent"][b] if "latent" in host
                                     else None, flag=host["flag"][b] if "flag" in host else None, sentinel=SENTINEL)
            gp = got["p"][b]
            assert same_bits(gp[:, 0], exp[:, 0]) and same_bits(gp[:, 13:], exp[:, 13:]), (mode, names, b)
            if mode == -2 or "latent" in host:
                np.testing.assert_allclose(gp[:, 1:13], exp[:, 1:13], rtol=POSE_RTOL, atol=0)
                worst = max(worst, float((np.abs(gp[:, 1:13] - exp[:, 1:13]) / np.abs(exp[:, 1:13])).max()))
            else:
                assert (gp[:, 1:13] == SENTINEL).all()
    print(f"\nref_pack modes -1 / -2 L={L} N={N}: pose max relative diff {worst:.2e}")


def test_refusals_leave_outputs_untouched(gpu_ctx):
    """Every condition sdfnmpc_pack_refs refuses returns the argument error before anything is launched: all five
    outputs keep the sentinel.  B = 0 succeeds and writes nothing."""
    N, n_wp, L = 3, 2, 4
    rng = np.random.default_rng(2)
    cfg = Config(mpc__N=N)
    base = dict(x0=np.stack([_state(rng, 10) for _ in range(2)]), wp_p=rng.normal(size=(2, n_wp, 3)),
                wp_q=np.tile([1.0, 0, 0, 0], (2, n_wp, 1)), wrow=R.weight_row(WS))
    pose = dict(W_p_Bo=rng.normal(size=(2, 3)), W_R_Bo=np.tile(np.eye(3).ravel(), (2, 1)))
    lat = dict(pose, latent=rng.normal(size=(2, L)))
    joy = dict(x0=base["x0"], wrow=base["wrow"], vw=rng.normal(size=(2, 4)))
    ok = dict(mode=0, nb=2, N=N, np_=17 + L, ny=11, nyN=4, host=base, n_wp=n_wp, L=0, drop=())
    bad = [dict(nb=-1), dict(N=0), dict(np_=16), dict(ny=10), dict(ny=13), dict(drop=("p",)), dict(mode=-3), dict(mode=3),
           dict(mode=-2, host={}), dict(mode=-2, host=dict(W_p_Bo=pose["W_p_Bo"])), dict(mode=-2, host=dict(W_R_Bo=pose["W_R_Bo"])),
           dict(host=dict(base, x0=base["x0"][:, :6])), dict(drop=("x0",)), dict(drop=("wrow",)), dict(drop=("yref",)),
           dict(drop=("W",)), dict(drop=("yNref",)), dict(drop=("WN",)), dict(n_wp=0), dict(n_wp=33), dict(drop=("wp_p",)),
           dict(drop=("wp_q",)), dict(mode=1, host=joy, drop=("vw",)), dict(mode=2, drop=("x0",)),
           dict(mode=-1, host=dict(latent=lat["latent"]), L=L), dict(mode=-1, host=dict(lat), drop=("W_R_Bo",), L=L),
           dict(mode=-1, host=lat, L=0), dict(mode=-1, host=lat, L=L + 1), dict(host=dict(base, **lat), L=L + 1),
           dict(nyN=3), dict(nyN=6), dict(nyN=-1)]
    for change in bad:
        a = dict(ok, **change)
        with pytest.raises(_lib.SdfnmpcError, match="sdfnmpc error -1"):  # SDFNMPC_E_ARG
            _launch(gpu_ctx, _lib.ref_opts(cfg, a["mode"]), a["nb"], a["N"], a["np_"], a["ny"], a["nyN"], a["host"],
                    n_wp=a["n_wp"], L=a["L"], drop=a["drop"], alloc=2)
        for k, v in _launch.last.items():
            assert (v == SENTINEL).all(), (change, k)
    got = _launch(gpu_ctx, _lib.ref_opts(cfg, 0), 0, N, 17 + L, 11, 4, base, n_wp=n_wp, alloc=2)  # B = 0: success
    for k, v in got.items():
        assert (v == SENTINEL).all(), k
    got = _launch(gpu_ctx, _lib.ref_opts(cfg, 0), 2, N, 17 + L, 11, 4, dict(base, **lat), n_wp=n_wp, L=L)  # and it does run
    assert (got["yref"] != SENTINEL).all() and same_bits(got["p"][:, :, 17:], np.repeat(lat["latent"][:, None], N + 1, 1))
