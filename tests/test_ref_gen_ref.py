"""tests/ref_gen_ref.py (the numpy restatement of RefGen + formate_ref + set_ref that test_gpu_ref_pack_general.py
holds csrc/ref_pack.hip to) against the reference's recorded outputs: refgen_golden.npz (make_golden.py) and
refgen_wide_golden.npz (make_refgen_wide_golden.py), bit for bit, and the wide fixture's case table counted."""
import os

import numpy as np
import pytest

import ref_gen_ref as R
from sdf_nmpc_amd.config import Config
from sdf_nmpc_amd.model import Quad
from sdf_nmpc_amd.reference import Ref

GOLDEN = os.path.join(os.path.dirname(__file__), "golden")
MODES = ["align", "ref", "current", "zero", "curent"]  # the mode index of refgen_golden.npz (make_golden.py:398)


def same_bits(got, want):
    """Equal bit patterns, NaN at the same entries counting as equal (and -0.0 != 0.0)."""
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    if got.shape != want.shape:
        return False
    nan = np.isnan(want)
    return bool(np.array_equal(np.isnan(got), nan) and
                np.array_equal(got[~nan].view(np.uint64), want[~nan].view(np.uint64)))


@pytest.fixture(scope="module")
def rg():
    return np.load(os.path.join(GOLDEN, "refgen_golden.npz"))


@pytest.fixture(scope="module")
def wide():
    """The cases of refgen_wide_golden.npz as dicts (ref_gen_ref.decisive's layout) with traj / len / tag."""
    z = np.load(os.path.join(GOLDEN, "refgen_wide_golden.npz"))
    cases, w0, t0 = [], 0, 0
    for i in range(len(z["kind"])):
        mode, st, dang, off, vref, dmin, wzref, T, N = z["knobs"][i]
        n_wp, N = int(z["n_wp"][i]), int(N)
        cases.append(dict(kind=("wps", "joystick", "from_x0")[int(z["kind"][i])], tag=str(z["tag"][i]), x0=z["x0"][i],
                          knobs=R.knobs(R.MODES[int(mode)], bool(st), dang, off, vref, dmin, wzref), T=float(T), N=N,
                          wp_p=z["wp_p"][w0:w0 + n_wp], wp_q=z["wp_q"][w0:w0 + n_wp], vw=z["vw"][i],
                          traj=z["traj"][t0:t0 + N + 1], len=int(z["len"][i]), joy_Wp=z["joy_Wp"][i]))
        w0, t0 = w0 + n_wp, t0 + N + 1
    assert w0 == len(z["wp_p"]) and t0 == len(z["traj"])
    return cases


def run(c):
    if c["kind"] == "wps":
        return R.wps(c["x0"], c["wp_p"], c["wp_q"], c["N"], c["T"], c["knobs"])
    if c["kind"] == "joystick":
        return R.joystick(c["x0"], c["vw"], c["N"], c["T"], c["knobs"])
    return R.from_x0(c["x0"], c["N"])


def test_restatement_equals_refgen_golden_bitwise(rg):
    """All 40 waypoint cases, the 9 joystick cases and from_x0 of refgen_golden.npz."""
    assert int(rg["n_wps_cases"]) == 40 and int(rg["n_joy_cases"]) == 9
    for c in range(40):
        mode, st_on, dang, off, vref, dmin, T, N = rg[f"w{c}/knobs"]
        case = dict(kind="wps", x0=rg[f"w{c}/x0"], wp_p=rg[f"w{c}/wp_p"], wp_q=rg[f"w{c}/wp_q"],
                    knobs=R.knobs(MODES[int(mode)], bool(st_on), dang, off, vref, dmin))
        rows, count = R.wps(case["x0"], case["wp_p"], case["wp_q"], int(N), float(T), case["knobs"])
        assert count == int(rg[f"w{c}/len"]), c
        assert same_bits(rows, rg[f"w{c}/traj"]), c
        assert R.decisive(case), c
    cfg = Config()
    N, T = int(cfg.mpc.N), float(cfg.mpc.T)
    for c in range(9):
        kn = R.knobs(["align", "ref", "curent"][int(rg[f"j{c}/mode"])], vref=cfg.ref.vref, dmin=cfg.ref.yaw_align_dmin,
                     wzref=cfg.ref.wzref)
        rows, count = R.joystick(rg[f"j{c}/x0"], rg[f"j{c}/vw"], N, T, kn)
        assert count == N + 1 and same_bits(rows, rg[f"j{c}/traj"]), c
        assert same_bits(rg[f"j{c}/Wp"], np.zeros(3)), c
    rows, count = R.from_x0(rg["from_x0/x0"], N)
    assert count == N and same_bits(rows[:N], rg["from_x0/traj"]) and np.isnan(rows[N]).all()


def test_restatement_equals_refgen_wide_golden_bitwise(wide):
    """Every case of the wide fixture, NaN in the same entries; NaN only where a case was built to divide by zero
    (a first waypoint on x0), or in the rows the reference did not return."""
    size = os.path.getsize(os.path.join(GOLDEN, "refgen_wide_golden.npz"))
    assert size < 300 * 1024, size
    nan_cases = 0
    for i, c in enumerate(wide):
        rows, count = run(c)
        assert count == c["len"], (i, c["tag"])
        assert same_bits(rows, c["traj"]), (i, c["tag"])
        assert np.isnan(c["traj"][count:]).all()
        has_nan = bool(np.isnan(c["traj"][:count]).any())
        assert has_nan == (c["tag"] == "first"), (i, c["tag"])
        nan_cases += has_nan
        if c["kind"] == "joystick":
            assert same_bits(c["joy_Wp"], np.zeros(3)), i
    assert nan_cases >= 3


def test_every_stored_case_is_decisive(wide):
    for i, c in enumerate(wide):
        assert R.decisive(c), (i, c["tag"])
    # and decisive() does refuse a case on its thresholds: a stop test and a dmin test made to tie
    x0 = np.array([0, 0, 0, 1.0, 0, 0, 0])
    tie = dict(kind="wps", x0=x0, wp_p=[[0.0, 0.1, 0.0]], wp_q=[[np.cos(0.25), 0, 0, np.sin(0.25)]],
               knobs=R.knobs("topic", True, dang_min=0.5))
    assert not R.decisive(tie)
    assert R.decisive(dict(tie, knobs=R.knobs("topic", True, dang_min=0.6)))
    assert not R.decisive(dict(tie, knobs=R.knobs("align", False, dmin=0.1)))
    assert not R.decisive(dict(kind="joystick", x0=x0, vw=[0.1, 0, 0, 0], knobs=R.knobs("align", vref=1.0, dmin=0.1)))


def test_wide_fixture_covers_its_case_table(wide):
    """The conditions the generator was written to meet, counted on the stored table (from the recorded rows and
    inputs, not from the tags), so that a regenerated fixture cannot lose a branch unnoticed."""
    w = [c for c in wide if c["kind"] == "wps"]
    info = [R.wps_full(c["x0"], c["wp_p"], c["wp_q"], c["N"], c["T"], c["knobs"])[3] for c in w]
    for c, f in zip(w, info):
        assert f["stop"] == (c["len"] == c["N"])
    # every yaw mode with stop-and-turn on and off
    assert {(c["knobs"]["yaw_mode"], c["knobs"]["st_enable"]) for c in w} == {(m, s) for m in R.MODES for s in (False, True)}
    # stop-and-turn decided both ways, 5 times each, for the two modes that can stop; no other mode stops
    for mode in ("align", "topic"):
        on = [f["stop"] for c, f in zip(w, info) if c["knobs"]["yaw_mode"] == mode and c["knobs"]["st_enable"]]
        assert sum(on) >= 5 and len(on) - sum(on) >= 5, (mode, on)
    assert not any(f["stop"] for c, f in zip(w, info) if c["knobs"]["yaw_mode"] not in ("align", "topic"))
    assert {len(c["wp_p"]) for c in w} == {1, 2, 7, 32}
    assert {c["N"] for c in w} == {1, 2, 3, 20, 63, 64, 65, 130}
    assert sum(c["N"] in (63, 64, 65, 130) for c in wide) >= 12
    # per horizon: a sampled path longer than vref T (no padding), a padded one and one of zero length
    for N in (1, 2, 3, 20, 63, 64, 65, 130):
        mine = [(c, f) for c, f in zip(w, info) if c["N"] == N and not f["stop"]]
        assert any(f["n_even"] == N + 1 and f["total"] > c["knobs"]["vref"] * c["T"] for c, f in mine), N
        assert any(0 < f["n_even"] < N + 1 for c, f in mine), N
        assert any(f["total"] == 0.0 and f["n_even"] == 0 for c, f in mine), N
    # samples exactly on a waypoint; a path whose length is a whole number of steps (the arange / ceil length)
    assert sum(f["on_waypoint"] > 0 for f in info) >= 4
    exact = 0
    for c, f in zip(w, info):
        if f["stop"] or not f["total"]:
            continue
        step = c["T"] / c["N"] * min(c["knobs"]["vref"], f["total"])
        exact += (f["total"] / step == f["n_even"]) and f["n_even"] < c["N"] + 1 and f["on_waypoint"] > 0
    assert exact >= 2
    # a repeated interior waypoint that the samples pass; a first waypoint on x0 with more after it
    dup = first = 0
    for c, f in zip(w, info):
        P = np.vstack([c["x0"][:3], c["wp_p"]])
        same = np.flatnonzero((np.diff(P, axis=0) == 0).all(axis=1))
        if f["stop"] or not f["total"]:
            continue
        cum = np.concatenate([[0], np.cumsum(np.linalg.norm(np.diff(P, axis=0), axis=1))])
        reach = (f["n_even"] - 1) * c["T"] / c["N"] * min(c["knobs"]["vref"], f["total"])
        dup += any(s > 0 and cum[s] < reach for s in same)
        first += 0 in same and len(c["wp_p"]) > 1
    assert dup >= 2 and first >= 3
    # joystick: N in {1, 2, 64, 130}, all six modes, |v_xy| above and below dmin, a zero command; from_x0 at those N
    j = [c for c in wide if c["kind"] == "joystick"]
    assert {c["N"] for c in j} == {1, 2, 64, 130} and {c["knobs"]["yaw_mode"] for c in j} == set(R.MODES)
    for mode in R.MODES:
        v = [np.hypot(*(c["vw"][:2] * c["knobs"]["vref"])) for c in j if c["knobs"]["yaw_mode"] == mode]
        assert any(x > 0.1 for x in v) and any(0 < x < 0.1 for x in v) and any(x == 0 for x in v), mode
    assert any(not c["vw"].any() for c in j)
    assert sorted(c["N"] for c in wide if c["kind"] == "from_x0") == [1, 2, 64, 130]


@pytest.mark.parametrize("sdf_cost", [False, True])
def test_packed_matches_formate_ref_and_set_ref(wide, sdf_cost):
    """packed() against Quad.formate_ref + Ref.use_weights per row (the path test_gpu_ref_pack.py::_expected takes),
    ny = 11 and 12, for a full trajectory, a stop (N references) and a joystick case."""
    cfg = Config()
    cfg.flags.sdf_cost = sdf_cost
    model = Quad(cfg)
    assert model.ny == (12 if sdf_cost else 11)
    ws = Ref(cfg).W_on
    wrow = R.weight_row(ws, model.extra_W)
    assert same_bits(wrow, model.weight_row(ws))
    picks = [next(c for c in wide if c["kind"] == "wps" and c["len"] == c["N"] + 1 and c["N"] == 3),
             next(c for c in wide if c["kind"] == "wps" and c["len"] == c["N"] and c["N"] == 3),
             next(c for c in wide if c["kind"] == "joystick" and c["N"] == 2)]
    for c in picks:
        N, n = c["N"], c["len"]
        for nyN in (4, 5):
            got = R.packed(c["traj"], n, wrow, model.np, ny=model.ny, nyN=nyN, sentinel=-7.0)
            want = dict(p=np.full((N + 1, model.np), -7.0), yref=np.full((N, model.ny), -7.0),
                        W=np.full((N, model.ny), -7.0), yNref=np.full(nyN, -7.0), WN=np.full(nyN, -7.0))
            for k in range(n):
                r = Ref(cfg).use_weights(ws)
                r.p, r.q, r.v, r.wz = c["traj"][k, 0:3], c["traj"][k, 3:7], c["traj"][k, 7:10], c["traj"][k, 10]
                want["p"][k, 13:17] = r.q
                y, W = model.formate_ref(r)
                if k < N:
                    want["yref"][k], want["W"][k] = y, W
                else:
                    want["yNref"][:], want["WN"][:] = y[:nyN], W[:nyN]
            for key in want:
                assert same_bits(got[key], want[key]), (c["tag"], nyN, key)
    if sdf_cost:
        assert (got["yref"][:, 11] == 0).all() and (got["W"][:, 11] == 20.0).all()


def test_pose_latent_flag_matches_set_latent():
    """pose_latent_flag's 3-term sums against numpy's matmul (set_latent, controller.py:50-54) and its column rules."""
    cfg = Config()
    rng = np.random.default_rng(5)
    R_, t = np.linalg.qr(rng.normal(size=(3, 3)))[0], rng.uniform(-3, 3, 3)
    lat = rng.normal(size=9)
    c, Rc = np.asarray(cfg.sensor.B_p_C, float).ravel(), np.asarray(cfg.sensor.B_R_C, float).reshape(3, 3)
    p = R.pose_latent_flag(-1, 4, 17 + 11, c, Rc, t, R_, latent=lat, flag=1.0)
    np.testing.assert_allclose(p[:, 1:4], np.tile(R_ @ c + t, (5, 1)), rtol=1e-15, atol=1e-15)
    np.testing.assert_allclose(p[:, 4:13], np.tile((R_ @ Rc).reshape(9), (5, 1)), rtol=1e-15, atol=1e-15)
    assert (p[:, 0] == 1.0).all() and (p[:, 13:17] == -7.0).all() and (p[:, 17:26] == lat).all() and (p[:, 26:] == -7.0).all()
    q = R.pose_latent_flag(-2, 4, 17 + 11, c, Rc, t, R_, latent=lat, flag=1.0)
    assert same_bits(q[:, 1:13], p[:, 1:13]) and (q[:, 0] == -7.0).all() and (q[:, 13:] == -7.0).all()
    f = R.pose_latent_flag(-1, 4, 17, c, Rc, flag=0.5)
    assert (f[:, 0] == 0.5).all() and (f[:, 1:] == -7.0).all()
