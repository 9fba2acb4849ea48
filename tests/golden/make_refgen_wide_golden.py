#!/usr/bin/env python3
"""Regenerates tests/golden/refgen_wide_golden.npz: the reference's own ``RefGen`` (sdf_nmpc/ref_gen.py:7-130) over
horizons, waypoint counts, yaw modes and path edges that refgen_golden.npz (make_golden.py:refgen_golden) leaves out.

    python tests/golden/make_refgen_wide_golden.py <path of the reference checkout>

Only recorded inputs and outputs are stored, packed into a few arrays (C cases):
  kind [C]      0 gen_ref_list_wps, 1 gen_ref_joystick, 2 from_x0
  tag [C]       what the case was built for (tests/test_ref_gen_ref.py counts them)
  x0 [C, 13]
  knobs [C, 9]  index in ref_gen_ref.MODES, stop-and-turn, dang_min, align_yaw_offset, vref, yaw_align_dmin, wzref, T, N
  n_wp [C], wp_p [sum n_wp, 3], wp_q [sum n_wp, 4]   the waypoints of the cases in order
  vw [C, 4]     the joystick command (0 elsewhere)
  len [C]       references returned (N or N + 1)
  traj [sum (N + 1), 11]   rows [p3 q4 v3 wz] of the cases in order, NaN where no reference was returned
  joy_Wp [C, 3] the Wp the joystick references carry (NaN elsewhere)
A draw whose branches hang on a last bit (ref_gen_ref.decisive) is drawn again, so nothing is masked at test time.
"""
import copy
import os
import sys
import types
import warnings

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))  # tests/: ref_gen_ref
import ref_gen_ref as R  # noqa: E402

SEED = 20611
SMALL_N, BIG_N = (1, 2, 3, 20), (63, 64, 65, 130)
N_WP = (1, 2, 7, 32)
T_OF = {1: 1.25, 2: 1.5, 3: 2.0, 20: 1.5, 63: 2.0, 64: 2.0, 65: 2.0, 130: 3.0}  # T >= 1: a short path is padded
AXES = np.array([[1, 0, 0], [0, 1, 0], [0, 0, 1], [-1, 0, 0], [0, 1, 0], [0, 0, -1], [1, 0, 0], [0, -1, 0]], float)


def load_reference(ref_root):
    """RefGen, euler2quat and the default Config of the reference; casadi / acados_template / l4casadi are only
    imported by it, never called on this path, so empty stand-in modules serve (as in make_golden.py)."""
    for name in ("casadi", "acados_template", "l4casadi"):
        mod = types.ModuleType(name)
        if name == "acados_template":
            mod.AcadosOcp = mod.AcadosOcpSolver = mod.AcadosModel = object
        sys.modules.setdefault(name, mod)
    sys.path.insert(0, ref_root)
    from sdf_nmpc.ref_gen import RefGen
    from sdf_nmpc.utils.config import Config
    from sdf_nmpc.utils.math import euler2quat
    return RefGen, euler2quat, Config(os.path.join(ref_root, "sdf_nmpc/config/default.yaml"))


def path(rng, kind, x0, n_wp, reach):
    """Waypoint positions of one path kind; `reach` = vref * T."""
    p0 = x0[:3]
    if kind == "zero":  # every waypoint on x0: zero length
        return np.tile(p0, (n_wp, 1))
    if kind == "grid":  # 0.25 m axis-aligned legs that turn at every waypoint
        return p0 + 0.25 * np.cumsum(AXES[np.arange(n_wp) % len(AXES)], axis=0)
    if kind == "short":  # total well below vref * T and below vref: padded
        leg = 0.5 * min(reach, 1.0) / n_wp
    else:  # "long", "dup", "first": more than vref * T of path
        leg = max(2.5 * reach / n_wp, 0.3)
    d = rng.normal(size=(n_wp, 3))
    d *= (leg * rng.uniform(1.0, 1.5, n_wp) / np.linalg.norm(d, axis=1))[:, None]
    if kind == "first":  # the first waypoint is x0 itself, more follow
        d[0] = 0.0
    if kind == "dup" and n_wp > 1:  # a waypoint twice (interior for n_wp > 2), within the sampled stretch
        d[1] = 0.0
    return p0 + np.cumsum(d, axis=0)


def main(ref_root):
    RefGen, euler2quat, CFG = load_reference(ref_root)
    rng = np.random.default_rng(SEED)
    cases = []

    def state(yaw=None):
        x0 = np.zeros(13)
        x0[:3] = rng.integers(-8, 9, 3) * 0.25  # binary fractions: the grid paths stay exact
        x0[3:7] = euler2quat(np.array([0.1, -0.1, rng.uniform(-np.pi, np.pi) if yaw is None else yaw]))
        x0[7:10] = rng.normal(0, 1, 3)
        return x0

    def wp_quats(n_wp):
        return np.array([euler2quat(np.array([0.05, -0.03, rng.uniform(-np.pi, np.pi)])) for _ in range(n_wp)])

    def add_wps(tag, N, n_wp, kind, mode, st_on, want_stop=None, T=None, vref=None, off=None):
        T = T_OF[N] if T is None else T
        for _ in range(1000):
            kn = R.knobs(mode, st_on, rng.uniform(0.3, 1.5), float(rng.choice([0.0, 0.2])) if off is None else off,
                         float(rng.choice([1.0, 3.0])) if vref is None else vref, CFG.ref.yaw_align_dmin, CFG.ref.wzref)
            x0 = state()
            case = dict(kind="wps", tag=tag, x0=x0, wp_p=path(rng, kind, x0, n_wp, kn["vref"] * T), wp_q=wp_quats(n_wp),
                        knobs=kn, N=N, T=T)
            if not R.decisive(case):
                continue
            if want_stop is None or R.wps_full(x0, case["wp_p"], case["wp_q"], N, T, kn)[3]["stop"] == want_stop:
                cases.append(case)
                return
        raise RuntimeError(f"no draw for {tag}")

    # every yaw mode, stop-and-turn off and on, over the waypoint counts and the small horizons
    i = 0
    for mode in R.MODES:
        for st_on in (False, True):
            for n_wp in N_WP:
                add_wps("sweep", SMALL_N[i % 4], n_wp, ("long", "short")[(i // 4) % 2], mode, st_on)
                i += 1
    # stop-and-turn decided both ways, for the two modes that can stop
    for mode in ("align", "topic"):
        for j in range(12):
            add_wps("stop" if j % 2 else "go", SMALL_N[j % 4], N_WP[(j // 2) % 4], "long", mode, True, want_stop=bool(j % 2))
    # per horizon: unpadded, padded and empty paths (modes that cannot stop, so the path is sampled)
    for j, N in enumerate(SMALL_N + BIG_N):
        for c, kind in enumerate(("long", "short", "zero")):
            add_wps(kind, N, N_WP[(j + c) % 4], kind, ("ref", "curent", "align", "zero")[(j + c) % 4], bool(c % 2) and
                    (j + c) % 4 != 2)
    # axis-aligned 0.25 m legs with T / N * vref_e dividing them: samples on waypoints, exact-multiple lengths
    for N, T, vref, n_wp, mode in ((20, 2.5, 1.0, 7, "ref"), (3, 1.5, 0.5, 2, "align"), (2, 1.0, 0.5, 7, "ref"),
                                   (1, 1.0, 0.25, 32, "align"), (20, 2.5, 1.0, 32, "curent")):
        add_wps("grid", N, n_wp, "grid", mode, False, T=T, vref=vref, off=0.2)
    for N, n_wp, mode in ((3, 7, "ref"), (20, 7, "align"), (20, 32, "zero")):
        add_wps("dup", N, n_wp, "dup", mode, False)
    for N, n_wp, mode in ((2, 2, "align"), (20, 7, "ref"), (3, 7, "topic"), (1, 2, "curent")):
        add_wps("first", N, n_wp, "first", mode, False)

    # joystick: every mode with |v_xy| above and below dmin and a zero command at N = 1, 2; a few at N = 64, 130
    def add_joy(N, mode, cmd):
        for _ in range(1000):
            kn = R.knobs(mode, False, 1.0, 0.0, float(rng.choice([1.0, 3.0])), CFG.ref.yaw_align_dmin, CFG.ref.wzref)
            vw = rng.uniform(-1, 1, 4)
            if cmd == "below":
                vw[:2] *= 0.5 * kn["dmin"] / kn["vref"]
            elif cmd == "zero":
                vw[:] = 0.0
            x0 = state()
            x0[10:] = 0.0
            case = dict(kind="joystick", tag="joy_" + cmd, x0=x0, vw=vw, knobs=kn, N=N, T=T_OF[N])
            above = np.hypot(*(vw[:2] * kn["vref"])) > kn["dmin"]
            if R.decisive(case) and above == (cmd == "above"):
                cases.append(case)
                return
        raise RuntimeError("no joystick draw")

    for N in (1, 2):
        for mode in R.MODES:
            for cmd in ("above", "below", "zero"):
                add_joy(N, mode, cmd)
    for N, picks in ((64, (("align", "above"), ("curent", "below"), ("ref", "zero"))),
                     (130, (("align", "below"), ("topic", "above"), ("curent", "zero")))):
        for mode, cmd in picks:
            add_joy(N, mode, cmd)
    for N in (1, 2, 64, 130):
        cases.append(dict(kind="from_x0", tag="from_x0", x0=state(), knobs=R.knobs(), N=N, T=T_OF[N]))

    # ---- run the reference
    C = len(cases)
    out = dict(kind=np.zeros(C, np.int64), tag=np.array([c["tag"] for c in cases]), x0=np.zeros((C, 13)),
               knobs=np.zeros((C, 9)), n_wp=np.zeros(C, np.int64), vw=np.zeros((C, 4)), len=np.zeros(C, np.int64),
               joy_Wp=np.full((C, 3), np.nan))
    wp_p, wp_q, traj = [], [], []
    for i, c in enumerate(cases):
        kn, N = c["knobs"], c["N"]
        cfg = copy.deepcopy(CFG)
        cfg.mpc.N, cfg.mpc.T = N, c["T"]
        cfg.ref.yaw_mode = kn["yaw_mode"]
        cfg.ref.stop_and_turn.enable = kn["st_enable"]
        cfg.ref.stop_and_turn.dang_min = kn["dang_min"]
        cfg.ref.align_yaw_offset = kn["align_off"]
        cfg.ref.vref, cfg.ref.yaw_align_dmin, cfg.ref.wzref = kn["vref"], kn["dmin"], kn["wzref"]
        g = RefGen(cfg)
        g.x0 = c["x0"]
        with warnings.catch_warnings():
            warnings.simplefilter("ignore", RuntimeWarning)  # the 0 / 0 of a first waypoint on x0
            if c["kind"] == "wps":
                refs = g.gen_ref_list_wps([types.SimpleNamespace(p=p, q=q) for p, q in zip(c["wp_p"], c["wp_q"])])
                out["n_wp"][i] = len(c["wp_p"])
                wp_p.append(c["wp_p"])
                wp_q.append(c["wp_q"])
            elif c["kind"] == "joystick":
                refs = g.gen_ref_joystick(c["vw"])
                out["vw"][i] = c["vw"]
                out["joy_Wp"][i] = refs[0].Wp
            else:
                refs = g.from_x0()
        rows = np.full((N + 1, 11), np.nan)
        for k, r in enumerate(refs):
            rows[k] = np.concatenate([np.asarray(r.p, float), np.asarray(r.q, float), np.asarray(r.v, float), [float(r.wz)]])
        traj.append(rows)
        out["kind"][i] = ("wps", "joystick", "from_x0").index(c["kind"])
        out["x0"][i] = c["x0"]
        out["knobs"][i] = [R.MODES.index(kn["yaw_mode"]), float(kn["st_enable"]), kn["dang_min"], kn["align_off"], kn["vref"],
                           kn["dmin"], kn["wzref"], c["T"], N]
        out["len"][i] = len(refs)
    out.update(wp_p=np.concatenate(wp_p), wp_q=np.concatenate(wp_q), traj=np.concatenate(traj))
    dst = os.path.join(HERE, "refgen_wide_golden.npz")
    np.savez_compressed(dst, **out)
    print(f"refgen_wide_golden.npz: {C} cases, {os.path.getsize(dst)} bytes")


if __name__ == "__main__":
    main(sys.argv[1])
