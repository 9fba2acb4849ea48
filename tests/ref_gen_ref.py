"""A plain restatement (numpy scalars, fp64) of the reference's RefGen (ref_gen.py:17-130), Quad.formate_ref
(quad_rollpitchyawrate.py:62-65), Nmpc.set_ref and set_latent / set_sdf_flag (controller.py:45-54,133-142), written
from those texts in their own operation order and not from csrc/ref_pack.hip.  tests/test_ref_gen_ref.py holds it
to the reference's recorded outputs bit for bit (tests/golden/refgen_golden.npz, refgen_wide_golden.npz); it is then
what tests/test_gpu_ref_pack_general.py compares the kernel with.

Rows are [p3 q4 v3 wz]; rows a generator does not return (from_x0 and stop-and-turn return N of N + 1) are NaN.
Every generator also returns, per quaternion entry, how far a second libm may move it (``Q_K``): 0 where the entry
is copied or constant, so those stay bitwise.
"""
import math

import numpy as np

MODES = ["align", "ref", "current", "zero", "curent", "topic"]  # 'curent' is the reference's spelling (ref_gen.py:12)

# ulp bound of double atan2 / sin / cos in a second libm.  The HIP math API page that documents the device
# functions' bounds is not installed beside the toolchain, so this is the value the work order falls back to.
Q_K = 2
_HALF_ULP_1 = 2.0 ** -53  # ulp of a value in [0.5, 1): the cos / sin results


def knobs(yaw_mode="align", st_enable=False, dang_min=1.0, align_off=0.0, vref=3.0, dmin=0.1, wzref=1.0):
    """The cfg.ref entries RefGen reads (default.yaml's values)."""
    assert yaw_mode in MODES
    return dict(yaw_mode=yaw_mode, st_enable=bool(st_enable), dang_min=float(dang_min), align_off=float(align_off),
                vref=float(vref), dmin=float(dmin), wzref=float(wzref))


# ---- utils/math.py:73-82,142-166 (numpy branches), each with the bound of its result
def _atan2(y, x):
    a = np.arctan2(y, x)
    return a, Q_K * math.ulp(abs(float(a)))


def quat2yaw(q):
    return _atan2(2 * (q[0] * q[3] + q[1] * q[2]), 1 - 2 * (q[2] * q[2] + q[3] * q[3]))


def _plus(yaw, err, off):
    """yaw + off: the bound grows by one rounding of the sum (none when the sum is exact)."""
    s = yaw + off
    return s, err + (math.ulp(abs(float(s))) if off != 0.0 else 0.0)


def yaw2quat(yaw, err):
    """Half the yaw's bound enters cos / sin (slope <= 1), whose own results move by Q_K ulp of a value below 1."""
    h = yaw * 0.5
    t = 0.5 * err + Q_K * _HALF_ULP_1
    return np.array([np.cos(h), 0.0, 0.0, np.sin(h)]), np.array([t, 0.0, 0.0, t])


def _norm(*a):  # numpy.linalg.norm of 2 or 3 entries: squares summed left to right
    s = a[0] * a[0]
    for x in a[1:]:
        s = s + x * x
    return np.sqrt(s)


def _f(a):
    return np.asarray(a, dtype=np.float64)


def _stop_target(x0, wp_p, wp_q, kn):
    """ref_gen.py:34-44: (yaw_curr, yaw_r, its bound, first-leg xy norm or None)."""
    yaw_curr, e0 = quat2yaw(x0[3:7])
    yaw_r, err, nrm = yaw_curr, e0, None
    if kn["yaw_mode"] == "topic":
        yaw_r, err = quat2yaw(wp_q[0])
    elif kn["yaw_mode"] == "align":
        dx, dy = wp_p[0][0] - x0[0], wp_p[0][1] - x0[1]
        nrm = _norm(dx, dy)
        if nrm > kn["dmin"]:
            yaw_r, err = _atan2(dy, dx)
        yaw_r, err = _plus(yaw_r, err, kn["align_off"])
    return yaw_curr, yaw_r, err, nrm


def wps_full(x0, wp_p, wp_q, N, T, kn):
    """gen_ref_list_wps (ref_gen.py:25-99) -> (rows [N+1, 11], count, qtol [N+1, 4], info)."""
    x0, wp_p, wp_q = _f(x0), _f(wp_p).reshape(-1, 3), _f(wp_q).reshape(-1, 4)
    N, T = int(N), float(T)
    n_wp = wp_p.shape[0]
    rows, qtol = np.full((N + 1, 11), np.nan), np.zeros((N + 1, 4))
    info = dict(stop=False, n_even=0, total=None, on_waypoint=0)
    P = np.vstack([x0[:3], wp_p])
    Q = np.vstack([x0[3:7], wp_q])
    mode = kn["yaw_mode"]

    if kn["st_enable"]:
        yaw_curr, yaw_r, err, _ = _stop_target(x0, wp_p, wp_q, kn)
        if abs(yaw_curr - yaw_r) > kn["dang_min"]:
            q, t = yaw2quat(yaw_r, err)
            rows[:N, 0:3], rows[:N, 3:7], rows[:N, 7:10], rows[:N, 10] = x0[:3], q, 0.0, 0.0
            qtol[:N] = t
            info["stop"] = True
            return rows, N, qtol, info

    dist = np.empty(n_wp)
    cum = np.empty(n_wp + 1)
    cum[0] = 0.0
    for s in range(n_wp):  # norm(diff(path_p), axis=1), cumsum, insert(0, 0)
        dist[s] = _norm(P[s + 1][0] - P[s][0], P[s + 1][1] - P[s][1], P[s + 1][2] - P[s][2])
        cum[s + 1] = cum[s] + dist[s]
    total = cum[-1]
    info["total"] = float(total)
    n = 0
    if total / 1e-3:
        vref_e = min(kn["vref"], total)
        step = T / N * vref_e
        n = min(int(math.ceil(total / step)), N + 1)  # len(arange(0, total, step)), cut by the break at N + 1
        align_on = mode == "align" and _norm(P[1][0] - x0[0], P[1][1] - x0[1]) > kn["dmin"]
        with np.errstate(invalid="ignore", divide="ignore"):
            for k in range(n):
                d = k * step
                info["on_waypoint"] += int(k > 0 and d in cum[1:])
                s = int(np.searchsorted(cum, d)) - 1
                s = max(0, min(s, n_wp - 1))
                direction = (P[s + 1] - P[s]) / dist[s]
                rows[k, 0:3] = P[s] + direction * (d - cum[s])
                rows[k, 7:10] = direction * vref_e
                rows[k, 10] = 0.0
                if mode == "curent":
                    rows[k, 3:7] = Q[0]
                elif mode == "ref":
                    rows[k, 3:7], qtol[k] = yaw2quat(*quat2yaw(Q[s + 1]))
                elif mode == "align":
                    if align_on:
                        rows[k, 3:7], qtol[k] = yaw2quat(*_plus(*_atan2(rows[k, 8], rows[k, 7]), kn["align_off"]))
                    else:
                        rows[k, 3:7] = Q[0]
                else:
                    rows[k, 3:7] = [1.0, 0.0, 0.0, 0.0]
    info["n_even"] = n
    for k in range(n, N + 1):  # padding (ref_gen.py:93-97): Ref's own v = 0, wz = 0
        rows[k, 0:3] = rows[n - 1, 0:3] if n else P[-1]
        rows[k, 3:7] = rows[n - 1, 3:7] if n else Q[-1]
        qtol[k] = qtol[n - 1] if n else 0.0
        rows[k, 7:11] = 0.0
    return rows, N + 1, qtol, info


def wps(x0, wp_p, wp_q, N, T, kn):
    rows, count, _, _ = wps_full(x0, wp_p, wp_q, N, T, kn)
    return rows, count


def joystick_full(x0, vw, N, T, kn):
    """gen_ref_joystick (ref_gen.py:101-130) -> (rows [N+1, 11], N + 1, qtol)."""
    x0, vw = _f(x0), _f(vw)
    N, T = int(N), float(T)
    v = vw[:3] * kn["vref"]
    wz = vw[3] * kn["wzref"]
    q, t = np.array([1.0, 0.0, 0.0, 0.0]), np.zeros(4)
    if kn["yaw_mode"] == "curent":
        q, t = yaw2quat(*quat2yaw(x0[3:7]))
    elif kn["yaw_mode"] == "align":
        if _norm(v[0], v[1]) > kn["dmin"]:
            q, t = yaw2quat(*_atan2(v[1], v[0]))
        else:
            q, t = yaw2quat(*quat2yaw(x0[3:7]))
    rows = np.empty((N + 1, 11))
    for i in range(N + 1):
        rows[i, 0:3] = x0[:3] + (v * i * T / N)
        rows[i, 3:7], rows[i, 7:10], rows[i, 10] = q, v, wz
    return rows, N + 1, np.tile(t, (N + 1, 1))


def joystick(x0, vw, N, T, kn):
    return joystick_full(x0, vw, N, T, kn)[:2]


def from_x0_full(x0, N):
    """from_x0 (ref_gen.py:17-23): N references -> (rows [N+1, 11] with row N NaN, N, qtol)."""
    x0, N = _f(x0), int(N)
    q, t = yaw2quat(*quat2yaw(x0[3:7]))
    rows, qtol = np.full((N + 1, 11), np.nan), np.zeros((N + 1, 4))
    rows[:N, 0:3], rows[:N, 3:7], rows[:N, 7:11] = x0[:3], q, 0.0
    qtol[:N] = t
    return rows, N, qtol


def from_x0(x0, N):
    return from_x0_full(x0, N)[:2]


def decisive(case):
    """No branch of the case hangs on a last bit of a trigonometric value or of a norm: the stop test and every
    dmin test are further than 1e-9 from their thresholds.  case: dict(kind 'wps' | 'joystick' | 'from_x0', x0,
    knobs, and wp_p / wp_q or vw)."""
    kn, x0 = case["knobs"], _f(case["x0"])
    if case["kind"] == "joystick":
        if kn["yaw_mode"] != "align":
            return True
        v = _f(case["vw"])[:3] * kn["vref"]
        return bool(abs(_norm(v[0], v[1]) - kn["dmin"]) > 1e-9)
    if case["kind"] != "wps":
        return True
    wp_p, wp_q = _f(case["wp_p"]).reshape(-1, 3), _f(case["wp_q"]).reshape(-1, 4)
    yaw_curr, yaw_r, _, _ = _stop_target(x0, wp_p, wp_q, kn)
    if kn["st_enable"] and not abs(abs(yaw_curr - yaw_r) - kn["dang_min"]) > 1e-9:
        return False
    if kn["yaw_mode"] == "align":
        return bool(abs(_norm(wp_p[0][0] - x0[0], wp_p[0][1] - x0[1]) - kn["dmin"]) > 1e-9)
    return True


# ---- formate_ref + set_ref
def weight_row(ws, extra_W=()):
    """formate_ref's W from a weight set (Wp, Wq, Wv, Ww, Wa) and the model's extra stage weights."""
    return np.concatenate([_f(ws["Wp"]), [ws["Wq"][2]], _f(ws["Wv"]), _f(ws["Wq"])[:2], _f(ws["Ww"])[2:], [ws["Wa"]],
                           _f(extra_W)]).astype(np.float64)


def packed(rows, count, wrow, np_, ny=11, nyN=4, sentinel=-7.0):
    """What set_ref leaves for `count` references: p[:, 13:17] = q, y / W of the nodes below N, yN / WN = the first
    nyN of node N's.  Everything else keeps the sentinel.  wrow [ny] is formate_ref's W (weight_row)."""
    N = rows.shape[0] - 1
    wrow = _f(wrow)
    assert wrow.shape == (ny,) and ny in (11, 12) and nyN in (4, 5)
    out = dict(p=np.full((N + 1, np_), sentinel), yref=np.full((N, ny), sentinel), W=np.full((N, ny), sentinel),
               yNref=np.full(nyN, sentinel), WN=np.full(nyN, sentinel))
    for k in range(count):
        r = rows[k]
        out["p"][k, 13:17] = r[3:7]
        y = np.concatenate([r[0:3], [0], r[7:10], [0, 0], [r[10]], [0], np.zeros(ny - 11)])
        if k < N:
            out["yref"][k], out["W"][k] = y, wrow
        else:
            out["yNref"][:], out["WN"][:] = y[:nyN], wrow[:nyN]
    return out


def pose_latent_flag(mode, N, np_, B_p_C, B_R_C, W_p_Bo=None, W_R_Bo=None, latent=None, flag=None, sentinel=-7.0):
    """set_latent / set_sdf_flag on every node: mode -1 writes the flag (column 0) when given and, with a latent,
    the camera pose (1..12) and the latent (17..17+L); mode -2 writes the pose alone whatever else is passed.
    The two products are 3-term sums left to right."""
    p = np.full((N + 1, np_), sentinel)
    if mode == -1 and flag is not None:
        p[:, 0] = flag
    if mode == -2 or latent is not None:
        R, t, c, Rc = _f(W_R_Bo).reshape(3, 3), _f(W_p_Bo), _f(B_p_C).ravel(), _f(B_R_C).reshape(3, 3)
        for i in range(3):
            p[:, 1 + i] = (R[i, 0] * c[0] + R[i, 1] * c[1] + R[i, 2] * c[2]) + t[i]
            for j in range(3):
                p[:, 4 + 3 * i + j] = R[i, 0] * Rc[0, j] + R[i, 1] * Rc[1, j] + R[i, 2] * Rc[2, j]
    if mode == -1 and latent is not None:
        lat = _f(latent)
        p[:, 17:17 + lat.size] = lat
    return p
