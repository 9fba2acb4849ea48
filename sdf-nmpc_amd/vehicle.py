"""A reproducible model of an imperfect vehicle and state estimator (csrc/vehicle.hip, sdfnmpc_vehicle_*): what
stands between the controller's command and the state it is told about.  Per plant call at frame f, in this order: an
input delay of ``delay`` control periods (a ring of the last commands; hover before the first has arrived), an
Ornstein-Uhlenbeck gust acceleration of stationary standard deviation ``gust_std`` and correlation time ``gust_tau``
advanced once and held over the period, a first-order thrust lag ``thrust_tau`` integrated as an 11th RK4 state, linear
rotor drag ``-R diag(drag) R^T v`` in the body frame, the plant's RK4, and the estimate handed to the next controller
step: position and velocity offset by a per-instance bias and white noise, the attitude turned about world z by a yaw
error.  Everything random is a function of (seed, stream, frame), so a run repeats bit for bit and a rollout cut into
chunks equals the uncut one (carry ``perceive_phase``, the frame number, across the chunks and do not ``reset``).

``VehicleModel.step`` is one plant call; ``Nmpc.rollout(vehicle=model)`` runs it inside the device loop.  A model
with everything off runs the plant's own kernel and returns its bits.

With ``body=RigidBody(...)`` (csrc/vehicle_body.hip) the thrust no longer points where the command says: the command
(thrust, roll, pitch, yaw rate) is the setpoint of an on-board attitude and rate controller, which drives four rotors
with a first-order speed lag and a speed range, which move a rigid body with inertia -- the physics of the reference's
model/quad_props.py.  Delay, gust, drag and the estimate stay as they are; the rotor lag replaces ``thrust_tau``.
"""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import _lib


def _axis_rot(axis, angle):
    c, s = np.cos(angle), np.sin(angle)
    return {"x": np.array([[1, 0, 0], [0, c, -s], [0, s, c]]), "y": np.array([[c, 0, s], [0, 1, 0], [-s, 0, c]]),
            "z": np.array([[c, -s, 0], [s, c, 0], [0, 0, 1]])}[axis]


def allocation(motors, cf, ct):
    """Gf, Gt [3, 4]: body force and torque = G Omega^2, from the motor rows (x, y, z, alpha, beta, sign) and the
    force and torque coefficients as the reference's model/quad_props.py:20-27 forms them: rotor i is turned by
    Rz(i pi / (n / 2)) Ry(beta_i) Rx((-1)^i alpha_i), pushes along its z axis, and adds the reaction torque
    (ct / cf) sign_i about it; both matrices carry the factor cf."""
    motors = np.asarray(motors, dtype=np.float64)
    n = len(motors)
    cols_f, cols_t = [], []
    for i, (px, py, pz, alpha, beta, sign) in enumerate(motors):
        z = (_axis_rot("z", i * (np.pi / (n / 2))) @ _axis_rot("y", beta) @ _axis_rot("x", (-1) ** i * alpha)) @ [0, 0, 1]
        cols_f.append(z)
        cols_t.append(np.cross([px, py, pz], z) + ct / cf * sign * z)
    return cf * np.column_stack(cols_f), cf * np.column_stack(cols_t)


class RigidBody:
    """The rigid body, rotors and inner loop of a vehicle.  mass (kg); inertia: the diagonal of J (kg m^2); motors:
    four rows (x, y, z, alpha, beta, sign) as the reference's robot.alloc.motors; cf, ct: force and torque coefficients
    of a rotor; wp_max: the largest rotor speed (robot.limits.wp; speeds are in its unit), wp_idle: the smallest
    (default 0.1 wp_max; rotors do not stop in flight); tau_att (s): time constant of the attitude loop; k_rate (1/s):
    the rate loop's three gains; tau_mot (s): the rotors' speed lag, 0 for none.  Gf, Gt [3, 4] and the mixer
    M = inv([Gf row z; Gt]) [4, 4] are formed here in fp64; the kernel is handed the matrices."""

    def __init__(self, mass, inertia, motors, cf, ct, wp_max, wp_idle=None, tau_att=0.1, k_rate=(20.0, 20.0, 8.0),
                 tau_mot=0.02):
        self.mass, self.cf, self.ct = float(mass), float(cf), float(ct)
        self.inertia = np.array(np.broadcast_to(np.asarray(inertia, dtype=np.float64), (3,)))
        self.motors = np.asarray(motors, dtype=np.float64)
        if self.motors.shape != (4, 6):
            raise ValueError(f"motors: four rows (x, y, z, alpha, beta, sign), not an array of shape {self.motors.shape}")
        self.wp_max = float(wp_max)
        self.wp_idle = 0.1 * self.wp_max if wp_idle is None else float(wp_idle)
        self.tau_att, self.tau_mot = float(tau_att), float(tau_mot)
        self.k_rate = np.array(np.broadcast_to(np.asarray(k_rate, dtype=np.float64), (3,)))
        self.Gf, self.Gt = allocation(self.motors, self.cf, self.ct)
        A = np.vstack([self.Gf[2:3], self.Gt])
        if not np.isfinite(A).all() or np.linalg.matrix_rank(A) < 4:
            raise ValueError("motors: [Gf row z; Gt] is singular -- thrust and the three torques cannot be commanded "
                             "independently")
        self.mixer = np.linalg.inv(A)

    @classmethod
    def from_cfg(cls, cfg, **kw):
        """From a config that carries the reference's robot.mass, robot.inertia, robot.alloc (motors, cf, ct) and
        robot.limits.wp; kw: wp_idle, tau_att, k_rate, tau_mot."""
        r = cfg.robot
        missing = [n for n, have in (("robot.mass", "mass" in r), ("robot.inertia", "inertia" in r),
                                     ("robot.alloc", "alloc" in r and all(k in r.alloc for k in ("motors", "cf", "ct"))),
                                     ("robot.limits.wp", "wp" in r.limits)) if not have]
        if missing:
            raise ValueError("RigidBody.from_cfg: the config lacks " + ", ".join(missing) + " (the reference's "
                             "default.yaml has them); give them there or build RigidBody(mass, inertia, motors, cf, ct, "
                             "wp_max) directly")
        return cls(r.mass, r.inertia, r.alloc.motors, r.alloc.cf, r.alloc.ct, r.limits.wp, **kw)

    def hover_speeds(self, g=9.81):
        """The rotor speeds of a reset: sqrt(M [m g; 0; 0; 0]), inside the speed range."""
        s = self.mixer @ np.array([self.mass * g, 0.0, 0.0, 0.0])
        return np.sqrt(np.clip(s, self.wp_idle ** 2, self.wp_max ** 2))

    def c(self) -> "_lib.BodyOptsC":
        return _lib.BodyOptsC(self.mass, (C.c_double * 3)(*self.inertia), (C.c_double * 12)(*self.Gf.ravel()),
                              (C.c_double * 12)(*self.Gt.ravel()), (C.c_double * 16)(*self.mixer.ravel()), self.wp_max,
                              self.wp_idle, self.tau_att, (C.c_double * 3)(*self.k_rate), self.tau_mot)

    def max_step(self) -> float:
        """The largest RK4 step dt / substeps a plant call admits: 1 / max(1 / tau_mot, max k_rate, 2 / tau_att)."""
        rate = max(float(self.k_rate.max()), 2.0 / self.tau_att)
        return 1.0 / (max(rate, 1.0 / self.tau_mot) if self.tau_mot > 0.0 else rate)


class VehicleModel:
    """The vehicle and estimator of ``batch`` instances on a context.  cfg: the config (robot.limits.gamma, for the
    hover input a reset writes); seed: the 64-bit key of every random number; delay: whole control periods, 0..8;
    thrust_tau: s; drag: three body-frame coefficients, 1/s; gust_std (m/s^2), gust_tau (s, 0: white from period to
    period); est_std_pos (m), est_std_vel (m/s), est_std_yaw (rad): the estimate's noise; est_bias: [batch, 7] or [7]
    constant offsets (p, v, yaw); stream_id: one int per instance, its identity in the random streams (None: its
    index); body: a ``RigidBody`` (excludes thrust_tau).  The hidden states (true state, actual thrust, gust, command
    ring, body rate, rotor speeds) live on the device."""

    def __init__(self, cfg, ctx, batch, seed=0, delay=0, thrust_tau=0.0, drag=(0, 0, 0), gust_std=0.0, gust_tau=0.0,
                 est_std_pos=0.0, est_std_vel=0.0, est_std_yaw=0.0, est_bias=None, stream_id=None, body=None):
        self.cfg, self.ctx, self.B, self.seed = cfg, ctx, int(batch), int(seed) & (2**64 - 1)
        self.delay, self.thrust_tau = int(delay), float(thrust_tau)
        self.drag = tuple(float(v) for v in np.broadcast_to(np.asarray(drag, dtype=np.float64), (3,)))
        self.gust_std, self.gust_tau = float(gust_std), float(gust_tau)
        self.est_std_pos, self.est_std_vel, self.est_std_yaw = float(est_std_pos), float(est_std_vel), float(est_std_yaw)
        self.est_bias = None if est_bias is None else np.ascontiguousarray(
            np.broadcast_to(np.asarray(est_bias, dtype=np.float64), (self.B, 7)))
        self.stream_id = None if stream_id is None else np.ascontiguousarray(stream_id, dtype=np.int32).ravel()
        if self.stream_id is not None and self.stream_id.size != self.B:
            raise ValueError(f"stream_id names {self.stream_id.size} instances, the batch has {self.B}")
        self._bias = None if self.est_bias is None else _lib.DeviceArray.from_numpy(ctx, self.est_bias)
        self._stream = None if self.stream_id is None else _lib.DeviceArray.from_numpy(ctx, self.stream_id)
        o = _lib.VehicleOptsC(self.seed, self.delay, self.thrust_tau, (C.c_double * 3)(*self.drag), self.gust_std,
                              self.gust_tau, self.est_std_pos, self.est_std_vel, self.est_std_yaw,
                              _lib._ptr(self._bias), _lib._ptr(self._stream), 9.81, float(cfg.robot.limits.gamma))
        h = C.c_void_p()
        _lib._check(_lib.load().sdfnmpc_vehicle_create(ctx.h, C.byref(o), self.B, C.byref(h)))  # refuses bad options
        self.h = h
        self.body = None
        if body is not None:
            try:
                self.set_body(body)
            except Exception:
                self.close()
                raise

    def set_body(self, body):
        """A ``RigidBody``: the vehicle's plant call becomes the rigid body's, its body rate and rotor speeds reset
        (zero, hover); None: the plain vehicle again, with the bits it had.  The library refuses bad parameters and a
        body beside a thrust lag."""
        _lib._check(_lib.load().sdfnmpc_vehicle_set_body(self.h, None if body is None else C.byref(body.c())))
        self.body = body

    def check_plant(self, plant):
        """Raise what a plant call with these options would refuse about the body's step size."""
        if self.body is not None and plant.dt / plant.substeps > self.body.max_step() * (1 + 1e-12):
            raise ValueError(f"the rigid body's inner loop admits RK4 steps of {self.body.max_step():.4g} s at the most; "
                             f"dt / substeps is {plant.dt / plant.substeps:.4g} s: give the plant more substeps")

    def _body_state(self):
        if self.body is None:
            raise ValueError("the vehicle has no body")
        om, ro = C.c_void_p(), C.c_void_p()
        _lib._check(_lib.load().sdfnmpc_vehicle_body_state(self.h, C.byref(om), C.byref(ro)))
        return om, ro

    @property
    def omega(self) -> np.ndarray:
        """The body rate [B, 3] in the body frame (a host copy, ordered on the context's stream)."""
        return _lib.FieldView(self._body_state()[0].value, (self.B, 3), np.float64, self.ctx).numpy()

    @property
    def rotor(self) -> np.ndarray:
        """The rotor speeds [B, 4] (a host copy)."""
        return _lib.FieldView(self._body_state()[1].value, (self.B, 4), np.float64, self.ctx).numpy()

    def set_body_state(self, omega, rotor):
        """Overwrite the body rate [B, 3] and the rotor speeds [B, 4] (synchronous): a start away from hover."""
        for p, a, n in zip(self._body_state(), (omega, rotor), (3, 4)):
            a = np.ascontiguousarray(np.broadcast_to(np.asarray(a, dtype=np.float64), (self.B, n)))
            if self.B:
                _lib._check(_lib.load().sdfnmpc_memcpy(self.ctx.h, p, a.ctypes.data, a.nbytes, 1))

    @property
    def neutral(self) -> bool:
        """Everything off: the model is the plant itself.  Never with a body."""
        return (self.body is None and self.delay == 0 and self.thrust_tau == 0.0 and self.gust_std == 0.0 and not any(self.drag)
                and self.est_std_pos == 0.0 and self.est_std_vel == 0.0 and self.est_std_yaw == 0.0
                and self.est_bias is None)

    def reset(self):
        """The hidden states as at creation: every ring slot the hover input, the actual thrust g, no gust; with a
        body no body rate and the hover rotor speeds."""
        _lib._check(_lib.load().sdfnmpc_vehicle_reset(self.h))

    def begin(self, x0_dev, frame):
        """x_true <- x0_dev; x0_dev <- the estimate of frame ``frame``: the one call before a loop's first step.
        x0_dev: a device float64 [B, 10] array holding the true state; it receives the estimate."""
        _lib._check(_lib.load().sdfnmpc_vehicle_begin(self.ctx.h, self.h, _lib._ptr(_lib.sync_producer(x0_dev)), int(frame)))

    def step(self, plant, u_dev, frame, x_est_out):
        """One plant call at frame ``frame`` on the model's own true state under the command u_dev [B, 4] (device
        float64); x_est_out [B, 10] receives the estimate of frame + 1.  plant: a ``_lib.plant_opts(...)``."""
        o = plant.c(self.ctx, self.B)
        _lib._check(_lib.load().sdfnmpc_plant_step_vehicle(self.ctx.h, C.byref(o), self.h, self.B,
                                                           _lib._ptr(_lib.sync_producer(u_dev)), int(frame),
                                                           _lib._ptr(x_est_out)))

    @property
    def x_true(self) -> np.ndarray:
        """The true state [B, 10] (a host copy, ordered on the context's stream)."""
        p = _lib.load().sdfnmpc_vehicle_x_true(self.h)
        return _lib.FieldView(p, (self.B, 10), np.float64, self.ctx).numpy()

    def close(self):
        if getattr(self, "h", None):
            _lib.load().sdfnmpc_vehicle_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass
