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
"""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import _lib


class VehicleModel:
    """The vehicle and estimator of ``batch`` instances on a context.  cfg: the config (robot.limits.gamma, for the
    hover input a reset writes); seed: the 64-bit key of every random number; delay: whole control periods, 0..8;
    thrust_tau: s; drag: three body-frame coefficients, 1/s; gust_std (m/s^2), gust_tau (s, 0: white from period to
    period); est_std_pos (m), est_std_vel (m/s), est_std_yaw (rad): the estimate's noise; est_bias: [batch, 7] or [7]
    constant offsets (p, v, yaw); stream_id: one int per instance, its identity in the random streams (None: its
    index).  The hidden states (true state, actual thrust, gust, command ring) live on the device."""

    def __init__(self, cfg, ctx, batch, seed=0, delay=0, thrust_tau=0.0, drag=(0, 0, 0), gust_std=0.0, gust_tau=0.0,
                 est_std_pos=0.0, est_std_vel=0.0, est_std_yaw=0.0, est_bias=None, stream_id=None):
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

    @property
    def neutral(self) -> bool:
        """Everything off: the model is the plant itself."""
        return (self.delay == 0 and self.thrust_tau == 0.0 and self.gust_std == 0.0 and not any(self.drag)
                and self.est_std_pos == 0.0 and self.est_std_vel == 0.0 and self.est_std_yaw == 0.0
                and self.est_bias is None)

    def reset(self):
        """The hidden states as at creation: every ring slot the hover input, the actual thrust g, no gust."""
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
