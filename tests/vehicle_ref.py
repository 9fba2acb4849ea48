"""CPU truth of the vehicle model (csrc/vehicle.hip, sdfnmpc_plant_step_vehicle): a numpy fp64 restatement written
from the model's equations, not from the kernel, on tests/plant_ref.f_expl and tests/sensor_ref.philox4x32_10.

One plant call at frame f with the command u_cmd, in this order:
  1. delay d: u_app = ring[f % d], ring[f % d] <- u_cmd (d = 0: u_app = u_cmd); after a reset every slot is hover,
     (g / gamma, 0, 0, 0);
  2. gust: w <- phi w + sigma_g sqrt(1 - phi^2) xi(f), phi = exp(-dt / tau_g) (tau_g = 0: phi = 0), constant over the
     period, added to dv/dt;
  3. thrust lag: d(gamma_act)/dt = (gamma_cmd - gamma_act) / tau_m with gamma_cmd = u_app[0] gamma gamma_scale, an 11th
     RK4 state; the thrust of f_expl is the stage's gamma_act (tau_m = 0: gamma_cmd); after a reset gamma_act = g;
  4. drag: dv/dt gains -R diag(drag) R^T v, R = Rz(yaw) euler2rot(roll_cmd, pitch_cmd, 0) for 'att' and
     quat2rot(q / |q|) for 'att_tau';
  5. classic RK4 with `substeps` steps of dt / substeps;
  6. the estimate of frame f + 1: p + bias_p + sigma_p n_p, v + bias_v + sigma_v n_v, q_hat = [cos(delta / 2), 0, 0,
     sin(delta / 2)] (x) q with delta = bias_yaw + sigma_yaw n_yaw.

Random numbers: Philox4x32-10 under the key (seed's low word, high word) with the counter (j, frame, stream, 1), j =
0..4; call j gives n[2j] = N(w0, w1) and n[2j+1] = N(w2, w3), N = sensor_ref.normal.  n[0..2] -> xi at the call's frame,
n[3..5] -> n_p, n[6..8] -> n_v, n[9] -> n_yaw at the estimate's frame.  With everything off the step is
plant_ref.step, operation for operation."""
import numpy as np

import plant_ref
import sensor_ref

G = plant_ref.G


def words(seed, j, frame, stream):
    """The four Philox words of call j of (frame, stream): the counter (j, frame, stream, 1)."""
    seed = int(seed) & (2**64 - 1)
    st = np.asarray(stream, dtype=np.int64) & 0xffffffff
    return sensor_ref.philox4x32_10(int(j), int(frame), st, 1, seed & 0xffffffff, seed >> 32)


def normals(seed, frame, stream):
    """n [B, 10] of a frame for the streams [B]."""
    n = []
    for j in range(5):
        w0, w1, w2, w3 = words(seed, j, frame, stream)
        n += [sensor_ref.normal(w0, w1), sensor_ref.normal(w2, w3)]
    return np.stack(n, -1)


def quat2rot(q):
    """[B, 4] unit quaternions -> [B, 3, 3] (utils/math.py quat2rot)."""
    q0, q1, q2, q3 = q.T
    return np.stack([
        np.stack([q0**2 + q1**2 - q2**2 - q3**2, 2 * (q1 * q2 - q0 * q3), 2 * (q1 * q3 + q0 * q2)], -1),
        np.stack([2 * (q1 * q2 + q0 * q3), q0**2 - q1**2 + q2**2 - q3**2, 2 * (q2 * q3 - q0 * q1)], -1),
        np.stack([2 * (q1 * q3 - q0 * q2), 2 * (q2 * q3 + q0 * q1), q0**2 - q1**2 - q2**2 + q3**2], -1)], 1)


def euler2rot(roll, pitch, yaw):
    """[B] angles -> [B, 3, 3], Z1 Y2 X3 (utils/math.py euler2rot)."""
    cr, sr, cp, sp, cy, sy = np.cos(roll), np.sin(roll), np.cos(pitch), np.sin(pitch), np.cos(yaw), np.sin(yaw)
    return np.stack([
        np.stack([cp * cy, sr * sp * cy - cr * sy, cr * sp * cy + sr * sy], -1),
        np.stack([cp * sy, sr * sp * sy + cr * cy, cr * sp * sy - sr * cy], -1),
        np.stack([-sp, sr * cp, cr * cp], -1)], 1)


def body_rotation(kind, x, u_app, lim):
    """R [B, 3, 3]: the body rotation the model's thrust uses."""
    q = x[:, 3:7] / np.linalg.norm(x[:, 3:7], axis=-1, keepdims=True)
    if kind == 0:
        yaw = 2.0 * np.arctan2(q[:, 3], q[:, 0])
        zero = np.zeros_like(yaw)
        return euler2rot(zero, zero, yaw) @ euler2rot(u_app[:, 1] * lim[1], u_app[:, 2] * lim[2], zero)
    return quat2rot(q)


def estimate(x, n, std_p=0.0, std_v=0.0, std_yaw=0.0, bias=None):
    """est(x) [B, 10] under the normals n [B, 10] of its frame; no noise and no bias: x itself."""
    if std_p == 0.0 and std_v == 0.0 and std_yaw == 0.0 and bias is None:
        return x.copy()
    b = np.zeros((x.shape[0], 7)) if bias is None else np.broadcast_to(np.asarray(bias, float), (x.shape[0], 7))
    xe = x.copy()
    xe[:, :3] = x[:, :3] + b[:, :3] + std_p * n[:, 3:6]
    xe[:, 7:] = x[:, 7:] + b[:, 3:6] + std_v * n[:, 6:9]
    delta = b[:, 6] + std_yaw * n[:, 9]
    zero = np.zeros_like(delta)
    xe[:, 3:7] = plant_ref._hprod(np.stack([np.cos(delta / 2), zero, zero, np.sin(delta / 2)], -1), x[:, 3:7])
    return xe


class Vehicle:
    """The hidden states of B instances and the plant call on them."""

    def __init__(self, cfg, B, seed=0, delay=0, thrust_tau=0.0, drag=(0, 0, 0), gust_std=0.0, gust_tau=0.0,
                 est_std_pos=0.0, est_std_vel=0.0, est_std_yaw=0.0, est_bias=None, stream_id=None):
        self.cfg, self.B, self.seed, self.d = cfg, int(B), int(seed), int(delay)
        self.tau_m, self.drag = float(thrust_tau), np.broadcast_to(np.asarray(drag, float), (3,)).copy()
        self.gust_std, self.gust_tau = float(gust_std), float(gust_tau)
        self.std = (float(est_std_pos), float(est_std_vel), float(est_std_yaw))
        self.bias = est_bias
        self.stream = np.arange(self.B) if stream_id is None else np.asarray(stream_id)
        self.lim = plant_ref.limits(cfg)
        self.x_true = np.zeros((self.B, 10))
        self.reset()

    def reset(self):
        self.ring = np.zeros((self.B, self.d, 4))
        self.ring[:, :, 0] = G / self.lim[0]
        self.gamma_act = np.full(self.B, G)
        self.w = np.zeros((self.B, 3))

    def est(self, frame):
        n = normals(self.seed, frame, self.stream) if any(self.std) else np.zeros((self.B, 10))
        return estimate(self.x_true, n, *self.std, bias=self.bias)

    def begin(self, x0, frame):
        """x_true <- x0; returns est(x_true, frame)."""
        self.x_true = np.array(x0, dtype=np.float64).reshape(self.B, 10)
        return self.est(frame)

    def step(self, kind, u_cmd, frame, dt, substeps=1, acc_dist=None, gamma_scale=None):
        """One plant call; returns the estimate of frame + 1.  self.u_app is the input it applied."""
        kind = plant_ref.KINDS.get(kind, kind)
        u_cmd = np.array(u_cmd, dtype=np.float64).reshape(self.B, 4)
        # 1. delay
        if self.d > 0:
            slot = int(frame) % self.d
            u_app = self.ring[:, slot].copy()
            self.ring[:, slot] = u_cmd
        else:
            u_app = u_cmd
        self.u_app = u_app
        # 2. gust
        gust = self.gust_std > 0.0
        if gust:
            phi = np.exp(-dt / self.gust_tau) if self.gust_tau > 0.0 else 0.0
            xi = normals(self.seed, frame, self.stream)[:, :3]
            self.w = phi * self.w + self.gust_std * np.sqrt(1.0 - phi * phi) * xi
        # 3. thrust
        lag = self.tau_m > 0.0
        gamma_cmd = u_app[:, 0] * self.lim[0]
        if gamma_scale is not None:
            gamma_cmd = gamma_cmd * gamma_scale
        has_drag = bool(np.any(self.drag))

        def f(z):
            x = z[:, :10]
            if lag:  # the stage's actual thrust, as the thrust input that produces it
                u = u_app.copy()
                u[:, 0] = z[:, 10] / self.lim[0]
                dx = plant_ref.f_expl(kind, x, u, self.lim, acc_dist, None)
            else:
                dx = plant_ref.f_expl(kind, x, u_app, self.lim, acc_dist, gamma_scale)
            if gust:
                dx[:, 7:] = dx[:, 7:] + self.w
            if has_drag:  # 4. drag
                R = body_rotation(kind, x, u_app, self.lim)
                vb = np.einsum("bji,bj->bi", R, x[:, 7:]) * self.drag
                dx[:, 7:] = dx[:, 7:] - np.einsum("bij,bj->bi", R, vb)
            if lag:
                dx = np.concatenate([dx, ((gamma_cmd - z[:, 10]) / self.tau_m)[:, None]], -1)
            return dx

        # 5. RK4
        z = np.concatenate([self.x_true, self.gamma_act[:, None]], -1) if lag else self.x_true.copy()
        h = dt / substeps
        for _ in range(substeps):
            k1 = f(z)
            k2 = f(z + h / 2 * k1)
            k3 = f(z + h / 2 * k2)
            k4 = f(z + h * k3)
            z = z + h / 6 * (k1 + 2 * k2 + 2 * k3 + k4)
        self.x_true = z[:, :10].copy()
        if lag:
            self.gamma_act = z[:, 10].copy()
        # 6. the estimate of the next frame
        return self.est(int(frame) + 1)
