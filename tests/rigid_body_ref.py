"""CPU truth of the rigid-body vehicle (csrc/vehicle_body.hip): a numpy fp64 restatement written from the model's
equations, not from the kernel, on tests/vehicle_ref.py (delay, gust and estimate reused) and tests/plant_ref.py.

Hidden state per instance: x_true [10] = (p, q, v) with the full attitude, the body rate omega [3] (body frame), the
rotor speeds Omega [4].  One plant call applies the delayed input u, draws the gust, and integrates 17 states with
`substeps` classic RK4 steps of dt / substeps.  With F = m u0 gamma, roll_d, pitch_d, wz_d from the limits, at every
stage and with q normalised:
    psi = quat2yaw(q);  q_d = q_z(psi) (x) q_y(pitch_d) (x) q_x(roll_d)
    q_e = q^-1 (x) q_d, negated if q_e[0] < 0;  omega_sp = (2 q_e[1] / tau_att, 2 q_e[2] / tau_att, wz_d)
    tau = J k_rate (omega_sp - omega) + omega x J omega
    s = clip(M [F; tau], wp_idle^2, wp_max^2);  Omega_cmd = sqrt(s)
    dOmega/dt = (Omega_cmd - Omega) / tau_mot                 (tau_mot = 0: Omega = Omega_cmd)
    dp/dt = v;  dq/dt = q (x) (0, omega) / 2                  (quad_props.py:41-48)
    dv/dt = R(q) Gf Omega^2 gamma_scale / m - g e_z + acc_dist + gust - R diag(drag) R^T v
    domega/dt = (Gt Omega^2 - omega x J omega) / J
A reset gives omega = 0 and Omega = sqrt(M [m g; 0; 0; 0]).  Gf, Gt from (motors, cf, ct) as quad_props.py:20-27,
M = inv([Gf row z; Gt])."""
import numpy as np

import plant_ref
import vehicle_ref

G = plant_ref.G

# the reference's default.yaml robot.* (mass, inertia, alloc, limits.wp) and the inner loop's suggested defaults
DEFAULT = dict(mass=1.46, inertia=(0.017, 0.018, 0.028),
               motors=[[0.09, -0.09, -0.005, 0, 0, -1], [-0.09, 0.09, -0.005, 0, 0, -1],
                       [0.09, 0.09, -0.005, 0, 0, 1], [-0.09, -0.09, -0.005, 0, 0, 1]],
               cf=0.02246, ct=0.00020673, wp_max=25.0)
LOOP = dict(tau_att=0.1, k_rate=(20.0, 20.0, 8.0), tau_mot=0.02)


def axis_rot(axis, a):
    c, s = np.cos(a), np.sin(a)
    if axis == "x":
        return np.array([[1, 0, 0], [0, c, -s], [0, s, c]])
    if axis == "y":
        return np.array([[c, 0, s], [0, 1, 0], [-s, 0, c]])
    return np.array([[c, -s, 0], [s, c, 0], [0, 0, 1]])


def allocation(motors, cf, ct):
    """Gf, Gt [3, n]: rotor i's thrust axis R_i e_z with R_i = Rz(i pi / (n / 2)) Ry(beta_i) Rx((-1)^i alpha_i); its
    torque column p_i x axis + (ct / cf) sign_i axis; both times cf."""
    m = np.asarray(motors, float)
    n = len(m)
    gf, gt = np.zeros((3, n)), np.zeros((3, n))
    for i in range(n):
        p, alpha, beta, sign = m[i, :3], m[i, 3], m[i, 4], m[i, 5]
        R = axis_rot("z", i * (np.pi / (n / 2))) @ axis_rot("y", beta) @ axis_rot("x", (-1) ** i * alpha)
        z = R @ np.array([0.0, 0.0, 1.0])
        gf[:, i] = z
        gt[:, i] = np.cross(p, z) + ct / cf * sign * z
    return cf * gf, cf * gt


def mixer(Gf, Gt):
    return np.linalg.inv(np.vstack([Gf[2:3], Gt]))


def quat2yaw(q):
    return np.arctan2(2 * (q[:, 0] * q[:, 3] + q[:, 1] * q[:, 2]), 1 - 2 * (q[:, 2] ** 2 + q[:, 3] ** 2))


def quat2euler(q):
    """[B, 4] -> roll, pitch, yaw [B] each (utils/math.py quat2euler), q normalised here."""
    q = q / np.linalg.norm(q, axis=-1, keepdims=True)
    roll = np.arctan2(2 * (q[:, 0] * q[:, 1] + q[:, 2] * q[:, 3]), 1 - 2 * (q[:, 1] ** 2 + q[:, 2] ** 2))
    pitch = np.arcsin(2 * (q[:, 0] * q[:, 2] - q[:, 3] * q[:, 1]))
    return roll, pitch, quat2yaw(q)


def body_f_expl(x13, wp, mass, inertia, Gf, Gt, g=G):
    """quad_props.py:41-48 on x13 [B, 13] = (p, q, v, omega) under the rotor speeds wp [B, 4]."""
    q = x13[:, 3:7] / np.linalg.norm(x13[:, 3:7], axis=-1, keepdims=True)
    w = x13[:, 10:13]
    J = np.asarray(inertia, float)
    s2 = wp ** 2
    R = vehicle_ref.quat2rot(q)
    W_a = np.einsum("bij,bj->bi", R, s2 @ Gf.T) / mass + np.array([0.0, 0.0, -g])
    dq = plant_ref._hprod(q, np.concatenate([np.zeros((len(q), 1)), w], -1)) / 2
    dw = (s2 @ Gt.T - np.cross(w, J * w)) / J
    return np.concatenate([x13[:, 7:10], dq, W_a, dw], -1)


class RigidBodyVehicle(vehicle_ref.Vehicle):
    """vehicle_ref.Vehicle with steps 3 and 5 of the plant call replaced by the rigid body."""

    def __init__(self, cfg, B, mass, inertia, motors, cf, ct, wp_max, wp_idle=None, tau_att=0.1, k_rate=(20.0, 20.0, 8.0),
                 tau_mot=0.02, **vehicle):
        self.m, self.J = float(mass), np.broadcast_to(np.asarray(inertia, float), (3,)).copy()
        self.Gf, self.Gt = allocation(motors, cf, ct)
        self.M = mixer(self.Gf, self.Gt)
        self.wp_max = float(wp_max)
        self.wp_idle = 0.1 * self.wp_max if wp_idle is None else float(wp_idle)
        self.tau_att, self.tau_mot = float(tau_att), float(tau_mot)
        self.k_rate = np.broadcast_to(np.asarray(k_rate, float), (3,)).copy()
        self.clipped_idle = self.clipped_max = 0  # stage evaluations with some rotor clipped, over the object's life
        super().__init__(cfg, B, **vehicle)
        assert self.tau_m == 0.0, "the rotor lag replaces the thrust lag"

    def reset(self):
        super().reset()
        self.omega = np.zeros((self.B, 3))
        s = self.M @ np.array([self.m * G, 0.0, 0.0, 0.0])
        self.rotor = np.tile(np.sqrt(np.clip(s, self.wp_idle ** 2, self.wp_max ** 2)), (self.B, 1))

    def rotor_cmd(self, z, u_app, count=False):
        """Omega_cmd [B, 4] of the inner loop at the states z [B, 17]."""
        q = z[:, 3:7] / np.linalg.norm(z[:, 3:7], axis=-1, keepdims=True)
        w = z[:, 10:13]
        F = self.m * u_app[:, 0] * self.lim[0]
        roll_d, pitch_d, wz_d = u_app[:, 1] * self.lim[1], u_app[:, 2] * self.lim[2], u_app[:, 3] * self.lim[3]
        zero = np.zeros(len(q))
        qz = np.stack([np.cos(quat2yaw(q) / 2), zero, zero, np.sin(quat2yaw(q) / 2)], -1)
        qy = np.stack([np.cos(pitch_d / 2), zero, np.sin(pitch_d / 2), zero], -1)
        qx = np.stack([np.cos(roll_d / 2), np.sin(roll_d / 2), zero, zero], -1)
        q_d = plant_ref._hprod(plant_ref._hprod(qz, qy), qx)
        q_e = plant_ref._hprod(q * np.array([1.0, -1.0, -1.0, -1.0]), q_d)
        q_e = np.where(q_e[:, :1] < 0, -q_e, q_e)
        w_sp = np.stack([2 * q_e[:, 1] / self.tau_att, 2 * q_e[:, 2] / self.tau_att, wz_d], -1)
        tau = self.J * (self.k_rate * (w_sp - w)) + np.cross(w, self.J * w)
        s = np.concatenate([F[:, None], tau], -1) @ self.M.T
        lo, hi = self.wp_idle ** 2, self.wp_max ** 2
        if count:
            self.clipped_idle += int((s < lo).any())
            self.clipped_max += int((s > hi).any())
        return np.sqrt(np.clip(s, lo, hi))

    def step(self, kind, u_cmd, frame, dt, substeps=1, acc_dist=None, gamma_scale=None):
        """One plant call (kind only names the limits' owner: ignored); returns the estimate of frame + 1."""
        u_cmd = np.array(u_cmd, dtype=np.float64).reshape(self.B, 4)
        if self.d > 0:  # 1. delay
            slot = int(frame) % self.d
            u_app = self.ring[:, slot].copy()
            self.ring[:, slot] = u_cmd
        else:
            u_app = u_cmd
        self.u_app = u_app
        gust = self.gust_std > 0.0
        if gust:  # 2. gust
            phi = np.exp(-dt / self.gust_tau) if self.gust_tau > 0.0 else 0.0
            xi = vehicle_ref.normals(self.seed, frame, self.stream)[:, :3]
            self.w = phi * self.w + self.gust_std * np.sqrt(1.0 - phi * phi) * xi
        lag = self.tau_mot > 0.0
        gs = np.ones(self.B) if gamma_scale is None else np.asarray(gamma_scale, float)
        has_drag = bool(np.any(self.drag))

        def f(z):
            oc = self.rotor_cmd(z, u_app, count=True)
            wp = z[:, 13:17] if lag else oc
            q = z[:, 3:7] / np.linalg.norm(z[:, 3:7], axis=-1, keepdims=True)
            R = vehicle_ref.quat2rot(q)
            d = body_f_expl(z[:, :13], wp, self.m, self.J, self.Gf, self.Gt)
            # the thrust-gain error scales the rotors' force, not gravity
            d[:, 7:10] = (d[:, 7:10] + np.array([0.0, 0.0, G])) * gs[:, None] - np.array([0.0, 0.0, G])
            if acc_dist is not None:
                d[:, 7:10] = d[:, 7:10] + acc_dist
            if gust:
                d[:, 7:10] = d[:, 7:10] + self.w
            if has_drag:
                vb = np.einsum("bji,bj->bi", R, z[:, 7:10]) * self.drag
                d[:, 7:10] = d[:, 7:10] - np.einsum("bij,bj->bi", R, vb)
            dO = (oc - z[:, 13:17]) / self.tau_mot if lag else np.zeros((self.B, 4))
            return np.concatenate([d, dO], -1)

        z = np.concatenate([self.x_true, self.omega, self.rotor], -1)
        h = dt / substeps
        for _ in range(substeps):
            k1 = f(z)
            k2 = f(z + h / 2 * k1)
            k3 = f(z + h / 2 * k2)
            k4 = f(z + h * k3)
            z = z + h / 6 * (k1 + 2 * k2 + 2 * k3 + k4)
        self.x_true, self.omega = z[:, :10].copy(), z[:, 10:13].copy()
        self.rotor = z[:, 13:17].copy() if lag else self.rotor_cmd(z, u_app)
        return self.est(int(frame) + 1)


def tilted_states(rng, B, rate=1.0, flip=True):
    """plant_ref.states with body rates of standard deviation `rate` rad/s, rotor speeds in 4..22, and (flip) every
    third quaternion given the sign that makes q0 < 0."""
    x, u = plant_ref.states(rng, B)
    if flip:
        x[::3, 3:7] *= -np.sign(x[::3, 3:4])
    return x, u, rng.normal(0, rate, (B, 3)), rng.uniform(4.0, 22.0, (B, 4))
