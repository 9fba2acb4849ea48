"""Batched GPU counterpart of the reference controller (sdf_nmpc/controller.py:Nmpc).

Same methods, argument meaning and array layouts as the reference; every per-instance array gains
an optional leading batch dimension (``batch`` instances solved together, one SQP-RTI iteration per
``solve``).  With ``batch=1`` the shapes are exactly the reference's.

  reset()                              controller.py:35    p, y, yN, W, WN zeroed, flag off, latent reset
  set_sdf_flag(flag)                   controller.py:45
  set_latent(latent, W_p_Bo, W_R_Bo)   controller.py:50    W_p_Co, W_R_Co (row-major 3x3), latent in p
  reset_latent()                       controller.py:57
  set_x0(x0)                           controller.py:65    first call initialises the OCP
  solve()                              controller.py:72    shift + one RTI iteration; returns fail_count
  get_matrices(), get_u(), get_cmd_acc(), get_cmd_TRPYr(), get_openloop_traj(), eval(k), set_ref(ref, k)

Host setters write the host arrays (``p``, ``y``, ``W``, ``yN``, ``WN``) and mark the rows and columns
they touched; ``solve`` uploads exactly those regions.  Device-side setters (``gen_refs_device``,
``set_latent_device``, ``VaeWrapper.encode_to``) write the solver's device buffers directly and clear
the host marks of what they wrote.  The last writer of a region wins, whichever side it is on.
No tensor library is used on this path.

``get_cmd_props`` exists in the reference only for the 'props' model; this build is the 'att' and 'att_tau'
models (model.Quad, cfg.mpc.model), where the reference raises AttributeError too.
"""
from __future__ import annotations

import numpy as np

from .model import Quad


class Rollout:
    """What ``Nmpc.rollout`` logged (numpy arrays, batch-leading): x [B, K+1, 10] plant states (row 0 the start),
    u [B, K, 4] applied inputs, status / iters [B, K] of every QP; with images also col [B, K+1] collision labels
    and pts [B, K+1, 3] the camera-frame positions they were taken at (else None); with a scene clearance [B, K+1],
    the exact signed distance of every logged position to the instance's scene at the time of that row, t [K+1]
    (the scene's clock at every log row), and with keep_img img [B, h, w] float32, the last images rendered (raw
    sensor values).  With a vehicle model x, col, pts and clearance are the true vehicle's, u the commands, and
    xhat [B, K+1, 10] the state estimates the controller was given (row 0 the one it started from), u_applied [B, K, 4]
    the inputs the vehicle applied (the delayed commands); else both None.  With a rigid-body vehicle omega [B, K+1, 3],
    its body rates, and rotor [B, K+1, 4], its rotor speeds (row 0 before the first step); else both None.  With
    ``swept`` swept_clearance, swept_gap and swept_s [B, K]: entry k is the minimum distance to the scene along the
    chord from log row k to row k+1 between t[k] and t[k+1], its certificate (the minimum lies in [swept_clearance -
    swept_gap, swept_clearance]) and the chord parameter it was found at; else all three None."""

    def __init__(self, x, u, status, iters, col=None, pts=None, clearance=None, img=None, t=None, xhat=None,
                 u_applied=None, omega=None, rotor=None):
        self.x, self.u, self.status, self.iters, self.col, self.pts = x, u, status, iters, col, pts
        self.clearance, self.img, self.t = clearance, img, t
        self.xhat, self.u_applied, self.omega, self.rotor = xhat, u_applied, omega, rotor
        self.swept_clearance = self.swept_gap = self.swept_s = None


class Nmpc:
    """Wrapper around the NMPC controller with range image-based collision prediction (batched)."""

    def __init__(self, cfg, rebuild=False, batch: int = 1, device: int = 0, weights=None, ocp=None,
                 braking_coeffs=None):
        """braking_coeffs: the braking-distance polynomial of flags.recursive_feasibility (default: the
        config's mpc.braking_dist.coeff_file under the cache dir, as gen_model.py:76-77 loads it)."""
        from .ocp import Ocp

        self.cfg = cfg
        self.model = getattr(ocp, "model", None) or Quad(cfg, braking_coeffs=braking_coeffs)
        self.T = cfg.mpc.T
        self.N = int(cfg.mpc.N)
        self.B = int(batch)
        self.ocp = ocp if ocp is not None else Ocp(self.model, build=rebuild, batch=batch, device=device,
                                                  weights=weights)
        lim = cfg.robot.limits
        self.cmd_acc_hover = np.array([0, 0, 0, 0])
        self.cmd_acc_min = [-lim.ax, -lim.ay, -lim.az, -lim.wz]
        self.cmd_acc_max = [lim.ax, lim.ay, lim.az, lim.wz]
        self.cmd_TRPYr_hover = np.array([cfg.robot.mass * self.model.g, 0, 0, 0])
        self.cmd_TRPYr_min = [0, -lim.roll, -lim.pitch, -lim.wz]
        self.cmd_TRPYr_max = [lim.gamma, lim.roll, lim.pitch, lim.wz]
        self._sdf_scene = None  # the scene whose exact distance replaces the network (set_sdf_scene)
        self._sdf_image = None  # or the image source: its option block and the device arrays it names (set_sdf_image)
        self.reset()

    # ---- state of the controller (host arrays, batch-leading; B == 1 keeps the reference's shapes)
    def _shape(self, *s):
        return s if self.B == 1 else (self.B,) + s

    # ---- dirty regions of the host arrays: (field, col0, ncol) -> row mask [B][nodes]
    def _groups(self):
        idx, m = self.cfg.mpc.p_idx, self.model
        return {"flag": ("p", int(idx.flag), 1), "pose": ("p", int(idx.W_p_Co[0]), 12),
                "q_d": ("p", int(idx.q_d[0]), 4), "latent": ("p", int(idx.latent), m.np - int(idx.latent)),
                "yref": ("yref", 0, m.ny), "W": ("W", 0, m.ny), "yNref": ("yNref", 0, m.nyN), "WN": ("WN", 0, m.nyN)}

    def _mark(self, group, b=None, k=None):
        """Mark rows (instance b or all, node k or all) of a column group dirty."""
        field, _, _ = self._groups()[group]
        nodes = {"p": self.N + 1, "yref": self.N, "W": self.N}.get(field, 1)
        m = self._dirty.setdefault(group, np.zeros((max(self.B, 1), nodes), bool))
        m[(slice(None) if b is None else b), (slice(None) if k is None else k)] = True

    def _flush(self):
        """Upload the dirty host regions into the solver's device buffers."""
        host = {"p": self.p, "yref": self.y, "W": self.W, "yNref": self.yN, "WN": self.WN}
        groups = self._groups()
        for g, mask in self._dirty.items():
            field, col0, ncol = groups[g]
            a = host[field]
            a = a[None] if self.B == 1 else a
            if field in ("yNref", "WN"):
                a = a[:, None]
            self.ocp.upload(field, a, col0, ncol, mask)
        self._dirty = {}

    def _clean(self, *groups):
        for g in groups:
            self._dirty.pop(g, None)

    def reset(self):
        """Reset internal matrices to default values (controller.py:35-44)."""
        m = self.model
        self._dirty = {}
        self.x0 = None
        self.p = np.zeros(self._shape(self.N + 1, m.np))
        self.y = np.zeros(self._shape(self.N, m.ny))
        self.yN = np.zeros(self._shape(m.nyN))
        self.W = np.zeros(self._shape(self.N, m.ny))
        self.WN = np.zeros(self._shape(m.nyN))
        self.fail_count = 0
        self.fail_counts = np.zeros(self.B, dtype=int)  # per-instance consecutive QP failures
        self.set_sdf_flag(False)
        self.reset_latent()
        for g in ("q_d", "yref", "W", "yNref", "WN"):
            self._mark(g)

    # ---- parameter setters
    def set_sdf_flag(self, flag):
        """Enable/disable the sdf constraint (controller.py:47-49); flag: scalar or [B]."""
        f = np.asarray(flag, dtype=float)
        self.p[..., self.cfg.mpc.p_idx.flag] = f[..., None] if f.ndim else f
        self._mark("flag")

    def set_latent(self, latent, W_p_Bo, W_R_Bo):
        """Latent and camera pose at the time of the image (controller.py:50-54), batched over a leading dim."""
        idx = self.cfg.mpc.p_idx
        W_R_Bo = np.asarray(W_R_Bo, dtype=float)
        W_p_Co = W_R_Bo @ np.asarray(self.cfg.sensor.B_p_C, dtype=float).ravel() + W_p_Bo
        W_R_Co = (W_R_Bo @ np.asarray(self.cfg.sensor.B_R_C, dtype=float)).reshape(W_R_Bo.shape[:-2] + (9,))
        self.p[..., idx.W_p_Co] = np.asarray(W_p_Co)[..., None, :]
        self.p[..., idx.W_R_Co] = W_R_Co[..., None, :]
        self.p[..., idx.latent:] = np.asarray(latent, dtype=float)[..., None, :]
        self._mark("pose")
        self._mark("latent")

    def reset_latent(self):
        """controller.py:59-63."""
        idx = self.cfg.mpc.p_idx
        self.p[..., idx.W_p_Co] = 0
        self.p[..., idx.W_R_Co] = 0
        self.p[..., idx.latent:] = 0
        self._mark("pose")
        self._mark("latent")

    # ---- the exact scene distance as the SDF (csrc/scene_sdf.hip)
    def set_sdf_scene(self, scene, max_df=None, predict=False):
        """The SDF row of the constraints (and the sdf cost) from the exact signed distance of ``scene`` (a
        ``scene.Scene`` on the controller's context) instead of the network, truncated at ``max_df`` (default
        model.max_df) as the network's training target is: the same controller with a perfect distance, the yardstick
        a learned one is measured against.  ``solve`` and ``rollout`` use it from the next call on; the scene is seen at
        the time of ``set_scene_time`` (``rollout`` sets it per step).  predict: node k of the horizon sees a moving
        scene at that time + the node's own time on the shooting grid, not as a static world.  None restores the
        network, and so does closing the scene while it is the source.  A mesh scene is taken when it was created with
        ``Scene.mesh(..., sdf_source=True)`` (else SdfnmpcError, error -4); without ``movers=`` it is static, so
        ``predict`` changes nothing, with them ``predict`` shows every node the movers at its own time.
        ValueError, before anything is enqueued: a batch split over several devices, a scene on another
        context, a ``scene_of`` that does not fit the batch, a model whose flags read no SDF."""
        if len(self.ocp.parts) != 1:
            raise ValueError("set_sdf_scene(): the batch is split over several devices; sharded batches are not built")
        solver = self.ocp.parts[0].solver
        if scene is None:
            solver.set_sdf_scene(None)
            if self._sdf_scene is not None:
                self._sdf_scene._sdf_users.discard(self)
            self._sdf_scene = self._sdf_image = None
            return
        if scene.ctx is not self.ocp.ctx:
            raise ValueError("set_sdf_scene(): the scene must be built on the controller's context (ctx=nmpc.ocp.ctx)")
        scene._batch(max(self.B, 1))
        if not self.model.need_sdf:
            raise ValueError("set_sdf_scene(): no constraint row or cost of this model's flags reads the SDF")
        md = float(self.model.max_df if max_df is None else max_df)
        if not (np.isfinite(md) and md > 0.0):
            raise ValueError(f"max_df {max_df}: positive and finite")
        solver.set_sdf_scene(scene.h, scene._scene_of, md, bool(predict))
        if self._sdf_scene is not None:
            self._sdf_scene._sdf_users.discard(self)
        self._sdf_scene = scene  # kept alive here; Scene.close() takes itself out of its users first
        self._sdf_image = None   # the two sources replace each other
        scene._sdf_users.add(self)

    # ---- the camera image's own field as the SDF (csrc/df_truth.hip: img_sdf_rows_kernel)
    def set_sdf_image(self, imgs, signed=True, max_df=None, img_of=None, reconstruct=None):
        """The SDF row of the constraints (and the sdf cost) from the distance field the camera image itself implies --
        ``DfComputer.get_df``, the network's training target -- instead of the network: the perfect network, with the
        learned one's partial observability and image staleness and no approximation error.  imgs: [B, H, W] (or [H, W]
        for one instance) float32 range images normalised by sensor.dmax, host or device (copied: the controller owns
        its image buffer, the pooled buffer of the unsigned mode and the device voxel grid of the signed one, and keeps
        them alive while they are the source).  signed: ``get_sdf`` over the voxel grid, clamped to [-0.3, max_df];
        else ``get_udf`` over the 5x5 min-pooled image, clamped to [0, max_df] (H and W multiples of 5).  max_df
        defaults to model.max_df.  img_of: int [B], the image of each instance (imgs then holds any number of images;
        a rollout that re-images needs one per instance, img_of None).  The camera pose is whatever ``set_latent`` /
        ``set_pose_device`` put in p.  ``solve`` and ``rollout`` use the source from the next call on; None restores the
        network.  ``set_sdf_scene`` and ``set_sdf_image`` replace each other.  reconstruct: a ``VaeWrapper`` with a
        decoder on the controller's context and ``batch=B`` -- the source then holds ``reconstruct.reconstruct(imgs)``,
        the image the VAE's latent retains (imgs: normalised images of the configured sensor, encoded with clip = 1 and
        Depth2Range when sensor.is_depth), the rung between the camera image and the network; the reconstruction is a
        RANGE image, so the source's image options have is_depth off.  A ``rollout(scene=...)`` of such a source
        re-images through the VAE (sdfnmpc_solver_rollout_image_recon).  reconstruct excludes img_of.  ValueError,
        before anything is enqueued: a batch split over several devices, a model whose flags read no SDF, a wrong image
        count, unsigned with H or W not a multiple of 5, a reconstruct wrapper without a decoder, on another context or
        of another batch size, reconstruct with img_of."""
        from . import _lib
        if len(self.ocp.parts) != 1:
            raise ValueError("set_sdf_image(): the batch is split over several devices; sharded batches are not built")
        solver, ctx, Bn = self.ocp.parts[0].solver, self.ocp.ctx, max(self.B, 1)
        if imgs is None:
            solver.set_sdf_image(None)
            if self._sdf_scene is not None:
                self._sdf_scene._sdf_users.discard(self)
            self._sdf_scene = self._sdf_image = None
            return
        if not self.model.need_sdf:
            raise ValueError("set_sdf_image(): no constraint row or cost of this model's flags reads the SDF")
        md = float(self.model.max_df if max_df is None else max_df)
        if not (np.isfinite(md) and md > 0.0):
            raise ValueError(f"max_df {max_df}: positive and finite")
        on_dev = hasattr(imgs, "data_ptr")
        if on_dev and np.dtype(str(imgs.dtype).replace("torch.", "")) != np.float32:
            raise TypeError(f"device images must be float32, got {imgs.dtype}")
        shape = tuple(int(v) for v in imgs.shape) if on_dev else np.shape(imgs)
        if len(shape) == 2:
            shape = (1,) + tuple(shape)
        if len(shape) != 3:
            raise ValueError("input image must have size [B, H, W] or [H, W]")
        io = None
        if img_of is not None:
            io = np.ascontiguousarray(np.asarray(img_of).reshape(-1), dtype=np.int32)
            if io.size != Bn or io.min() < 0 or io.max() >= shape[0]:
                raise ValueError(f"img_of: {Bn} entries in [0, {shape[0]})")
        elif shape[0] != Bn:
            raise ValueError(f"expected {Bn} images, got {shape[0]}")
        if not signed and (shape[1] % 5 or shape[2] % 5):
            raise ValueError(f"unsigned mode: H and W must be multiples of 5, got {shape[1]} x {shape[2]}")
        if reconstruct is not None:
            if getattr(reconstruct, "dec", None) is None:
                raise ValueError("set_sdf_image(): reconstruct needs a VaeWrapper with a decoder (decoder=...)")
            if reconstruct.ctx is not ctx:
                raise ValueError("set_sdf_image(): the VaeWrapper must be built on the controller's context (ctx=nmpc.ocp.ctx)")
            if reconstruct.B != Bn:
                raise ValueError(f"set_sdf_image(): the VaeWrapper reconstructs {reconstruct.B} images, the batch has {Bn}")
            if img_of is not None:
                raise ValueError("set_sdf_image(): reconstruct excludes img_of (one reconstruction per instance)")
        if on_dev:  # a copy on the device, once the producer has finished
            dimg = _lib.DeviceArray(ctx, shape, np.float32)
            _lib._check(_lib.load().sdfnmpc_memcpy(ctx.h, dimg.data_ptr(), _lib.sync_producer(imgs).data_ptr(), dimg.nbytes, 3))
        else:
            dimg = _lib.DeviceArray.from_numpy(ctx, np.asarray(imgs, dtype=np.float32).reshape(shape))
        keep = {"images": dimg, "img_of": None if io is None else _lib.DeviceArray.from_numpy(ctx, io)}
        sn = self.cfg.sensor
        is_depth = sn.is_depth
        if reconstruct is not None:  # the source holds what the latent retains of the camera image: a range image
            keep.update(camera=dimg, recon=reconstruct,
                        images=reconstruct.reconstruct(dimg, normalized=True, out=_lib.DeviceArray(ctx, shape, np.float32)))
            dimg, is_depth = keep["images"], False
        io_c = _lib.img_opts(sn.dmax, sn.hfov, sn.vfov, is_depth, sn.is_spherical)
        if signed:
            keep.update(self._image_grid())
            o = _lib.img_sdf_opts(io_c, dimg, True, -0.3, md, keep["grid"], keep["dist"], keep["orig_idx"],
                                  img_of=keep["img_of"])
        else:
            keep["pooled"] = _lib.DeviceArray(ctx, (shape[0], shape[1] // 5, shape[2] // 5), np.float32)
            o = _lib.img_sdf_opts(io_c, dimg, False, -0.3, md, pooled=keep["pooled"], img_of=keep["img_of"])
            _lib.img_sdf_pool(ctx, o, shape[0])
        solver.set_sdf_image(o, keep)
        if self._sdf_scene is not None:
            self._sdf_scene._sdf_users.discard(self)
        self._sdf_scene = None
        self._sdf_image = {"opts": o, "shape": shape, "signed": bool(signed), **keep}

    def _image_grid(self):
        """The distance-sorted voxel grid ``DfComputer`` builds (its ``generate_dist_grid``), on the controller's
        device: built once per controller."""
        from . import _lib
        g = getattr(self, "_img_grid", None)
        if g is None:
            from .df_computer import DfComputer
            sn, ctx = self.cfg.sensor, self.ocp.ctx
            grid, dist, orig = DfComputer(True, sn.dmax, sn.hfov, sn.vfov, 1, sn.is_depth, sn.is_spherical, device=ctx)._sorted
            g = self._img_grid = {"grid": _lib.DeviceArray.from_numpy(ctx, grid.numpy(), dtype=np.float32),
                                  "dist": _lib.DeviceArray.from_numpy(ctx, dist.numpy(), dtype=np.float32),
                                  "orig_idx": _lib.DeviceArray.from_numpy(ctx, orig.numpy(), dtype=np.int32)}
        return g

    def set_scene_time(self, t):
        """The time a scene source is seen at by the next ``solve`` (0 at creation)."""
        if not np.isfinite(float(t)):
            raise ValueError(f"scene time {t}: a finite time")
        for part in self.ocp.parts:
            part.solver.set_scene_time(float(t))

    # ---- control iteration
    def set_x0(self, x0):
        """Current state feedback (controller.py:67-71); the first call initialises the OCP iterate."""
        x0 = np.asarray(x0, dtype=float)[..., : self.model.nx]
        if self.x0 is None:
            self.ocp.init(x0)
        self.x0 = x0

    def solve(self):
        """One SQP-RTI iteration for every instance (controller.py:72-81)."""
        try:
            self.ocp.shift(self.cfg.mpc.shift)
            self._flush()  # host-set regions; device-set regions are already in place
            self.ocp.solve(self.x0, None, None, None, None, None)
            self.fail_count = 0
        except Exception as e:  # same contract as the reference: report, count, keep running
            print("solver failed:", e)
            self.fail_count += 1
        # fail_count is batch-wide (any failed instance counts, as one reference solver per instance would
        # for that instance); fail_counts holds the per-instance consecutive failures
        mask = getattr(self.ocp, "fail_mask", None)
        if mask is not None:
            self.fail_counts = np.where(mask, getattr(self, "fail_counts", 0) + 1, 0)
        return self.fail_count

    def rollout(self, steps, refs=None, wps=None, vw=None, weights=None, plant=None, imgs=None, safe_ball_size=0.0,
                outside='col', scene=None, vae=None, perceive_every=1, img_shape=None, keep_img=False,
                perceive_phase=0, scene_t0=0.0, scene_dt=None, sensor=None, vehicle=None, swept=None):
        """``steps`` closed-loop control steps on the device, without a host round trip between them: per
        step the references from the current state (``refs``), the shift (mpc.shift), one SQP-RTI iteration
        and the plant advanced by u_0 -- the loop ``set_x0``; ``gen_refs_device``; ``solve``; simulate,
        enqueued as one launch sequence and waited for once (sdfnmpc_solver_rollout, csrc/plant.hip).

        It starts from the state of the last ``set_x0`` (required).  refs: None keeps the references as they
        are (host setters are flushed once at the start); 'wps' / 'joystick' / 'hover' regenerate them from the
        plant state before every step as ``gen_refs_device(mode, wps, vw, weights)`` does.  plant: a
        ``_lib.plant_opts(...)`` (another model kind, RK4 substeps, a disturbance acceleration, a thrust-gain
        error); default: the controller's own model over ocp.dt[0] with one RK4 step, the perfect-model plant.
        imgs: float32 [B, H, W] range images normalised by sensor.dmax (host or device, as
        ``check_openloop_traj``): every logged plant position is labelled against its instance's image in one
        launch of the collision-check kernel after the loop, in the camera frame of node 0's pose parameters.

        scene: a ``scene.Scene`` on the controller's context -- perception inside the loop.  Before every
        ``perceive_every``-th step (starting with the first) each instance's camera pose is taken from its plant
        state, its scene is rendered from there as a raw sensor image of ``img_shape`` (h, w; default
        sensor.shape_imgs[-2:]), ``vae`` (a ``VaeWrapper`` built with ``ctx=nmpc.ocp.ctx`` and ``batch=B``) encodes
        it and the latent and the body pose go into p as ``set_latent`` writes them (the sdf flag stays): the loop
        ``render_from_state``; ``set_img``; ``encode_to`` a user writes in front of each step, without leaving the
        device (sdfnmpc_solver_rollout_perceive, csrc/scene.hip).  The result gains ``clearance`` [B, K+1], the
        exact signed distance of every logged position to the scene (one launch after the loop), and with
        ``keep_img`` the last rendered images.  ``perceive_phase``: steps already taken since the schedule began
        (an image before step k when (k + phase) % perceive_every == 0), so that a rollout cut into chunks
        perceives where the uncut one does.  ``scene`` excludes ``imgs`` (the image changes inside the loop).
        A scene with moving primitives (``Scene.moving``) has a clock: the image before step k shows it at
        ``scene_t0 + (perceive_phase + k) * scene_dt`` (``scene_dt``: default the plant's control period), the result
        carries ``t`` [K+1], that time for every log row, and ``clearance[b, j]`` is the distance of row j to the
        scene at ``t[j]``.  The controller treats every image as a static world.
        sensor: a ``sensor.SensorModel`` on the controller's context (requires ``scene``) -- every new image is
        degraded as frame ``perceive_phase + k`` before the encoder sees it (noise, lost pixels, erased boxes, outlier
        removal; sdfnmpc_solver_rollout_perceive_sensor): the loop ``render_from_state``; ``sensor.apply(img, frame)``;
        ``set_img``; ``encode_to``.  ``keep_img`` then returns the degraded image the encoder saw; ``clearance`` stays
        the exact distance to the scene -- the clearance kept under a degraded camera.

        With an image source (``set_sdf_image``) ``scene`` needs no ``vae`` (giving one is a ValueError): before every
        ``perceive_every``-th step the scene is rendered from the plant state as a normalised image of the source's
        own shape (``img_shape``, when given, must equal it) into the source's buffer (a source set with ``reconstruct=``:
        into its camera buffer, then encoded and decoded into the source, sdfnmpc_solver_rollout_image_recon -- the loop
        ``render_from_state(normalized=True)``; ``sensor.apply``; ``set_sdf_image(img, reconstruct=vae)``;
        ``set_pose_device``; ``keep_img`` then returns the reconstruction), degraded by ``sensor`` as frame
        ``perceive_phase + k`` (normalised units), min-pooled in the unsigned mode, and the camera pose goes into p
        (sdfnmpc_solver_rollout_image_sdf): the loop ``render_from_state(normalized=True)``; ``sensor.apply``;
        ``set_sdf_image``; ``set_pose_device``.  ``keep_img`` returns the image the source last held; ``clearance``
        and ``t`` are measured against the scene as above.  Without ``scene`` the image and the pose stay as set, and
        ``imgs`` labelling works as without a source.

        vehicle: a ``vehicle.VehicleModel`` on the controller's context with ``batch`` instances -- the plant call of
        every step is the model's (input delay, thrust lag, rotor drag, gusts) on its own true state, at frame
        ``perceive_phase + k``, and the controller is given the model's estimate of that state
        (sdfnmpc_rollout_args.vehicle): the loop ``vehicle.begin``; [``set_x0(estimate)``; ``gen_refs_device``;
        ``solve``; ``vehicle.step``].  The rollout starts from the true state of the last ``set_x0``; ``x``, ``col``,
        ``pts`` and ``clearance`` are the true vehicle's, ``u`` the commands, and the result gains ``xhat`` and
        ``u_applied``.  With ``scene`` the camera sees from the true state while the body pose in p comes from the
        estimate; references (and a scene source's pose refresh) read the estimate.  The model keeps its hidden states
        from call to call (``vehicle.reset()`` starts afresh), so chunks with ``perceive_phase`` carried equal the uncut
        rollout.  Afterwards ``self.x0`` is the true final state.  A model with a ``body`` (``vehicle.RigidBody``) flies a
        rigid body under an attitude and rate loop with lagging, saturating rotors; the result gains ``omega`` and
        ``rotor``, and a plant whose ``dt / substeps`` the inner loop does not admit is refused (ValueError).

        swept: True (eps = 1e-3 m) or a float eps -- the clearance between the log rows, wherever ``clearance`` is
        produced (``scene``, or a scene source; else a ValueError).  One launch after the loop
        (``Scene.swept_distance``, csrc/scene_swept.hip) over the K chords of every instance: entry k of
        ``swept_clearance`` / ``swept_gap`` / ``swept_s`` [B, K] is the minimum distance to the scene along the straight
        segment from ``x[:, k, :3]`` at ``t[k]`` to ``x[:, k+1, :3]`` at ``t[k+1]`` (the true vehicle's rows), with the
        movers moving meanwhile, its certificate and where on the chord it lies.  The segment is the chord between the
        rows: the plant's path leaves it by at most a dt^2 / 8 for an acceleration a, about 1.4 cm at 20 m/s^2 and 75 ms.
        None: nothing is computed and the three attributes are None.

        Returns a ``Rollout`` of numpy arrays, batch-leading also for one instance: x [B, K+1, 10] (row 0 the
        start), u [B, K, 4], status / iters [B, K]; with imgs also col [B, K+1] bool and pts [B, K+1, 3] float32.
        Afterwards ``self.x0`` is the final plant state and ``ocp.u`` / ``ocp.status`` / ``ocp.iters`` are the last
        step's.  An instance whose QP fails (status >= 2) keeps its iterate and is advanced with the u_0 the
        failed step leaves, its unchanged u[:, 0] (``Ocp.solve`` substitutes the previous call's u instead)."""
        from . import _lib
        from .reference import Ref
        if self.x0 is None:
            raise ValueError("set_x0 before rollout (the loop starts at the current state)")
        if len(self.ocp.parts) != 1:
            raise ValueError("rollout(): the batch is split over several devices; sharded rollouts are not built")
        if refs not in (None, "wps", "joystick", "hover"):
            raise ValueError(f"refs {refs!r}: None, 'wps', 'joystick' or 'hover'")
        assert outside in _lib.OUTSIDE
        K, Bn, ctx, solver = int(steps), max(self.B, 1), self.ocp.ctx, self.ocp.parts[0].solver
        if K < 1:
            raise ValueError(f"rollout of {K} steps: at least one")
        if vehicle is not None:
            if vehicle.ctx is not ctx:
                raise ValueError("rollout(): the VehicleModel must be built on the controller's context (ctx=nmpc.ocp.ctx)")
            if vehicle.B != Bn:
                raise ValueError(f"rollout(): the VehicleModel has {vehicle.B} instances, the batch has {Bn}")
            if int(perceive_phase) < 0:
                raise ValueError(f"perceive_phase {perceive_phase}: the vehicle's first frame, at least 0")
        # every refusal before anything is uploaded or enqueued: what the SDF source admits, then what perception needs
        src = self._sdf_scene
        isrc = self._sdf_image if src is None else None
        if src is not None:  # a scene source: the exact distance, no perception
            if scene is not None or vae is not None or sensor is not None:
                raise ValueError("rollout(): scene, vae and sensor exclude a scene source (set_sdf_scene): the "
                                 "controller reads the scene's exact distance, not an image")
        elif isrc is not None:  # an image source: re-imaged from ``scene`` inside the loop, no encoder
            if vae is not None:
                raise ValueError("rollout(): vae excludes an image source (set_sdf_image): the controller reads the "
                                 "image's own distance field, not a latent")
            if img_shape is not None and tuple(int(v) for v in img_shape) != isrc["shape"][1:]:
                raise ValueError(f"rollout(): img_shape {tuple(img_shape)} is not the image source's {isrc['shape'][1:]}")
            if scene is None and sensor is not None:
                raise ValueError("rollout(): sensor degrades a scene's images; give scene too")
        elif scene is None:
            if vae is not None:
                raise ValueError("rollout(): vae is the encoder of a scene's images; give scene too")
            if sensor is not None:
                raise ValueError("rollout(): sensor degrades a scene's images; give scene (and vae) too")
        elif vae is None:
            raise ValueError("rollout(): scene needs vae (a VaeWrapper on the controller's context)")
        if scene is not None:  # perception inside the loop, into the latent (vae) or into the image source
            if imgs is not None:
                raise ValueError("rollout(): scene and imgs exclude each other (the image changes inside the loop)")
            if vae is not None:
                if vae.ctx is not ctx or scene.ctx is not ctx:
                    raise ValueError("rollout(): the scene and the VaeWrapper must be built on the controller's context "
                                     "(ctx=nmpc.ocp.ctx)")
                if vae.B != Bn:
                    raise ValueError(f"rollout(): the VaeWrapper encodes {vae.B} images, the batch has {Bn}")
            else:
                if scene.ctx is not ctx:
                    raise ValueError("rollout(): the scene must be built on the controller's context (ctx=nmpc.ocp.ctx)")
                if isrc["img_of"] is not None:
                    raise ValueError("rollout(): re-imaging renders one image per instance; the source maps instances to "
                                     "images (img_of)")
        if scene is not None or src is not None:
            _check_schedule(perceive_every, perceive_phase, scene_t0, scene_dt)
        swept_eps = None
        if swept is not None and swept is not False:
            if scene is None and src is None:
                raise ValueError("rollout(): swept measures the clearance to a scene; give scene, or set a scene source "
                                 "(set_sdf_scene)")
            swept_eps = 1e-3 if swept is True else float(swept)
            if not (np.isfinite(swept_eps) and swept_eps >= 1e-6):
                raise ValueError(f"rollout(): swept {swept!r}: True, or an eps of at least 1e-6 m")
        if scene is not None:
            scene._batch(Bn)
            if sensor is not None and sensor.ctx is not ctx:
                raise ValueError("rollout(): the SensorModel must be built on the controller's context (ctx=nmpc.ocp.ctx)")
        kw = {}
        if refs is not None:
            code = {"wps": 0, "joystick": 1, "hover": 2}[refs]
            wrow = self.model.weight_row(weights if weights is not None else Ref(self.cfg).W_on)
            if code == 1:
                wrow[:3] = 0.0  # ref.Wp = [0, 0, 0] (ref_gen.py:122)
            kw = {"ref": _lib.ref_opts(self.cfg, code), "wrow": self._dev(wrow)}
            if code == 0:
                if isinstance(wps, (list, tuple)) and len(wps) and hasattr(wps[0], "p"):
                    wps = (np.array([w.p for w in wps])[None], np.array([w.q for w in wps])[None])
                wp_p = np.reshape(np.asarray(wps[0], float), (Bn, -1, 3))
                kw.update(wp_p=self._dev(wp_p), wp_q=self._dev(np.reshape(np.asarray(wps[1], float), (Bn, -1, 4))),
                          n_wp=wp_p.shape[1])
            elif code == 1:
                kw["vw"] = self._dev(np.reshape(np.asarray(vw, float), (Bn, 4)))
        if plant is None:
            plant = _lib.plant_opts(self.cfg, dt=float(self.ocp.dt[0]))
        if vehicle is not None:
            vehicle.check_plant(plant)  # a rigid body's step size, before anything is enqueued
        t0, dts = float(scene_t0), float(plant.dt if scene_dt is None else scene_dt)  # step k is at t0 + (phase + k) dts
        perc = rv = sn = None
        if scene is not None:  # pose, render, sensor, then into the latent, or (normalised) into the image source
            ws = _pose_workspaces(ctx, Bn)
            if isrc is None:  # a raw sensor image for ``vae``
                shape = tuple(int(v) for v in (img_shape if img_shape is not None else self.cfg.sensor.shape_imgs[-2:]))
                ws["images"] = _lib.DeviceArray(ctx, (Bn,) + shape, np.float32)
                enc = (vae, float(vae.opts.clip), ws["images"])
            else:  # into the source itself; with ``reconstruct=`` into its camera buffer, encoded, and decoded into it
                shape, rv = isrc["shape"][1:], isrc.get("recon")
                enc = None if rv is None else (rv, 1.0, isrc["camera"])
            perc = _perceive_args(self.cfg, scene, Bn, shape, isrc is not None, perceive_every, perceive_phase, ws, enc)
            if sensor is not None:  # in the units of the image the renderer writes
                sn = sensor.opts(Bn, *shape, normalized=isrc is not None)
        dimg = None
        if imgs is not None:
            dimg, ishape = self._dev_imgs(imgs)
        if refs is not None:  # the references are regenerated on the device before every step: as after
            self._clean("q_d", "yref", "W", "yNref", "WN")  # gen_refs_device, host-set references are dropped
        self._flush()  # the other host-set regions, once
        self.ocp.upload("x0", np.reshape(np.asarray(self.x0, dtype=np.float64), (Bn, 1, 10)))
        log = {"x_log": _lib.DeviceArray(ctx, (Bn, K + 1, 10)), "u_log": _lib.DeviceArray(ctx, (Bn, max(K, 1), 4)),
               "status_log": _lib.DeviceArray(ctx, (Bn, max(K, 1)), np.int32),
               "iters_log": _lib.DeviceArray(ctx, (Bn, max(K, 1)), np.int32)}
        if dimg is not None:
            log["pts_log"] = _lib.DeviceArray(ctx, (Bn, K + 1, 3), np.float32)
        if vehicle is not None:  # x0 holds the truth: the model takes it and leaves its estimate there
            vehicle.begin(solver.field("x0"), int(perceive_phase))
            vlog = (_lib.DeviceArray(ctx, (Bn, K + 1, 10)), _lib.DeviceArray(ctx, (Bn, max(K, 1), 4)))
            if vehicle.body is not None:
                vlog += (_lib.DeviceArray(ctx, (Bn, K + 1, 3)), _lib.DeviceArray(ctx, (Bn, K + 1, 4)))
            kw["vehicle"] = (vehicle.h, int(perceive_phase)) + vlog
        if src is not None:  # the pose the FOV rows read is refreshed from the plant state, the scene's clock per step
            ws = _pose_workspaces(ctx, Bn)
            pose = _lib.PoseRefreshArgsC(int(perceive_every), *_extrinsics(self.cfg), *[ws[k].data_ptr() for k in POSE_WS])
            solver.rollout_scene_sdf(K, plant, pose=pose, phase=int(perceive_phase), t0=t0, dt=dts,
                                     shift=int(self.cfg.mpc.shift), **kw, **log)
            self._clean("pose")  # written on the device, as after set_pose_device
        elif isrc is not None:
            clock = (t0, dts) if perc is not None else (0.0, 0.0)
            solver.rollout_image_sdf(K, plant, perceive=perc, t0=clock[0], dt=clock[1], sensor=sn,
                                     dec=None if rv is None else rv.dec, shift=int(self.cfg.mpc.shift), **kw, **log)
            if perc is not None:
                self._clean("pose")
        else:  # a static scene has no use for the clock: the call the method has always made
            solver.rollout(K, plant, perceive=perc, sensor=sn, shift=int(self.cfg.mpc.shift),
                           scene_clock=(t0, dts) if perc is not None and scene.is_dynamic else None, **kw, **log)
        u0 = solver.wait().copy()
        out = Rollout(log["x_log"].numpy(), log["u_log"].numpy(), log["status_log"].numpy(), log["iters_log"].numpy())
        if vehicle is not None:
            out.xhat, out.u_applied = vlog[0].numpy(), vlog[1].numpy()
            if vehicle.body is not None:
                out.omega, out.rotor = vlog[2].numpy(), vlog[3].numpy()
        if dimg is not None:
            s = self.cfg.sensor
            pts = _lib.FieldView(log["pts_log"].data_ptr(), (Bn * (K + 1), 3), np.float32, ctx)
            lab = _lib.DeviceArray(ctx, (Bn * (K + 1),), np.uint8)
            _lib.colcheck(ctx, _lib.img_opts(s.dmax, s.hfov, s.vfov, s.is_depth, s.is_spherical), _lib.OUTSIDE[outside],
                          safe_ball_size, _lib.FieldView(dimg.data_ptr(), ishape, np.float32, ctx), pts, None, lab)
            out.col = lab.numpy().astype(bool).reshape(Bn, K + 1)  # point j belongs to image j / (K + 1)
            out.pts = log["pts_log"].numpy()
        if perc is not None or src is not None:  # against the rendered scene, or the source scene
            _log_clearance(out, scene if perc is not None else src, t0 + (int(perceive_phase) + np.arange(K + 1)) * dts)
            if swept_eps is not None:
                _log_swept(out, scene if perc is not None else src, swept_eps)
            if perc is not None and keep_img and isrc is None:
                out.img = ws["images"].numpy()
        if isrc is not None and keep_img:  # the (normalised) image the source last held
            out.img = isrc["images"].numpy()
        self.x0 = out.x[:, -1].copy() if self.B > 1 else out.x[0, -1].copy()
        ocp = self.ocp
        ocp.status, ocp.iters = solver.status.copy(), solver.iters.copy()
        ocp.fail_mask = ocp.status >= 2
        ocp.u = u0[0] if self.B == 1 else u0
        return out

    def _dev_imgs(self, imgs):
        """Range images [B, H, W] (or [H, W]) float32 on the device, and their 3-d shape."""
        from . import _lib
        Bn = max(self.B, 1)
        if hasattr(imgs, "data_ptr"):
            if np.dtype(str(imgs.dtype).replace("torch.", "")) != np.float32:
                raise TypeError(f"device images must be float32, got {imgs.dtype}")
            dimg = _lib.sync_producer(imgs)
            shape = tuple(int(v) for v in imgs.shape)
        else:
            a = np.asarray(imgs, dtype=np.float32)
            shape = a.shape
            dimg = _lib.DeviceArray.from_numpy(self.ocp.ctx, a)
        if len(shape) == 2:
            shape = (1,) + shape
        if len(shape) != 3:
            raise AssertionError('input image must have size [B, H, W] or [H, W]')
        if shape[0] != Bn:
            raise ValueError(f"expected {Bn} images, got {shape[0]}")
        return dimg, shape

    # ---- getters
    def get_matrices(self):
        """x [.., N+1, nx], u [.., N, nu] of the current iterate (controller.py:87-96)."""
        x = self.ocp.download("x")
        u = self.ocp.download("u")
        return (x[0], u[0]) if self.B == 1 else (x, u)

    def get_u(self):
        """Last computed MPC inputs (controller.py:99-101)."""
        return self.ocp.get_u()

    def get_cmd_acc(self):
        """controller.py:104-106."""
        return np.clip(self.model.u_to_acc(self.x0, self.get_u()), self.cmd_acc_min, self.cmd_acc_max)

    def get_cmd_TRPYr(self):
        """controller.py:109-111."""
        return np.clip(self.model.u_to_TRPYr(self.x0, self.get_u()), self.cmd_TRPYr_min, self.cmd_TRPYr_max)

    def get_openloop_traj(self):
        """Predicted (position, quaternion) path, node 0 = x0 (controller.py:119-125); batched: per instance."""
        x, _ = self.get_matrices()
        x = x if self.B > 1 else x[None]
        x0 = self.x0 if self.B > 1 else self.x0[None]
        paths = []
        for b in range(x.shape[0]):
            path = [(x0[b][[0, 1, 2]], x0[b][[3, 4, 5, 6]])]
            for k in range(1, self.N + 1):
                path.append((x[b, k][[0, 1, 2]], x[b, k][[3, 4, 5, 6]]))
            paths.append(path)
        return paths[0] if self.B == 1 else paths

    def eval(self, k):
        """The model's evaluation vector at node k (controller.py:125-130, base_model.py:119-125): [0] without
        flags.enable_sdf; else the SDF value with flag = 1 (gen_model.py:64, computed by the HIP SDF kernel),
        and with recursive_feasibility the braking distance poly(v) and sdf - poly(v), flag = 1
        (gen_model.py:116-117)."""
        m = self.model
        if not m.enable_sdf:
            return [0] if self.B == 1 else np.zeros((self.B, 1))
        from .model import poly_eval
        idx = self.cfg.mpc.p_idx
        x = self.ocp.download("x")[:, k]
        p = self.p if self.B > 1 else self.p[None]
        pk = p[:, k]
        W_R_Co = pk[:, idx.W_R_Co].reshape(-1, 3, 3)
        Co_p_B = np.einsum("bji,bj->bi", W_R_Co, x[:, :3] - pk[:, idx.W_p_Co])
        df, _ = self.ocp.net.eval_host(np.concatenate([Co_p_B, pk[:, idx.latent:]], axis=1), want_grad=False)
        out = df[:, None]
        if m.rec_feas:
            bd, _ = poly_eval(m.poly, m.poly_deg, x[:, 7:10])
            out = np.concatenate([out, bd[:, None], (df - bd)[:, None]], axis=1)
        return out[0] if self.B == 1 else out

    def check_openloop_traj(self, imgs, safe_ball_size=0.0, outside='col'):
        """Collision labels of the predicted positions against the raw images the latents came from: the runtime
        monitor behind mpc.allow_dead_reck ("if current position is unsafe"), one launch of the collision-check
        kernel (csrc/df_truth.hip, the reference's utils/collision_checker.py) for the B x (N+1) nodes.

        imgs: [B, H, W] (or [H, W] for one instance) float32, normalised by sensor.dmax: a host array, or a
        device array used in place (DeviceArray or torch tensor, e.g. the images already there for the VAE in
        config C5).  Node k of instance b is checked in the camera frame ``eval`` uses, Co_p = W_R_Co^T (x_k[:3]
        - W_p_Co) with node k's parameters as the host setters left them (set_latent), against image b.
        outside: what holds beyond the field of view ('col', 'free' or 'extrapolate').
        Returns a numpy bool array [N+1], or [B, N+1] for a batch.  No tensor library is needed."""
        from . import _lib
        assert outside in _lib.OUTSIDE
        s, idx, ctx = self.cfg.sensor, self.cfg.mpc.p_idx, self.ocp.ctx
        Bn = max(self.B, 1)
        dimg, shape = self._dev_imgs(imgs)
        x = self.ocp.download("x")
        p = self.p if self.B > 1 else self.p[None]
        W_R_Co = p[..., idx.W_R_Co].reshape(Bn, self.N + 1, 3, 3)
        Co_p = np.einsum("bkji,bkj->bki", W_R_Co, x[..., :3] - p[..., idx.W_p_Co])
        pts = _lib.DeviceArray.from_numpy(ctx, Co_p.reshape(-1, 3), dtype=np.float32)
        out = _lib.DeviceArray(ctx, (pts.shape[0],), np.uint8)
        _lib.colcheck(ctx, _lib.img_opts(s.dmax, s.hfov, s.vfov, s.is_depth, s.is_spherical), _lib.OUTSIDE[outside],
                      safe_ball_size, _lib.FieldView(dimg.data_ptr(), shape, np.float32, ctx), pts, None, out)
        lab = out.numpy().astype(bool)  # the copy waits for the launch; point j belongs to image j / (N+1)
        return lab if self.B == 1 else lab.reshape(self.B, self.N + 1)

    # ---- device-side parameter packing (csrc/ref_pack.hip)
    def _dev(self, a):
        """Host array -> device (fp64); a device array (DeviceArray / FieldView / torch tensor) passes through."""
        from . import _lib
        if hasattr(a, "data_ptr"):
            if np.dtype(str(a.dtype).replace("torch.", "")) != np.float64:
                raise TypeError(f"device input must be float64, got {a.dtype}")
            return _lib.sync_producer(a)  # a torch tensor may still be in flight on torch's stream
        return _lib.DeviceArray.from_numpy(self.ocp.ctx, np.asarray(a, dtype=np.float64))

    def gen_refs_device(self, mode="wps", wps=None, vw=None, weights=None):
        """RefGen + formate_ref + set_ref for every instance and node in one kernel launch, written straight
        into the solver's device buffers (p[:, :, q_d], y, W, yN, WN).

        mode 'wps': ``RefGen.gen_ref_list_wps`` (ref_gen.py:25-99) from x0 (``set_x0``) through the
        waypoints ``wps = (p [B][n][3], q [B][n][4])`` (or a list of ``Waypoint`` for B = 1); 'joystick':
        ``gen_ref_joystick(vw)`` (ref_gen.py:101-130), vw [B][4]; 'hover': ``from_x0`` (ref_gen.py:17-23).
        ``weights`` is the weight set formate_ref reads (e.g. ``Ref(cfg).W_on``); the joystick mode zeroes
        its position weights as gen_ref_joystick does.  The host arrays of these regions are not updated;
        a later host setter of a region (e.g. set_ref at one node) overrides it at the next ``solve``.
        """
        from . import _lib
        from .reference import Ref
        if self.x0 is None:
            raise ValueError("set_x0 before gen_refs_device (the references start at the current state)")
        Bn = max(self.B, 1)
        ws = weights if weights is not None else Ref(self.cfg).W_on
        wrow = self.model.weight_row(ws)
        code = {"wps": 0, "joystick": 1, "hover": 2}[mode]
        if code == 1:
            wrow[:3] = 0.0  # ref.Wp = [0, 0, 0] (ref_gen.py:122)
        args = {"x0": self._dev(np.reshape(self.x0, (Bn, -1))), "wrow": self._dev(wrow)}
        n_wp = 0
        if code == 0:
            if isinstance(wps, (list, tuple)) and len(wps) and hasattr(wps[0], "p"):
                wps = (np.array([w.p for w in wps])[None], np.array([w.q for w in wps])[None])
            wp_p = np.reshape(np.asarray(wps[0], float), (Bn, -1, 3))
            wp_q = np.reshape(np.asarray(wps[1], float), (Bn, -1, 4))
            n_wp = wp_p.shape[1]
            args.update(wp_p=self._dev(wp_p), wp_q=self._dev(wp_q))
        elif code == 1:
            args["vw"] = self._dev(np.reshape(np.asarray(vw, float), (Bn, 4)))
        for k in ("p", "yref", "W", "yNref", "WN"):
            args[k] = self.ocp.field(k)
        _lib.pack_refs(self.ocp.ctx, _lib.ref_opts(self.cfg, code), Bn, self.N, self.model.np, self.model.ny, args,
                       n_wp=n_wp, nyN=self.model.nyN)
        self.ocp.ctx.synchronize()  # the temporary inputs are freed on return
        self._clean("q_d", "yref", "W", "yNref", "WN")

    def set_latent_device(self, latent, W_p_Bo, W_R_Bo, flag=None):
        """set_latent (+ set_sdf_flag) on the device buffers for every instance (controller.py:45-54);
        latent: host array or a device array [B][L] fp64 (e.g. VaeWrapper's latents, no host round trip).
        With the batch split over devices (Ocp(devices=...), shard.plan) each part packs its own instance
        rows on its own device: a device array on that device is read in place (a view at the part's first
        row), one on another device goes through the host once."""
        from . import _lib
        Bn = max(self.B, 1)
        L = int(self.cfg.nn.size_latent)
        cols = {"latent": L, "W_p_Bo": 3, "W_R_Bo": 9, "flag": 1}
        given = {"latent": latent, "W_p_Bo": W_p_Bo, "W_R_Bo": W_R_Bo}
        if flag is not None:
            given["flag"] = flag if hasattr(flag, "data_ptr") else np.broadcast_to(np.asarray(flag, float), (Bn,))
        host = {}
        for k, v in given.items():
            if not hasattr(v, "data_ptr"):
                host[k] = np.reshape(np.asarray(v, dtype=np.float64), (Bn, cols[k]))
            elif np.dtype(str(v.dtype).replace("torch.", "")) != np.float64:
                raise TypeError(f"device input must be float64, got {v.dtype}")
        parts = self.ocp.parts
        synced = set()
        for part in parts:
            lo, nb = part.lo, part.hi - part.lo
            args = {"p": part.solver.field("p")}
            for k, v in given.items():
                if k in host:
                    args[k] = _lib.DeviceArray.from_numpy(part.ctx, np.ascontiguousarray(host[k][lo:part.hi]))
                elif len(parts) == 1:
                    args[k] = _producer_done(v, part.ctx, synced)
                elif _device_of(v) == part.ctx.device:  # a view of the part's rows, in place
                    v = given[k] = _producer_done(v, part.ctx, synced)
                    args[k] = _lib.FieldView(v.data_ptr() + lo * cols[k] * 8, (nb, cols[k]), np.float64, part.ctx)
                else:  # another device: through the host, once per array
                    host[k] = _download(v, Bn, cols[k])
                    args[k] = _lib.DeviceArray.from_numpy(part.ctx, np.ascontiguousarray(host[k][lo:part.hi]))
            _lib.pack_refs(part.ctx, _lib.ref_opts(self.cfg, -1), nb, self.N, self.model.np, self.model.ny, args, L=L,
                           nyN=self.model.nyN)
        for part in parts:
            part.ctx.synchronize()
        self._clean("pose", "latent", *(("flag",) if flag is not None else ()))

    def set_pose_device(self, W_p_Bo, W_R_Bo):
        """``set_latent_device`` without the latent: the camera pose in p (the columns the field-of-view rows read) of
        every node from the body pose W_p_Bo [B][3], W_R_Bo [B][9] (host or device fp64 arrays), on the device
        buffers; the flag and the latent stay.  What a loop without an encoder (``set_sdf_scene``) refreshes."""
        from . import _lib
        Bn = max(self.B, 1)
        cols = {"W_p_Bo": 3, "W_R_Bo": 9}
        given = {"W_p_Bo": W_p_Bo, "W_R_Bo": W_R_Bo}
        host = {}
        for k, v in given.items():
            if not hasattr(v, "data_ptr"):
                host[k] = np.reshape(np.asarray(v, dtype=np.float64), (Bn, cols[k]))
            elif np.dtype(str(v.dtype).replace("torch.", "")) != np.float64:
                raise TypeError(f"device input must be float64, got {v.dtype}")
        parts = self.ocp.parts
        synced = set()
        for part in parts:
            lo, nb = part.lo, part.hi - part.lo
            args = {"p": part.solver.field("p")}
            for k, v in given.items():
                if k not in host and len(parts) > 1 and _device_of(v) != part.ctx.device:
                    host[k] = _download(v, Bn, cols[k])  # another device: through the host, once per array
                if k in host:
                    args[k] = _lib.DeviceArray.from_numpy(part.ctx, np.ascontiguousarray(host[k][lo:part.hi]))
                else:
                    v = given[k] = _producer_done(v, part.ctx, synced)
                    args[k] = v if len(parts) == 1 else _lib.FieldView(v.data_ptr() + lo * cols[k] * 8, (nb, cols[k]),
                                                                       np.float64, part.ctx)
            _lib.pack_refs(part.ctx, _lib.ref_opts(self.cfg, -2), nb, self.N, self.model.np, self.model.ny, args,
                           nyN=self.model.nyN)
        for part in parts:
            part.ctx.synchronize()
        self._clean("pose")

    def set_ref(self, ref, k, b=None):
        """y, W and q_d of node k from a reference object (controller.py:136-142); b selects one instance
        of a batch (None: all)."""
        sel = () if self.B == 1 else (slice(None),) if b is None else (b,)
        self.p[sel + (k, self.cfg.mpc.p_idx.q_d)] = ref.q
        self._mark("q_d", b, k)
        y, W = self.model.formate_ref(ref)
        if k < self.N:
            self.y[sel + (k,)] = y
            self.W[sel + (k,)] = W
            self._mark("yref", b, k)
            self._mark("W", b, k)
        else:
            self.WN[sel] = W[: self.model.nyN]
            self.yN[sel] = y[: self.model.nyN]
            self._mark("yNref", b)
            self._mark("WN", b)


POSE_WS = ("W_p_Bo", "W_R_Bo", "W_p_C", "W_R_C")  # the pose workspaces of a rollout, [B][3] / [B][9]


def _check_schedule(perceive_every, perceive_phase, scene_t0, scene_dt):
    """The perception / pose-refresh schedule and the scene clock of ``rollout``: ValueError before anything is enqueued."""
    if int(perceive_every) < 1 or int(perceive_phase) < 0:
        raise ValueError(f"perceive_every {perceive_every} / perceive_phase {perceive_phase}: at least 1 / 0")
    if not np.isfinite(float(scene_t0)):
        raise ValueError(f"scene_t0 {scene_t0}: a finite time")
    if scene_dt is not None and not (np.isfinite(float(scene_dt)) and float(scene_dt) >= 0.0):
        raise ValueError(f"scene_dt {scene_dt}: finite and not negative")


def _pose_workspaces(ctx, Bn):
    from . import _lib
    return {k: _lib.DeviceArray(ctx, (Bn, 3 if "_p_" in k else 9)) for k in POSE_WS}


def _perceive_args(cfg, scene, Bn, shape, normalized, every, phase, ws, enc=None):
    """The sdfnmpc_perceive_args of ``rollout``: ``scene`` rendered as ``shape`` images (normalized: in units of
    sensor.dmax, else raw) on the schedule, the pose into ``ws``.  enc: (VaeWrapper, clip, camera buffer) -- the image
    goes into that buffer and through the wrapper's encoder; None: no encoder (the solver's image source is rendered
    into).  The result keeps ``ws`` alive."""
    from . import _lib
    stage = (None, _lib.VaeOptsC(), None, None, None)
    if enc is not None:
        v, clip, cam = enc
        vo = _lib.VaeOptsC(Bn, *shape, 0, clip, _lib._ptr(v.yz) if v.depth2range else None)
        stage = (v.vae.h, vo, cam.data_ptr(), v.latent.data_ptr(), v.latent64.data_ptr())
    perc = _lib.PerceiveArgsC(scene.h, _lib._ptr(scene._scene_of), scene.img_opts(cfg), *shape,
                              scene.scale(cfg, normalized=normalized), *_extrinsics(cfg), *stage[:2], int(every),
                              int(phase), *stage[2:], *[ws[k].data_ptr() for k in POSE_WS])
    perc._keep = ws
    return perc


def _extrinsics(cfg):
    """sensor.B_p_C, sensor.B_R_C (row-major) as the C structures take them"""
    from . import _lib
    s = cfg.sensor
    return ((_lib.C.c_double * 3)(*[float(v) for v in np.asarray(s.B_p_C, float).ravel()]),
            (_lib.C.c_double * 9)(*[float(v) for v in np.asarray(s.B_R_C, float).ravel()]))


def _log_clearance(out, scene, t):
    """``Rollout.t`` and ``Rollout.clearance``: one distance launch over the logged positions (point j belongs to
    instance j // (K + 1)), row j of a dynamic set against the scene at t[j]."""
    Bn, K1 = out.x.shape[:2]
    p2s = None if scene.S == 1 else np.repeat(scene.scene_of if scene.scene_of is not None else np.zeros(Bn, np.int32), K1)
    rows = np.ascontiguousarray(out.x[:, :, :3]).reshape(-1, 3)
    out.t = t
    if scene.is_dynamic:
        out.clearance = scene.distance(rows, p2s, t=np.tile(t, Bn)).reshape(Bn, K1)
    else:
        out.clearance = scene.distance(rows, p2s).reshape(Bn, K1)


def _log_swept(out, scene, eps):
    """``Rollout.swept_clearance``, ``swept_gap`` and ``swept_s``: one swept launch over the chords between the logged
    positions (segment j belongs to instance j // K), row k -> k + 1 between out.t[k] and out.t[k + 1]."""
    Bn, K = out.x.shape[0], out.x.shape[1] - 1
    p2s = None if scene.S == 1 else np.repeat(scene.scene_of if scene.scene_of is not None else np.zeros(Bn, np.int32), K)
    p0 = np.ascontiguousarray(out.x[:, :-1, :3]).reshape(-1, 3)
    p1 = np.ascontiguousarray(out.x[:, 1:, :3]).reshape(-1, 3)
    r = scene.swept_distance(p0, p1, p2s, t0=np.tile(out.t[:-1], Bn), t1=np.tile(out.t[1:], Bn), eps=eps)
    out.swept_clearance, out.swept_gap, out.swept_s = (a.reshape(Bn, K) for a in (r.dmin, r.gap, r.s))


def _producer_done(a, ctx, synced: set):
    """A device array about to be read in place by a kernel on ``ctx``'s stream, once everything that
    produces it has finished: a torch tensor waits for torch's current stream (made contiguous first: the
    in-place views assume row-major [B][cols]); an array owned by another context (a DeviceArray or solver
    FieldView, e.g. VaeWrapper.latent64 written by the encoder's stream) waits for that context's stream.
    Each array is synchronised once per call (``synced``)."""
    from . import _lib
    if type(a).__module__.split(".")[0] == "torch":
        if not a.is_contiguous():
            a = a.contiguous()
        return _lib.sync_producer(a)
    owner = getattr(a, "ctx", None)
    if owner is not None and owner is not ctx and id(a) not in synced:
        owner.synchronize()
        synced.add(id(a))
    return a


def _device_of(a) -> int:
    """HIP device of a device array: DeviceArray / FieldView (its context's), torch tensor (its own)."""
    ctx = getattr(a, "ctx", None)
    if ctx is not None:
        return int(ctx.device)
    if type(a).__module__.split(".")[0] == "torch":
        return int(a.device.index or 0)
    raise TypeError(f"device of {type(a).__name__} unknown (expected a DeviceArray, FieldView or torch tensor)")


def _download(a, rows, cols):
    """Host copy [rows][cols] fp64 of a device array (DeviceArray or torch tensor)."""
    if hasattr(a, "numpy") and not type(a).__module__.startswith("torch"):
        return np.reshape(a.numpy(), (rows, cols))
    return np.reshape(a.detach().cpu().numpy(), (rows, cols))
