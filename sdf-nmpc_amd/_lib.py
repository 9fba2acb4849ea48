"""ctypes binding of libsdfnmpc.so (include/sdfnmpc.h).

This is the only way Python reaches the hot path: every compute call goes through the C ABI into
the HIP kernels.  There is deliberately no CPU fallback -- if the library is missing, or no gfx950
device is visible, construction raises.

Device buffers are plain device pointers (ints).  Callers normally pass torch CUDA(HIP) tensors,
which are used for allocation and streams only (``tensor.data_ptr()``).
"""
from __future__ import annotations

import ctypes as C
import os

import numpy as np

PKG_DIR = os.path.dirname(os.path.abspath(__file__))
LIB_DIR = os.path.join(PKG_DIR, "lib")
# SDFNMPC_LIB: a diagnostic build of the same library (tools/build_variant.sh, tools/exp/*.sh)
LIB_PATH = os.environ.get("SDFNMPC_LIB") or os.path.join(LIB_DIR, "libsdfnmpc.so")
L4C_PATH = os.path.join(LIB_DIR, "libsdf_l4c.so")

# exported symbols declared in include/sdfnmpc.h (checked by tests/test_abi.py)
SYMBOLS = [
    "sdfnmpc_abi_version", "sdfnmpc_last_error", "sdfnmpc_ctx_create", "sdfnmpc_ctx_destroy",
    "sdfnmpc_ctx_set_stream", "sdfnmpc_ctx_use_null_stream", "sdfnmpc_ctx_stream", "sdfnmpc_ctx_synchronize", "sdfnmpc_ctx_set_tile_rows",
    "sdfnmpc_ctx_set_qp_kernel", "sdfnmpc_ctx_set_sdf_server", "sdfnmpc_ctx_sdf_server_stats", "sdfnmpc_ctx_qp_kernel", "sdfnmpc_ctx_qp_kernel_for", "sdfnmpc_qp_seg_count", "sdfnmpc_qp_lds_bytes", "sdfnmpc_qp_capacity", "sdfnmpc_qp_capacity_for",
    "sdfnmpc_ctx_enable_timing", "sdfnmpc_ctx_kernel_stats", "sdfnmpc_ctx_reset_stats", "sdfnmpc_net_load",
    "sdfnmpc_net_load_file", "sdfnmpc_net_siren", "sdfnmpc_net_free", "sdfnmpc_net_max_df",
    "sdfnmpc_net_size_latent", "sdfnmpc_net_fingerprint", "sdfnmpc_sdf_eval", "sdfnmpc_sdf_eval_host",
    "sdfnmpc_linearize", "sdfnmpc_shooting_grid", "sdfnmpc_qp_solve", "sdfnmpc_rti_prepare", "sdfnmpc_qp_feedback",
    "sdfnmpc_rti_apply", "sdfnmpc_step_create", "sdfnmpc_step_launch", "sdfnmpc_step_destroy", "sdfnmpc_pack_refs",
    "sdfnmpc_vae_load", "sdfnmpc_vae_free", "sdfnmpc_vae_size_latent", "sdfnmpc_vae_encode",
    "sdfnmpc_vae_dec_load", "sdfnmpc_vae_dec_free", "sdfnmpc_vae_dec_size_latent", "sdfnmpc_vae_decode",
    "sdfnmpc_colcheck", "sdfnmpc_udf", "sdfnmpc_sdf_truth",
    "sdfnmpc_ctx_device", "sdfnmpc_dev_alloc", "sdfnmpc_dev_free", "sdfnmpc_memcpy",
    "sdfnmpc_solver_create", "sdfnmpc_solver_destroy", "sdfnmpc_solver_field", "sdfnmpc_solver_upload",
    "sdfnmpc_solver_download", "sdfnmpc_solver_init", "sdfnmpc_solver_shift", "sdfnmpc_solver_step",
    "sdfnmpc_solver_wait", "sdfnmpc_plant_step", "sdfnmpc_solver_rollout",
    "sdfnmpc_scene_create", "sdfnmpc_scene_free", "sdfnmpc_scene_render", "sdfnmpc_scene_pose",
    "sdfnmpc_scene_distance", "sdfnmpc_solver_rollout_perceive",
    "sdfnmpc_scene_create_moving", "sdfnmpc_scene_is_dynamic", "sdfnmpc_scene_render_at", "sdfnmpc_scene_distance_at",
    "sdfnmpc_solver_rollout_perceive_at",
    "sdfnmpc_morph", "sdfnmpc_outlier_rm", "sdfnmpc_sensor_apply", "sdfnmpc_solver_rollout_perceive_sensor",
    "sdfnmpc_scene_sdf_rows", "sdfnmpc_solver_set_sdf_scene", "sdfnmpc_solver_set_scene_time",
    "sdfnmpc_solver_rollout_scene_sdf",
    "sdfnmpc_img_sdf_rows", "sdfnmpc_img_sdf_pool", "sdfnmpc_solver_set_sdf_image", "sdfnmpc_solver_rollout_image_sdf",
    "sdfnmpc_solver_rollout_image_recon",
    "sdfnmpc_scene_create_large", "sdfnmpc_scene_is_indexed", "sdfnmpc_scene_create_mixed",
    "sdfnmpc_vehicle_create", "sdfnmpc_vehicle_destroy", "sdfnmpc_vehicle_reset", "sdfnmpc_vehicle_begin",
    "sdfnmpc_vehicle_x_true", "sdfnmpc_plant_step_vehicle", "sdfnmpc_vehicle_set_body", "sdfnmpc_vehicle_body_state",
    "sdfnmpc_scene_swept_distance", "sdfnmpc_scene_speed_bound",
    "sdfnmpc_scene_create_mesh", "sdfnmpc_scene_is_mesh", "sdfnmpc_scene_is_sdf_source",
    "sdfnmpc_scene_create_mesh_mixed",
    "sdfnmpc_scene_create_instanced", "sdfnmpc_scene_is_instanced",
]
L4C_SYMBOLS = [
    f"{p}sdf_l4c{s}" for p in ("", "jac_", "adj1_")
    for s in ("", "_n_in", "_n_out", "_sparsity_in", "_sparsity_out", "_work")
] + ["sdf_l4c_name_in", "sdf_l4c_name_out", "sdf_l4c_checkout", "sdf_l4c_release", "sdf_l4c_incref",
     "sdf_l4c_decref", "sdf_l4c_configure", "sdf_l4c_last_error"]


class SdfnmpcError(RuntimeError):
    pass


POLY_MAX, NHN_MAX = 84, 8  # SDFNMPC_POLY_MAX, SDFNMPC_NHN_MAX


class QuadModelC(C.Structure):
    _fields_ = [("gamma", C.c_double), ("roll", C.c_double), ("pitch", C.c_double), ("wz", C.c_double),
                ("g", C.c_double), ("B_p_C", C.c_double * 3), ("B_R_C", C.c_double * 9),
                ("fov_const_offset", C.c_double), ("rec_feas", C.c_int), ("stability", C.c_int),
                ("poly_deg", C.c_int), ("poly", C.c_double * POLY_MAX), ("kind", C.c_int),
                ("tau_roll", C.c_double), ("tau_pitch", C.c_double)]


MODEL_KINDS = {"att": 0, "att_tau": 1}  # SDFNMPC_MODEL_ATT, SDFNMPC_MODEL_ATT_TAU
TAU_ROLL = TAU_PITCH = 0.12  # quad_rollpitchyawrate_tau.py:19-20


LIN_PTRS = ("x", "u", "p", "dt", "xn", "AB", "y", "Jy", "yN", "JyN", "h", "Jh", "sdf")


class SceneSdfOptsC(C.Structure):
    _fields_ = [("scene", C.c_void_p), ("scene_of", C.c_void_p), ("max_df", C.c_double), ("t0", C.c_double),
                ("tau", C.c_void_p)]


class ImgOptsC(C.Structure):
    _fields_ = [("dmax", C.c_float), ("hfov", C.c_float), ("vfov", C.c_float), ("is_depth", C.c_int),
                ("is_spherical", C.c_int)]


class ImgSdfOptsC(C.Structure):
    _fields_ = [("img", ImgOptsC), ("H", C.c_int), ("W", C.c_int), ("images", C.c_void_p), ("img_of", C.c_void_p),
                ("is_signed", C.c_int), ("min_df", C.c_float), ("max_df", C.c_float), ("grid", C.c_void_p),
                ("dist", C.c_void_p), ("orig_idx", C.c_void_p), ("G", C.c_int), ("pooled", C.c_void_p)]


class LinArgsC(C.Structure):
    _fields_ = [("B", C.c_int), ("N", C.c_int), ("np", C.c_int), ("latent_mode", C.c_int)] + [
        (n, C.c_void_p) for n in LIN_PTRS] + [("nyN", C.c_int), ("no_sdf", C.c_int), ("hE", C.c_void_p),
                                             ("JhE", C.c_void_p), ("sdf_scene", C.POINTER(SceneSdfOptsC)),
                                             ("sdf_image", C.POINTER(ImgSdfOptsC))]


class QpOptsC(C.Structure):
    _fields_ = [("lbu", C.c_double * 4), ("ubu", C.c_double * 4), ("lh", C.c_double * 3), ("uh", C.c_double * 3),
                ("zl", C.c_double * 3), ("Zl", C.c_double * 3), ("lm", C.c_double), ("cost_scaling", C.c_int),
                ("max_iter", C.c_int), ("tol", C.c_double), ("ny", C.c_int), ("lm_scaling", C.c_int),
                ("warm_start", C.c_int), ("nh", C.c_int), ("h_col", C.c_int * 3), ("nhN", C.c_int), ("nsN", C.c_int),
                ("hN_col", C.c_int * NHN_MAX), ("hE_col", C.c_int * NHN_MAX), ("lhN", C.c_double * NHN_MAX),
                ("uhN", C.c_double * NHN_MAX), ("zlN", C.c_double * 3), ("ZlN", C.c_double * 3), ("nyN", C.c_int),
                ("nhs", C.c_int)]


class RefOptsC(C.Structure):
    _fields_ = [("mode", C.c_int), ("yaw_mode", C.c_int), ("st_enable", C.c_int), ("st_mode", C.c_int),
                ("st_dang", C.c_double), ("align_off", C.c_double), ("dmin", C.c_double), ("vref", C.c_double),
                ("wzref", C.c_double), ("T", C.c_double), ("B_p_C", C.c_double * 3), ("B_R_C", C.c_double * 9)]


REF_IN = ("wp_p", "wp_q", "vw", "wrow", "latent", "W_p_Bo", "W_R_Bo", "flag")
REF_OUT = ("p", "yref", "W", "yNref", "WN")


class RefArgsC(C.Structure):
    _fields_ = [("B", C.c_int), ("N", C.c_int), ("np", C.c_int), ("ny", C.c_int), ("n_wp", C.c_int),
                ("L", C.c_int), ("x0", C.c_void_p), ("x0_stride", C.c_int)] + [
        (n, C.c_void_p) for n in REF_IN + REF_OUT] + [("nyN", C.c_int)]


QP_IN = ("xn", "AB", "y", "Jy", "yN", "JyN", "h", "Jh", "hE", "JhE", "x", "u", "x0", "yref", "W", "yNref", "WN", "dt")
QP_OUT = ("dx", "du", "slack", "status", "iters", "res")


class VaeOptsC(C.Structure):
    _fields_ = [("B", C.c_int), ("in_h", C.c_int), ("in_w", C.c_int), ("dtype", C.c_int), ("clip", C.c_float),
                ("yz", C.c_void_p)]


class SolverOptsC(C.Structure):
    _fields_ = [("B", C.c_int), ("N", C.c_int), ("np", C.c_int), ("ny", C.c_int), ("latent_mode", C.c_int),
                ("dt", C.POINTER(C.c_double)), ("model", QuadModelC), ("qp", QpOptsC)]


class QpArgsC(C.Structure):
    _fields_ = [("B", C.c_int), ("N", C.c_int)] + [(n, C.c_void_p) for n in QP_IN + QP_OUT]


class PlantOptsC(C.Structure):
    _fields_ = [("kind", C.c_int)] + [(n, C.c_double) for n in ("gamma", "roll", "pitch", "wz", "g", "tau_roll",
                                                                "tau_pitch", "dt")] + [
        ("substeps", C.c_int), ("acc_dist", C.c_void_p), ("gamma_scale", C.c_void_p)]


class RolloutArgsC(C.Structure):
    _fields_ = [("steps", C.c_int), ("shift", C.c_int), ("ref", C.POINTER(RefOptsC))] + [
        (n, C.c_void_p) for n in ("wp_p", "wp_q", "vw", "wrow")] + [("n_wp", C.c_int), ("plant", PlantOptsC)] + [
        (n, C.c_void_p) for n in ("x_log", "u_log", "status_log", "iters_log", "pts_log")] + [
        ("vehicle", C.c_void_p), ("frame0", C.c_int), ("xhat_log", C.c_void_p), ("uapp_log", C.c_void_p),
        ("omega_log", C.c_void_p), ("rotor_log", C.c_void_p)]


class VehicleOptsC(C.Structure):
    _fields_ = [("seed", C.c_uint64), ("d", C.c_int), ("tau_m", C.c_double), ("drag", C.c_double * 3)] + [
        (n, C.c_double) for n in ("gust_std", "gust_tau", "est_std_p", "est_std_v", "est_std_yaw")] + [
        ("est_bias", C.c_void_p), ("stream_id", C.c_void_p), ("g", C.c_double), ("gamma", C.c_double)]


class BodyOptsC(C.Structure):
    _fields_ = [("mass", C.c_double), ("inertia", C.c_double * 3), ("Gf", C.c_double * 12), ("Gt", C.c_double * 12),
                ("mixer", C.c_double * 16), ("wp_max", C.c_double), ("wp_idle", C.c_double), ("tau_att", C.c_double),
                ("k_rate", C.c_double * 3), ("tau_mot", C.c_double)]


SCENE_MAX_PRIMS = 32  # SDFNMPC_SCENE_MAX_PRIMS
PRIM_KINDS = {"sphere": 0, "box": 1, "cylinder": 2}  # SDFNMPC_PRIM_*


class PrimC(C.Structure):
    _fields_ = [("kind", C.c_int), ("a", C.c_double * 6)]


class MeshOptsC(C.Structure):  # sdfnmpc_mesh_opts
    _fields_ = [("leaf_size", C.c_int), ("closed", C.c_int), ("sdf_source", C.c_int)]


class PrimMotionC(C.Structure):
    _fields_ = [("q", C.c_double * 4), ("yaw_rate", C.c_double), ("v", C.c_double * 3), ("amp", C.c_double * 3),
                ("omega", C.c_double), ("phase", C.c_double)]


SCENE_MAX_INSTANCES = 256  # SDFNMPC_SCENE_MAX_INSTANCES


class MeshInstanceC(C.Structure):  # sdfnmpc_mesh_instance
    _fields_ = [("part", C.c_int), ("p", C.c_double * 3), ("motion", PrimMotionC)]


class PerceiveArgsC(C.Structure):
    _fields_ = [("scene", C.c_void_p), ("scene_of", C.c_void_p), ("img", ImgOptsC), ("h", C.c_int), ("w", C.c_int),
                ("scale", C.c_float), ("B_p_C", C.c_double * 3), ("B_R_C", C.c_double * 9), ("vae", C.c_void_p),
                ("vae_opts", VaeOptsC), ("every", C.c_int), ("phase", C.c_int)] + [
        (n, C.c_void_p) for n in ("images", "latent", "latent64", "W_p_Bo", "W_R_Bo", "W_p_C", "W_R_C")]


class PoseRefreshArgsC(C.Structure):
    _fields_ = [("every", C.c_int), ("B_p_C", C.c_double * 3), ("B_R_C", C.c_double * 9)] + [
        (n, C.c_void_p) for n in ("W_p_Bo", "W_R_Bo", "W_p_C", "W_R_C")]


class SensorOptsC(C.Structure):
    _fields_ = [("seed", C.c_uint64), ("a", C.c_float), ("b", C.c_float), ("vmax", C.c_float),
                ("p_thresh", C.c_uint32), ("miss_invalid", C.c_int), ("outlier_rm", C.c_int), ("min_range", C.c_float),
                ("boxes", C.c_void_p), ("n_frames", C.c_int), ("max_boxes", C.c_int), ("stream_id", C.c_void_p)]


MORPH_OPS = {"dilate": 0, "erode": 1}  # SDFNMPC_MORPH_*
MORPH_TILE = 16  # output pixels per block edge of csrc/morph.hip (tests cross its seams)
SENSOR_MAX_BOXES = 8

_lib = None


def load():
    """Load libsdfnmpc.so (raises if it has not been built)."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise SdfnmpcError(f"{LIB_PATH} not built: run `python -c 'import __graft_entry__ as g; g.build()'` "
                           "(the HIP extension is the only compute path)")
    lib = C.CDLL(LIB_PATH)
    vp, i, f, d, ll, sz = C.c_void_p, C.c_int, C.c_float, C.c_double, C.c_longlong, C.c_size_t
    P = C.POINTER
    sig = {
        "sdfnmpc_abi_version": (i, []),
        "sdfnmpc_last_error": (C.c_char_p, []),
        "sdfnmpc_ctx_create": (i, [i, vp, P(vp)]),
        "sdfnmpc_ctx_destroy": (None, [vp]),
        "sdfnmpc_ctx_set_stream": (i, [vp, vp]),
        "sdfnmpc_ctx_use_null_stream": (i, [vp]),
        "sdfnmpc_ctx_stream": (vp, [vp]),
        "sdfnmpc_ctx_synchronize": (i, [vp]),
        "sdfnmpc_ctx_set_tile_rows": (i, [vp, i]),
        "sdfnmpc_ctx_set_qp_kernel": (i, [vp, i]),
        "sdfnmpc_ctx_set_sdf_server": (i, [vp, i]),
        "sdfnmpc_ctx_sdf_server_stats": (i, [vp, P(d)]),
        "sdfnmpc_ctx_qp_kernel": (i, [vp, i, i]),
        "sdfnmpc_ctx_qp_kernel_for": (i, [vp, i, i, P(QpOptsC)]),
        "sdfnmpc_qp_seg_count": (i, [i]),
        "sdfnmpc_qp_lds_bytes": (C.c_longlong, [i]),
        "sdfnmpc_qp_capacity": (C.c_longlong, [vp, i]),
        "sdfnmpc_qp_capacity_for": (C.c_longlong, [vp, i, P(QpOptsC)]),
        "sdfnmpc_ctx_enable_timing": (i, [vp, i]),
        "sdfnmpc_ctx_kernel_stats": (i, [vp, C.c_char_p, P(d), P(ll)]),
        "sdfnmpc_ctx_reset_stats": (i, [vp]),
        "sdfnmpc_net_load": (i, [vp, vp, sz, P(vp)]),
        "sdfnmpc_net_load_file": (i, [vp, C.c_char_p, P(vp)]),
        "sdfnmpc_net_siren": (i, [vp, C.c_uint64, f, f, P(vp)]),
        "sdfnmpc_net_free": (None, [vp]),
        "sdfnmpc_net_max_df": (f, [vp]),
        "sdfnmpc_net_size_latent": (i, [vp]),
        "sdfnmpc_net_fingerprint": (C.c_uint64, [vp]),
        "sdfnmpc_sdf_eval": (i, [vp, vp, ll, vp, vp, i, vp, vp]),
        "sdfnmpc_sdf_eval_host": (i, [vp, vp, i, P(d), P(d), P(d)]),
        "sdfnmpc_linearize": (i, [vp, vp, P(QuadModelC), P(LinArgsC)]),
        "sdfnmpc_shooting_grid": (i, [i, d, i, i, d, P(d), P(d)]),
        "sdfnmpc_qp_solve": (i, [vp, P(QpOptsC), P(QpArgsC)]),
        "sdfnmpc_rti_prepare": (i, [vp, vp, P(QuadModelC), P(LinArgsC), P(QpOptsC), P(QpArgsC)]),
        "sdfnmpc_qp_feedback": (i, [vp, P(QpOptsC), P(QpArgsC)]),
        "sdfnmpc_rti_apply": (i, [vp, i, i, vp, vp, vp, vp, vp, vp]),
        "sdfnmpc_step_create": (i, [vp, vp, P(QuadModelC), P(LinArgsC), P(QpOptsC), P(QpArgsC), vp, vp, P(vp)]),
        "sdfnmpc_step_launch": (i, [vp, vp]),
        "sdfnmpc_step_destroy": (None, [vp]),
        "sdfnmpc_pack_refs": (i, [vp, P(RefOptsC), P(RefArgsC)]),
        "sdfnmpc_vae_load": (i, [vp, vp, sz, P(vp)]),
        "sdfnmpc_vae_free": (None, [vp]),
        "sdfnmpc_vae_size_latent": (i, [vp]),
        "sdfnmpc_vae_encode": (i, [vp, vp, P(VaeOptsC), vp, vp, vp]),
        "sdfnmpc_vae_dec_load": (i, [vp, vp, sz, P(vp)]),
        "sdfnmpc_vae_dec_free": (None, [vp]),
        "sdfnmpc_vae_dec_size_latent": (i, [vp]),
        "sdfnmpc_vae_decode": (i, [vp, vp, i, vp, i, i, vp, vp]),
        "sdfnmpc_colcheck": (i, [vp, P(ImgOptsC), i, f, vp, i, i, i, vp, vp, ll, vp]),
        "sdfnmpc_udf": (i, [vp, P(ImgOptsC), f, vp, i, i, i, vp, vp, ll, vp, vp, vp]),
        "sdfnmpc_sdf_truth": (i, [vp, P(ImgOptsC), f, f, vp, vp, vp, i, vp, i, i, i, vp, vp, ll, vp, vp, vp]),
        "sdfnmpc_ctx_device": (i, [vp]),
        "sdfnmpc_dev_alloc": (i, [vp, sz, P(vp)]),
        "sdfnmpc_dev_free": (None, [vp, vp]),
        "sdfnmpc_memcpy": (i, [vp, vp, vp, sz, i]),
        "sdfnmpc_solver_create": (i, [vp, vp, P(SolverOptsC), P(vp)]),
        "sdfnmpc_solver_destroy": (None, [vp]),
        "sdfnmpc_solver_field": (i, [vp, C.c_char_p, P(vp), P(i), P(i)]),
        "sdfnmpc_solver_upload": (i, [vp, C.c_char_p, i, i, vp, vp]),
        "sdfnmpc_solver_download": (i, [vp, C.c_char_p, vp]),
        "sdfnmpc_solver_init": (i, [vp, vp, vp]),
        "sdfnmpc_solver_shift": (i, [vp, i]),
        "sdfnmpc_solver_step": (i, [vp]),
        "sdfnmpc_solver_wait": (i, [vp, vp, vp, vp]),
        "sdfnmpc_plant_step": (i, [vp, P(PlantOptsC), i, vp, vp, vp]),
        "sdfnmpc_solver_rollout": (i, [vp, P(RolloutArgsC)]),
        "sdfnmpc_scene_create": (i, [vp, i, P(i), P(PrimC), P(vp)]),
        "sdfnmpc_scene_free": (None, [vp]),
        "sdfnmpc_scene_render": (i, [vp, vp, vp, P(ImgOptsC), i, i, f, i, vp, vp, vp]),
        "sdfnmpc_scene_pose": (i, [vp, P(d), P(d), i, vp, vp, vp, vp, vp]),
        "sdfnmpc_scene_distance": (i, [vp, vp, vp, vp, ll, vp]),
        "sdfnmpc_solver_rollout_perceive": (i, [vp, P(RolloutArgsC), P(PerceiveArgsC)]),
        "sdfnmpc_scene_create_moving": (i, [vp, i, P(i), P(PrimC), P(PrimMotionC), P(vp)]),
        "sdfnmpc_scene_is_dynamic": (i, [vp]),
        "sdfnmpc_scene_create_large": (i, [vp, i, P(i), P(PrimC), d, P(vp)]),
        "sdfnmpc_scene_is_indexed": (i, [vp]),
        "sdfnmpc_scene_create_mixed": (i, [vp, i, P(i), P(PrimC), d, P(i), P(PrimC), P(PrimMotionC), P(vp)]),
        "sdfnmpc_scene_render_at": (i, [vp, vp, vp, P(ImgOptsC), i, i, f, i, vp, vp, d, vp]),
        "sdfnmpc_scene_distance_at": (i, [vp, vp, vp, vp, vp, ll, vp]),
        "sdfnmpc_scene_swept_distance": (i, [vp, vp, vp, vp, vp, vp, vp, ll, d, i, vp, vp, vp, vp]),
        "sdfnmpc_scene_speed_bound": (i, [vp, P(d)]),
        "sdfnmpc_scene_create_mesh": (i, [vp, i, P(i), P(d), P(i), P(i), P(MeshOptsC), P(vp)]),
        "sdfnmpc_scene_create_mesh_mixed": (i, [vp, i, P(i), P(d), P(i), P(i), P(MeshOptsC), P(i), P(PrimC),
                                                P(PrimMotionC), P(vp)]),
        "sdfnmpc_scene_is_mesh": (i, [vp]),
        "sdfnmpc_scene_create_instanced": (i, [vp, i, P(i), P(d), P(i), P(i), P(MeshOptsC), i, P(i), P(MeshInstanceC),
                                               P(vp)]),
        "sdfnmpc_scene_is_instanced": (i, [vp]),
        "sdfnmpc_scene_is_sdf_source": (i, [vp]),
        "sdfnmpc_solver_rollout_perceive_at": (i, [vp, P(RolloutArgsC), P(PerceiveArgsC), d, d]),
        "sdfnmpc_morph": (i, [vp, i, vp, i, i, i, vp, i, i, i, vp]),
        "sdfnmpc_outlier_rm": (i, [vp, i, f, vp, i, i, i, vp]),
        "sdfnmpc_sensor_apply": (i, [vp, P(SensorOptsC), i, vp, i, i, i, vp]),
        "sdfnmpc_solver_rollout_perceive_sensor": (i, [vp, P(RolloutArgsC), P(PerceiveArgsC), d, d, P(SensorOptsC), vp]),
        "sdfnmpc_scene_sdf_rows": (i, [vp, P(SceneSdfOptsC), i, i, i, vp, vp, vp, vp]),
        "sdfnmpc_solver_set_sdf_scene": (i, [vp, vp, vp, d, i]),
        "sdfnmpc_solver_set_scene_time": (i, [vp, d]),
        "sdfnmpc_solver_rollout_scene_sdf": (i, [vp, P(RolloutArgsC), P(PoseRefreshArgsC), i, d, d]),
        "sdfnmpc_img_sdf_rows": (i, [vp, P(ImgSdfOptsC), i, i, i, vp, vp, vp, vp, vp]),
        "sdfnmpc_img_sdf_pool": (i, [vp, P(ImgSdfOptsC), i]),
        "sdfnmpc_solver_set_sdf_image": (i, [vp, P(ImgSdfOptsC)]),
        "sdfnmpc_solver_rollout_image_sdf": (i, [vp, P(RolloutArgsC), P(PerceiveArgsC), d, d, P(SensorOptsC), vp]),
        "sdfnmpc_solver_rollout_image_recon": (i, [vp, P(RolloutArgsC), P(PerceiveArgsC), d, d, P(SensorOptsC), vp, vp]),
        "sdfnmpc_vehicle_create": (i, [vp, P(VehicleOptsC), i, P(vp)]),
        "sdfnmpc_vehicle_destroy": (None, [vp]),
        "sdfnmpc_vehicle_reset": (i, [vp]),
        "sdfnmpc_vehicle_begin": (i, [vp, vp, vp, i]),
        "sdfnmpc_vehicle_x_true": (vp, [vp]),
        "sdfnmpc_plant_step_vehicle": (i, [vp, P(PlantOptsC), vp, i, vp, i, vp]),
        "sdfnmpc_vehicle_set_body": (i, [vp, P(BodyOptsC)]),
        "sdfnmpc_vehicle_body_state": (i, [vp, P(vp), P(vp)]),
    }
    for name, (res, args) in sig.items():
        fn = getattr(lib, name)
        fn.restype, fn.argtypes = res, args
    if lib.sdfnmpc_abi_version() != 19:
        raise SdfnmpcError("libsdfnmpc.so ABI version mismatch")
    _lib = lib
    return lib


def l4c_path() -> str:
    """Path of the CasADi external-function shim (include/sdf_l4c.h); raises if it has not been built."""
    if not os.path.exists(L4C_PATH):
        raise SdfnmpcError(f"{L4C_PATH} not built")
    return L4C_PATH


def _check(rc):
    if rc != 0:
        raise SdfnmpcError(f"sdfnmpc error {rc}: {load().sdfnmpc_last_error().decode()}")


def _ptr(t):
    if t is None:
        return None
    if isinstance(t, int):
        return t
    return t.data_ptr()


def sync_producer(a):
    """A torch CUDA tensor handed to a kernel of ours (which runs on a context stream, not torch's): wait
    until torch's current stream on its device -- where a producing kernel or non_blocking copy was queued --
    has finished.  DeviceArray / FieldView / host arrays need nothing.  torch is imported only here."""
    if type(a).__module__.split(".")[0] == "torch" and getattr(a, "is_cuda", False):
        import torch
        torch.cuda.current_stream(a.device).synchronize()
    return a


class Context:
    """One HIP device + stream (sdfnmpc_ctx)."""

    def __init__(self, device: int = 0, stream=None, tile_rows: int = 32):
        """stream: None -> a private non-blocking stream; a HIP stream handle (int) -> that stream, where
        0 is the legacy null stream (PyTorch's default stream), so the kernels are ordered with torch's."""
        lib = load()
        h = C.c_void_p()
        _check(lib.sdfnmpc_ctx_create(device, stream or None, C.byref(h)))
        self.h = h
        if stream is not None and int(stream) == 0:
            _check(lib.sdfnmpc_ctx_use_null_stream(h))
        self.device = device
        self.set_tile_rows(tile_rows)

    def set_tile_rows(self, rows: int):
        _check(load().sdfnmpc_ctx_set_tile_rows(self.h, rows))

    QP_KERNELS = {"auto": 0, "serial": 1, "segmented": 2}

    def set_qp_kernel(self, kind: str):
        """'auto' (segmented for B <= 256 -- 512 from N = 48 -- at 36 <= N <= 63, else serial), 'serial' or
        'segmented' (include/sdfnmpc.h)."""
        _check(load().sdfnmpc_ctx_set_qp_kernel(self.h, self.QP_KERNELS[kind]))

    def set_sdf_server(self, on: bool):
        """Serve the host-pointer SDF path (sdf_eval_host, <= 16 rows) from the resident server kernel
        (default) or with one launch per call (include/sdfnmpc.h)."""
        _check(load().sdfnmpc_ctx_set_sdf_server(self.h, int(bool(on))))

    def sdf_server_stats(self) -> dict:
        """Mean microseconds per served request since the last call (diagnostics)."""
        o = (C.c_double * 18)()
        _check(load().sdfnmpc_ctx_sdf_server_stats(self.h, o))
        return {"stage_us": o[0], "eval_us": o[1], "wait_us": o[2], "requests": int(o[3]),
                "phases_us": [round(v, 2) for v in o[4:18]]}

    def qp_kernel(self, N: int, B: int, opts: "QpOptsC" = None) -> str:
        """The kernel a QP batch of B instances at horizon N runs ('serial' or 'segmented'); with opts: for that
        constraint set (sdfnmpc_ctx_qp_kernel_for)."""
        lib = load()
        k = lib.sdfnmpc_ctx_qp_kernel(self.h, N, B) if opts is None else lib.sdfnmpc_ctx_qp_kernel_for(self.h, N, B, C.byref(opts))
        return {1: "serial", 2: "segmented"}.get(k, "invalid")

    def qp_capacity(self, N: int, opts: "QpOptsC" = None) -> int:
        """Instances this device solves in one wave of QP workgroups at horizon N (sdfnmpc_qp_capacity; with
        opts: for that constraint set, sdfnmpc_qp_capacity_for)."""
        lib = load()
        n = int(lib.sdfnmpc_qp_capacity(self.h, N) if opts is None else lib.sdfnmpc_qp_capacity_for(self.h, N, C.byref(opts)))
        if n < 0:
            raise SdfnmpcError(f"sdfnmpc_qp_capacity: bad arguments (N={N})")
        return n

    def set_stream(self, stream):
        if stream is not None and int(stream) == 0:
            _check(load().sdfnmpc_ctx_use_null_stream(self.h))
        else:
            _check(load().sdfnmpc_ctx_set_stream(self.h, stream))

    def synchronize(self):
        _check(load().sdfnmpc_ctx_synchronize(self.h))

    @property
    def stream(self) -> int:
        return load().sdfnmpc_ctx_stream(self.h)

    @property
    def device_index(self) -> int:
        return int(load().sdfnmpc_ctx_device(self.h))

    def enable_timing(self, on=True):
        _check(load().sdfnmpc_ctx_enable_timing(self.h, int(on)))

    def kernel_stats(self, name: str):
        ms, n = C.c_double(), C.c_longlong()
        _check(load().sdfnmpc_ctx_kernel_stats(self.h, name.encode(), C.byref(ms), C.byref(n)))
        return ms.value, n.value

    def reset_stats(self):
        _check(load().sdfnmpc_ctx_reset_stats(self.h))

    def close(self):
        if getattr(self, "h", None):
            load().sdfnmpc_ctx_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class Net:
    """Device-resident packed NeuralDF (sdfnmpc_net)."""

    def __init__(self, ctx: Context, handle):
        self.ctx, self.h = ctx, handle

    @classmethod
    def siren(cls, ctx: Context, seed: int = 0, weight_gain: float = 1.0, bias_gain: float = 0.0):
        h = C.c_void_p()
        _check(load().sdfnmpc_net_siren(ctx.h, seed, weight_gain, bias_gain, C.byref(h)))
        return cls(ctx, h)

    @classmethod
    def from_blob(cls, ctx: Context, blob: bytes):
        h = C.c_void_p()
        buf = C.create_string_buffer(blob, len(blob))
        _check(load().sdfnmpc_net_load(ctx.h, buf, len(blob), C.byref(h)))
        return cls(ctx, h)

    @classmethod
    def from_file(cls, ctx: Context, path: str):
        h = C.c_void_p()
        _check(load().sdfnmpc_net_load_file(ctx.h, path.encode(), C.byref(h)))
        return cls(ctx, h)

    @property
    def max_df(self) -> float:
        return float(load().sdfnmpc_net_max_df(self.h))

    @property
    def size_latent(self) -> int:
        return int(load().sdfnmpc_net_size_latent(self.h))

    @property
    def fingerprint(self) -> int:
        return int(load().sdfnmpc_net_fingerprint(self.h))

    def eval(self, rows, pos4, latent, rows_per_inst, out4, grad_latent=None):
        """Device-pointer SDF evaluation (asynchronous on the context stream)."""
        _check(load().sdfnmpc_sdf_eval(self.ctx.h, self.h, rows, _ptr(pos4), _ptr(latent), rows_per_inst,
                                       _ptr(out4), _ptr(grad_latent)))

    def eval_host(self, inp: np.ndarray, want_grad=True):
        """Host-pointer synchronous evaluation: inp [rows, 3 + L] fp64 -> (df [rows], grad [rows, 3 + L])
        (L = size_latent, 128 for the deployed net: the 131 of jac_sdf_l4c)."""
        inp = np.ascontiguousarray(inp, dtype=np.float64)
        rows = inp.shape[0]
        df = np.empty(rows)
        g = np.empty_like(inp) if want_grad else None
        P = C.POINTER(C.c_double)
        _check(load().sdfnmpc_sdf_eval_host(self.ctx.h, self.h, rows, inp.ctypes.data_as(P), df.ctypes.data_as(P),
                                            None if g is None else g.ctypes.data_as(P)))
        return df, g

    def close(self):
        if getattr(self, "h", None):
            load().sdfnmpc_net_free(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def quad_model(cfg, model=None) -> QuadModelC:
    """Model constants of a config; ``model`` (model.Quad) adds the terminal extras of its flags
    (recursive_feasibility: the braking polynomial; stability).  The kind follows cfg.mpc.model ('att' 0,
    'att_tau' 1 with the lags' time constants: the model's, else the reference's 0.12 s)."""
    lim = cfg.robot.limits
    name = str(cfg.mpc.get("model", "att"))
    if name not in MODEL_KINDS:
        from .model import UnsupportedConfig
        raise UnsupportedConfig(f"mpc.model '{name}': only {sorted(MODEL_KINDS)} are built")
    R = np.asarray(cfg.sensor.B_R_C, dtype=np.float64).ravel()
    m = QuadModelC(float(lim.gamma), float(lim.roll), float(lim.pitch), float(lim.wz), 9.81,
                   (C.c_double * 3)(*[float(v) for v in cfg.sensor.B_p_C]), (C.c_double * 9)(*R),
                   float(cfg.mpc.fov_const_offset))
    m.kind = MODEL_KINDS[name]
    if m.kind == 1:
        m.tau_roll = float(getattr(model, "tau_roll", TAU_ROLL))
        m.tau_pitch = float(getattr(model, "tau_pitch", TAU_PITCH))
    if model is not None:
        m.rec_feas, m.stability = int(model.rec_feas), int(model.stability)
        m.poly_deg = int(model.poly_deg)
        for i, c in enumerate(model.poly):
            m.poly[i] = float(c)
    return m


def scene_sdf_opts(scene_h, max_df: float, scene_of=None, t0: float = 0.0, tau=None) -> SceneSdfOptsC:
    """sdfnmpc_scene_sdf_opts: a scene handle as the source of the SDF row; scene_of [B] int32 / tau [N+1] float64
    device arrays or None.  The caller keeps what it names alive."""
    return SceneSdfOptsC(scene_h.value if isinstance(scene_h, C.c_void_p) else scene_h, _ptr(scene_of), float(max_df),
                         float(t0), _ptr(tau))


def img_sdf_opts(opts: "ImgOptsC", images, signed=True, min_df=-0.3, max_df=1.0, grid=None, dist=None, orig_idx=None,
                 pooled=None, img_of=None) -> ImgSdfOptsC:
    """sdfnmpc_img_sdf_opts: images device float32 [n_img][H][W] (normalised) as the source of the SDF row; signed: the
    voxel grid [G][3] / dist [G] / orig_idx [G] or None as sdf_truth takes them; unsigned: pooled device float32
    [n_img][H/5][W/5] (img_sdf_pool fills it); img_of device int32 [B] or None.  The caller keeps what it names alive."""
    _, H, W = (int(v) for v in images.shape)
    return ImgSdfOptsC(opts, H, W, _ptr(images), _ptr(img_of), int(bool(signed)), float(min_df), float(max_df),
                       _ptr(grid), _ptr(dist), _ptr(orig_idx), 0 if dist is None else int(dist.shape[0]), _ptr(pooled))


def img_sdf_rows(ctx: "Context", opts: ImgSdfOptsC, B: int, N: int, np_: int, x, p, h, Jh, pts=None):
    """Enqueue sdfnmpc_img_sdf_rows: the field of the camera image as the SDF row of h [B][N+1][3] / Jh [B][N+1][10][3]
    (column 2) at the positions x [B][N+1][10][:3] seen through the pose in p [B][N+1][np]; pts: device float32
    [B][N+1][3] or None, the camera-frame points."""
    _check(load().sdfnmpc_img_sdf_rows(ctx.h, C.byref(opts), int(B), int(N), int(np_), _ptr(x), _ptr(p), _ptr(h),
                                       _ptr(Jh), _ptr(pts)))


def img_sdf_pool(ctx: "Context", opts: ImgSdfOptsC, n_img: int):
    """Enqueue sdfnmpc_img_sdf_pool: the 5x5 min-pool of opts.images [n_img] into opts.pooled."""
    _check(load().sdfnmpc_img_sdf_pool(ctx.h, C.byref(opts), int(n_img)))


def lin_args(B: int, N: int, np_: int, bufs: dict, latent_mode=0, nyN=4, no_sdf=False, sdf_scene=None,
             sdf_image=None) -> LinArgsC:
    """sdf_scene: a SceneSdfOptsC (scene_sdf_opts) -- the scene's exact distance as the SDF row, no network;
    sdf_image: an ImgSdfOptsC (img_sdf_opts) -- the camera image's own field."""
    a = LinArgsC(B, N, np_, latent_mode, *[_ptr(bufs.get(k)) for k in LIN_PTRS], int(nyN), int(bool(no_sdf)),
                 _ptr(bufs.get("hE")), _ptr(bufs.get("JhE")))
    if sdf_scene is not None:
        a.sdf_scene = C.pointer(sdf_scene)
        a._keep = sdf_scene
    if sdf_image is not None:
        a.sdf_image = C.pointer(sdf_image)
        a._keep_img = sdf_image
    return a


def linearize(ctx: Context, net, model: QuadModelC, B: int, N: int, np_: int, bufs: dict, latent_mode=0, nyN=4,
              no_sdf=False, sdf_scene=None, sdf_image=None):
    """Enqueue the batched preparation phase.  bufs: device tensors named as sdfnmpc_lin_args (net may be
    None with no_sdf, sdf_scene or sdf_image)."""
    a = lin_args(B, N, np_, bufs, latent_mode, nyN, no_sdf, sdf_scene, sdf_image)
    _check(load().sdfnmpc_linearize(ctx.h, None if net is None else net.h, C.byref(model), C.byref(a)))


def qp_opts(model, lm=10.0, cost_scaling=True, max_iter=100, tol=1e-8, lm_scaling=True, warm_start=False) -> QpOptsC:
    """QP data of the 'att' / 'att_tau' model (model.Quad: bounds, the constraint set of its flags) + solver options
    (ocp.py:113-120 defaults).  lm_scaling: the Levenberg-Marquardt term is lm dt_k at stages k < N and lm at
    N (acados' Ts-scaled term).  warm_start: HPIPM's primal warm start (ocp.py:116) -- the IPM starts from
    the du buffer's entry values."""
    v = lambda a, n: (C.c_double * n)(*([float(x) for x in a] + [0.0] * (n - len(a))))
    iv = lambda a, n: (C.c_int * n)(*([int(x) for x in a] + [-1] * (n - len(a))))
    rows = model.term_rows
    return QpOptsC(v(model.lbu, 4), v(model.ubu, 4), v(model.lh, 3), v(model.uh, 3), v(model.zl, 3),
                   v(model.Zl, 3), float(lm), int(bool(cost_scaling)), int(max_iter), float(tol), int(model.ny),
                   int(bool(lm_scaling)), int(bool(warm_start)), int(model.nh), iv(model.h_cols, 3), int(model.nhN),
                   int(model.nsN), iv([r[0] for r in rows], NHN_MAX), iv([r[1] for r in rows], NHN_MAX),
                   v(model.lhN, NHN_MAX), v(model.uhN, NHN_MAX), v(model.zlN, 3), v(model.ZlN, 3), int(model.nyN),
                   int(getattr(model, "nhs", 0)))


def qp_solve(ctx: Context, opts: QpOptsC, B: int, N: int, bufs: dict):
    """Enqueue the batched feedback-phase QP.  bufs: device tensors named as sdfnmpc_qp_args."""
    a = QpArgsC(B, N, *[_ptr(bufs.get(k)) for k in QP_IN + QP_OUT])
    _check(load().sdfnmpc_qp_solve(ctx.h, C.byref(opts), C.byref(a)))


def rti_prepare(ctx: Context, net, model: QuadModelC, opts: QpOptsC, B: int, N: int, np_: int, bufs: dict,
                latent_mode=0, no_sdf=False, sdf_scene=None, sdf_image=None):
    """Enqueue the RTI preparation phase acados-style: linearisation + the QP's stage records (everything
    but x0).  bufs: device tensors named as sdfnmpc_lin_args and sdfnmpc_qp_args."""
    la = lin_args(B, N, np_, bufs, latent_mode, opts.nyN, no_sdf, sdf_scene, sdf_image)
    qa = QpArgsC(B, N, *[_ptr(bufs.get(k)) for k in QP_IN + QP_OUT])
    _check(load().sdfnmpc_rti_prepare(ctx.h, None if net is None else net.h, C.byref(model), C.byref(la),
                                      C.byref(opts), C.byref(qa)))


def qp_seg_count(N: int) -> int:
    """Segments (wavefronts) per instance of the segmented QP kernel at horizon N; 0: it does not serve N
    (sdfnmpc_qp_seg_count; follows SDFNMPC_QP_NSEG as the launch does)."""
    return int(load().sdfnmpc_qp_seg_count(N))


def qp_feedback(ctx: Context, opts: QpOptsC, B: int, N: int, bufs: dict):
    """Enqueue the RTI feedback phase: the IPM on the records of the last rti_prepare."""
    a = QpArgsC(B, N, *[_ptr(bufs.get(k)) for k in QP_IN + QP_OUT])
    _check(load().sdfnmpc_qp_feedback(ctx.h, C.byref(opts), C.byref(a)))


class RtiStep:
    """One SQP-RTI control step (rti_prepare + qp_feedback + rti_apply) over buffers bound once: the ctypes
    argument blocks are built here, not per call (the per-call form spends ~15 us of Python per phase
    building them, on the B = 1 latency path).  graph=True: the step is captured into a HIP graph
    (sdfnmpc_step_create, which runs it once eagerly) and a call is one graph launch.  The bound tensors
    must stay alive and at the same addresses."""

    def __init__(self, ctx: Context, net, model: QuadModelC, opts: QpOptsC, B: int, N: int, np_: int, bufs: dict,
                 u0=None, latent_mode=0, no_sdf=False, graph=False, sdf_scene=None, sdf_image=None):
        self._lib = load()
        self._ctx, self._net = ctx.h, None if net is None else net.h
        self._model, self._opts, self._B, self._N = model, opts, B, N
        self._la = lin_args(B, N, np_, bufs, latent_mode, opts.nyN, no_sdf, sdf_scene, sdf_image)
        self._qa = QpArgsC(B, N, *[_ptr(bufs.get(k)) for k in QP_IN + QP_OUT])
        self._apply = (_ptr(bufs["x"]), _ptr(bufs["u"]), _ptr(bufs["dx"]), _ptr(bufs["du"]), _ptr(u0),
                       _ptr(bufs.get("status")))
        self._keep = (bufs, u0, ctx, net)
        self._step = None
        if graph:
            for t in list(bufs.values()) + [u0]:
                sync_producer(t)
            h = C.c_void_p()
            _check(self._lib.sdfnmpc_step_create(self._ctx, self._net, C.byref(model), C.byref(self._la),
                                                 C.byref(opts), C.byref(self._qa), self._apply[4], self._apply[5],
                                                 C.byref(h)))
            self._step = h

    def __call__(self):
        lib, r = self._lib, C.byref
        if self._step is not None:
            _check(lib.sdfnmpc_step_launch(self._ctx, self._step))
            return
        _check(lib.sdfnmpc_rti_prepare(self._ctx, self._net, r(self._model), r(self._la), r(self._opts), r(self._qa)))
        _check(lib.sdfnmpc_qp_feedback(self._ctx, r(self._opts), r(self._qa)))
        _check(lib.sdfnmpc_rti_apply(self._ctx, self._B, self._N, *self._apply))

    def __del__(self):
        if getattr(self, "_step", None) is not None:
            self._lib.sdfnmpc_step_destroy(self._step)
            self._step = None


def rti_apply(ctx: Context, B: int, N: int, x, u, dx, du, u0=None, status=None):
    """x += dx, u += du, u0 = u[:, 0]; instances whose QP status is >= 2 (numerical failure) keep x, u."""
    _check(load().sdfnmpc_rti_apply(ctx.h, B, N, _ptr(x), _ptr(u), _ptr(dx), _ptr(du), _ptr(u0), _ptr(status)))


def shooting_grid(N: int, T: float, uniform=True, nb_short_nodes=2, dt_short=0.01):
    nodes, dt = np.empty(N + 1), np.empty(N)
    P = C.POINTER(C.c_double)
    _check(load().sdfnmpc_shooting_grid(N, T, int(bool(uniform)), nb_short_nodes, dt_short, nodes.ctypes.data_as(P),
                                        dt.ctypes.data_as(P)))
    return nodes, dt


def ref_opts(cfg, mode: int) -> RefOptsC:
    """RefGen knobs of a config (ref_gen.py) for sdfnmpc_pack_refs; mode 0 waypoints, 1 joystick, 2 from_x0,
    -1 latent / flag only, -2 pose only."""
    r = cfg.ref
    ym = str(r.yaw_mode)
    yaw_mode = {"ref": 1, "align": 2, "curent": 3}.get(ym, 0)  # 'current' / 'zero': identity (ref_gen.py:12, sic)
    st_mode = {"topic": 1, "align": 2}.get(ym, 0)
    v = lambda a, n: (C.c_double * n)(*[float(x) for x in np.asarray(a, dtype=float).ravel()])
    return RefOptsC(int(mode), yaw_mode, int(bool(r.stop_and_turn.enable)), st_mode, float(r.stop_and_turn.dang_min),
                    float(r.align_yaw_offset), float(r.yaw_align_dmin), float(r.vref), float(r.wzref), float(cfg.mpc.T),
                    v(cfg.sensor.B_p_C, 3), v(cfg.sensor.B_R_C, 9))


def pack_refs(ctx: Context, opts: RefOptsC, B: int, N: int, np_: int, ny: int, bufs: dict, n_wp: int = 0, L: int = 0,
              nyN: int = 4):
    """Enqueue sdfnmpc_pack_refs.  bufs: device tensors named as sdfnmpc_ref_args (x0 [B][stride])."""
    x0 = bufs.get("x0")
    stride = int(x0.shape[-1]) if x0 is not None else 0
    a = RefArgsC(B, N, np_, ny, n_wp, L, _ptr(x0), stride, *[_ptr(bufs.get(k)) for k in REF_IN + REF_OUT], int(nyN))
    _check(load().sdfnmpc_pack_refs(ctx.h, C.byref(opts), C.byref(a)))


class Vae:
    """Device-resident VAE encoder (sdfnmpc_vae) from a `.vaew` blob (sdf_nmpc_amd.vae.pack)."""

    def __init__(self, ctx: Context, blob: bytes, batch: int = 1):
        self.ctx = ctx
        h = C.c_void_p()
        buf = C.create_string_buffer(blob, len(blob))
        _check(load().sdfnmpc_vae_load(ctx.h, buf, len(blob), C.byref(h)))
        self.h = h
        self.batch = batch

    @property
    def size_latent(self) -> int:
        return int(load().sdfnmpc_vae_size_latent(self.h))

    def close(self):
        if getattr(self, "h", None):
            load().sdfnmpc_vae_free(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class VaeDec:
    """Device-resident VAE decoder (sdfnmpc_vae_dec) from a `.vaed` blob (sdf_nmpc_amd.vae.pack_decoder)."""

    def __init__(self, ctx: Context, blob: bytes):
        self.ctx = ctx
        h = C.c_void_p()
        buf = C.create_string_buffer(blob, len(blob))
        _check(load().sdfnmpc_vae_dec_load(ctx.h, buf, len(blob), C.byref(h)))
        self.h = h

    @property
    def size_latent(self) -> int:
        return int(load().sdfnmpc_vae_dec_size_latent(self.h))

    def close(self):
        if getattr(self, "h", None):
            load().sdfnmpc_vae_dec_free(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def vae_decode(ctx: Context, dec: VaeDec, latent, img, logits=None):
    """Enqueue sdfnmpc_vae_decode: latent device [B][L] fp32 -> img device [B][H][W] fp32 (the output size is
    img's), logits optional device [B][128][240] fp32."""
    _check(load().sdfnmpc_vae_decode(ctx.h, dec.h, int(latent.shape[0]), _ptr(latent), int(img.shape[-2]),
                                     int(img.shape[-1]), _ptr(img), _ptr(logits)))


def vae_opts(cfg, clip: float) -> VaeOptsC:
    """Per-call options from the config (sensor.dmax / mm_resolution, is_depth); B / size / dtype / yz per call."""
    o = VaeOptsC()
    o.clip = float(clip)
    o.dtype = 0
    return o


def vae_encode(ctx: Context, vae: Vae, opts: VaeOptsC, img, yz, latent, latent64=None, depth2range=True):
    """Enqueue sdfnmpc_vae_encode: img device array [B][H][W] (float32 or uint16; a DeviceArray or a torch
    tensor), latent [B][L] fp32."""
    o = VaeOptsC(int(img.shape[0]), int(img.shape[-2]), int(img.shape[-1]), 1 if "uint16" in str(img.dtype) else 0,
                 float(opts.clip), _ptr(yz) if depth2range else None)
    _check(load().sdfnmpc_vae_encode(ctx.h, vae.h, C.byref(o), _ptr(img), _ptr(latent), _ptr(latent64)))


# ---- ground truth from range images (csrc/df_truth.hip) ----
OUTSIDE = {"free": 0, "col": 1, "extrapolate": 2}  # collision_checker.py:18


def img_opts(dmax, hfov, vfov, is_depth=False, is_spherical=False) -> ImgOptsC:
    return ImgOptsC(float(dmax), float(hfov), float(vfov), int(bool(is_depth)), int(bool(is_spherical)))


def _img_dims(img):
    n_img, H, W = (int(v) for v in img.shape)
    return _ptr(img), n_img, H, W


def colcheck(ctx: Context, opts: ImgOptsC, outside: int, safe_ball: float, img, points, p_to_i, out):
    """Enqueue sdfnmpc_colcheck: img device float32 [n_img][H][W], points device float32 [n][3], p_to_i device
    int32 [n] or None, out device uint8 [n]."""
    _check(load().sdfnmpc_colcheck(ctx.h, C.byref(opts), int(outside), float(safe_ball), *_img_dims(img),
                                   _ptr(points), _ptr(p_to_i), int(points.shape[0]), _ptr(out)))


def udf(ctx: Context, opts: ImgOptsC, max_df: float, img, points, p_to_i, out_udf, out_grad, pix_idx=None):
    """Enqueue sdfnmpc_udf: outputs device float32 [n], [n][3] and optionally int32 [n]."""
    _check(load().sdfnmpc_udf(ctx.h, C.byref(opts), float(max_df), *_img_dims(img), _ptr(points), _ptr(p_to_i),
                              int(points.shape[0]), _ptr(out_udf), _ptr(out_grad), _ptr(pix_idx)))


def sdf_truth(ctx: Context, opts: ImgOptsC, min_df: float, max_df: float, grid, dist, orig_idx, img, points, p_to_i,
              out_sdf, out_grad, vox_idx=None):
    """Enqueue sdfnmpc_sdf_truth: grid device float32 [G][3], dist [G]; orig_idx device int32 [G] when the grid is
    sorted by dist, else None (full scan)."""
    _check(load().sdfnmpc_sdf_truth(ctx.h, C.byref(opts), float(min_df), float(max_df), _ptr(grid), _ptr(dist),
                                    _ptr(orig_idx), int(dist.shape[0]), *_img_dims(img), _ptr(points), _ptr(p_to_i),
                                    int(points.shape[0]), _ptr(out_sdf), _ptr(out_grad), _ptr(vox_idx)))


# ---- analytic scenes (csrc/scene.hip); the user-facing object is sdf_nmpc_amd.scene.Scene ----
def _prims_c(prims):
    """a flat list of (kind, values) -> PrimC array (one unused entry for an empty list)"""
    pr = (PrimC * max(len(prims), 1))()
    for k, (kind, vals) in enumerate(prims):
        pr[k].kind = int(kind)
        for j, v in enumerate(vals):
            pr[k].a[j] = float(v)
    return pr


def _motion_c(motion, n):
    """one dict per primitive (keys q, yaw_rate, v, amp, omega, phase; None: no motion) -> PrimMotionC array"""
    mo = (PrimMotionC * max(n, 1))()
    for k, m in enumerate(motion):
        m = m or {}
        mo[k].q[:] = [float(v) for v in m.get("q", (1.0, 0.0, 0.0, 0.0))]
        mo[k].v[:] = [float(v) for v in m.get("v", (0.0, 0.0, 0.0))]
        mo[k].amp[:] = [float(v) for v in m.get("amp", (0.0, 0.0, 0.0))]
        mo[k].yaw_rate, mo[k].omega, mo[k].phase = (float(m.get(n, 0.0)) for n in ("yaw_rate", "omega", "phase"))
    return mo


def scene_create(ctx: "Context", counts, prims, motion=None):
    """sdfnmpc_scene_create: counts [S] primitives per scene, prims a flat list of (kind, values) scene after
    scene.  Returns the handle; the C entry point refuses malformed scenes.  motion: one dict per primitive (keys
    q, yaw_rate, v, amp, omega, phase; None: no motion) -- sdfnmpc_scene_create_moving."""
    cn = (C.c_int * len(counts))(*[int(c) for c in counts])
    pr = _prims_c(prims)
    h = C.c_void_p()
    if motion is None:
        _check(load().sdfnmpc_scene_create(ctx.h, len(counts), cn, pr, C.byref(h)))
        return h
    mo = _motion_c(motion, len(prims))
    _check(load().sdfnmpc_scene_create_moving(ctx.h, len(counts), cn, pr, mo, C.byref(h)))
    return h


def scene_create_mixed(ctx: "Context", counts, prims, cell, mcounts, mprims, mmotion):
    """sdfnmpc_scene_create_mixed: scene_create_large's static primitives plus mcounts [S] movers per scene (at most
    32 each), mprims / mmotion as scene_create takes prims / motion (mmotion None: no motion records)."""
    cn = (C.c_int * len(counts))(*[int(c) for c in counts])
    mc = (C.c_int * len(mcounts))(*[int(c) for c in mcounts])
    h = C.c_void_p()
    _check(load().sdfnmpc_scene_create_mixed(ctx.h, len(counts), cn, _prims_c(prims), float(cell), mc, _prims_c(mprims),
                                             None if mmotion is None else _motion_c(mmotion, len(mprims)), C.byref(h)))
    return h


def scene_create_large(ctx: "Context", counts, prims, cell: float = 0.0):
    """sdfnmpc_scene_create_large: scene_create for scenes of up to 65536 static primitives each, with a uniform grid
    of cell edge `cell` [m] (<= 0: the library's default)."""
    cn = (C.c_int * len(counts))(*[int(c) for c in counts])
    pr = _prims_c(prims)
    h = C.c_void_p()
    _check(load().sdfnmpc_scene_create_large(ctx.h, len(counts), cn, pr, float(cell), C.byref(h)))
    return h


def scene_create_mesh(ctx: "Context", verts, tris, leaf_size: int = 0, closed: bool = False, sdf_source=False,
                      mcounts=None, mprims=None, mmotion=None):
    """sdfnmpc_scene_create_mesh: one (verts [nv, 3] float64, tris [nt, 3] int32) pair per scene, the indices local to
    the scene; leaf_size 1..8, 0 (the default) or -1 (no hierarchy); closed: signed distance, and the library checks
    that every scene is a closed, consistently oriented manifold; sdf_source: the set is accepted as a controller's SDF
    source (False, True or the integer the library is to see: it refuses all but 0 and 1).  Returns the handle.
    mcounts [S] (not None): sdfnmpc_scene_create_mesh_mixed, with mcounts movers per scene (at most 32 each) beside the
    meshes, mprims / mmotion as scene_create takes prims / motion (mmotion None: no motion records)."""
    vs = [np.ascontiguousarray(v, dtype=np.float64).reshape(-1, 3) for v in verts]
    ts = [np.ascontiguousarray(t, dtype=np.int32).reshape(-1, 3) for t in tris]
    nv = (C.c_int * len(vs))(*[v.shape[0] for v in vs])
    nt = (C.c_int * len(ts))(*[t.shape[0] for t in ts])
    va = np.ascontiguousarray(np.concatenate(vs, 0)) if vs else np.zeros((0, 3))
    ta = np.ascontiguousarray(np.concatenate(ts, 0)) if ts else np.zeros((0, 3), np.int32)
    o = MeshOptsC(int(leaf_size), int(bool(closed)), int(sdf_source))
    h = C.c_void_p()
    if mcounts is not None:
        mc = (C.c_int * len(mcounts))(*[int(c) for c in mcounts])
        _check(load().sdfnmpc_scene_create_mesh_mixed(
            ctx.h, len(vs), nv, va.ctypes.data_as(C.POINTER(C.c_double)), nt, ta.ctypes.data_as(C.POINTER(C.c_int)),
            C.byref(o), mc, _prims_c(mprims), None if mmotion is None else _motion_c(mmotion, len(mprims)), C.byref(h)))
        return h
    _check(load().sdfnmpc_scene_create_mesh(ctx.h, len(vs), nv, va.ctypes.data_as(C.POINTER(C.c_double)), nt,
                                            ta.ctypes.data_as(C.POINTER(C.c_int)), C.byref(o), C.byref(h)))
    return h


def scene_create_instanced(ctx: "Context", verts, tris, counts, instances, leaf_size: int = 0, closed: bool = False,
                           sdf_source=False):
    """sdfnmpc_scene_create_instanced: one (verts [nv, 3] float64, tris [nt, 3] int32) pair per part of the pool, as
    scene_create_mesh takes them per scene, with leaf_size, closed and sdf_source of that function; counts [S] instances
    per scene and instances, a flat list scene after scene of (part, p, motion) with motion a dict as scene_create takes
    it (None: no motion).  Returns the handle; the library refuses malformed parts and instances."""
    vs = [np.ascontiguousarray(v, dtype=np.float64).reshape(-1, 3) for v in verts]
    ts = [np.ascontiguousarray(t, dtype=np.int32).reshape(-1, 3) for t in tris]
    nv = (C.c_int * max(len(vs), 1))(*[v.shape[0] for v in vs])
    nt = (C.c_int * max(len(ts), 1))(*[t.shape[0] for t in ts])
    va = np.ascontiguousarray(np.concatenate(vs, 0)) if vs else np.zeros((0, 3))
    ta = np.ascontiguousarray(np.concatenate(ts, 0)) if ts else np.zeros((0, 3), np.int32)
    o = MeshOptsC(int(leaf_size), int(bool(closed)), int(sdf_source))
    cn = (C.c_int * max(len(counts), 1))(*[int(c) for c in counts])
    ins = (MeshInstanceC * max(len(instances), 1))()
    mo = _motion_c([m for _, _, m in instances], len(instances))
    for k, (part, pos, _) in enumerate(instances):
        ins[k].part = int(part)
        ins[k].p[:] = [float(v) for v in pos]
        ins[k].motion = mo[k]
    h = C.c_void_p()
    _check(load().sdfnmpc_scene_create_instanced(ctx.h, len(vs), nv, va.ctypes.data_as(C.POINTER(C.c_double)), nt,
                                                 ta.ctypes.data_as(C.POINTER(C.c_int)), C.byref(o), len(counts), cn, ins,
                                                 C.byref(h)))
    return h


def scene_render(ctx: "Context", scene_h, scene_of, opts: ImgOptsC, H: int, W: int, scale: float, B: int, W_p_C, W_R_C,
                 img):
    """Enqueue sdfnmpc_scene_render: W_p_C [B][3], W_R_C [B][9] device float64 -> img [B][H][W] device float32."""
    _check(load().sdfnmpc_scene_render(ctx.h, scene_h, _ptr(scene_of), C.byref(opts), int(H), int(W), float(scale),
                                       int(B), _ptr(W_p_C), _ptr(W_R_C), _ptr(img)))


def scene_render_at(ctx: "Context", scene_h, scene_of, opts: ImgOptsC, H: int, W: int, scale: float, B: int, W_p_C,
                    W_R_C, t: float, img):
    """Enqueue sdfnmpc_scene_render_at: scene_render of the scene at time t."""
    _check(load().sdfnmpc_scene_render_at(ctx.h, scene_h, _ptr(scene_of), C.byref(opts), int(H), int(W), float(scale),
                                          int(B), _ptr(W_p_C), _ptr(W_R_C), float(t), _ptr(img)))


def scene_distance_at(ctx: "Context", scene_h, points, p_to_scene, times, n: int, out):
    """Enqueue sdfnmpc_scene_distance_at: times [n] device float64 (None: t = 0), the time of every point."""
    _check(load().sdfnmpc_scene_distance_at(ctx.h, scene_h, _ptr(points), _ptr(p_to_scene), _ptr(times), int(n),
                                            _ptr(out)))


def scene_swept_distance(ctx: "Context", scene_h, p0, p1, p_to_scene, t0, t1, n: int, eps: float, max_evals: int, dmin,
                         s=None, gap=None, evals=None):
    """Enqueue sdfnmpc_scene_swept_distance: segments p0 -> p1 [n][3] device float64 between the times t0, t1 [n] (both
    None: t = 0) -> dmin, s, gap [n] device float64 and evals [n] device int32 (the last three optional)."""
    _check(load().sdfnmpc_scene_swept_distance(ctx.h, scene_h, _ptr(p0), _ptr(p1), _ptr(p_to_scene), _ptr(t0), _ptr(t1),
                                               int(n), float(eps), int(max_evals), _ptr(dmin), _ptr(s), _ptr(gap),
                                               _ptr(evals)))


def scene_speed_bound(scene_h, S: int) -> np.ndarray:
    """sdfnmpc_scene_speed_bound: [S] float64, the bound on the speed of any surface point of each scene's movers."""
    out = np.zeros(int(S), dtype=np.float64)
    _check(load().sdfnmpc_scene_speed_bound(scene_h, out.ctypes.data_as(C.POINTER(C.c_double))))
    return out


def scene_pose(ctx: "Context", B_p_C, B_R_C, B: int, x, W_p_Bo, W_R_Bo, W_p_C, W_R_C):
    """Enqueue sdfnmpc_scene_pose: x [B][10] device float64 -> body and camera poses (device float64)."""
    pv = (C.c_double * 3)(*[float(v) for v in np.asarray(B_p_C, dtype=float).ravel()])
    rv = (C.c_double * 9)(*[float(v) for v in np.asarray(B_R_C, dtype=float).ravel()])
    _check(load().sdfnmpc_scene_pose(ctx.h, pv, rv, int(B), _ptr(x), _ptr(W_p_Bo), _ptr(W_R_Bo),
                                     _ptr(W_p_C), _ptr(W_R_C)))


def scene_sdf_rows(ctx: "Context", scene_h, B: int, N: int, np_: int, x, p, h, Jh, max_df: float, scene_of=None,
                   t0: float = 0.0, tau=None):
    """Enqueue sdfnmpc_scene_sdf_rows: the scene's exact distance as the SDF row of h [B][N+1][3] / Jh
    [B][N+1][10][3] (column 2) at the positions x [B][N+1][10][:3], flag p [B][N+1][np][0]; node k at t0 + tau[k]."""
    o = scene_sdf_opts(scene_h, max_df, scene_of, t0, tau)
    _check(load().sdfnmpc_scene_sdf_rows(ctx.h, C.byref(o), int(B), int(N), int(np_), _ptr(x), _ptr(p), _ptr(h),
                                         _ptr(Jh)))


def scene_distance(ctx: "Context", scene_h, points, p_to_scene, n: int, out):
    """Enqueue sdfnmpc_scene_distance: points [n][3] device float64 -> out [n] device float64."""
    _check(load().sdfnmpc_scene_distance(ctx.h, scene_h, _ptr(points), _ptr(p_to_scene), int(n), _ptr(out)))


# ---- image morphology and the sensor stage (csrc/morph.hip, csrc/sensor.hip); the user-facing objects are
# sdf_nmpc_amd.preprocessing.* and sdf_nmpc_amd.sensor.SensorModel ----
def morph(ctx: "Context", op: int, kernel, ignore_zeros: bool, img, out):
    """Enqueue sdfnmpc_morph: kernel a host uint8 array [k_h][k_w]; img / out device float32 [B][H][W]."""
    k = np.ascontiguousarray(kernel, dtype=np.uint8)
    _check(load().sdfnmpc_morph(ctx.h, int(op), k.ctypes.data, int(k.shape[0]), int(k.shape[1]), int(bool(ignore_zeros)),
                                *_img_dims(img), _ptr(out)))


def outlier_rm(ctx: "Context", kernel_size: int, min_range: float, img, out):
    """Enqueue sdfnmpc_outlier_rm: img / out device float32 [B][H][W]; min_range in the image's units."""
    _check(load().sdfnmpc_outlier_rm(ctx.h, int(kernel_size), float(min_range), *_img_dims(img), _ptr(out)))


def sensor_apply(ctx: "Context", opts: SensorOptsC, frame: int, img, scratch=None):
    """Enqueue sdfnmpc_sensor_apply in place on img, device float32 [B][H][W]; scratch: the same shape, needed with
    opts.outlier_rm."""
    _check(load().sdfnmpc_sensor_apply(ctx.h, C.byref(opts), int(frame), *_img_dims(img), _ptr(scratch)))


# ---- the plant of a closed loop (csrc/plant.hip) ----
class PlantOpts:
    """sdfnmpc_plant_opts with its per-instance mismatch arrays (host arrays are uploaded once per context, at
    the first call that uses them; device arrays are used in place).  Nothing is checked here: the C entry
    points refuse bad options."""

    def __init__(self, kind, gamma, roll, pitch, wz, g, tau_roll, tau_pitch, dt, substeps=1, acc_dist=None,
                 gamma_scale=None):
        self.kind, self.dt, self.substeps = int(kind), float(dt), int(substeps)
        self.gamma, self.roll, self.pitch, self.wz, self.g = (float(v) for v in (gamma, roll, pitch, wz, g))
        self.tau_roll, self.tau_pitch = float(tau_roll), float(tau_pitch)
        self.acc_dist, self.gamma_scale = acc_dist, gamma_scale
        self._dev = {}

    def _array(self, ctx: "Context", name: str, B: int, cols):
        a = getattr(self, name)
        if a is None:
            return None
        if hasattr(a, "data_ptr"):
            if np.dtype(str(a.dtype).replace("torch.", "")) != np.float64:
                raise TypeError(f"device {name} must be float64, got {a.dtype}")
            return sync_producer(a)
        key = (id(ctx), name, B)
        if key not in self._dev:
            h = np.broadcast_to(np.asarray(a, dtype=np.float64), (B,) + cols)
            self._dev[key] = DeviceArray.from_numpy(ctx, h)
        return self._dev[key]

    def c(self, ctx: "Context", B: int) -> PlantOptsC:
        """The C struct for B instances on a context (the object keeps the device arrays it names alive)."""
        return PlantOptsC(self.kind, self.gamma, self.roll, self.pitch, self.wz, self.g, self.tau_roll, self.tau_pitch,
                          self.dt, self.substeps, _ptr(self._array(ctx, "acc_dist", B, (3,))),
                          _ptr(self._array(ctx, "gamma_scale", B, ())))


def plant_opts(cfg, model=None, dt=None, substeps=1, acc_dist=None, gamma_scale=None) -> PlantOpts:
    """The plant of a config: model 'att' / 'att_tau' (None: cfg.mpc.model, the controller's own), control period
    dt in seconds (required), RK4 substeps per period, and the optional per-instance mismatch -- acc_dist [B][3],
    a constant world-frame acceleration, and gamma_scale [B], a factor on the thrust input (host or device
    fp64 arrays; a host array broadcasts over the batch)."""
    if dt is None:
        raise ValueError("plant_opts: dt (the control period) is required")
    name = str(cfg.mpc.get("model", "att")) if model is None else str(model)
    if name not in MODEL_KINDS:
        raise ValueError(f"plant model '{name}': only {sorted(MODEL_KINDS)} are built")
    lim = cfg.robot.limits
    return PlantOpts(MODEL_KINDS[name], lim.gamma, lim.roll, lim.pitch, lim.wz, 9.81, TAU_ROLL, TAU_PITCH, dt, substeps,
                     acc_dist, gamma_scale)


def plant_step(ctx: "Context", opts: PlantOpts, B: int, x, u, x_next):
    """Enqueue sdfnmpc_plant_step: x_next [B][10] = plant(x [B][10], u [B][4]), device fp64 arrays; x_next may
    be x."""
    o = opts.c(ctx, B)
    _check(load().sdfnmpc_plant_step(ctx.h, C.byref(o), int(B), _ptr(x), _ptr(u), _ptr(x_next)))


class DeviceArray:
    """A device buffer on a context, with numpy-style shape / dtype (the tensor-free way to hand device
    inputs to the entry points).  ``data_ptr()`` makes it usable wherever a torch tensor is accepted."""

    def __init__(self, ctx: Context, shape, dtype=np.float64):
        self.ctx, self.shape, self.dtype = ctx, tuple(int(v) for v in shape), np.dtype(dtype)
        self.nbytes = int(np.prod(self.shape, dtype=np.int64)) * self.dtype.itemsize
        p = C.c_void_p()
        _check(load().sdfnmpc_dev_alloc(ctx.h, self.nbytes, C.byref(p)))
        self.ptr = p.value

    @classmethod
    def from_numpy(cls, ctx: Context, a, dtype=None):
        a = np.ascontiguousarray(a, dtype=dtype)
        d = cls(ctx, a.shape, a.dtype)
        d.upload(a)
        return d

    def data_ptr(self) -> int:
        return self.ptr

    def upload(self, a):
        a = np.ascontiguousarray(a, dtype=self.dtype)
        if a.nbytes != self.nbytes:
            raise ValueError(f"upload of {a.nbytes} bytes into a {self.nbytes}-byte device array")
        _check(load().sdfnmpc_memcpy(self.ctx.h, self.ptr, a.ctypes.data, self.nbytes, 1))

    def numpy(self) -> np.ndarray:
        out = np.empty(self.shape, self.dtype)
        _check(load().sdfnmpc_memcpy(self.ctx.h, out.ctypes.data, self.ptr, self.nbytes, 2))
        return out

    def close(self):
        if getattr(self, "ptr", None):
            load().sdfnmpc_dev_free(self.ctx.h, self.ptr)
            self.ptr = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class FieldView:
    """A solver field's device memory (borrowed: owned by the Solver) -- data_ptr() / shape for the
    lower-level entry points that write it in place (sdfnmpc_pack_refs, sdfnmpc_vae_encode)."""

    def __init__(self, ptr: int, shape, dtype, ctx: "Context" = None):
        self.ptr, self.shape, self.dtype, self.ctx = ptr, tuple(shape), np.dtype(dtype), ctx

    def data_ptr(self) -> int:
        return self.ptr

    @property
    def device(self) -> int:
        if self.ctx is None:
            raise SdfnmpcError("FieldView without a context: its device is unknown")
        return int(self.ctx.device)

    def numpy(self) -> np.ndarray:
        """Host copy (synchronous, ordered on the owning context's stream)."""
        if self.ctx is None:
            raise SdfnmpcError("FieldView without a context cannot be downloaded")
        out = np.empty(self.shape, self.dtype)
        _check(load().sdfnmpc_memcpy(self.ctx.h, out.ctypes.data, self.ptr, out.nbytes, 2))
        return out


def _vehicle_fields(vehicle):
    """The trailing fields of sdfnmpc_rollout_args: (handle, frame0, xhat_log, uapp_log[, omega_log, rotor_log]) or
    None."""
    if vehicle is None:
        return None, 0, None, None, None, None
    h, frame0, xhat_log, uapp_log, *body = tuple(vehicle) + (None, None)
    return h, int(frame0), _ptr(xhat_log), _ptr(uapp_log), _ptr(body[0]), _ptr(body[1])


def _sensor_args(sensor):
    """The (sensor options, scratch) pair the sensing rollouts end with, from (SensorOptsC, scratch or None) or None."""
    return (None, None) if sensor is None else (C.byref(sensor[0]), _ptr(sensor[1]))


class Solver:
    """sdfnmpc_solver: B instances' SQP-RTI workspace on one context, driven with host arrays."""

    INT_FIELDS = ("status", "iters")

    def __init__(self, ctx: Context, net, model: QuadModelC, qp: QpOptsC, B: int, N: int, np_: int, ny: int,
                 dt, latent_mode: int = 0):
        """net may be None when the constraint set and the cost never read the SDF (model.Quad.need_sdf)."""
        self.ctx, self.net, self.B, self.N, self.np, self.ny = ctx, net, int(B), int(N), int(np_), int(ny)
        self._dt = np.ascontiguousarray(dt, dtype=np.float64)
        o = SolverOptsC(self.B, self.N, self.np, self.ny, int(latent_mode),
                        self._dt.ctypes.data_as(C.POINTER(C.c_double)), model, qp)
        h = C.c_void_p()
        _check(load().sdfnmpc_solver_create(ctx.h, None if net is None else net.h, C.byref(o), C.byref(h)))
        self.h = h
        self._shapes = {}
        self.u0 = np.zeros((self.B, 4))
        self.status = np.zeros(self.B, np.int32)
        self.iters = np.zeros(self.B, np.int32)

    def shape(self, name: str):
        shp = self._shapes.get(name)  # fixed at creation: cached (the per-step upload path asks for it)
        if shp is None:
            nodes, width = C.c_int(), C.c_int()
            _check(load().sdfnmpc_solver_field(self.h, name.encode(), None, C.byref(nodes), C.byref(width)))
            shp = self._shapes[name] = (self.B, nodes.value, width.value)
        return shp

    def field(self, name: str) -> FieldView:
        p, nodes, width = C.c_void_p(), C.c_int(), C.c_int()
        _check(load().sdfnmpc_solver_field(self.h, name.encode(), C.byref(p), C.byref(nodes), C.byref(width)))
        return FieldView(p.value, (self.B, nodes.value, width.value), np.int32 if name in self.INT_FIELDS else np.float64,
                         self.ctx)

    def upload(self, name: str, host, col0: int = 0, ncol=None, mask=None):
        """host: the full [B][nodes][width] mirror (or anything broadcastable to it); mask [B][nodes] of rows."""
        shp = self.shape(name)
        a = np.ascontiguousarray(np.broadcast_to(np.asarray(host, dtype=np.float64), shp))
        ncol = shp[2] - col0 if ncol is None else int(ncol)
        m = None
        if mask is not None:
            m = np.ascontiguousarray(np.broadcast_to(np.asarray(mask, dtype=bool), shp[:2]), dtype=np.uint8)
            if not m.any():
                return
        _check(load().sdfnmpc_solver_upload(self.h, name.encode(), int(col0), ncol,
                                             None if m is None else m.ctypes.data, a.ctypes.data))

    def download(self, name: str) -> np.ndarray:
        shp = self.shape(name)
        out = np.empty(shp, np.int32 if name in self.INT_FIELDS else np.float64)
        _check(load().sdfnmpc_solver_download(self.h, name.encode(), out.ctypes.data))
        return out

    def init(self, x0, u_init):
        x0 = np.ascontiguousarray(np.broadcast_to(np.asarray(x0, dtype=np.float64), (self.B, 10)))
        u = np.ascontiguousarray(u_init, dtype=np.float64)
        _check(load().sdfnmpc_solver_init(self.h, x0.ctypes.data, u.ctypes.data))

    def shift(self, k: int):
        _check(load().sdfnmpc_solver_shift(self.h, int(k)))

    def step(self):
        _check(load().sdfnmpc_solver_step(self.h))

    def rollout(self, steps: int, plant: PlantOpts, x_log, u_log, status_log=None, iters_log=None, pts_log=None,
                shift: int = 0, ref: RefOptsC = None, wp_p=None, wp_q=None, vw=None, wrow=None, n_wp: int = 0,
                perceive: "PerceiveArgsC" = None, scene_clock=None, sensor=None, vehicle=None):
        """Enqueue sdfnmpc_solver_rollout: `steps` closed-loop steps (references from x0 when ref is given,
        shift, RTI step, plant) from the x0 field, logged into the device arrays x_log [B][K+1][10], u_log
        [B][K][4], status_log / iters_log [B][K] int32 and pts_log [B][K+1][3] float32.  Asynchronous: `wait`
        finishes it (the arrays are kept alive until then).  perceive: a PerceiveArgsC -- a new image, latent and
        pose before every `every`-th step (sdfnmpc_solver_rollout_perceive); the caller keeps what it names alive.
        scene_clock: (t0, dt) -- the image before step k shows the scene at t0 + (phase + k) dt
        (sdfnmpc_solver_rollout_perceive_at).  sensor: (SensorOptsC, scratch [B][h][w] float32 or None) -- the
        degradation of every new image before it is encoded (sdfnmpc_solver_rollout_perceive_sensor).  vehicle:
        (handle, frame0, xhat_log [B][K+1][10] or None, uapp_log [B][K][4] or None[, omega_log [B][K+1][3] or None,
        rotor_log [B][K+1][4] or None]) -- the vehicle model whose plant call replaces the plant's
        (sdfnmpc_rollout_args.vehicle), after sdfnmpc_vehicle_begin on the x0 field; the last two for a rigid body."""
        a = self._rollout_args(steps, plant, x_log, u_log, status_log, iters_log, pts_log, shift, ref, wp_p, wp_q, vw,
                               wrow, n_wp, vehicle, perceive, sensor)
        if sensor is not None:
            t0, dt = (0.0, 0.0) if scene_clock is None else scene_clock
            _check(load().sdfnmpc_solver_rollout_perceive_sensor(
                self.h, a, None if perceive is None else C.byref(perceive), float(t0), float(dt), *_sensor_args(sensor)))
        elif perceive is None:
            _check(load().sdfnmpc_solver_rollout(self.h, a))
        elif scene_clock is None:
            _check(load().sdfnmpc_solver_rollout_perceive(self.h, a, C.byref(perceive)))
        else:
            _check(load().sdfnmpc_solver_rollout_perceive_at(self.h, a, C.byref(perceive),
                                                             float(scene_clock[0]), float(scene_clock[1])))

    def _rollout_args(self, steps, plant, x_log, u_log, status_log, iters_log, pts_log, shift, ref, wp_p, wp_q, vw, wrow,
                      n_wp, vehicle, *keep):
        """The sdfnmpc_rollout_args block every rollout method passes, by reference; it, what it names and ``keep``
        (what the method's own arguments name) stay alive until ``wait``."""
        a = RolloutArgsC(int(steps), int(shift), None if ref is None else C.pointer(ref), _ptr(wp_p), _ptr(wp_q),
                         _ptr(vw), _ptr(wrow), int(n_wp), plant.c(self.ctx, self.B), _ptr(x_log), _ptr(u_log),
                         _ptr(status_log), _ptr(iters_log), _ptr(pts_log), *_vehicle_fields(vehicle))
        self._rollout_keep = (vehicle, a, ref, plant, wp_p, wp_q, vw, wrow, x_log, u_log, status_log, iters_log,
                              pts_log) + keep
        return C.byref(a)

    def set_sdf_scene(self, scene_h, scene_of=None, max_df: float = 1.0, predict: bool = False):
        """sdfnmpc_solver_set_sdf_scene: the scene's exact distance instead of the network from the next step on;
        scene_h None returns to the network.  scene_of: a device int32 [B] array, kept alive here."""
        _check(load().sdfnmpc_solver_set_sdf_scene(self.h, scene_h, _ptr(scene_of), float(max_df), int(bool(predict))))
        self._sdf_scene_keep = (scene_h, scene_of)
        self._sdf_image_keep = None  # setting either source replaces the other

    def set_scene_time(self, t: float):
        _check(load().sdfnmpc_solver_set_scene_time(self.h, float(t)))

    def rollout_scene_sdf(self, steps: int, plant: PlantOpts, x_log, u_log, pose: "PoseRefreshArgsC" = None, phase: int = 0,
                          t0: float = 0.0, dt: float = 0.0, status_log=None, iters_log=None, pts_log=None, shift: int = 0,
                          ref: RefOptsC = None, wp_p=None, wp_q=None, vw=None, wrow=None, n_wp: int = 0, vehicle=None):
        """Enqueue sdfnmpc_solver_rollout_scene_sdf: `rollout` for a solver with a scene source -- before step k the
        scene time t0 + (phase + k) dt, and with pose (a PoseRefreshArgsC) the camera pose of p refreshed from the
        plant state before every `every`-th step."""
        a = self._rollout_args(steps, plant, x_log, u_log, status_log, iters_log, pts_log, shift, ref, wp_p, wp_q, vw,
                               wrow, n_wp, vehicle, pose)
        _check(load().sdfnmpc_solver_rollout_scene_sdf(self.h, a, None if pose is None else C.byref(pose),
                                                       int(phase), float(t0), float(dt)))

    def set_sdf_image(self, opts: "ImgSdfOptsC" = None, keep=()):
        """sdfnmpc_solver_set_sdf_image: the field of a camera image instead of the network from the next step on; None
        returns to the network.  keep: the device arrays the options name, kept alive here while they are the source."""
        _check(load().sdfnmpc_solver_set_sdf_image(self.h, None if opts is None else C.byref(opts)))
        self._sdf_image_keep = (opts, keep)
        self._sdf_scene_keep = None

    def rollout_image_sdf(self, steps: int, plant: PlantOpts, x_log, u_log, perceive: "PerceiveArgsC" = None,
                          t0: float = 0.0, dt: float = 0.0, sensor=None, status_log=None, iters_log=None, pts_log=None,
                          shift: int = 0, ref: RefOptsC = None, wp_p=None, wp_q=None, vw=None, wrow=None, n_wp: int = 0,
                          dec: "VaeDec" = None, vehicle=None):
        """Enqueue sdfnmpc_solver_rollout_image_sdf: `rollout` for a solver with an image source -- with perceive (a
        PerceiveArgsC without an encoder) a new normalised image rendered into the source, degraded by sensor
        ((SensorOptsC, scratch), normalised units), pooled in unsigned mode, and the camera pose of p refreshed, before
        every `every`-th step.  dec: a VaeDec -- sdfnmpc_solver_rollout_image_recon: the image is rendered into
        the camera buffer perceive names, encoded by perceive's encoder, and its reconstruction goes into the source."""
        a = self._rollout_args(steps, plant, x_log, u_log, status_log, iters_log, pts_log, shift, ref, wp_p, wp_q, vw,
                               wrow, n_wp, vehicle, perceive, sensor, dec)
        args = (self.h, a, None if perceive is None else C.byref(perceive), float(t0), float(dt), *_sensor_args(sensor))
        if dec is not None:
            _check(load().sdfnmpc_solver_rollout_image_recon(*args, dec.h))
        else:
            _check(load().sdfnmpc_solver_rollout_image_sdf(*args))

    def wait(self):
        _check(load().sdfnmpc_solver_wait(self.h, self.u0.ctypes.data, self.status.ctypes.data, self.iters.ctypes.data))
        self._rollout_keep = None  # the stream has drained: a rollout's arrays may go
        return self.u0

    def close(self):
        if getattr(self, "h", None):
            load().sdfnmpc_solver_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass
