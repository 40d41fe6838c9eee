"""Loader for libgtsfm_hip.so, the gfx950 C-ABI library behind every gtsfm_amd plugin.

There is no fallback: if the library is missing or cannot be loaded, importing the product path raises.
torch is imported first so that the process has exactly one HIP runtime (torch's bundled libamdhip64.so.7 and
ours share the SONAME, so the loader reuses torch's copy).
"""
from __future__ import annotations

import ctypes
import os
import subprocess
from typing import Optional

import torch  # noqa: F401  (must precede the CDLL load: one HIP runtime per process)

_PKG_DIR = os.path.dirname(os.path.abspath(__file__))
# GTSFM_HIP_LIB: development override (instrumented or experimental builds of the same ABI); unset in production
LIB_PATH = os.environ.get("GTSFM_HIP_LIB") or os.path.join(_PKG_DIR, "_lib", "libgtsfm_hip.so")
CSRC_DIR = os.path.join(_PKG_DIR, "csrc")

_lib: Optional[ctypes.CDLL] = None

c_void_p = ctypes.c_void_p
c_int = ctypes.c_int
c_double = ctypes.c_double
c_float = ctypes.c_float
c_size_t = ctypes.c_size_t
c_uint64 = ctypes.c_uint64
c_longlong = ctypes.c_longlong

# Mirrors include/gtsfm_hip.h
ABI_VERSION = 407  # GTSFM_HIP_ABI_VERSION: lib() refuses a library built for another ABI
GTSFM_OK = 0
GTSFM_ERR_ARG = -1
GTSFM_ERR_HIP = -2
GTSFM_ERR_CAPACITY = -3
GTSFM_MATCH_EXACT_F32 = 0
GTSFM_MATCH_INT_F16 = 1
GTSFM_MATCH_F16_RERANK = 2
GTSFM_MATCH_F16_MAX_DIM = 512  # wider descriptors run the EXACT_F32 kernels under F16_RERANK
GTSFM_SAMPSON_F64 = 0
GTSFM_SAMPSON_F32_VERIFIER = 1
RANSAC_STATUS_OK = 0
RANSAC_STATUS_TOO_FEW = 1
RANSAC_STATUS_NO_MODEL = 2
RANSAC_DEFAULT_SEED = 0x5EED5EED
GTSFM_RANSAC_SCORING_RANSAC = 0
GTSFM_RANSAC_SCORING_MSAC = 1
BA2_STATUS_OK = 0
BA2_STATUS_NO_TRACKS = 1
BA2_STATUS_NONE_VALID = 2
BA2_STATUS_NOT_RUN = 3
GTSFM_VG_MIN_EDGE_ERROR = 0
GTSFM_VG_MEDIAN_EDGE_ERROR = 1
VG_MAX_IMAGES = 8192  # gtsfm_viewgraph_cycle_filter's n_img ceiling
GTSFM_TRI_NO_RANSAC = 0
GTSFM_TRI_RANSAC_SAMPLE_UNIFORM = 1
GTSFM_TRI_RANSAC_SAMPLE_BIASED_BASELINE = 2
GTSFM_TRI_RANSAC_TOPK_BASELINES = 3
GBA_STATUS_OK = 0
GBA_STATUS_NOTHING = 1  # no participating track or no modelled camera: the reference's early return
GBA_STATS_FIELDS = ("initial_error", "final_error", "lm_iterations", "lm_trials", "pcg_iterations", "pcg_cap_hits",
                    "cameras_modelled", "tracks_participating", "tracks_kept", "status")
# gtsfm_global_ba_calib's d_stats: the ten above, then the calibration variables and the largest |f_out - f_in| / f_in
GBA_CALIB_STATS_FIELDS = GBA_STATS_FIELDS + ("calibration_variables", "max_rel_focal_change")
TA_STATUS_OK = 0
TA_STATUS_NOTHING = 1  # no measurement kept
TA_STATUS_NOT_FINITE = 2
TA_MFAS_MAX_NODES = 8000  # GTSFM_TRANSAVG_MFAS_MAX_NODES
TA_STATS_FIELDS = ("initial_error", "final_error", "lm_iterations", "lm_trials", "pcg_iterations", "pcg_cap_hits",
                   "sets_optimised", "factors", "cameras_valid", "status")
RA_STATUS_CERTIFIED = 0
RA_STATUS_NOTHING = 1  # no valid edge
RA_STATUS_UNCERTIFIED = 2  # p_max reached without a certificate; the rotations are still returned
RA_STATUS_NOT_FINITE = 3
RA_STATS_FIELDS = ("initial_cost", "final_cost", "final_p", "min_eigenvalue", "eigen_residual", "lm_iterations",
                   "pcg_iterations", "pcg_cap_hits", "lanczos_steps", "cameras_valid", "edges_used", "status")
BA_INPUT_STATS_FIELDS = ("components", "cameras_kept", "tracks_kept", "measurements_kept", "accepted_tracks",
                         "valid_cameras")
MVS_VIEWS_STATS_FIELDS = ("valid_cameras", "source_views", "cameras_without_depth", "score_terms")
MVS_FUSE_COUNT_FIELDS = ("geometric_pixels", "confidence_pixels", "joint_pixels", "reprojection_errors")
MVS_SCORE_SCALE = 2.0 ** 40  # gtsfm_mvs_select_views' scores are integers in units of 2^-40
GTSFM_D2NET_STAGE_TRUNK = 0  # gtsfm_d2net_stages' last_stage
GTSFM_D2NET_STAGE_DILATED = 1
GTSFM_D2NET_STAGE_DETECT = 2
GTSFM_D2NET_STAGE_DESCRIBE = 3
PATCHMATCHNET_INIT_BINS = 48  # inverse-depth bins of the random initialisation (gtsfm_patchmatchnet_batched)


class PatchmatchNetConfig(ctypes.Structure):
    """gtsfm_patchmatchnet_config; the default is the reference's (the only one the library takes)."""

    _fields_ = [("interval_scale", c_double * 3), ("propagation_range", c_int * 3), ("iterations", c_int * 3),
                ("num_samples", c_int * 3), ("propagate_neighbors", c_int * 3), ("evaluate_neighbors", c_int * 3),
                ("groups", c_int * 3)]

    def __init__(self, interval_scale=(0.005, 0.0125, 0.025), propagation_range=(6, 4, 2), iterations=(1, 2, 2),
                 num_samples=(8, 8, 16), propagate_neighbors=(0, 8, 16), evaluate_neighbors=(9, 9, 9),
                 groups=(4, 8, 8)):
        super().__init__((c_double * 3)(*interval_scale), (c_int * 3)(*propagation_range), (c_int * 3)(*iterations),
                         (c_int * 3)(*num_samples), (c_int * 3)(*propagate_neighbors),
                         (c_int * 3)(*evaluate_neighbors), (c_int * 3)(*groups))


TRI_STATS_FIELDS = ("success", "cheirality_failure", "inliers_underconstrained", "poses_underconstrained",
                    "exceeds_reproj_thresh", "low_triangulation_angle", "inlier_measurements", "hypotheses")

# (name, restype, argtypes) of every symbol declared in include/gtsfm_hip.h
SIGNATURES = {
    "gtsfm_hip_abi_version": (c_int, []),
    "gtsfm_hip_target": (ctypes.c_char_p, []),
    "gtsfm_match_workspace_bytes": (c_size_t, [c_int, c_int, c_int, c_int, c_int]),
    "gtsfm_match_batched": (
        c_int,
        [c_void_p, c_void_p, c_int, c_int, c_int, c_void_p, c_int, c_double, c_int, c_void_p, c_size_t, c_void_p,
         c_void_p, c_void_p],
    ),
    "gtsfm_match_batched_grouped": (
        c_int,
        [c_void_p, c_void_p, c_int, c_int, c_int, c_void_p, c_int, c_void_p, c_int, c_int, c_double, c_int, c_void_p,
         c_size_t, c_void_p, c_void_p, c_void_p],
    ),
    "gtsfm_match_max_group": (c_int, [c_int, c_int]),
    "gtsfm_match_set_kernel_events": (c_int, [c_void_p, c_void_p]),
    "gtsfm_match_rerank_stats": (c_int, [c_void_p, c_size_t, c_int, c_int, c_int, c_int, c_void_p, c_void_p, c_void_p]),
    "gtsfm_ransac_workspace_bytes": (c_size_t, [c_int, c_int]),
    "gtsfm_ransac_E_batched": (
        c_int,
        [c_void_p, c_void_p, c_int, c_int, c_void_p, c_int, c_void_p, c_void_p, c_int, c_double, c_double, c_int, c_int,
         c_uint64, c_int, c_void_p, c_void_p, c_size_t, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p,
         c_void_p, c_void_p],
    ),
    "gtsfm_ransac_F_workspace_bytes": (c_size_t, [c_int, c_int]),
    "gtsfm_ransac_F_batched": (
        c_int,
        [c_void_p, c_void_p, c_int, c_int, c_void_p, c_int, c_void_p, c_void_p, c_int, c_double, c_double, c_int,
         c_uint64, c_int, c_void_p, c_void_p, c_size_t, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p,
         c_void_p, c_void_p, c_void_p],
    ),
    "gtsfm_superpoint_weights_floats": (c_size_t, []),
    "gtsfm_superpoint_workspace_bytes": (c_size_t, [c_int, c_int, c_int, c_int]),
    "gtsfm_superpoint_batched": (
        c_int,
        [c_void_p, c_void_p, c_int, c_int, c_int, c_int, c_void_p, c_int, c_float, c_int, c_int, c_void_p, c_size_t,
         c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p],
    ),
    "gtsfm_d2net_weights_floats": (c_size_t, []),
    "gtsfm_d2net_workspace_bytes": (c_size_t, [c_int, c_int, c_int, c_int]),
    "gtsfm_d2net_batched": (
        c_int,
        [c_void_p, c_int, c_int, c_int, c_int, c_void_p, c_int, c_float, c_float, c_void_p, c_size_t, c_void_p,
         c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p],
    ),
    "gtsfm_d2net_stages": (
        c_int,
        [c_void_p, c_int, c_int, c_int, c_int, c_void_p, c_int, c_float, c_float, c_void_p, c_size_t, c_void_p,
         c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_int, c_void_p],
    ),
    "gtsfm_superglue_weights_floats": (c_size_t, [c_int]),
    "gtsfm_superglue_workspace_bytes": (c_size_t, [c_int, c_int]),
    "gtsfm_superglue_batched": (
        c_int,
        [c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_int, c_int, c_void_p, c_int, c_void_p, c_int, c_int,
         c_float, c_void_p, c_size_t, c_void_p, c_void_p, c_void_p, c_void_p],
    ),
    "gtsfm_superglue_log_assignment": (c_int, [c_void_p, c_size_t, c_int, c_int, c_int, c_void_p, c_void_p]),
    "gtsfm_lightglue_weights_floats": (c_size_t, [c_int]),
    "gtsfm_lightglue_workspace_bytes": (c_size_t, [c_int, c_int]),
    "gtsfm_lightglue_batched": (
        c_int,
        [c_void_p, c_void_p, c_void_p, c_void_p, c_int, c_int, c_void_p, c_int, c_void_p, c_int, c_float, c_float,
         c_void_p, c_size_t, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p],
    ),
    "gtsfm_lightglue_log_assignment": (c_int, [c_void_p, c_size_t, c_int, c_int, c_int, c_void_p, c_void_p]),
    "gtsfm_retrieval_similarity": (c_int, [c_void_p, c_int, c_int, c_int, c_void_p, c_void_p]),
    "gtsfm_retrieval_pairs": (c_int, [c_void_p, c_int, c_int, c_void_p, c_int, ctypes.c_float, c_int, c_void_p, c_void_p,
                                      c_void_p]),
    "gtsfm_netvlad_weights_floats": (c_size_t, []),
    "gtsfm_netvlad_workspace_bytes": (c_size_t, [c_int, c_int, c_int]),
    "gtsfm_netvlad_batched": (
        c_int, [c_void_p, c_int, c_int, c_int, c_int, c_void_p, c_int, c_void_p, c_void_p, c_void_p, c_size_t, c_void_p]),
    "gtsfm_compact_verified": (
        c_int,
        [c_void_p, c_void_p, c_int, c_void_p, c_void_p, c_void_p, c_void_p, c_int, c_int, c_double, c_void_p, c_void_p,
         c_int, c_void_p, c_void_p],
    ),
    "gtsfm_ba2_workspace_bytes": (c_size_t, [c_int, c_int]),
    "gtsfm_ba2_batched": (
        c_int,
        [c_void_p, c_void_p, c_int, c_int, c_void_p, c_int, c_void_p, c_void_p, c_int, c_void_p, c_void_p, c_void_p,
         c_void_p, c_void_p, c_void_p, c_int, c_int, c_double, c_double, c_void_p, c_size_t, c_void_p, c_void_p,
         c_void_p, c_void_p, c_void_p, c_void_p, c_void_p],
    ),
    "gtsfm_sampson_sq_batched": (
        c_int, [c_void_p, c_int, c_void_p, c_void_p, c_void_p, c_int, c_int, c_void_p, c_void_p]),
    "gtsfm_sift_workspace_bytes": (c_size_t, [c_int, c_int, c_int, c_int]),
    "gtsfm_sift_batched": (
        c_int,
        [c_void_p, c_void_p, c_int, c_int, c_int, c_int, c_int, c_void_p, c_size_t, c_void_p, c_void_p, c_void_p,
         c_void_p, c_void_p, c_void_p],
    ),
    "gtsfm_viewgraph_workspace_bytes": (c_size_t, [c_int, c_int]),
    "gtsfm_viewgraph_cycle_filter": (
        c_int,
        [c_void_p, c_void_p, c_void_p, c_int, c_int, c_int, c_double, c_void_p, c_size_t, c_void_p, c_void_p, c_void_p,
         c_void_p, c_void_p],
    ),
    "gtsfm_tracks_workspace_bytes": (c_size_t, [c_int, c_int, c_int, c_longlong]),
    "gtsfm_tracks_from_matches": (
        c_int,
        [c_void_p, c_void_p, c_void_p, c_void_p, c_int, c_longlong, c_void_p, c_void_p, c_int, c_int, c_void_p,
         c_size_t, c_void_p, c_longlong, c_void_p, c_void_p, c_void_p, c_longlong, c_void_p, c_void_p],
    ),
    "gtsfm_triangulate_workspace_bytes": (c_size_t, [c_longlong, c_longlong, c_int]),
    "gtsfm_triangulate_tracks": (
        c_int,
        [c_void_p, c_void_p, c_void_p, c_int, c_void_p, c_longlong, c_void_p, c_longlong, c_void_p, c_void_p, c_void_p,
         c_void_p, c_int, c_int, c_double, c_double, c_int, c_uint64, c_void_p, c_size_t, c_void_p, c_void_p, c_void_p,
         c_void_p, c_void_p, c_void_p, c_void_p, c_longlong, c_void_p],
    ),
    "gtsfm_global_ba_workspace_bytes": (c_size_t, [c_longlong, c_longlong, c_int]),
    "gtsfm_global_ba": (
        c_int,
        [c_void_p, c_void_p, c_void_p, c_int, c_longlong, c_void_p, c_longlong, c_void_p, c_void_p, c_void_p, c_void_p,
         c_void_p, c_void_p, c_void_p, c_int, c_int, c_double, c_double, c_int, c_double, c_int, c_double, c_void_p,
         c_size_t, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p],
    ),
    "gtsfm_global_ba_calib_workspace_bytes": (c_size_t, [c_longlong, c_longlong, c_int]),
    "gtsfm_global_ba_calib": (
        c_int,
        [c_void_p, c_void_p, c_void_p, c_int, c_longlong, c_void_p, c_longlong, c_void_p, c_void_p, c_void_p, c_void_p,
         c_void_p, c_void_p, c_void_p, c_int, c_int, c_double, c_double, c_int, c_double, c_int, c_double, c_int,
         c_double, c_void_p, c_size_t, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p],
    ),
    "gtsfm_transavg_measurements_workspace_bytes": (c_size_t, [c_int, c_longlong, c_longlong, c_int]),
    "gtsfm_transavg_measurements": (
        c_int,
        [c_void_p, c_void_p, c_void_p, c_int, c_void_p, c_void_p, c_int, c_void_p, c_void_p, c_void_p, c_int,
         c_longlong, c_void_p, c_longlong, c_void_p, c_int, c_void_p, c_size_t, c_void_p, c_void_p, c_void_p, c_void_p,
         c_void_p, c_void_p, c_void_p],
    ),
    "gtsfm_transavg_mfas_workspace_bytes": (c_size_t, [c_longlong, c_int, c_int]),
    "gtsfm_transavg_mfas": (
        c_int,
        [c_void_p, c_void_p, c_void_p, c_longlong, c_int, c_void_p, c_int, c_double, c_void_p, c_size_t, c_void_p,
         c_void_p, c_void_p, c_void_p],
    ),
    "gtsfm_transavg_recover_workspace_bytes": (c_size_t, [c_longlong, c_int, c_int]),
    "gtsfm_transavg_recover": (
        c_int,
        [c_void_p, c_void_p, c_void_p, c_longlong, c_int, c_int, c_void_p, c_int, c_double, c_uint64, c_int, c_double,
         c_int, c_void_p, c_size_t, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p],
    ),
    "gtsfm_rotavg_workspace_bytes": (c_size_t, [c_int, c_int, c_int]),
    "gtsfm_rotavg_shonan": (
        c_int,
        [c_void_p, c_void_p, c_void_p, c_void_p, c_int, c_int, c_void_p, c_uint64, c_int, c_int, c_double, c_double,
         c_int, c_double, c_int, c_double, c_int, c_void_p, c_size_t, c_void_p, c_void_p, c_void_p, c_void_p],
    ),
    "gtsfm_assemble_ba_input_workspace_bytes": (c_size_t, [c_longlong, c_int]),
    "gtsfm_assemble_ba_input": (
        c_int,
        [c_void_p, c_void_p, c_longlong, c_void_p, c_longlong, c_void_p, c_void_p, c_void_p, c_int, c_void_p, c_int,
         c_void_p, c_size_t, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p],
    ),
    "gtsfm_mvs_select_views_workspace_bytes": (c_size_t, [c_longlong, c_longlong, c_int]),
    "gtsfm_mvs_select_views": (
        c_int,
        [c_void_p, c_void_p, c_longlong, c_longlong, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_int,
         c_int, c_void_p, c_size_t, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p],
    ),
    "gtsfm_mvs_fuse_depth_workspace_bytes": (c_size_t, [c_int, c_int, c_int]),
    "gtsfm_mvs_fuse_depth": (
        c_int,
        [c_void_p, c_void_p, c_int, c_int, c_int, c_void_p, c_void_p, c_void_p, c_void_p, c_int, c_double, c_double,
         c_double, c_int, c_void_p, c_size_t, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p],
    ),
    "gtsfm_mvs_gather_points_workspace_bytes": (c_size_t, [c_int, c_int, c_int]),
    "gtsfm_mvs_gather_points": (
        c_int,
        [c_void_p, c_void_p, c_int, c_int, c_int, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_int, c_int, c_int,
         c_longlong, c_void_p, c_size_t, c_void_p, c_void_p, c_void_p, c_void_p],
    ),
    "gtsfm_mvs_voxel_stats_workspace_bytes": (c_size_t, [c_longlong]),
    "gtsfm_mvs_voxel_stats": (c_int, [c_void_p, c_longlong, c_void_p, c_size_t, c_void_p, c_void_p]),
    "gtsfm_mvs_voxel_keys": (c_int, [c_void_p, c_longlong, c_void_p, c_double, c_void_p, c_void_p]),
    "gtsfm_mvs_voxel_downsample_workspace_bytes": (c_size_t, [c_longlong]),
    "gtsfm_mvs_voxel_downsample": (
        c_int,
        [c_void_p, c_void_p, c_void_p, c_void_p, c_longlong, c_void_p, c_size_t, c_void_p, c_void_p, c_void_p, c_void_p,
         c_void_p, c_void_p],
    ),
    "gtsfm_patchmatchnet_set_phase_events": (c_int, [c_void_p]),
    "gtsfm_patchmatchnet_weights_floats": (c_size_t, []),
    "gtsfm_patchmatchnet_workspace_bytes": (c_size_t, [c_int, c_int, c_int, c_int]),
    "gtsfm_patchmatchnet_batched": (
        c_int,
        [c_void_p, c_int, c_int, c_int, c_void_p, c_void_p, c_void_p, c_void_p, c_int, c_void_p, c_void_p, c_void_p,
         c_void_p, c_void_p, c_size_t, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p],
    ),
}


class NativeError(RuntimeError):
    pass


def build(jobs: int = 8) -> str:
    """Compiles every HIP source under gtsfm_amd/csrc for gfx950 into gtsfm_amd/_lib/libgtsfm_hip.so."""
    subprocess.run(["make", "-s", f"-j{jobs}", "-C", CSRC_DIR], check=True)
    return LIB_PATH


def lib() -> ctypes.CDLL:
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise NativeError(
                f"{LIB_PATH} is missing: run `python -c 'import __graft_entry__ as g; g.build()'` "
                "(the gtsfm_amd product path has no CPU fallback)"
            )
        handle = ctypes.CDLL(LIB_PATH)
        ver = getattr(handle, "gtsfm_hip_abi_version", None)
        if ver is None:
            raise NativeError(f"{LIB_PATH} does not export gtsfm_hip_abi_version")
        ver.restype, ver.argtypes = c_int, []
        if ver() != ABI_VERSION:
            raise NativeError(f"{LIB_PATH} implements ABI {ver()}, this binding expects {ABI_VERSION}: rebuild it")
        for name, (restype, argtypes) in SIGNATURES.items():
            fn = getattr(handle, name, None)
            if fn is None:
                raise NativeError(f"{LIB_PATH} does not export {name}")
            fn.restype = restype
            fn.argtypes = argtypes
        _lib = handle
    return _lib


def check(rc: int, what: str) -> None:
    if rc != GTSFM_OK:
        raise NativeError(f"{what} failed with status {rc}")


def stream_handle(stream: Optional["torch.cuda.Stream"] = None) -> int:
    s = stream if stream is not None else torch.cuda.current_stream()
    return int(s.cuda_stream)


def require_gpu() -> None:
    if not torch.cuda.is_available():
        raise NativeError("gtsfm_amd needs an MI355X (gfx950) GPU: torch.cuda.is_available() is False")
