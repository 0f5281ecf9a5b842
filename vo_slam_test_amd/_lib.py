"""ctypes binding of libvo_hip.so (include/vo_hip.h).  No CPU fallback: loading or calling
without the HIP library / a gfx950 device raises."""
from __future__ import annotations

import ctypes as C
import os
import pathlib

import numpy as np

PKG = pathlib.Path(__file__).resolve().parent
SO = PKG / "libvo_hip.so"

KP_DTYPE = np.dtype([("x", "<f4"), ("y", "<f4"), ("size", "<f4"), ("angle", "<f4"),
                     ("response", "<f4"), ("octave", "<i4"), ("class_id", "<i4")])


class VoError(RuntimeError):
    pass


class LmSummary(C.Structure):
    _fields_ = [("iterations", C.c_int32), ("accepted", C.c_int32), ("termination", C.c_int32),
                ("reserved", C.c_int32), ("initial_cost", C.c_double), ("final_cost", C.c_double),
                ("final_radius", C.c_double)]


class FrameView(C.Structure):
    _fields_ = [("n", C.c_int32), ("x", C.c_void_p), ("y", C.c_void_p), ("octave", C.c_void_p),
                ("angle", C.c_void_p), ("uright", C.c_void_p), ("desc", C.c_void_p),
                ("xmin", C.c_float), ("ymin", C.c_float), ("xmax", C.c_float), ("ymax", C.c_float)]


_lib = None

# every symbol include/vo_hip.h declares (tests check the .so exports all of them)
SYMBOLS = [
    "vo_last_error", "vo_device_count", "vo_version", "vo_release_thread_scratch",
    "vo_orb_create", "vo_orb_destroy", "vo_orb_set_stream", "vo_orb_set_option", "vo_orb_set_stage_hook", "vo_orb_debug_level_pass", "vo_orb_levels", "vo_orb_scale_factor",
    "vo_orb_scale_factors", "vo_orb_features_per_level", "vo_orb_max_keypoints", "vo_orb_extract",
    "vo_orb_extract_batch_dev", "vo_orb_sync", "vo_orb_get_level", "vo_orb_get_candidates",
    "vo_orb_get_level_counts", "vo_orb_set_timing", "vo_orb_get_timing",
    "vo_hamming_matrix_dev", "vo_hamming_matrix_batch_dev", "vo_hamming_matrix", "vo_median_descriptor",
    "vo_frames_create", "vo_frames_destroy", "vo_frames_capacity", "vo_frames_set_camera", "vo_frames_build_dev",
    "vo_frames_upload", "vo_frames_construct", "vo_frames_download", "vo_frames_features_in_area", "vo_match_guided_dev", "vo_match_guided_status",
    "vo_vocab_load", "vo_bow_score", "vo_pnp_ransac", "vo_pnp_ransac_dev", "vo_pnp_workspace_bytes", "vo_sim3_ransac_eval", "vo_triangulate", "vo_rgb_to_gray", "vo_rgb_to_gray_dev",
    "vo_dataset_open", "vo_dataset_size", "vo_dataset_entry", "vo_dataset_close", "vo_png_info", "vo_png_read",
    "vo_trajectory_write", "vo_tracking_time_stats",
    "vo_track_project_dev", "vo_track_scatter_dev", "vo_track_gather_dev", "vo_track_scatter_gather_dev", "vo_pose_only_solve_ranges_dev",
    "vo_tracker_track_first", "vo_tracker_track_first_dev", "vo_tracker_track_local_map", "vo_tracker_set_ref_keyframe",
    "vo_tracker_track_ref_keyframe", "vo_tracker_track_ref_keyframe_dev",
    "vo_tracker_set_reloc_candidates", "vo_tracker_relocalize", "vo_tracker_relocalize_dev",
    "vo_kfstore_create", "vo_kfstore_destroy", "vo_kfstore_set_stream", "vo_kfstore_size", "vo_kfstore_insert", "vo_kfstore_insert_dev",
    "vo_kfstore_set_bad", "vo_kfstore_update_points", "vo_tracker_relocalize_store", "vo_tracker_relocalize_store_dev",
    "vo_tracker_relocalize_db", "vo_tracker_relocalize_db_dev", "vo_tracker_get_reloc_timing",
    "vo_tracker_track_ref_keyframe_store", "vo_tracker_track_ref_keyframe_store_dev", "vo_tracker_set_local_map_ids",
    "vo_tracker_set_last_frame_ids", "vo_tracker_set_last_pose", "vo_tracker_end_frame", "vo_tracker_begin_frame",
    "vo_tracker_handover_arrays",
    "vo_tracker_point_stats", "vo_tracker_point_stats_arrays", "vo_tracker_record_ref_pose", "vo_tracker_refresh_last_pose",
    "vo_tracker_end_frame_store", "vo_tracker_point_stats_store",
    "vo_kfstore_set_graph", "vo_kfstore_set_graph_batch", "vo_kfstore_set_normals", "vo_tracker_build_local_map",
    "vo_kfstore_enable_connections", "vo_kfstore_update_connections", "vo_kfstore_update_connections_dev",
    "vo_kfstore_connections_status", "vo_kfstore_get_connections",
    "vo_kfstore_enable_culling", "vo_kfstore_set_keypoints", "vo_kfstore_set_keypoints_dev", "vo_kfstore_set_erase_lock",
    "vo_kfstore_cull_keyframes", "vo_kfstore_erase_keyframe", "vo_kfstore_cull_result", "vo_kfstore_cull_state", "vo_kfstore_get_flags",
    "vo_kfstore_enable_mapping", "vo_kfstore_set_pose", "vo_kfstore_set_pose_dev", "vo_kfstore_set_keypoint_xy", "vo_kfstore_set_keypoint_xy_dev",
    "vo_kfstore_next_point_id", "vo_kfstore_create_map_points", "vo_kfstore_new_points_result", "vo_kfstore_get_points",
    "vo_kfstore_enable_local_ba", "vo_kfstore_set_point_refs", "vo_kfstore_set_point_refs_dev", "vo_kfstore_get_point_refs",
    "vo_kfstore_local_ba_window", "vo_kfstore_local_ba_window_result", "vo_kfstore_local_ba_apply", "vo_kfstore_refresh_points",
    "vo_kfstore_get_pose", "vo_kfstore_local_ba",
    "vo_kfstore_enable_point_upkeep", "vo_kfstore_compute_descriptors", "vo_kfstore_compute_descriptors_dev",
    "vo_kfstore_process_new_keyframe", "vo_kfstore_add_point_stats", "vo_kfstore_add_point_stats_dev", "vo_kfstore_cull_map_points",
    "vo_kfstore_recent_points", "vo_kfstore_upkeep_result",
    "vo_kfstore_enable_fuse", "vo_kfstore_fuse_map_points", "vo_kfstore_fuse_map_points_dev", "vo_kfstore_search_in_neighbors",
    "vo_kfstore_fuse_result",
    "vo_kfstore_enable_loop", "vo_kfstore_compute_sim3", "vo_kfstore_compute_sim3_dev", "vo_kfstore_compute_sim3_continue",
    "vo_kfstore_loop_result", "vo_kfstore_loop_solver_inputs", "vo_kfstore_loop_ransac_max_iters",
    "vo_kfstore_enable_pose_graph", "vo_kfstore_add_loop_edge", "vo_kfstore_get_loop_edges", "vo_kfstore_pose_graph_window",
    "vo_kfstore_pose_graph_window_dev", "vo_kfstore_pose_graph_window_result", "vo_kfstore_pose_graph_apply", "vo_kfstore_pose_graph",
    "vo_kfstore_enable_keyframe_create", "vo_kfstore_create_keyframe", "vo_kfstore_create_keyframe_dev",
    "vo_kfstore_create_keyframe_from_frames", "vo_kfstore_keyframe_result", "vo_kfstore_get_features",
    "vo_kfstore_keyframe_need_stats", "vo_kfstore_keyframe_need_stats_dev",
    "vo_kfstore_enable_loop_fuse", "vo_kfstore_search_and_fuse", "vo_kfstore_search_and_fuse_dev", "vo_kfstore_search_and_fuse_loop",
    "vo_kfstore_loop_fuse_result",
    "vo_kfstore_enable_loop_correct", "vo_kfstore_propagate_loop", "vo_kfstore_propagate_loop_dev", "vo_kfstore_propagate_loop_sim3",
    "vo_kfstore_loop_connections", "vo_kfstore_loop_correct_result", "vo_kfstore_loop_correct_arrays",
    "vo_kfstore_enable_loop_merge", "vo_kfstore_merge_loop_matches", "vo_kfstore_merge_loop_matches_dev",
    "vo_kfstore_merge_loop_matches_loop", "vo_kfstore_loop_merge_result", "vo_kfstore_correct_loop",
    "vo_kfstore_enable_detect_loop", "vo_kfstore_detect_loop", "vo_kfstore_detect_loop_result", "vo_kfstore_detect_loop_groups",
    "vo_kfstore_compute_sim3_detected", "vo_kfstore_compute_sim3_detected_dev", "vo_kfstore_release_loop_locks",
    "vo_kfstore_loop_locks_result", "vo_kfstore_set_last_loop_keyframe", "vo_kfstore_get_last_loop_keyframe",
    "vo_kfstore_loop_closing_step", "vo_kfdb_get_neighbors",
    "vo_tracker_create", "vo_tracker_destroy", "vo_tracker_info", "vo_tracker_extractor", "vo_tracker_frames",
    "vo_tracker_stream", "vo_tracker_set_last_frame", "vo_tracker_set_local_map", "vo_tracker_track_dev", "vo_tracker_track",
    "vo_tracker_results", "vo_tracker_get", "vo_tracker_sync", "vo_tracker_set_timing", "vo_tracker_get_timing",
    "vo_match_frame_projection", "vo_match_local_map", "vo_match_frame_keyframe", "vo_match_bow",
    "vo_match_triangulation", "vo_match_bow_batch", "vo_match_triangulation_batch", "vo_match_fuse", "vo_match_area_best", "vo_match_sim3_projection",
    "vo_match_sim3_mutual", "vo_vocab_create", "vo_vocab_destroy", "vo_bow_transform",
    "vo_vocab_train", "vo_vocab_train_dev", "vo_vocab_tree", "vo_vocab_save",
    "vo_bow_vector", "vo_bow_vector_dev", "vo_kfdb_create", "vo_kfdb_destroy", "vo_kfdb_set_stream", "vo_kfdb_size", "vo_kfdb_set_option",
    "vo_kfdb_insert", "vo_kfdb_insert_dev", "vo_kfdb_set_neighbors", "vo_kfdb_set_neighbors_batch", "vo_kfdb_query_reloc", "vo_kfdb_query_reloc_dev",
    "vo_kfdb_query_loop", "vo_kfdb_query_loop_dev",
    "vo_pose_only_solve", "vo_sim3_solve", "vo_pose_graph_solve", "vo_sim3_reanchor_points", "vo_chol_solve", "vo_chol_solve_split", "vo_pose_only_solve_dev",
    "vo_ba_create", "vo_ba_reset", "vo_ba_destroy", "vo_ba_set_stream", "vo_ba_set_shard", "vo_ba_set_option", "vo_set_option", "vo_ba_set_allreduce", "vo_ba_set_state",
    "vo_ba_get_state", "vo_ba_n_free_cams", "vo_ba_local_ba", "vo_ba_local_ba_enqueue",
    "vo_ba_local_ba_finish", "vo_ba_solve", "vo_ba_lm_begin",
    "vo_ba_linearize", "vo_ba_step", "vo_ba_update", "vo_ba_lm_end", "vo_ba_reduced_system",
    "vo_ba_reduced_cost", "vo_ba_set_reduce_buffers", "vo_ba_classify",
    "vo_ba_lm_begin_inliers", "vo_ba_get_edge_outliers", "vo_ba_debug_schur", "vo_ba_debug_stamps", "vo_ba_debug_order", "vo_se3_exp", "vo_se3_log",
]


def lib():
    global _lib
    if _lib is not None:
        return _lib
    so = pathlib.Path(os.environ.get("VO_HIP_LIB", SO))  # alternative install location / developer builds
    if not so.exists():
        raise VoError(f"{so} is missing: run `python -m vo_slam_test_amd.build` (hipcc, gfx950). "
                      "There is no CPU fallback.")
    # PyTorch-ROCm bundles its own libamdhip64.so.7 / libhsa-runtime64; two HIP runtimes in one
    # process cannot both open the GPU.  Importing torch first makes the loader resolve our
    # NEEDED libamdhip64.so.7 to the copy torch already mapped (same SONAME).  Without torch the
    # library falls back to its RUNPATH (/opt/rocm/lib).
    try:
        import torch  # noqa: F401
    except Exception:  # pragma: no cover - torch is plumbing only
        pass
    L = C.CDLL(str(so))
    L.vo_last_error.restype = C.c_char_p
    L.vo_version.restype = C.c_char_p
    L.vo_release_thread_scratch.restype = C.c_size_t
    L.vo_orb_scale_factor.restype = C.c_float
    L.vo_pnp_workspace_bytes.restype = C.c_size_t
    for name in SYMBOLS:
        f = getattr(L, name, None)
        if f is not None and f.restype is C.c_int:
            f.restype = C.c_int
    L.vo_orb_destroy.restype = None
    if hasattr(L, "vo_dataset_close"):
        L.vo_dataset_close.restype = None
    if hasattr(L, "vo_frames_destroy"):
        L.vo_frames_destroy.restype = None
    if hasattr(L, "vo_ba_destroy"):
        L.vo_ba_destroy.restype = None
    if hasattr(L, "vo_vocab_destroy"):
        L.vo_vocab_destroy.restype = None
    if hasattr(L, "vo_kfdb_destroy"):
        L.vo_kfdb_destroy.restype = None
    if hasattr(L, "vo_kfstore_destroy"):
        L.vo_kfstore_destroy.restype = None
    if hasattr(L, "vo_tracker_destroy"):
        L.vo_tracker_destroy.restype = None
        L.vo_tracker_extractor.restype = C.c_void_p
        L.vo_tracker_frames.restype = C.c_void_p
        L.vo_tracker_stream.restype = C.c_void_p
    _lib = L
    return L


def check(rc: int, what: str = ""):
    if rc != 0:
        raise VoError(f"{what} failed with status {rc}: {lib().vo_last_error().decode()}")


def _p(a):
    """pointer of a numpy array / torch tensor / int / None as c_void_p"""
    if a is None:
        return C.c_void_p(0)
    if isinstance(a, int):
        return C.c_void_p(a)
    if isinstance(a, np.ndarray):
        return C.c_void_p(a.ctypes.data)
    if hasattr(a, "data_ptr"):
        return C.c_void_p(a.data_ptr())
    raise TypeError(type(a))


def _need_tensor(t, dtype, numel, what):
    """a device tensor handed through as a raw pointer: its element type, contiguity and (where fixed) its length"""
    if str(t.dtype) != "torch." + dtype or not t.is_contiguous() or (numel is not None and t.numel() != numel):
        raise VoError(f"{what}: a contiguous {dtype} tensor{'' if numel is None else f' of {numel} elements'} is required, "
                      f"got {t.dtype} with shape {tuple(t.shape)}")


class OrbExtractor:
    """Mirror of ORB_SLAM2::ORBextractor (reference include/myslam/ORBextractor.h:45-111)."""

    def __init__(self, nfeatures=1000, scaleFactor=1.2, nlevels=8, iniThFAST=20, minThFAST=7):
        self._h = C.c_void_p()
        check(lib().vo_orb_create(C.byref(self._h), int(nfeatures), C.c_float(scaleFactor), int(nlevels),
                                  int(iniThFAST), int(minThFAST)), "vo_orb_create")
        self.nlevels = nlevels

    @classmethod
    def borrowed(cls, handle, nlevels=8):
        """a view of an extractor another object owns (vo_tracker_extractor): never destroyed from here"""
        o = cls.__new__(cls)
        o._h, o.nlevels, o._borrowed = handle, nlevels, True
        return o

    def close(self):
        if getattr(self, "_borrowed", False):
            self._h = C.c_void_p()
        if getattr(self, "_h", None) and self._h.value and _lib is not None:   # (_lib is gone at interpreter exit)
            _lib.vo_orb_destroy(self._h)
            self._h = C.c_void_p()

    __del__ = close

    def GetLevels(self):
        return lib().vo_orb_levels(self._h)

    def GetScaleFactor(self):
        return lib().vo_orb_scale_factor(self._h)

    def GetScaleFactors(self):
        s = np.zeros(self.nlevels, np.float32)
        check(lib().vo_orb_scale_factors(self._h, _p(s), None))
        return s

    def GetInverseScaleFactors(self):
        s = np.zeros(self.nlevels, np.float32)
        i = np.zeros(self.nlevels, np.float32)
        check(lib().vo_orb_scale_factors(self._h, _p(s), _p(i)))
        return i

    def features_per_level(self):
        q = np.zeros(self.nlevels, np.int32)
        check(lib().vo_orb_features_per_level(self._h, _p(q)))
        return q

    def max_keypoints(self):
        return lib().vo_orb_max_keypoints(self._h)

    def set_stream(self, stream_ptr: int):
        check(lib().vo_orb_set_stream(self._h, C.c_void_p(stream_ptr)))

    def set_fused(self, on: bool):
        """vo_orb_set_option(VO_ORB_OPT_FUSED_LEVEL_PASS): the fused per-level pass, or the three separate kernels (default)"""
        check(lib().vo_orb_set_option(self._h, 1, int(on)), "vo_orb_set_option")

    def set_early_level0(self, on: bool):
        """vo_orb_set_option(VO_ORB_OPT_EARLY_LEVEL0): level 0's FAST cells and blur next to the resize chain (default off)"""
        check(lib().vo_orb_set_option(self._h, 2, int(on)), "vo_orb_set_option")

    def set_stage_hook(self, fn):
        """vo_orb_set_stage_hook: fn(stage, stream_ptr) is called when a stage's launches have been enqueued (None removes it)"""
        if fn is None:
            self._hook = None
            check(lib().vo_orb_set_stage_hook(self._h, None, None), "vo_orb_set_stage_hook")
            return
        HOOK = C.CFUNCTYPE(None, C.c_int, C.c_void_p, C.c_void_p)
        self._hook = HOOK(lambda stage, stream, user: fn(stage, stream))  # (kept alive with the handle)
        check(lib().vo_orb_set_stage_hook(self._h, self._hook, None), "vo_orb_set_stage_hook")

    def set_describe_blur(self, kind: int):
        """vo_orb_set_option(VO_ORB_OPT_DESCRIBE_BLUR): 0 = the descriptor kernel blurs its windows itself (default), 1 = blurred planes"""
        check(lib().vo_orb_set_option(self._h, 4, int(kind)), "vo_orb_set_option")

    def set_blur_kernel(self, kind: int):
        """vo_orb_set_option(VO_ORB_OPT_BLUR_KERNEL): 0 = int8 matrix-core products (default), 1 = the VALU form"""
        check(lib().vo_orb_set_option(self._h, 3, int(kind)), "vo_orb_set_option")

    def level_pass_plan(self, width, height):
        """per level: dict(fused, tile_pitch, tile_rows, score_rows, blocks, lds_bytes, list_cap) of the fused pass"""
        out = []
        for l in range(self.nlevels):
            v = (C.c_int * 8)()
            check(lib().vo_orb_debug_level_pass(self._h, int(width), int(height), l, v), "vo_orb_debug_level_pass")
            out.append(dict(zip(("fused", "tile_pitch", "tile_rows", "score_rows", "blocks", "lds_bytes", "list_cap"), list(v)[:7])))
        return out

    def __call__(self, image: np.ndarray, mask=None):
        """operator()(image, mask, keypoints, descriptors): host image -> (keypoints, descriptors)."""
        if image is None or image.size == 0:
            return np.zeros(0, KP_DTYPE), np.zeros((0, 32), np.uint8)
        image = np.ascontiguousarray(image, np.uint8)
        cap = self.max_keypoints()
        kps = np.zeros(cap, KP_DTYPE)
        desc = np.zeros((cap, 32), np.uint8)
        n = C.c_int(0)
        check(lib().vo_orb_extract(self._h, _p(image), image.shape[1], image.shape[0], image.strides[0],
                                   _p(kps), _p(desc), cap, C.byref(n)), "vo_orb_extract")
        return kps[:n.value].copy(), desc[:n.value].copy()

    def extract_batch_dev(self, images, kps, desc, counts):
        """torch uint8 [B,H,W] device tensor -> device outputs (asynchronous)."""
        B, H, W = images.shape
        cap = kps.shape[1]
        check(lib().vo_orb_extract_batch_dev(self._h, _p(images), B, W, H, images.stride(1),
                                             C.c_size_t(images.stride(0)), _p(kps), _p(desc), cap, _p(counts)),
              "vo_orb_extract_batch_dev")

    def sync(self):
        check(lib().vo_orb_sync(self._h), "vo_orb_sync")

    def get_level(self, frame, level, blurred=False):
        w, h = C.c_int(), C.c_int()
        check(lib().vo_orb_get_level(self._h, frame, level, int(blurred), None, 0, C.byref(w), C.byref(h)))
        out = np.zeros((h.value, w.value), np.uint8)
        check(lib().vo_orb_get_level(self._h, frame, level, int(blurred), _p(out), w.value, C.byref(w), C.byref(h)))
        return out

    def get_candidates(self, frame, level, cap=70000):
        x, y, r = (np.zeros(cap, np.float32) for _ in range(3))
        n = C.c_int()
        check(lib().vo_orb_get_candidates(self._h, frame, level, _p(x), _p(y), _p(r), cap, C.byref(n)))
        return x[:n.value].copy(), y[:n.value].copy(), r[:n.value].copy()

    STAGES = ("pyramid", "fast", "octree", "offsets", "blur", "describe")

    def set_timing(self, enabled: bool):
        check(lib().vo_orb_set_timing(self._h, int(enabled)))

    def get_timing(self):
        ms = np.zeros(len(self.STAGES))
        n = C.c_int()
        check(lib().vo_orb_get_timing(self._h, _p(ms), C.byref(n)))
        return dict(zip(self.STAGES, ms.tolist())), n.value

    def get_level_counts(self, frame=0):
        c = np.zeros(self.nlevels, np.int32)
        check(lib().vo_orb_get_level_counts(self._h, frame, _p(c)))
        return c


def hamming_matrix(a: np.ndarray, b: np.ndarray) -> np.ndarray:
    a = np.ascontiguousarray(a, np.uint8)
    b = np.ascontiguousarray(b, np.uint8)
    d = np.zeros((len(a), len(b)), np.uint16)
    check(lib().vo_hamming_matrix(_p(a), len(a), _p(b), len(b), _p(d)), "vo_hamming_matrix")
    return d


def hamming_matrix_dev(a, b, d, stream=0):
    check(lib().vo_hamming_matrix_dev(_p(a), a.shape[0], _p(b), b.shape[0], _p(d), C.c_void_p(stream)))


def hamming_matrix_batch_dev(a, b, d, stream=0):
    """a [P,na,32], b [P,nb,32], d [P,na,nb] device tensors"""
    P, na, nb = a.shape[0], a.shape[1], b.shape[1]
    check(lib().vo_hamming_matrix_batch_dev(_p(a), na, C.c_size_t(a.stride(0) // 32), _p(b), nb,
                                            C.c_size_t(b.stride(0) // 32), _p(d), C.c_size_t(d.stride(0)), P,
                                            C.c_void_p(stream)))


def median_descriptor(sets):
    """MapPoint::computeDescriptor for a batch of map points: sets = list of [n_i, 32] uint8 arrays -> best index per set
    (one kernel launch for the whole batch)."""
    offs = np.zeros(len(sets) + 1, np.int32)
    for i, d in enumerate(sets):
        offs[i + 1] = offs[i] + len(d)
    cat = np.ascontiguousarray(np.concatenate([np.asarray(d, np.uint8).reshape(-1, 32) for d in sets])
                               if offs[-1] else np.zeros((0, 32), np.uint8))
    best = np.zeros(max(len(sets), 1), np.int32)
    check(lib().vo_median_descriptor(_p(cat), len(sets), _p(offs), _p(best)), "vo_median_descriptor")
    return best[:len(sets)]


class GuidedQueries(C.Structure):
    _fields_ = [("n_queries", C.c_int32), ("stride", C.c_int32), ("n_per_frame", C.c_void_p), ("flags", C.c_void_p),
                ("u", C.c_void_p), ("v", C.c_void_p), ("aux", C.c_void_p), ("level", C.c_void_p), ("angle", C.c_void_p),
                ("viewcos", C.c_void_p), ("desc", C.c_void_p)]


class GuidedParams(C.Structure):
    _fields_ = [("mode", C.c_int32), ("radius", C.c_float), ("bf", C.c_float), ("ratio", C.c_float),
                ("dist_threshold", C.c_float), ("direction", C.c_int32), ("check_rot", C.c_int32),
                ("n_levels", C.c_int32), ("max_dist", C.c_int32), ("scale_factors", C.c_void_p),
                ("retry_below", C.c_int32), ("retry_n_per_frame", C.c_void_p)]


class Frames:
    """Device-resident frame store (vo_frames): Frame::Frame post-processing + grid on the GPU, guided matching."""

    MODE_FRAME, MODE_LOCAL_MAP, MODE_KEYFRAME, MODE_FUSE, MODE_AREA, MODE_SIM3 = range(6)

    def __init__(self, max_frames, max_features=2048, intrinsics=None, dist_coef=None, width=640.0, height=480.0):
        self._h = C.c_void_p()
        check(lib().vo_frames_create(C.byref(self._h), int(max_frames), int(max_features)), "vo_frames_create")
        self.max_frames, self.cap = max_frames, max_features
        if intrinsics is not None:
            self.set_camera(intrinsics, dist_coef, width, height)

    def close(self):
        if getattr(self, "_h", None) and self._h.value and _lib is not None:
            _lib.vo_frames_destroy(self._h)
            self._h = C.c_void_p()

    __del__ = close

    def set_camera(self, intrinsics, dist_coef=None, width=640.0, height=480.0):
        k = np.ascontiguousarray(intrinsics, np.float32)
        d = None if dist_coef is None else np.ascontiguousarray(dist_coef, np.float32)
        check(lib().vo_frames_set_camera(self._h, _p(k), _p(d), C.c_float(width), C.c_float(height)), "vo_frames_set_camera")

    def build_dev(self, kps, desc, counts, depth=None, inv_depth_scale=1.0, slot0=0, stream=0):
        """torch device tensors as written by OrbExtractor.extract_batch_dev; depth: float32 [B,H,W] metres or
        uint16/int16 [B,H,W] raw."""
        B, cap = kps.shape[0], kps.shape[1]
        kind, fs, pitch = 0, 0, 0
        if depth is not None:
            kind = 1 if depth.element_size() == 4 else 2
            fs, pitch = depth.stride(0) * depth.element_size(), depth.stride(1) * depth.element_size()
        check(lib().vo_frames_build_dev(self._h, int(slot0), B, _p(kps), _p(desc), _p(counts), cap, _p(depth), kind,
                                        C.c_size_t(fs), pitch, C.c_float(inv_depth_scale), C.c_void_p(stream)),
              "vo_frames_build_dev")

    def construct(self, slot, ext: "OrbExtractor", image, depth=None, inv_depth_scale=1.0):
        """Frame::Frame for one host image (vo_frames_construct): -> raw key-points (KP_DTYPE); the rest via download()"""
        image = np.ascontiguousarray(image, np.uint8)
        kind, dp, pitch = 0, None, 0
        if depth is not None:
            dp = np.ascontiguousarray(depth)
            kind, pitch = (1 if dp.dtype == np.float32 else 2), dp.strides[0]
        cap = ext.max_keypoints()
        kps = np.zeros(cap, KP_DTYPE)
        n = C.c_int()
        check(lib().vo_frames_construct(self._h, int(slot), ext._h, _p(image), image.shape[1], image.shape[0], image.strides[0],
                                        _p(dp), kind, int(pitch), C.c_float(inv_depth_scale), _p(kps), cap, C.byref(n)),
              "vo_frames_construct")
        return kps[:n.value].copy()

    def upload(self, slot, fa: "FrameArrays", depth=None, stream=0):
        dp = None if depth is None else np.ascontiguousarray(depth, np.float32)
        check(lib().vo_frames_upload(self._h, int(slot), C.byref(fa.view), _p(dp), C.c_void_p(stream)), "vo_frames_upload")

    def download(self, slot, stream=0):
        n = C.c_int()
        cap = self.cap
        out = dict(x=np.zeros(cap, np.float32), y=np.zeros(cap, np.float32), octave=np.zeros(cap, np.int32),
                   angle=np.zeros(cap, np.float32), uright=np.zeros(cap, np.float32), depth=np.zeros(cap, np.float32),
                   desc=np.zeros((cap, 32), np.uint8), cell_start=np.zeros(64 * 48 + 1, np.int32),
                   cell_items=np.zeros(cap, np.uint16))
        check(lib().vo_frames_download(self._h, int(slot), C.byref(n), _p(out["x"]), _p(out["y"]), _p(out["octave"]),
                                       _p(out["angle"]), _p(out["uright"]), _p(out["depth"]), _p(out["desc"]),
                                       _p(out["cell_start"]), _p(out["cell_items"]), C.c_void_p(stream)), "vo_frames_download")
        k = n.value
        for key in ("x", "y", "octave", "angle", "uright", "depth", "desc", "cell_items"):
            out[key] = out[key][:k].copy()
        out["n"] = k
        return out

    def getFeaturesInArea(self, slot, u, v, radius, min_level=None, max_level=None, max_out=256):
        """Frame::getFeaturesInArea / KeyFrame::getFeaturesInArea for arrays of windows -> list of index arrays
        (reference order), one per window"""
        u, v = np.ascontiguousarray(u, np.float32), np.ascontiguousarray(v, np.float32)
        r = np.ascontiguousarray(np.broadcast_to(np.asarray(radius, np.float32), u.shape))
        lo = None if min_level is None else np.ascontiguousarray(np.broadcast_to(np.asarray(min_level, np.int32), u.shape))
        hi = None if max_level is None else np.ascontiguousarray(np.broadcast_to(np.asarray(max_level, np.int32), u.shape))
        out = np.full((len(u), max_out), -1, np.int32)
        cnt = np.zeros(len(u), np.int32)
        check(lib().vo_frames_features_in_area(self._h, int(slot), len(u), _p(u), _p(v), _p(r), _p(lo), _p(hi), _p(out),
                                               int(max_out), _p(cnt)), "vo_frames_features_in_area")
        return [out[i, :min(int(cnt[i]), max_out)].copy() for i in range(len(u))], cnt

    def match_dev(self, n_frames, q, mode, scale_factors, radius=0.0, bf=0.0, ratio=0.0, dist_threshold=0.0, direction=0,
                  check_rot=0, max_dist=0, feature_mask=None, assigned=None, best_idx=None, n_matches=None, slot0=0,
                  pool_per_frame=0, stream=0):
        """q: dict of torch device tensors [n_frames, stride(, 32)] (flags,u,v,aux,level,angle,viewcos,desc; missing
        ones None) + optional 'n_per_frame'; outputs are torch device tensors."""
        sf = np.ascontiguousarray(scale_factors, np.float32)
        gq = GuidedQueries()
        stride = q["flags"].shape[1]
        gq.n_queries, gq.stride = int(q.get("n_queries", stride)), int(stride)
        for k in ("n_per_frame", "flags", "u", "v", "aux", "level", "angle", "viewcos", "desc"):
            t = q.get(k)
            setattr(gq, k, 0 if t is None else t.data_ptr())
        gp = GuidedParams(int(mode), float(radius), float(bf), float(ratio), float(dist_threshold), int(direction),
                          int(check_rot), len(sf), int(max_dist), sf.ctypes.data)
        check(lib().vo_match_guided_dev(self._h, int(slot0), int(n_frames), C.byref(gq), C.byref(gp), _p(feature_mask),
                                        _p(assigned), _p(best_idx), _p(n_matches), C.c_size_t(pool_per_frame),
                                        C.c_void_p(stream)), "vo_match_guided_dev")

    def match_status(self, stream=0):
        check(lib().vo_match_guided_status(self._h, C.c_void_p(stream)), "vo_match_guided_status")


class TrackerConfig(C.Structure):
    _fields_ = [("batch", C.c_int32), ("width", C.c_int32), ("height", C.c_int32), ("nfeatures", C.c_int32),
                ("nlevels", C.c_int32), ("ini_th_fast", C.c_int32), ("min_th_fast", C.c_int32), ("scale_factor", C.c_float),
                ("intrinsics", C.c_float * 5), ("dist_coef", C.c_float * 5), ("has_distortion", C.c_int32),
                ("inv_depth_scale", C.c_float), ("max_last", C.c_int32), ("max_local", C.c_int32),
                ("max_features", C.c_int32), ("single_stream", C.c_int32), ("stream", C.c_void_p),
                ("extract_stream", C.c_void_p), ("max_reloc_candidates", C.c_int32), ("max_reloc_features", C.c_int32)]


class RelocCandidate(C.Structure):
    _fields_ = [("n", C.c_int32), ("bad", C.c_int32), ("angle", C.c_void_p), ("desc", C.c_void_p), ("nodes", C.c_void_p),
                ("flags", C.c_void_p), ("points", C.c_void_p), ("ids", C.c_void_p), ("point_desc", C.c_void_p),
                ("min_distance", C.c_void_p), ("max_distance", C.c_void_p)]


class HandoverParams(C.Structure):
    _fields_ = [("th_depth", C.c_float), ("min_tracked", C.c_int32)]


class TrackerParams(C.Structure):
    _fields_ = [("radius", C.c_float), ("th_radius", C.c_float), ("ratio", C.c_float), ("direction", C.c_int32),
                ("ref_ratio", C.c_float), ("no_retry", C.c_int32)]


class Tracker:
    """vo_tracker: VisualOdometry::trackWithMotion + trackLocalMap for a batch of camera streams, one C call per
    batch (include/vo_hip.h).  This class only marshals arrays; torch appears where the caller hands over device
    tensors (images, depth) or streams."""
    (ASSIGNED_LAST, ASSIGNED_LOCAL, POSE_FIRST, INLIERS_FIRST, OBSERVED_INLIERS_FIRST, FEATURE_HAS_POINT, FEATURE_POINTS,
     LOCAL_FLAGS, LOCAL_U, LOCAL_V, LOCAL_UR, LOCAL_LEVEL, LOCAL_VIEWCOS, KEYPOINT_COUNTS, FEATURE_OUTLIER,
     RELOC_WINNER, RELOC_POINT_IDS, RELOC_BOW_MATCHES, RELOC_PNP_INLIERS, RELOC_OUTCOME, RELOC_PNP_MASK,
     RELOC_CANDIDATES, RELOC_N_CANDIDATES, LOCAL_KEYFRAMES, LOCAL_N_KEYFRAMES, LOCAL_N_POINTS, LOCAL_REF_KF, LOCAL_POINT_IDS,
     LOCAL_POINTS, LOCAL_NORMALS, LOCAL_MIN_DISTANCE, LOCAL_MAX_DISTANCE, LOCAL_DESC, LOCAL_MAP_FLAGS, LOCAL_LINK,
     POSE_START, SLOT_IDS, SLOT_DESC, FRAME_POSE, VELOCITY, MOTION_STATE, TEMP_COUNT, LAST_POINTS, LAST_FLAGS, LAST_OCTAVE,
     LAST_ANGLE, LAST_DESC, LAST_IDS, LAST_N, TCW_START, FIRST_SLOT_IDS, STAT_IDS, STAT_VISIBLE, STAT_FOUND, REF_TCR, REF_KF,
     FEATURE_OBSERVED) = range(57)
    LOCAL_MAX_KEYFRAMES = 84
    RELOC_STAGES = ("featvec", "gather", "local_ids", "bow_walk")
    STAGES = ("extract", "frame_post", "match_last_frame", "pose_only_1", "match_local_map", "pose_only_2")
    FEW_MATCHES, FEW_INLIERS, RELOC_FAILED = 1, 2, 4

    def __init__(self, batch, intrinsics5, dist_coef=None, width=640, height=480, max_last=1024, max_local=2048,
                 inv_depth_scale=1.0, nfeatures=1000, scale_factor=1.2, nlevels=8, ini_th=20, min_th=7, max_features=0,
                 stream=None, extract_stream=None, single_stream=False, max_reloc_candidates=0, max_reloc_features=0):
        cfg = TrackerConfig()
        cfg.max_reloc_candidates, cfg.max_reloc_features = int(max_reloc_candidates), int(max_reloc_features)
        self.max_reloc_candidates = int(max_reloc_candidates)
        cfg.batch, cfg.width, cfg.height = int(batch), int(width), int(height)
        cfg.nfeatures, cfg.nlevels, cfg.ini_th_fast, cfg.min_th_fast = int(nfeatures), int(nlevels), int(ini_th), int(min_th)
        cfg.scale_factor = float(scale_factor)
        cfg.intrinsics = (C.c_float * 5)(*[float(v) for v in intrinsics5])
        if dist_coef is not None:
            cfg.dist_coef = (C.c_float * 5)(*[float(v) for v in dist_coef])
            cfg.has_distortion = 1
        cfg.inv_depth_scale = float(inv_depth_scale)
        cfg.max_last, cfg.max_local, cfg.max_features = int(max_last), int(max_local), int(max_features)
        cfg.single_stream = int(bool(single_stream))
        cfg.stream = stream if stream is None else int(stream)
        cfg.extract_stream = extract_stream if extract_stream is None else int(extract_stream)
        self._h = C.c_void_p()
        check(lib().vo_tracker_create(C.byref(self._h), C.byref(cfg)), "vo_tracker_create")
        b, cap, kcap, nl = C.c_int(), C.c_int(), C.c_int(), C.c_int()
        check(lib().vo_tracker_info(self._h, C.byref(b), C.byref(cap), C.byref(kcap), C.byref(nl)), "vo_tracker_info")
        self.B, self.cap, self.kcap, self.n_levels = b.value, cap.value, kcap.value, nl.value
        self.W, self.H, self.max_last, self.max_local = int(width), int(height), int(max_last), int(max_local)
        self.st = lib().vo_tracker_stream(self._h)

    def close(self):
        if getattr(self, "_h", None) and self._h.value and _lib is not None:
            _lib.vo_tracker_destroy(self._h)
            self._h = C.c_void_p()

    __del__ = close

    @property
    def frames_handle(self):
        return C.c_void_p(lib().vo_tracker_frames(self._h))

    @property
    def extractor_handle(self):
        return C.c_void_p(lib().vo_tracker_extractor(self._h))

    def extractor(self):
        """the tracker's extractor as an OrbExtractor view (per-kernel timing, candidates)"""
        return OrbExtractor.borrowed(self.extractor_handle, self.n_levels)

    def scale_factors(self):
        sf = np.zeros(self.n_levels, np.float32)
        check(lib().vo_orb_scale_factors(self.extractor_handle, _p(sf), None), "vo_orb_scale_factors")
        return sf

    def set_last_frame(self, Tcw12, points, flags, octave, angle, desc):
        """arrays [B, n, ...] (numpy)"""
        n = np.asarray(flags).shape[1]
        a = lambda x, dt: np.ascontiguousarray(x, dt)
        check(lib().vo_tracker_set_last_frame(self._h, int(n), _p(a(Tcw12, np.float64)), _p(a(points, np.float64)),
                                              _p(a(flags, np.uint8)), _p(a(octave, np.int32)), _p(a(angle, np.float32)),
                                              _p(a(desc, np.uint8))), "vo_tracker_set_last_frame")

    def set_local_map(self, points, normals, min_dist, max_dist, flags, desc, link=None):
        n = np.asarray(flags).shape[1]
        a = lambda x, dt: np.ascontiguousarray(x, dt)
        lk = None if link is None else a(link, np.int32)
        check(lib().vo_tracker_set_local_map(self._h, int(n), _p(a(points, np.float64)), _p(a(normals, np.float64)),
                                             _p(a(min_dist, np.float32)), _p(a(max_dist, np.float32)), _p(a(flags, np.uint8)),
                                             _p(lk), _p(a(desc, np.uint8))), "vo_tracker_set_local_map")

    @staticmethod
    def _params(radius, th_radius, ratio, direction, no_retry=False):
        return TrackerParams(float(radius), float(th_radius), float(ratio), int(direction), 0.7, int(bool(no_retry)))

    def track_dev(self, images, depth=None, radius=15.0, th_radius=3.0, ratio=0.8, direction=0, no_retry=False):
        """images: uint8 [B,H,W] device tensor; depth: float32 or (u)int16 [B,H,W] device tensor or None.  Asynchronous."""
        kind, fs, pitch = 0, 0, 0
        if depth is not None:
            kind = 1 if depth.element_size() == 4 else 2
            fs, pitch = depth.stride(0) * depth.element_size(), depth.stride(1) * depth.element_size()
        pr = self._params(radius, th_radius, ratio, direction, no_retry)
        check(lib().vo_tracker_track_dev(self._h, _p(images), int(images.stride(1)), C.c_size_t(images.stride(0)), _p(depth),
                                         kind, C.c_size_t(fs), int(pitch), C.byref(pr)), "vo_tracker_track_dev")

    def track(self, images, depth=None, radius=15.0, th_radius=3.0, ratio=0.8, direction=0, no_retry=False):
        """host arrays: images uint8 [B,H,W]; depth float32 / uint16 [B,H,W] or None (uploads included)."""
        img = np.ascontiguousarray(images, np.uint8)
        kind, dp = 0, None
        if depth is not None:
            dp = np.ascontiguousarray(depth)
            kind = 1 if dp.dtype == np.float32 else 2
        pr = self._params(radius, th_radius, ratio, direction, no_retry)
        check(lib().vo_tracker_track(self._h, _p(img), _p(dp), kind, C.byref(pr)), "vo_tracker_track")

    def track_first(self, images, depth=None, radius=15.0, direction=0, no_retry=False):
        """trackWithMotion alone (host arrays): Frame construction, search (+ retry), solve, culling; results() then holds
        the first solve's pose / counts / status"""
        img = np.ascontiguousarray(images, np.uint8)
        kind, dp = 0, None
        if depth is not None:
            dp = np.ascontiguousarray(depth)
            kind = 1 if dp.dtype == np.float32 else 2
        pr = self._params(radius, 3.0, 0.8, direction, no_retry)
        check(lib().vo_tracker_track_first(self._h, _p(img), _p(dp), kind, C.byref(pr)), "vo_tracker_track_first")

    def track_first_dev(self, images, depth=None, radius=15.0, direction=0, no_retry=False):
        """trackWithMotion alone from device tensors (see track_dev).  Asynchronous."""
        kind, fs, pitch = 0, 0, 0
        if depth is not None:
            kind = 1 if depth.element_size() == 4 else 2
            fs, pitch = depth.stride(0) * depth.element_size(), depth.stride(1) * depth.element_size()
        pr = self._params(radius, 3.0, 0.8, direction, no_retry)
        check(lib().vo_tracker_track_first_dev(self._h, _p(images), int(images.stride(1)), C.c_size_t(images.stride(0)), _p(depth),
                                               kind, C.c_size_t(fs), int(pitch), C.byref(pr)), "vo_tracker_track_first_dev")

    def set_local_map_ids(self, ids):
        """map-point ids [B, n] of the local points set by set_local_map (n = its n), in the id space get(RELOC_POINT_IDS)
        reports: track_local_map after relocalize* skips the local points whose id the frame already holds"""
        ids = np.ascontiguousarray(ids, np.int32)
        check(lib().vo_tracker_set_local_map_ids(self._h, int(ids.shape[1]), _p(ids)), "vo_tracker_set_local_map_ids")

    def set_last_frame_ids(self, ids):
        """map-point ids [B, n] of the last-frame list (n = its n), negative = none: the counterpart of set_local_map_ids.
        set_last_frame forgets them"""
        ids = np.ascontiguousarray(ids, np.int32)
        check(lib().vo_tracker_set_last_frame_ids(self._h, int(ids.shape[1]), _p(ids)), "vo_tracker_set_last_frame_ids")

    def set_last_pose(self, Tcw12, valid):
        """frame_last_->Tcw_ [B, 12] and poseExist_ [B]: the seed of the motion model"""
        T, v = np.ascontiguousarray(Tcw12, np.float64), np.ascontiguousarray(valid, np.uint8)
        assert T.shape == (self.B, 12) and v.shape == (self.B,)
        check(lib().vo_tracker_set_last_pose(self._h, _p(T), _p(v)), "vo_tracker_set_last_pose")

    def end_frame(self, th_depth, min_tracked=0):
        """vo_tracker_end_frame: the tracked frame becomes the last frame, on the device (visualOdometry.cpp:80-128).
        Asynchronous; get(SLOT_IDS / SLOT_DESC / FRAME_POSE / VELOCITY / MOTION_STATE / LAST_*) after."""
        pr = HandoverParams(float(th_depth), int(min_tracked))
        check(lib().vo_tracker_end_frame(self._h, C.byref(pr)), "vo_tracker_end_frame")

    def begin_frame(self, th_depth, is_keyframe=None):
        """vo_tracker_begin_frame: updateLastFrame's temporary points, the motion-model start pose and the link by id
        (visualOdometry.cpp:233-236).  is_keyframe: uint8 [B] DEVICE tensor or None.  Asynchronous."""
        pr = HandoverParams(float(th_depth), 0)
        check(lib().vo_tracker_begin_frame(self._h, C.byref(pr), _p(is_keyframe)), "vo_tracker_begin_frame")
        self._is_keyframe_keep = is_keyframe  # the enqueued kernel reads it

    def handover_arrays(self):
        """device addresses (ints) of SLOT_IDS [B, max_features], FRAME_POSE [B, 12] and MOTION_STATE [B]"""
        a, b, c = C.c_void_p(), C.c_void_p(), C.c_void_p()
        check(lib().vo_tracker_handover_arrays(self._h, C.byref(a), C.byref(b), C.byref(c)), "vo_tracker_handover_arrays")
        return a.value, b.value, c.value

    def point_stats(self):
        """vo_tracker_point_stats: addVisible / addFound of the frame as three rows per frame, on the device, after
        track_first + track_local_map with ids on the local map and on the last list.  Asynchronous; get(STAT_IDS /
        STAT_VISIBLE / STAT_FOUND) after."""
        check(lib().vo_tracker_point_stats(self._h), "vo_tracker_point_stats")

    def point_stats_arrays(self):
        """device addresses (ints) of STAT_IDS, STAT_VISIBLE, STAT_FOUND [B, row_len] and row_len = max_features + max_local"""
        a, b, c, n = C.c_void_p(), C.c_void_p(), C.c_void_p(), C.c_int32()
        check(lib().vo_tracker_point_stats_arrays(self._h, C.byref(a), C.byref(b), C.byref(c), C.byref(n)), "vo_tracker_point_stats_arrays")
        return a.value, b.value, c.value, n.value

    def end_frame_store(self, store, th_depth, min_tracked=0):
        """vo_tracker_end_frame_store: end_frame behind relocalize_store / relocalize_db or track_ref_keyframe_store(first_stage_only=
        True), each followed by build_local_map(store) + track_local_map: the slot ids and descriptors come from `store`.
        Asynchronous; the outputs and the calls that may follow are end_frame's."""
        pr = HandoverParams(float(th_depth), int(min_tracked))
        check(lib().vo_tracker_end_frame_store(self._h, store._h, C.byref(pr)), "vo_tracker_end_frame_store")
        self._end_store_keep = store  # the enqueued kernel reads it

    def point_stats_store(self, store):
        """vo_tracker_point_stats_store: point_stats' three rows per frame behind the same two routes.  Asynchronous;
        get(STAT_IDS / STAT_VISIBLE / STAT_FOUND) after."""
        check(lib().vo_tracker_point_stats_store(self._h, store._h), "vo_tracker_point_stats_store")
        self._stats_store_keep = store  # the enqueued kernel reads it

    def record_ref_pose(self, store, ref_kf=None):
        """vo_tracker_record_ref_pose: Tcr = frame pose * pose(ref)^-1 per frame after end_frame (visualOdometry.cpp:130-140).
        ref_kf: int32 [B] DEVICE tensor, or None: get(LOCAL_REF_KF).  Asynchronous; get(REF_TCR / REF_KF) after."""
        check(lib().vo_tracker_record_ref_pose(self._h, store._h, _p(ref_kf)), "vo_tracker_record_ref_pose")
        # the enqueued kernels read them: the last four calls' arguments stay alive (a frame records once), whatever else is called
        self._record_keep = (getattr(self, "_record_keep", []) + [(store, ref_kf)])[-4:]

    def refresh_last_pose(self, store):
        """vo_tracker_refresh_last_pose: last pose = Tcr * pose(ref) between end_frame and begin_frame (:547-549).  Asynchronous."""
        check(lib().vo_tracker_refresh_last_pose(self._h, store._h), "vo_tracker_refresh_last_pose")
        self._refresh_keep = store  # the enqueued kernel reads it

    def track_local_map(self, th_radius=3.0, ratio=0.8):
        """trackLocalMap on the state the first stage left, against the local map set in between.  After relocalize /
        relocalize_dev / relocalize_store / relocalize_db it runs on the frame state the relocalisation left (pass
        th_radius=5, visualOdometry.cpp:768): set_local_map + set_local_map_ids in between; frames whose relocalisation
        failed are not touched.  Without a local map set: VoError (VO_ERR_INVALID)."""
        pr = self._params(15.0, th_radius, ratio, 0)
        check(lib().vo_tracker_track_local_map(self._h, C.byref(pr)), "vo_tracker_track_local_map")

    def set_ref_keyframe(self, vocab, Tcw12, points, flags, angle, desc, node_of_feature):
        """arrays [B, n, ...]; node_of_feature [B, n]: the key-frame's DBoW3::FeatureVector as per-feature node ids"""
        n = np.asarray(flags).shape[1]
        a = lambda x, dt: np.ascontiguousarray(x, dt)
        nodes = [BowNodes(np.asarray(node_of_feature)[f]) for f in range(self.B)]
        arr = (C.POINTER(BowView) * self.B)(*[C.pointer(nd.view) for nd in nodes])
        check(lib().vo_tracker_set_ref_keyframe(self._h, vocab._h, int(n), _p(a(Tcw12, np.float64)), _p(a(points, np.float64)),
                                                _p(a(flags, np.uint8)), _p(a(angle, np.float32)), _p(a(desc, np.uint8)), arr),
              "vo_tracker_set_ref_keyframe")
        self._ref_vocab = vocab  # the C side keeps the pointer

    def track_ref_keyframe(self, images, depth=None, th_radius=3.0, ratio=0.8, ref_ratio=0.7, first_stage_only=False):
        """trackRefKeyFrame (+ trackLocalMap) from host arrays"""
        img = np.ascontiguousarray(images, np.uint8)
        kind, dp = 0, None
        if depth is not None:
            dp = np.ascontiguousarray(depth)
            kind = 1 if dp.dtype == np.float32 else 2
        pr = self._params(15.0, th_radius, ratio, 0)
        pr.ref_ratio = float(ref_ratio)
        check(lib().vo_tracker_track_ref_keyframe(self._h, _p(img), _p(dp), kind, C.byref(pr), int(bool(first_stage_only))),
              "vo_tracker_track_ref_keyframe")

    def track_ref_keyframe_store(self, store, vocab, ref_kf, Tcw12, images, depth=None, th_radius=3.0, ratio=0.8, ref_ratio=0.7,
                                 first_stage_only=False):
        """vo_tracker_track_ref_keyframe_store[_dev]: trackRefKeyFrame (+ trackLocalMap) with frame f's reference key-frame
        read from `store` by number.  ref_kf: int32 [B] and Tcw12: float64 [B, 12] DEVICE tensors (frame_last_->Tcw_); images /
        depth host arrays or device tensors.  Asynchronous: no host step, no synchronisation; results() / get() after."""
        pr = self._params(15.0, th_radius, ratio, 0)
        pr.ref_ratio = float(ref_ratio)
        head = (self._h, store._h, vocab._h, _p(ref_kf), _p(Tcw12))
        if hasattr(images, "data_ptr"):
            check(lib().vo_tracker_track_ref_keyframe_store_dev(*head, *self._dev_frames(images, depth), C.byref(pr),
                                                                int(bool(first_stage_only))), "vo_tracker_track_ref_keyframe_store_dev")
        else:
            img, dp, kind = self._host_frames(images, depth)
            check(lib().vo_tracker_track_ref_keyframe_store(*head, _p(img), _p(dp), kind, C.byref(pr), int(bool(first_stage_only))),
                  "vo_tracker_track_ref_keyframe_store")
        self._ref_store_keep = (store, vocab, ref_kf, Tcw12)  # the enqueued kernels read them

    def track_ref_keyframe_dev(self, images, depth=None, th_radius=3.0, ratio=0.8, ref_ratio=0.7, first_stage_only=False):
        """trackRefKeyFrame (+ trackLocalMap) from device tensors (uint8 [B,H,W]; depth float32 / (u)int16 [B,H,W] or None)"""
        pr = self._params(15.0, th_radius, ratio, 0)
        pr.ref_ratio = float(ref_ratio)
        check(lib().vo_tracker_track_ref_keyframe_dev(self._h, *self._dev_frames(images, depth), C.byref(pr), int(bool(first_stage_only))),
              "vo_tracker_track_ref_keyframe_dev")

    def set_reloc_candidates(self, vocab, candidates):
        """candidates[f] = the frame's candidate key-frames in the order VisualOdometry::relocalization walks them, each a
        dict(angle, desc, nodes (per-feature node ids), flags, points, ids, point_desc, min_dist, max_dist, bad=False)"""
        assert len(candidates) == self.B
        mc = max([len(c) for c in candidates] + [0])
        n_cand = np.array([len(c) for c in candidates], np.int32)
        arr = (RelocCandidate * max(self.B * mc, 1))()
        keep = []
        for f, cl in enumerate(candidates):
            for c, k in enumerate(cl):
                a = dict(angle=np.ascontiguousarray(k["angle"], np.float32), desc=np.ascontiguousarray(k["desc"], np.uint8),
                         flags=np.ascontiguousarray(k["flags"], np.uint8), points=np.ascontiguousarray(k["points"], np.float64),
                         ids=np.ascontiguousarray(k["ids"], np.int32), point_desc=np.ascontiguousarray(k["point_desc"], np.uint8),
                         min_distance=np.ascontiguousarray(k["min_dist"], np.float32),
                         max_distance=np.ascontiguousarray(k["max_dist"], np.float32))
                nodes = BowNodes(np.asarray(k["nodes"]))
                keep.append((a, nodes))
                rc = arr[f * mc + c]
                rc.n, rc.bad = len(a["flags"]), int(bool(k.get("bad", False)))
                for key, v in a.items():
                    setattr(rc, key, v.ctypes.data)
                rc.nodes = C.addressof(nodes.view)
        check(lib().vo_tracker_set_reloc_candidates(self._h, vocab._h, int(mc), _p(n_cand), arr), "vo_tracker_set_reloc_candidates")
        self._reloc_vocab = vocab  # the C side keeps the pointer

    def relocalize(self, images, depth=None):
        """VisualOdometry::relocalization() from host arrays (Frame construction to pose); results() / get(RELOC_*) after"""
        img = np.ascontiguousarray(images, np.uint8)
        kind, dp = 0, None
        if depth is not None:
            dp = np.ascontiguousarray(depth)
            kind = 1 if dp.dtype == np.float32 else 2
        check(lib().vo_tracker_relocalize(self._h, _p(img), _p(dp), kind, None), "vo_tracker_relocalize")

    def relocalize_dev(self, images, depth=None):
        """the same from device tensors (uint8 [B,H,W]; depth float32 / (u)int16 [B,H,W] or None)"""
        kind, fs, pitch = 0, 0, 0
        if depth is not None:
            kind = 1 if depth.element_size() == 4 else 2
            fs, pitch = depth.stride(0) * depth.element_size(), depth.stride(1) * depth.element_size()
        check(lib().vo_tracker_relocalize_dev(self._h, _p(images), int(images.stride(1)), C.c_size_t(images.stride(0)), _p(depth),
                                              kind, C.c_size_t(fs), int(pitch), None), "vo_tracker_relocalize_dev")

    @staticmethod
    def _host_frames(images, depth):
        img = np.ascontiguousarray(images, np.uint8)
        kind, dp = 0, None
        if depth is not None:
            dp = np.ascontiguousarray(depth)
            kind = 1 if dp.dtype == np.float32 else 2
        return img, dp, kind

    @staticmethod
    def _dev_frames(images, depth):
        kind, fs, pitch = 0, 0, 0
        if depth is not None:
            kind = 1 if depth.element_size() == 4 else 2
            fs, pitch = depth.stride(0) * depth.element_size(), depth.stride(1) * depth.element_size()
        return (_p(images), int(images.stride(1)), C.c_size_t(images.stride(0)), _p(depth), kind, C.c_size_t(fs), int(pitch))

    def relocalize_store(self, store, vocab, n_cand, cand, images, depth=None):
        """vo_tracker_relocalize_store[_dev]: n_cand [B] and cand [B, stride] int32 DEVICE tensors of key-frame numbers of
        `store` in walk order (the output layout of KeyFrameDatabase.query_reloc_dev); images / depth host arrays or device
        tensors.  Asynchronous; results() / get(RELOC_*) after."""
        stride = int(cand.stride(0)) if cand.dim() > 1 else int(cand.numel() // max(self.B, 1))
        head = (self._h, store._h, vocab._h, _p(n_cand), _p(cand), stride)
        if hasattr(images, "data_ptr"):
            check(lib().vo_tracker_relocalize_store_dev(*head, *self._dev_frames(images, depth), None), "vo_tracker_relocalize_store_dev")
        else:
            img, dp, kind = self._host_frames(images, depth)
            check(lib().vo_tracker_relocalize_store(*head, _p(img), _p(dp), kind, None), "vo_tracker_relocalize_store")
        self._reloc_keep = (store, vocab, n_cand, cand)  # the enqueued kernels read them

    def relocalize_db(self, db, store, vocab, images, depth=None, stale_score=None):
        """vo_tracker_relocalize_db[_dev]: Map::detectRelocalizationCandidates on `db` (a KeyFrameDatabase over the same
        key-frames as `store`), then the walk; stale_score: float32 [size] device tensor or None"""
        head = (self._h, db._h, store._h, vocab._h, _p(stale_score))
        if hasattr(images, "data_ptr"):
            check(lib().vo_tracker_relocalize_db_dev(*head, *self._dev_frames(images, depth), None), "vo_tracker_relocalize_db_dev")
        else:
            img, dp, kind = self._host_frames(images, depth)
            check(lib().vo_tracker_relocalize_db(*head, _p(img), _p(dp), kind, None), "vo_tracker_relocalize_db")
        self._reloc_keep = (db, store, vocab, stale_score)

    def build_local_map(self, store):
        """vo_tracker_build_local_map: updateLocalKeyFrames + updateLocalMapPoints on the device from `store`, after
        relocalize_store / relocalize_db or track_ref_keyframe_store(first_stage_only=True); track_local_map follows without
        set_local_map.  Asynchronous; get(LOCAL_KEYFRAMES / LOCAL_N_KEYFRAMES / LOCAL_N_POINTS / LOCAL_REF_KF / LOCAL_*) after."""
        check(lib().vo_tracker_build_local_map(self._h, store._h), "vo_tracker_build_local_map")
        self._local_store_keep = store  # the enqueued kernels read it

    def get_reloc_timing(self):
        """milliseconds of the four new stages of the last store route run with set_timing(True)"""
        ms = (C.c_double * len(self.RELOC_STAGES))()
        check(lib().vo_tracker_get_reloc_timing(self._h, ms), "vo_tracker_get_reloc_timing")
        return {k: ms[i] for i, k in enumerate(self.RELOC_STAGES)}

    def results(self):
        B = self.B
        out = dict(pose=np.zeros((B, 6)), Tcw=np.zeros((B, 12)), n_tracked=np.zeros(B, np.int32), n_inliers=np.zeros(B, np.int32),
                   n_matches_last=np.zeros(B, np.int32), n_matches_local=np.zeros(B, np.int32), status=np.zeros(B, np.int32))
        check(lib().vo_tracker_results(self._h, _p(out["pose"]), _p(out["Tcw"]), _p(out["n_tracked"]), _p(out["n_inliers"]),
                                       _p(out["n_matches_last"]), _p(out["n_matches_local"]), _p(out["status"])),
              "vo_tracker_results")
        return out

    def get(self, what):
        B, cap, nl, mrc, ml = self.B, self.cap, self.max_local, max(self.max_reloc_candidates, 1), self.max_last
        shape, dt = {
            self.ASSIGNED_LAST: ((B, cap), np.int32), self.ASSIGNED_LOCAL: ((B, cap), np.int32),
            self.POSE_FIRST: ((B, 6), np.float64), self.INLIERS_FIRST: ((B,), np.int32),
            self.OBSERVED_INLIERS_FIRST: ((B,), np.int32), self.FEATURE_HAS_POINT: ((B, cap), np.uint8),
            self.FEATURE_POINTS: ((B, cap, 3), np.float64), self.LOCAL_FLAGS: ((B, max(nl, 1)), np.uint8),
            self.LOCAL_U: ((B, max(nl, 1)), np.float32), self.LOCAL_V: ((B, max(nl, 1)), np.float32),
            self.LOCAL_UR: ((B, max(nl, 1)), np.float32), self.LOCAL_LEVEL: ((B, max(nl, 1)), np.int32),
            self.LOCAL_VIEWCOS: ((B, max(nl, 1)), np.float32), self.KEYPOINT_COUNTS: ((B,), np.int32),
            self.FEATURE_OUTLIER: ((B, cap), np.uint8), self.RELOC_WINNER: ((B,), np.int32),
            self.RELOC_POINT_IDS: ((B, cap), np.int32), self.RELOC_BOW_MATCHES: ((B, mrc), np.int32),
            self.RELOC_PNP_INLIERS: ((B, mrc), np.int32), self.RELOC_OUTCOME: ((B, mrc), np.int32),
            self.RELOC_PNP_MASK: ((B, mrc, cap), np.uint8), self.RELOC_CANDIDATES: ((B, mrc), np.int32),
            self.RELOC_N_CANDIDATES: ((B,), np.int32),
            self.LOCAL_KEYFRAMES: ((B, self.LOCAL_MAX_KEYFRAMES), np.int32), self.LOCAL_N_KEYFRAMES: ((B,), np.int32),
            self.LOCAL_N_POINTS: ((B,), np.int32), self.LOCAL_REF_KF: ((B,), np.int32),
            self.LOCAL_POINT_IDS: ((B, max(nl, 1)), np.int32), self.LOCAL_POINTS: ((B, max(nl, 1), 3), np.float64),
            self.LOCAL_NORMALS: ((B, max(nl, 1), 3), np.float64), self.LOCAL_MIN_DISTANCE: ((B, max(nl, 1)), np.float32),
            self.LOCAL_MAX_DISTANCE: ((B, max(nl, 1)), np.float32), self.LOCAL_DESC: ((B, max(nl, 1), 32), np.uint8),
            self.LOCAL_MAP_FLAGS: ((B, max(nl, 1)), np.uint8), self.LOCAL_LINK: ((B, max(nl, 1)), np.int32),
            self.POSE_START: ((B, 6), np.float64),
            self.SLOT_IDS: ((B, cap), np.int32), self.SLOT_DESC: ((B, cap, 32), np.uint8), self.FRAME_POSE: ((B, 12), np.float64),
            self.VELOCITY: ((B, 12), np.float64), self.MOTION_STATE: ((B,), np.int32), self.TEMP_COUNT: ((B,), np.int32),
            self.LAST_POINTS: ((B, ml, 3), np.float64), self.LAST_FLAGS: ((B, ml), np.uint8), self.LAST_OCTAVE: ((B, ml), np.int32),
            self.LAST_ANGLE: ((B, ml), np.float32), self.LAST_DESC: ((B, ml, 32), np.uint8), self.LAST_IDS: ((B, ml), np.int32),
            self.LAST_N: ((1,), np.int32), self.TCW_START: ((B, 12), np.float64),
            self.FIRST_SLOT_IDS: ((B, cap), np.int32), self.STAT_IDS: ((B, cap + nl), np.int32), self.STAT_VISIBLE: ((B, cap + nl), np.int32),
            self.STAT_FOUND: ((B, cap + nl), np.int32), self.REF_TCR: ((B, 12), np.float64), self.REF_KF: ((B,), np.int32),
            self.FEATURE_OBSERVED: ((B, cap), np.uint8)}[what]
        out = np.zeros(shape, dt)
        check(lib().vo_tracker_get(self._h, int(what), _p(out), C.c_size_t(out.nbytes)), "vo_tracker_get")
        return out

    def sync(self):
        check(lib().vo_tracker_sync(self._h), "vo_tracker_sync")

    def set_timing(self, enabled=True):
        check(lib().vo_tracker_set_timing(self._h, int(bool(enabled))), "vo_tracker_set_timing")

    def get_timing(self):
        ms = (C.c_double * len(self.STAGES))()
        n = C.c_int()
        check(lib().vo_tracker_get_timing(self._h, ms, C.byref(n)), "vo_tracker_get_timing")
        return {k: ms[i] for i, k in enumerate(self.STAGES)}, n.value

    def download_frame(self, slot):
        """the frame store's slot (tests): dict of numpy arrays as Frames.download"""
        fr = Frames.__new__(Frames)
        fr._h, fr.cap, fr.max_frames = self.frames_handle, self.cap, self.B
        try:
            return fr.download(slot, stream=self.st)
        finally:
            fr._h = C.c_void_p()  # not ours to destroy


class FrameArrays:
    def __init__(self, x, y, octave, angle, uright, desc, w=640.0, h=480.0):
        self.x = np.ascontiguousarray(x, np.float32)
        self.y = np.ascontiguousarray(y, np.float32)
        self.octave = np.ascontiguousarray(octave, np.int32)
        self.angle = np.ascontiguousarray(angle, np.float32)
        self.uright = np.ascontiguousarray(uright, np.float32)
        self.desc = np.ascontiguousarray(desc, np.uint8)
        v = FrameView()
        v.n = len(self.x)
        v.x, v.y, v.octave = self.x.ctypes.data, self.y.ctypes.data, self.octave.ctypes.data
        v.angle, v.uright, v.desc = self.angle.ctypes.data, self.uright.ctypes.data, self.desc.ctypes.data
        v.xmin, v.ymin, v.xmax, v.ymax = 0.0, 0.0, w, h
        self.view = v


class BowView(C.Structure):
    _fields_ = [("n_nodes", C.c_int32), ("node_id", C.c_void_p), ("start", C.c_void_p), ("feat", C.c_void_p)]


class BowNodes:
    """DBoW3::FeatureVector as CSR built from a per-feature node id array (ascending node ids)."""

    def __init__(self, node_of_feature):
        node_of_feature = np.asarray(node_of_feature)
        order = np.argsort(node_of_feature, kind="stable")
        ids, counts = np.unique(node_of_feature, return_counts=True)
        self.node_id = np.ascontiguousarray(ids, np.uint32)
        self.start = np.ascontiguousarray(np.concatenate([[0], np.cumsum(counts)]), np.int32)
        self.feat = np.ascontiguousarray(order, np.uint32)
        v = BowView()
        v.n_nodes = len(self.node_id)
        v.node_id, v.start, v.feat = self.node_id.ctypes.data, self.start.ctypes.data, self.feat.ctypes.data
        self.view = v


class Vocabulary:
    """Device copy of a DBoW3 vocabulary tree; transform() = DBoW3::Vocabulary::transform's per-feature part."""

    def __init__(self, depth_L, child_start, children, node_desc, node_weight, word_id):
        self._h = C.c_void_p()
        cs, ch = np.ascontiguousarray(child_start, np.int32), np.ascontiguousarray(children, np.int32)
        nd, nw = np.ascontiguousarray(node_desc, np.uint8), np.ascontiguousarray(node_weight, np.float64)
        wi = np.ascontiguousarray(word_id, np.int32)
        check(lib().vo_vocab_create(C.byref(self._h), len(wi), int(depth_L), _p(cs), _p(ch), _p(nd), _p(nw), _p(wi)),
              "vo_vocab_create")

    def close(self):
        if getattr(self, "_h", None) and self._h.value and _lib is not None:
            _lib.vo_vocab_destroy(self._h)
            self._h = C.c_void_p()

    __del__ = close

    def transform(self, desc, levelsup=3):
        desc = np.ascontiguousarray(desc, np.uint8)
        n = len(desc)
        word, weight, node = np.zeros(n, np.int32), np.zeros(n, np.float64), np.zeros(n, np.int32)
        check(lib().vo_bow_transform(self._h, n, _p(desc), int(levelsup), _p(word), _p(weight), _p(node)), "vo_bow_transform")
        return word, weight, node

    def tree(self):
        """the tree back on the host (vo_vocab_tree): dict in vo_vocab_create's layout"""
        nn, L = C.c_int(), C.c_int()
        check(lib().vo_vocab_tree(self._h, C.byref(nn), C.byref(L), None, None, None, None, None), "vo_vocab_tree")
        n = nn.value
        cs = np.zeros(n + 1, np.int32)
        check(lib().vo_vocab_tree(self._h, None, None, _p(cs), None, None, None, None), "vo_vocab_tree")
        ch, nd = np.zeros(max(int(cs[n]), 1), np.int32), np.zeros((n, 32), np.uint8)
        nw, wi = np.zeros(n, np.float64), np.zeros(n, np.int32)
        check(lib().vo_vocab_tree(self._h, None, None, None, _p(ch), _p(nd), _p(nw), _p(wi)), "vo_vocab_tree")
        return dict(L=L.value, child_start=cs, children=ch[:int(cs[n])], node_desc=nd, node_weight=nw, word_id=wi)

    def save(self, path, k=10):
        """DBoW3::Vocabulary::save(path, false): the plain binary stream load_vocabulary reads"""
        check(lib().vo_vocab_save(self._h, int(k), str(path).encode()), "vo_vocab_save")


class VocabTrainInfo(C.Structure):
    _fields_ = [(n, C.c_int32) for n in ("n_nodes", "n_words", "n_levels", "lloyd_iterations_max", "n_capped")]


def train_vocabulary(desc, image_offsets, k=10, L=5, seed=0, stream=None):
    """Map::createVocabulary's DBoW3::Vocabulary::create on the device -> (Vocabulary, info dict).  desc [n, 32] uint8 and
    image_offsets [n_images + 1] int32: numpy arrays (vo_vocab_train) or torch device tensors (vo_vocab_train_dev, `stream`)."""
    h, info = C.c_void_p(), VocabTrainInfo()
    if isinstance(desc, np.ndarray) or not hasattr(desc, "data_ptr"):
        d = np.ascontiguousarray(desc, np.uint8).reshape(-1, 32)
        off = np.ascontiguousarray(image_offsets, np.int32)
        check(lib().vo_vocab_train(len(d), _p(d), len(off) - 1, _p(off), int(k), int(L), C.c_uint64(int(seed)), C.byref(h),
                                   C.byref(info)), "vo_vocab_train")
    else:
        assert desc.is_contiguous() and image_offsets.is_contiguous()
        check(lib().vo_vocab_train_dev(int(desc.numel() // 32), _p(desc), int(image_offsets.numel()) - 1, _p(image_offsets), int(k),
                                       int(L), C.c_uint64(int(seed)), _p(stream), C.byref(h), C.byref(info)), "vo_vocab_train_dev")
    v = Vocabulary.__new__(Vocabulary)
    v._h = h
    return v, {n: int(getattr(info, n)) for n, _ in VocabTrainInfo._fields_}


class Matcher:
    """Mirror of myslam::Matcher's search routines (reference include/myslam/matcher.h:9-45)."""

    def __init__(self, ratio: float = 0.8):
        self.ratio_ = ratio

    def searchByProjection_frame(self, cur: FrameArrays, q, radius, bf, direction, checkRot, scale_factors,
                                 blocked=None):
        nq = len(q["flags"])
        assigned = np.full(cur.view.n, -1, np.int32)
        n = C.c_int()
        sf = np.ascontiguousarray(scale_factors, np.float32)
        check(lib().vo_match_frame_projection(
            C.byref(cur.view), nq, _p(q["flags"]), _p(q["u"]), _p(q["v"]), _p(q["invz"]), _p(q["octave"]),
            _p(q["angle"]), _p(q["desc"]), C.c_float(radius), C.c_float(bf), int(direction), int(checkRot),
            len(sf), _p(sf), _p(blocked), _p(assigned), C.byref(n)), "vo_match_frame_projection")
        return n.value, assigned

    def searchByProjection_localmap(self, cur: FrameArrays, q, thRadius, scale_factors, blocked=None):
        nq = len(q["flags"])
        assigned = np.full(cur.view.n, -1, np.int32)
        n = C.c_int()
        sf = np.ascontiguousarray(scale_factors, np.float32)
        check(lib().vo_match_local_map(
            C.byref(cur.view), nq, _p(q["flags"]), _p(q["u"]), _p(q["v"]), _p(q["ur"]), _p(q["level"]),
            _p(q["viewcos"]), _p(q["desc"]), C.c_float(thRadius), C.c_float(self.ratio_), _p(sf), _p(blocked),
            _p(assigned), C.byref(n)), "vo_match_local_map")
        return n.value, assigned

    def searchByProjection_keyframe(self, cur: FrameArrays, q, radius, distThreshold, checkRot, scale_factors,
                                    has_map_point=None):
        nq = len(q["flags"])
        assigned = np.full(cur.view.n, -1, np.int32)
        n = C.c_int()
        sf = np.ascontiguousarray(scale_factors, np.float32)
        check(lib().vo_match_frame_keyframe(
            C.byref(cur.view), nq, _p(q["flags"]), _p(q["u"]), _p(q["v"]), _p(q["level"]), _p(q["angle"]),
            _p(q["desc"]), C.c_float(radius), C.c_float(distThreshold), int(checkRot), _p(sf), _p(has_map_point),
            _p(assigned), C.byref(n)), "vo_match_frame_keyframe")
        return n.value, assigned

    def searchByBoW(self, a: FrameArrays, a_valid, a_nodes: BowNodes, b: FrameArrays, b_valid, b_nodes: BowNodes,
                    keyframe_to_keyframe: bool, checkRot=True):
        mode = 1 if keyframe_to_keyframe else 0
        match = np.full((a.view.n if mode else b.view.n), -1, np.int32)
        n = C.c_int()
        av, bv = np.ascontiguousarray(a_valid, np.uint8), np.ascontiguousarray(b_valid, np.uint8)  # alive across the call
        check(lib().vo_match_bow(C.byref(a.view), _p(av), C.byref(a_nodes.view),
                                 C.byref(b.view), _p(bv), C.byref(b_nodes.view),
                                 mode, C.c_float(self.ratio_), int(checkRot), _p(match), C.byref(n)), "vo_match_bow")
        return n.value, match

    def searchForTriangulation(self, a: FrameArrays, a_has, a_nodes, b: FrameArrays, b_has, b_nodes, F12, ex, ey,
                               scale_factors, checkRot=True):
        match = np.full(a.view.n, -1, np.int32)
        n = C.c_int()
        sf = np.ascontiguousarray(scale_factors, np.float32)
        F = np.ascontiguousarray(F12, np.float64).reshape(-1)
        ah, bh = np.ascontiguousarray(a_has, np.uint8), np.ascontiguousarray(b_has, np.uint8)
        check(lib().vo_match_triangulation(
            C.byref(a.view), _p(ah), C.byref(a_nodes.view), C.byref(b.view),
            _p(bh), C.byref(b_nodes.view), _p(F), C.c_float(ex), C.c_float(ey),
            _p(sf), int(checkRot), _p(match), C.byref(n)), "vo_match_triangulation")
        return n.value, match

    def searchForTriangulation_batch(self, a: FrameArrays, a_has, a_nodes, pairs, scale_factors, checkRot=True):
        """pairs: list of (b: FrameArrays, b_has, b_nodes: BowNodes, F12, ex, ey) -- the neighbours of key-frame a
        (LocalMapping::createNewMapPoints); ONE launch.  -> (counts [n], matches [n][a.n])"""
        n = len(pairs)
        sf = np.ascontiguousarray(scale_factors, np.float32)
        ah = np.ascontiguousarray(a_has, np.uint8)
        bh = [np.ascontiguousarray(p[1], np.uint8) for p in pairs]
        F = np.ascontiguousarray(np.stack([np.asarray(p[3], np.float64).reshape(9) for p in pairs]) if n else np.zeros((0, 9)))
        ex = np.ascontiguousarray([p[4] for p in pairs], np.float32)
        ey = np.ascontiguousarray([p[5] for p in pairs], np.float32)
        match = np.full((n, a.view.n), -1, np.int32)
        counts = np.zeros(max(n, 1), np.int32)
        bptr = (C.c_void_p * max(n, 1))(*[C.addressof(p[0].view) for p in pairs])
        hptr = (C.c_void_p * max(n, 1))(*[h.ctypes.data for h in bh])
        nptr = (C.c_void_p * max(n, 1))(*[C.addressof(p[2].view) for p in pairs])
        mptr = (C.c_void_p * max(n, 1))(*[match[i].ctypes.data for i in range(n)])
        check(lib().vo_match_triangulation_batch(n, C.byref(a.view), _p(ah), C.byref(a_nodes.view), bptr, hptr, nptr, _p(F), _p(ex),
                                                 _p(ey), _p(sf), int(checkRot), mptr, _p(counts)),
              "vo_match_triangulation_batch")
        return counts[:n].copy(), match

    def searchByBoW_batch(self, pairs, keyframe_to_keyframe: bool, checkRot=True):
        """pairs: list of (a, a_valid, a_nodes, b, b_valid, b_nodes); ONE launch -> (counts, list of match arrays)"""
        n, mode = len(pairs), (1 if keyframe_to_keyframe else 0)
        av = [np.ascontiguousarray(p[1], np.uint8) for p in pairs]
        bv = [np.ascontiguousarray(p[4], np.uint8) for p in pairs]
        match = [np.full((p[0].view.n if mode else p[3].view.n), -1, np.int32) for p in pairs]
        counts = np.zeros(max(n, 1), np.int32)
        arr = lambda xs: (C.c_void_p * max(n, 1))(*xs)
        check(lib().vo_match_bow_batch(n, arr([C.addressof(p[0].view) for p in pairs]), arr([x.ctypes.data for x in av]),
                                       arr([C.addressof(p[2].view) for p in pairs]), arr([C.addressof(p[3].view) for p in pairs]),
                                       arr([x.ctypes.data for x in bv]), arr([C.addressof(p[5].view) for p in pairs]), mode,
                                       C.c_float(self.ratio_), int(checkRot), arr([m.ctypes.data for m in match]), _p(counts)),
              "vo_match_bow_batch")
        return counts[:n].copy(), match

    def fuseMapPoints_match(self, kf: FrameArrays, q, threshold, scale_factors):
        nq = len(q["flags"])
        best = np.full(nq, -1, np.int32)
        n = C.c_int()
        sf = np.ascontiguousarray(scale_factors, np.float32)
        check(lib().vo_match_fuse(C.byref(kf.view), nq, _p(q["flags"]), _p(q["u"]), _p(q["v"]), _p(q["ur"]),
                                  _p(q["level"]), _p(q["desc"]), C.c_float(threshold), _p(sf), _p(best), C.byref(n)),
              "vo_match_fuse")
        return n.value, best

    def areaBest(self, kf: FrameArrays, q, th, scale_factors, max_dist):
        """inner search of searchBySim3 / fuseByPose"""
        nq = len(q["flags"])
        best = np.full(nq, -1, np.int32)
        n = C.c_int()
        sf = np.ascontiguousarray(scale_factors, np.float32)
        check(lib().vo_match_area_best(C.byref(kf.view), nq, _p(q["flags"]), _p(q["u"]), _p(q["v"]), _p(q["level"]),
                                       _p(q["desc"]), C.c_float(th), _p(sf), int(max_dist), _p(best), C.byref(n)),
              "vo_match_area_best")
        return n.value, best

    def searchByProjection_sim3(self, kf: FrameArrays, q, th, scale_factors, occupied=None):
        nq = len(q["flags"])
        assigned = np.full(kf.view.n, -1, np.int32)
        n = C.c_int()
        sf = np.ascontiguousarray(scale_factors, np.float32)
        occ = None if occupied is None else np.ascontiguousarray(occupied, np.uint8)
        check(lib().vo_match_sim3_projection(C.byref(kf.view), nq, _p(q["flags"]), _p(q["u"]), _p(q["v"]), _p(q["level"]),
                                             _p(q["desc"]), int(th), _p(sf), _p(occ), _p(assigned), C.byref(n)),
              "vo_match_sim3_projection")
        return n.value, assigned

    def searchBySim3(self, kf1: FrameArrays, kf2: FrameArrays, q1, q2, th, sf1, sf2):
        match12 = np.full(kf1.view.n, -1, np.int32)
        n = C.c_int()
        sf1 = np.ascontiguousarray(sf1, np.float32)
        sf2 = np.ascontiguousarray(sf2, np.float32)
        check(lib().vo_match_sim3_mutual(C.byref(kf1.view), C.byref(kf2.view), _p(q1["flags"]), _p(q1["u"]), _p(q1["v"]),
                                         _p(q1["level"]), _p(q1["desc"]), _p(q2["flags"]), _p(q2["u"]), _p(q2["v"]),
                                         _p(q2["level"]), _p(q2["desc"]), C.c_float(th), _p(sf1), _p(sf2), _p(match12),
                                         C.byref(n)), "vo_match_sim3_mutual")
        return n.value, match12

    @staticmethod
    def computeDistance(a, b) -> int:
        """Matcher::computeDistance (matcher.cpp:1240-1256) of ONE pair: a host popcount, like the inline in the C++
        shim (a GPU round trip per 256-bit popcount would turn microseconds into milliseconds); sets of
        descriptors go through hamming_matrix / median_descriptor."""
        x = np.bitwise_xor(np.asarray(a, np.uint8).reshape(32), np.asarray(b, np.uint8).reshape(32))
        return int(np.unpackbits(x).sum())


class Optimizer:
    """Mirror of myslam::Optimizer's static entry points on flat arrays
    (reference include/myslam/optimizer_ceres.h:12-27)."""

    @staticmethod
    def solvePoseOnlySE3(problems, summaries=False):
        """problems: list of dicts(pts, obs, inv_sigma, cam, pose0) -> (poses, outlier masks, inlier counts)."""
        P = len(problems)
        offs = np.zeros(P + 1, np.int32)
        for i, pr in enumerate(problems):
            offs[i + 1] = offs[i] + len(pr["pts"])
        tot = int(offs[-1])
        pts = np.ascontiguousarray(np.concatenate([pr["pts"] for pr in problems]) if tot else np.zeros((0, 3)))
        obs = np.ascontiguousarray(np.concatenate([pr["obs"] for pr in problems]) if tot else np.zeros((0, 3)))
        isg = np.ascontiguousarray(np.concatenate([pr["inv_sigma"] for pr in problems]) if tot else np.zeros(0))
        poses = np.ascontiguousarray(np.stack([pr["pose0"] for pr in problems]).astype(np.float64))
        cam = np.ascontiguousarray(problems[0]["cam"], np.float64)
        outl = np.zeros(max(tot, 1), np.uint8)
        ninl = np.zeros(P, np.int32)
        sums = (LmSummary * (2 * P))()
        check(lib().vo_pose_only_solve(P, _p(offs), _p(pts), _p(obs), _p(isg), _p(cam), _p(poses), _p(outl),
                                       _p(ninl), C.byref(sums) if summaries else None), "vo_pose_only_solve")
        masks = [outl[offs[i]:offs[i + 1]].copy() for i in range(P)]
        if summaries:
            return poses, masks, ninl, sums
        return poses, masks, ninl


    @staticmethod
    def solveLoopSim3(problems, fixScaleFlag=True, summaries=False):
        """problems: list of synth.make_sim3_problem-style dicts -> (poses[P,6], scales[P], outlier masks, inliers)."""
        P = len(problems)
        offs = np.zeros(P + 1, np.int32)
        for i, pr in enumerate(problems):
            offs[i + 1] = offs[i] + len(pr["cam_match"])
        cat = lambda k, w: np.ascontiguousarray(np.concatenate([pr[k].reshape(-1, w) for pr in problems]).astype(np.float64))
        tot = int(offs[-1])
        poses = np.ascontiguousarray(np.stack([pr["pose0"] for pr in problems]).astype(np.float64))
        scales = np.ascontiguousarray([float(pr["scale0"]) for pr in problems], np.float64)
        cam = np.ascontiguousarray(problems[0]["cam"][:4], np.float64)
        outl = np.zeros(max(tot, 1), np.uint8)
        ninl = np.zeros(P, np.int32)
        sums = (LmSummary * (2 * P))()
        # keep the packed arrays alive across the call (_p only takes their addresses)
        a_pm, a_pc, a_ic = cat("cam_match", 3), cat("pix_curr", 2), cat("isig_curr", 1)
        a_Pc, a_xm, a_im = cat("cam_curr", 3), cat("pix_match", 2), cat("isig_match", 1)
        check(lib().vo_sim3_solve(P, _p(offs), _p(a_pm), _p(a_pc), _p(a_ic), _p(a_Pc), _p(a_xm), _p(a_im), _p(cam),
                                  int(bool(fixScaleFlag)), _p(poses), _p(scales), _p(outl), _p(ninl),
                                  C.byref(sums) if summaries else None), "vo_sim3_solve")
        masks = [outl[offs[i]:offs[i + 1]].copy() for i in range(P)]
        if summaries:
            return poses, scales, masks, ninl, sums
        return poses, scales, masks, ninl


    @staticmethod
    def solvePoseGraphLoop(g, max_iterations=20):
        """g: synth.make_pose_graph-style dict -> (quats, trans, summary)"""
        q = np.ascontiguousarray(g["quats"], np.float64).copy()
        t = np.ascontiguousarray(g["trans"], np.float64).copy()
        sc = np.ascontiguousarray(g["scales"], np.float64)
        ei, ej = np.ascontiguousarray(g["e_i"], np.int32), np.ascontiguousarray(g["e_j"], np.int32)
        qm, tm = np.ascontiguousarray(g["q_meas"], np.float64), np.ascontiguousarray(g["t_meas"], np.float64)
        sm = np.ascontiguousarray(g["s_meas"], np.float64)
        s = LmSummary()
        check(lib().vo_pose_graph_solve(len(q), _p(q), _p(t), _p(sc), int(g["fixed"]), len(ei), _p(ei), _p(ej), _p(qm),
                                        _p(tm), _p(sm), 1, int(max_iterations), C.byref(s)), "vo_pose_graph_solve")
        return q, t, s


def chol_solve(A, b):
    """dense SPD solve through the device Cholesky kernels -> (x, L)"""
    A = np.ascontiguousarray(A, np.float64).copy()
    x = np.ascontiguousarray(b, np.float64).copy()
    check(lib().vo_chol_solve(len(x), _p(A), _p(x)), "vo_chol_solve")
    return x, np.tril(A)


def chol_solve_split(A, b, c0_tiles, col_part, n_ranks):
    """the split (per-rank segment) solve of a sharded global BA, its ranks emulated on one GPU -> x"""
    A = np.ascontiguousarray(A, np.float64)
    x = np.ascontiguousarray(b, np.float64).copy()
    cp = np.ascontiguousarray(col_part, np.int32)
    check(lib().vo_chol_solve_split(len(x), _p(A), _p(x), int(c0_tiles), _p(cp), int(n_ranks)), "vo_chol_solve_split")
    return x


def sim3_reanchor_points(points, ref, S_rw, S_wr):
    points = np.ascontiguousarray(points, np.float64)
    ref = np.ascontiguousarray(ref, np.int32)
    S_rw, S_wr = np.ascontiguousarray(S_rw, np.float64), np.ascontiguousarray(S_wr, np.float64)
    out = np.zeros_like(points)
    check(lib().vo_sim3_reanchor_points(len(points), _p(points), _p(ref), len(S_rw), _p(S_rw), _p(S_wr), _p(out)),
          "vo_sim3_reanchor_points")
    return out


def set_option(option, value):
    """vo_set_option: 'ba_graph' (1: hipGraph replay of unsharded LM loops) / 'pose_block' (0, 64, 128, 256) /
    'hamming_kernel' (0: int8 matrix cores, 1: xor + popcount on the VALU) / 'ba_pairs_kernel' (0: blocks staged through LDS, 1: lane = couple)."""
    code = {"ba_graph": 1, "pose_block": 2, "hamming_kernel": 3, "ba_pairs_kernel": 4}.get(option, option)
    check(lib().vo_set_option(int(code), int(value)), "vo_set_option")


class BundleAdjuster:
    """Handle over vo_ba_* (the arrays Optimizer::solveLocalBAPoseAndPoint gathers)."""

    OPT_SEGMENTS, OPT_COLLECTIVES_AT_ONE_RANK, OPT_ORDER_PARTS = 1, 2, 3

    def __init__(self, prob, shard=0, n_shards=1, stream=None, options=None):
        self.prob = prob
        self.n_cams, self.n_pts, self.n_edges = len(prob["poses"]), len(prob["points"]), len(prob["e_cam"])
        self._h = C.c_void_p()
        a = {k: np.ascontiguousarray(v) for k, v in prob.items() if isinstance(v, np.ndarray)}
        check(lib().vo_ba_create(C.byref(self._h), self.n_cams, _p(a["poses"]), _p(a["fixed"]), self.n_pts,
                                 _p(a["points"]), self.n_edges, _p(a["e_cam"]), _p(a["e_pt"]), _p(a["e_obs"]),
                                 _p(a["e_inv_sigma"]), _p(a["cam"])), "vo_ba_create")
        if n_shards > 1:
            check(lib().vo_ba_set_shard(self._h, shard, n_shards), "vo_ba_set_shard")
        if stream is not None:
            check(lib().vo_ba_set_stream(self._h, C.c_void_p(stream)))
        for k, v in (options or {}).items():
            self.set_option(k, v)

    def reset(self, prob):
        """vo_ba_reset: a new problem in this handle (buffers, stream, options kept)"""
        self.prob = prob
        self.n_cams, self.n_pts, self.n_edges = len(prob["poses"]), len(prob["points"]), len(prob["e_cam"])
        a = {k: np.ascontiguousarray(v) for k, v in prob.items() if isinstance(v, np.ndarray)}
        check(lib().vo_ba_reset(self._h, self.n_cams, _p(a["poses"]), _p(a["fixed"]), self.n_pts, _p(a["points"]), self.n_edges,
                                _p(a["e_cam"]), _p(a["e_pt"]), _p(a["e_obs"]), _p(a["e_inv_sigma"]), _p(a["cam"])), "vo_ba_reset")

    def set_option(self, option, value):
        """vo_ba_set_option: 'segments' / 'collectives_at_one_rank' / 'order_parts' (or the integer codes); before the
        first use of the handle, the same on every rank."""
        code = {"segments": 1, "collectives_at_one_rank": 2, "order_parts": 3}.get(option, option)
        check(lib().vo_ba_set_option(self._h, int(code), int(value)), "vo_ba_set_option")

    def close(self):
        if getattr(self, "_h", None) and self._h.value and _lib is not None:
            _lib.vo_ba_destroy(self._h)
            self._h = C.c_void_p()

    __del__ = close

    ALLREDUCE_FN = C.CFUNCTYPE(C.c_int, C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p)

    def set_allreduce(self, fn):
        """fn(dev_ptr, n_doubles, stream_ptr) -> 0: sums the buffer over the shards, ordered on the stream.  The
        C-ABI drives the sharded LM loop itself once this is set (vo_ba_set_allreduce)."""
        self._ar = self.ALLREDUCE_FN(lambda user, buf, n, st: int(fn(buf, n, st) or 0))  # keep the thunk alive
        check(lib().vo_ba_set_allreduce(self._h, self._ar, None), "vo_ba_set_allreduce")

    def n_free_cams(self):
        return lib().vo_ba_n_free_cams(self._h)

    def state(self):
        poses = np.zeros((self.n_cams, 6))
        pts = np.zeros((self.n_pts, 3))
        check(lib().vo_ba_get_state(self._h, _p(poses), _p(pts)), "vo_ba_get_state")
        return poses, pts

    def set_state(self, poses=None, points=None):
        po = None if poses is None else np.ascontiguousarray(poses, np.float64)
        pt = None if points is None else np.ascontiguousarray(points, np.float64)
        check(lib().vo_ba_set_state(self._h, _p(po), _p(pt)))

    def solve(self, huber_mono=0.0, huber_stereo=0.0, max_iterations=10, edge_active=None):
        s = LmSummary()
        act = None if edge_active is None else np.ascontiguousarray(edge_active, np.uint8)
        check(lib().vo_ba_solve(self._h, C.c_double(huber_mono), C.c_double(huber_stereo), int(max_iterations),
                                _p(act), C.byref(s)), "vo_ba_solve")
        return s

    def local_ba(self, stop=None):
        """Optimizer::solveLocalBAPoseAndPoint numerics; returns (edge_erase, summaries, status)."""
        erase = np.zeros(max(self.n_edges, 1), np.uint8)
        sums = (LmSummary * 2)()
        rc = lib().vo_ba_local_ba(self._h, stop, _p(erase), C.byref(sums))
        if rc not in (0, -5):
            check(rc, "vo_ba_local_ba")
        return erase[:self.n_edges], sums, rc

    def local_ba_enqueue(self, stop=None):
        return lib().vo_ba_local_ba_enqueue(self._h, stop)

    def local_ba_finish(self):
        erase = np.zeros(max(self.n_edges, 1), np.uint8)
        sums = (LmSummary * 2)()
        check(lib().vo_ba_local_ba_finish(self._h, _p(erase), C.byref(sums)), "vo_ba_local_ba_finish")
        return erase[:self.n_edges], sums

    # split-phase interface (multi-GPU driver)
    def lm_begin(self, huber_mono, huber_stereo, max_iterations, edge_active=None):
        act = None if edge_active is None else np.ascontiguousarray(edge_active, np.uint8)
        check(lib().vo_ba_lm_begin(self._h, C.c_double(huber_mono), C.c_double(huber_stereo), int(max_iterations),
                                   _p(act)), "vo_ba_lm_begin")

    def linearize(self):
        check(lib().vo_ba_linearize(self._h), "vo_ba_linearize")

    def step(self):
        check(lib().vo_ba_step(self._h), "vo_ba_step")

    def update(self):
        check(lib().vo_ba_update(self._h), "vo_ba_update")

    def lm_end(self):
        s = LmSummary()
        check(lib().vo_ba_lm_end(self._h, C.byref(s)), "vo_ba_lm_end")
        return s

    def reduced_system(self):
        p, n = C.c_void_p(), C.c_size_t()
        check(lib().vo_ba_reduced_system(self._h, C.byref(p), C.byref(n)))
        return p.value, n.value

    def reduced_cost(self):
        p, n = C.c_void_p(), C.c_size_t()
        check(lib().vo_ba_reduced_cost(self._h, C.byref(p), C.byref(n)))
        return p.value, n.value

    def classify(self, final_pass: bool):
        check(lib().vo_ba_classify(self._h, int(final_pass)), "vo_ba_classify")

    def lm_begin_inliers(self, huber_mono, huber_stereo, max_iterations):
        check(lib().vo_ba_lm_begin_inliers(self._h, C.c_double(huber_mono), C.c_double(huber_stereo),
                                           int(max_iterations)), "vo_ba_lm_begin_inliers")

    def edge_outliers(self):
        out = np.zeros(max(self.n_edges, 1), np.uint8)
        check(lib().vo_ba_get_edge_outliers(self._h, _p(out)), "vo_ba_get_edge_outliers")
        return out[:self.n_edges]

    def set_reduce_buffers(self, system, cost):
        check(lib().vo_ba_set_reduce_buffers(self._h, _p(system), _p(cost)))

    def debug_order(self):
        """-> dict(parts, cyclic, sep, depth, tiles, tile_rows): the key-frame order of a large reduced system"""
        out = (C.c_int * 8)()
        check(lib().vo_ba_debug_order(self._h, out), "vo_ba_debug_order")
        return dict(zip(("parts", "cyclic", "sep", "depth", "tiles", "tile_rows", "tile_products"), list(out)[:7]))

    def segment_c0(self):
        """first separator tile column when this (sharded) handle runs the per-rank segment factorisation, else 0"""
        out = (C.c_int * 8)()
        check(lib().vo_ba_debug_order(self._h, out), "vo_ba_debug_order")
        return int(out[7])

    def debug_schur(self, huber=(0.0, 0.0), edge_active=None):
        n = 6 * self.n_free_cams()
        S, b, cost = np.zeros((n, n)), np.zeros(n), C.c_double()
        act = None if edge_active is None else np.ascontiguousarray(edge_active, np.uint8)
        check(lib().vo_ba_debug_schur(self._h, C.c_double(huber[0]), C.c_double(huber[1]), C.c_double(0.0), _p(act),
                                      _p(S), _p(b), C.byref(cost)), "vo_ba_debug_schur")
        return S, b, cost.value


def se3_exp(xi):
    R, t = np.zeros(9), np.zeros(3)
    xi = np.ascontiguousarray(xi, np.float64)
    check(lib().vo_se3_exp(_p(xi), _p(R), _p(t)))
    return R.reshape(3, 3), t


def se3_log(R, t):
    xi = np.zeros(6)
    Rf, tf = np.ascontiguousarray(R, np.float64).reshape(-1), np.ascontiguousarray(t, np.float64)
    check(lib().vo_se3_log(_p(Rf), _p(tf), _p(xi)))
    return xi


class PnpDiag(C.Structure):
    _fields_ = [("samples", C.c_void_p), ("counts", C.c_void_p), ("hyp_Tcw12", C.c_void_p), ("best_iter", C.c_void_p),
                ("final_niters", C.c_void_p)]


def pnp_ransac(problems, cam4, iterations=100, reproj_error=8.0, confidence=0.99, diagnostics=False):
    """cv::solvePnPRansac(..., SOLVEPNP_EPNP) of poseEstimateByPnP (visualOdometry.cpp:778-830) for a batch of problems
    [(pts3d [n, 3], pts2d [n, 2]), ...] (float32) in one call.  Returns dict: Tcw [P, 3, 4], pose6 [P, 6] (se3),
    n_inliers [P], status [P] (1 found), inliers [list of bool [n]]; with diagnostics also samples [P, it, 5],
    counts [P, it], hyp_Tcw [P, it, 3, 4], best_iter [P], final_niters [P]."""
    P = len(problems)
    ns = [len(np.asarray(a).reshape(-1, 3)) for a, _ in problems]
    off = np.zeros(P + 1, np.int32)
    off[1:] = np.cumsum(ns)
    N = int(off[-1])
    p3 = np.ascontiguousarray(np.concatenate([np.asarray(a, np.float32).reshape(-1, 3) for a, _ in problems]) if N else np.zeros((0, 3), np.float32))
    p2 = np.ascontiguousarray(np.concatenate([np.asarray(b, np.float32).reshape(-1, 2) for _, b in problems]) if N else np.zeros((0, 2), np.float32))
    cam = np.ascontiguousarray(cam4, np.float32)[:4].copy()
    T, x6 = np.zeros((max(P, 1), 12)), np.zeros((max(P, 1), 6))
    mask, ninl, st = np.zeros(max(N, 1), np.uint8), np.zeros(max(P, 1), np.int32), np.zeros(max(P, 1), np.int32)
    out = {}
    d = None
    if diagnostics:
        it = int(iterations)
        out.update(samples=np.zeros((P, it, 5), np.int32), counts=np.zeros((P, it), np.int32), hyp_Tcw=np.zeros((P, it, 3, 4)),
                   best_iter=np.zeros(P, np.int32), final_niters=np.zeros(P, np.int32))
        d = PnpDiag(*(out[k].ctypes.data for k in ("samples", "counts", "hyp_Tcw", "best_iter", "final_niters")))
    check(lib().vo_pnp_ransac(P, _p(off), _p(p3), _p(p2), _p(cam), int(iterations), C.c_float(reproj_error), C.c_double(confidence),
                              _p(T), _p(x6), _p(mask), _p(ninl), _p(st), C.byref(d) if d is not None else None), "vo_pnp_ransac")
    out.update(Tcw=T[:P].reshape(P, 3, 4), pose6=x6[:P], n_inliers=ninl[:P], status=st[:P],
               inliers=[mask[off[p]:off[p + 1]].astype(bool) for p in range(P)])
    return out


def pnp_workspace_bytes(n_problems, iterations=100):
    return int(lib().vo_pnp_workspace_bytes(int(n_problems), int(iterations)))


def pnp_ransac_dev(n_problems, offsets, pts3d, pts2d, cam4, Tcw12, inlier, n_inliers, status, iterations=100, reproj_error=8.0,
                   confidence=0.99, diag=None, workspace=None, stream=0):
    """vo_pnp_ransac_dev on device tensors (offsets int32 [P+1], pts3d float32 [N, 3], pts2d float32 [N, 2]; outputs Tcw12
    float64 [P, 12], inlier uint8 [N], n_inliers / status int32 [P]); diag: dict of device tensors keyed as PnpDiag.
    workspace: a device uint8 tensor of at least pnp_workspace_bytes(P, iterations) bytes, not shared with a call still in
    flight on another stream (None: one is allocated for this call on the current device)."""
    cam = np.ascontiguousarray(cam4, np.float32)[:4].copy()
    d = None
    if diag is not None:
        d = PnpDiag(*(diag[k].data_ptr() if diag.get(k) is not None else None
                      for k in ("samples", "counts", "hyp_Tcw12", "best_iter", "final_niters")))
    if workspace is None:
        import torch
        workspace = torch.empty(max(pnp_workspace_bytes(n_problems, iterations), 1), dtype=torch.uint8, device=Tcw12.device)
    check(lib().vo_pnp_ransac_dev(int(n_problems), _p(offsets), _p(pts3d), _p(pts2d), _p(cam), int(iterations), C.c_float(reproj_error),
                                  C.c_double(confidence), _p(Tcw12), _p(inlier), _p(n_inliers), _p(status),
                                  C.byref(d) if d is not None else None, _p(workspace), C.c_size_t(workspace.numel()),
                                  _p(stream)), "vo_pnp_ransac_dev")
    return workspace


# ----------------------------------------------------------------------------- loop closing / local mapping / harness I/O
def sim3_ransac_eval(pc1, pc2, px1, px2, maxerr1, maxerr2, cam4, triplets, fix_scale=True, want_flags=True, resident_n=None):
    """Sim3Solver hypotheses (sim3Solver.cpp:98-280) in one launch -> (counts [K], flags [K, n], sims [K, 13]).
    resident_n: pass None arrays and the previous call's n to evaluate against the correspondences that call uploaded."""
    tr = np.ascontiguousarray(triplets, np.int32).reshape(-1, 3)
    cam = np.ascontiguousarray(cam4, np.float32)
    if resident_n is not None:
        a, e1, e2, n = [None] * 4, None, None, int(resident_n)
    else:
        a = [np.ascontiguousarray(v, np.float64) for v in (pc1, pc2, px1, px2)]
        e1, e2 = np.ascontiguousarray(maxerr1, np.int32), np.ascontiguousarray(maxerr2, np.int32)
        n = len(a[0])
    K = len(tr)
    counts, flags, sims = np.zeros(K, np.int32), np.zeros((K, max(n, 1)), np.uint8), np.zeros((K, 13))
    check(lib().vo_sim3_ransac_eval(n, _p(a[0]), _p(a[1]), _p(a[2]), _p(a[3]), _p(e1), _p(e2), _p(cam), K, _p(tr),
                                    int(bool(fix_scale)), _p(counts), _p(flags) if want_flags else None, _p(sims)),
          "vo_sim3_ransac_eval")
    return counts, flags[:, :n], sims


def triangulate(xn1, xn2, Tcw1, Tcw2):
    xn1, xn2 = np.ascontiguousarray(xn1, np.float32), np.ascontiguousarray(xn2, np.float32)
    T1, T2 = np.ascontiguousarray(Tcw1, np.float32).reshape(12), np.ascontiguousarray(Tcw2, np.float32)
    per_pair = T2.size > 12
    n = len(xn1)
    pts, ok = np.zeros((n, 3), np.float32), np.zeros(max(n, 1), np.uint8)
    check(lib().vo_triangulate(n, _p(xn1), _p(xn2), _p(T1), _p(T2), int(per_pair), _p(pts), _p(ok)), "vo_triangulate")
    return pts, ok[:n]


def bow_score(query_words, query_values, cand_words_list, cand_values_list):
    qw, qv = np.ascontiguousarray(query_words, np.int32), np.ascontiguousarray(query_values, np.float64)
    start = np.zeros(len(cand_words_list) + 1, np.int32)
    for i, w in enumerate(cand_words_list):
        start[i + 1] = start[i] + len(w)
    cw = np.ascontiguousarray(np.concatenate(cand_words_list) if start[-1] else np.zeros(0), np.int32)
    cv = np.ascontiguousarray(np.concatenate(cand_values_list) if start[-1] else np.zeros(0), np.float64)
    out = np.zeros(max(len(cand_words_list), 1))
    check(lib().vo_bow_score(len(qw), _p(qw), _p(qv), len(cand_words_list), _p(start), _p(cw), _p(cv), _p(out)), "vo_bow_score")
    return out[:len(cand_words_list)]


def _csr(lists, dtype):
    start = np.zeros(len(lists) + 1, np.int32)
    for i, w in enumerate(lists):
        start[i + 1] = start[i] + len(w)
    flat = np.ascontiguousarray(np.concatenate([np.asarray(w, dtype) for w in lists]) if start[-1] else np.zeros(0, dtype), dtype)
    return start, flat


def bow_vector(words_list, weights_list):
    """vo_bow_vector: per-feature (word, weight) of each frame (vo_bow_transform's output) -> list of (words, values), the
    L1-normalised DBoW3::BowVector of every frame (ascending distinct words)."""
    start, w = _csr(words_list, np.int32)
    _, wt = _csr(weights_list, np.float64)
    nf, n = len(words_list), int(start[-1])
    os_, ow, ov = np.zeros(nf + 1, np.int32), np.zeros(max(n, 1), np.int32), np.zeros(max(n, 1), np.float64)
    check(lib().vo_bow_vector(nf, _p(start), _p(w), _p(wt), _p(os_), _p(ow), _p(ov)), "vo_bow_vector")
    return [(ow[os_[f]:os_[f + 1]].copy(), ov[os_[f]:os_[f + 1]].copy()) for f in range(nf)]


def bow_vector_dev(n_frames, n_features, feat_start, word, weight, out_start, out_words, out_values, stream=0):
    """vo_bow_vector_dev on device tensors (int32 / float64; outputs sized n_frames + 1 and n_features)"""
    check(lib().vo_bow_vector_dev(int(n_frames), int(n_features), _p(feat_start), _p(word), _p(weight), _p(out_start), _p(out_words),
                                  _p(out_values), _p(stream)), "vo_bow_vector_dev")


class KeyFrameDatabase:
    """vo_kfdb: the inverted index of Map::insertKeyFrame with Map::detectRelocalizationCandidates / detectLoopCandidates
    for a batch of queries.  Key-frames are known by their insertion number."""

    OPT_LDS_KEYFRAMES = 1

    def __init__(self, n_words, max_keyframes, max_words_per_keyframe, max_batch, stream=None):
        self._h = C.c_void_p()
        check(lib().vo_kfdb_create(C.byref(self._h), int(n_words), int(max_keyframes), int(max_words_per_keyframe), int(max_batch)),
              "vo_kfdb_create")
        if stream is not None:
            check(lib().vo_kfdb_set_stream(self._h, _p(stream)), "vo_kfdb_set_stream")

    def close(self):
        if getattr(self, "_h", None) and self._h.value and _lib is not None:
            _lib.vo_kfdb_destroy(self._h)
            self._h = C.c_void_p()

    __del__ = close

    def __len__(self):
        return int(lib().vo_kfdb_size(self._h))

    def set_option(self, option, value):
        check(lib().vo_kfdb_set_option(self._h, int(option), int(value)), "vo_kfdb_set_option")

    def insert(self, words, values):
        """numpy arrays (vo_kfdb_insert) or device tensors (vo_kfdb_insert_dev) -> insertion number"""
        idx = C.c_int32(-1)
        if hasattr(words, "data_ptr"):
            check(lib().vo_kfdb_insert_dev(self._h, int(words.numel()), _p(words), _p(values), C.byref(idx)), "vo_kfdb_insert_dev")
        else:
            w, v = np.ascontiguousarray(words, np.int32), np.ascontiguousarray(values, np.float64)
            check(lib().vo_kfdb_insert(self._h, len(w), _p(w), _p(v), C.byref(idx)), "vo_kfdb_insert")
        return int(idx.value)

    def set_neighbors(self, keyframe, ids):
        ids = np.ascontiguousarray(ids, np.int32)
        check(lib().vo_kfdb_set_neighbors(self._h, int(keyframe), len(ids), _p(ids)), "vo_kfdb_set_neighbors")

    def set_neighbors_batch(self, first, lists):
        """set_neighbors for the key-frames first, first + 1, ... in one call"""
        n = np.array([len(x) for x in lists], np.int32)
        ids = np.full((len(lists), 10), -1, np.int32)
        for k, x in enumerate(lists):
            if len(x) > 10:
                raise VoError("at most 10 neighbours per key-frame")
            ids[k, :len(x)] = x
        check(lib().vo_kfdb_set_neighbors_batch(self._h, int(first), len(lists), _p(n), _p(ids)), "vo_kfdb_set_neighbors_batch")

    def neighbors(self, keyframe):
        """the neighbour row of a key-frame as the database holds it -> list; synchronises"""
        n, ids = C.c_int32(0), np.full(10, -1, np.int32)
        check(lib().vo_kfdb_get_neighbors(self._h, int(keyframe), C.byref(n), _p(ids)), "vo_kfdb_get_neighbors")
        return [int(x) for x in ids[:n.value]]

    def _unpack(self, rc, what, n_cand, cand, score, want_scores, max_out):
        if rc == -4 and max_out >= 0:  # VO_ERR_CAPACITY: n_cand still holds the true counts
            raise VoError(f"{what} failed with status {rc}: {lib().vo_last_error().decode()}", n_cand)
        check(rc, what)
        out = [cand[i, :n_cand[i]].copy() for i in range(len(n_cand))]
        return (out, score) if want_scores else out

    def query_reloc(self, queries, stale_score=None, max_out=64, scores=False):
        """queries: list of (words, values) BoW vectors -> list of candidate arrays (insertion numbers, reference order)
        [, score_out [nq, size] float32]"""
        qs, qw = _csr([q[0] for q in queries], np.int32)
        _, qv = _csr([q[1] for q in queries], np.float64)
        nq, size = len(queries), len(self)
        st = None if stale_score is None else np.ascontiguousarray(stale_score, np.float32)
        assert st is None or len(st) == size
        n_cand, cand = np.zeros(max(nq, 1), np.int32), np.zeros((max(nq, 1), max(max_out, 1)), np.int32)
        so = np.zeros((nq, size), np.float32) if scores else None
        rc = lib().vo_kfdb_query_reloc(self._h, nq, _p(qs), _p(qw), _p(qv), _p(st), int(max_out), _p(n_cand), _p(cand), _p(so))
        return self._unpack(rc, "vo_kfdb_query_reloc", n_cand[:nq], cand, so, scores, max_out)

    def query_loop(self, queries, excluded, min_score=None, connected=None, max_out=64, scores=False):
        """excluded: per query, getConnectKFs() and the key-frame itself; min_score: per-query floats, or None with
        connected = per query the non-bad orderedConnectKFs_ (the minimum is then computed as detectLoop does)"""
        qs, qw = _csr([q[0] for q in queries], np.int32)
        _, qv = _csr([q[1] for q in queries], np.float64)
        nq, size = len(queries), len(self)
        es, ex = _csr(excluded, np.int32)
        ms = None if min_score is None else np.ascontiguousarray(min_score, np.float32)
        cs, cn = (None, None) if connected is None else _csr(connected, np.int32)
        n_cand, cand = np.zeros(max(nq, 1), np.int32), np.zeros((max(nq, 1), max(max_out, 1)), np.int32)
        so = np.zeros((nq, size), np.float32) if scores else None
        rc = lib().vo_kfdb_query_loop(self._h, nq, _p(qs), _p(qw), _p(qv), _p(es), _p(ex), _p(ms), _p(cs), _p(cn), int(max_out),
                                      _p(n_cand), _p(cand), _p(so))
        return self._unpack(rc, "vo_kfdb_query_loop", n_cand[:nq], cand, so, scores, max_out)

    def query_reloc_dev(self, nq, q_start, q_words, q_values, stale_score, max_out, n_cand, cand, score_out=None):
        check(lib().vo_kfdb_query_reloc_dev(self._h, int(nq), _p(q_start), _p(q_words), _p(q_values), _p(stale_score), int(max_out),
                                            _p(n_cand), _p(cand), _p(score_out)), "vo_kfdb_query_reloc_dev")

    def query_loop_dev(self, nq, q_start, q_words, q_values, excl_start, excl, min_score, conn_start, conn, max_out, n_cand, cand,
                       score_out=None):
        check(lib().vo_kfdb_query_loop_dev(self._h, int(nq), _p(q_start), _p(q_words), _p(q_values), _p(excl_start), _p(excl),
                                           _p(min_score), _p(conn_start), _p(conn), int(max_out), _p(n_cand), _p(cand), _p(score_out)),
              "vo_kfdb_query_loop_dev")


class KeyFrameStore:
    """vo_kfstore: the features of the key-frames the relocalisation route reads, resident on the device (DESIGN.md
    section 4f).  Key-frames are known by their insertion number, the numbering of KeyFrameDatabase."""

    def __init__(self, max_keyframes, max_features, stream=None):
        self._h = C.c_void_p()
        check(lib().vo_kfstore_create(C.byref(self._h), int(max_keyframes), int(max_features)), "vo_kfstore_create")
        self.max_features = int(max_features)
        self._ba_caps = (1, 1, 1)   # (until enable_local_ba: the library refuses the calls that size their arrays by it)
        if stream is not None:
            check(lib().vo_kfstore_set_stream(self._h, _p(stream)), "vo_kfstore_set_stream")

    def close(self):
        if getattr(self, "_h", None) and self._h.value and _lib is not None:
            _lib.vo_kfstore_destroy(self._h)
            self._h = C.c_void_p()

    __del__ = close

    def __len__(self):
        return int(lib().vo_kfstore_size(self._h))

    def insert(self, k):
        """k: the dict Tracker.set_reloc_candidates takes per candidate (numpy arrays) -> insertion number"""
        a = dict(angle=np.ascontiguousarray(k["angle"], np.float32), desc=np.ascontiguousarray(k["desc"], np.uint8),
                 flags=np.ascontiguousarray(k["flags"], np.uint8), points=np.ascontiguousarray(k["points"], np.float64),
                 ids=np.ascontiguousarray(k["ids"], np.int32), point_desc=np.ascontiguousarray(k["point_desc"], np.uint8),
                 min_distance=np.ascontiguousarray(k["min_dist"], np.float32), max_distance=np.ascontiguousarray(k["max_dist"], np.float32))
        nodes = BowNodes(np.asarray(k["nodes"]))
        rc = RelocCandidate()
        rc.n, rc.bad = len(a["flags"]), int(bool(k.get("bad", False)))
        for key, v in a.items():
            setattr(rc, key, v.ctypes.data)
        rc.nodes = C.addressof(nodes.view)
        idx = C.c_int32(-1)
        check(lib().vo_kfstore_insert(self._h, C.byref(rc), C.byref(idx)), "vo_kfstore_insert")
        return int(idx.value)

    def insert_dev(self, k):
        """the same from device tensors (angle f32 [n], desc u8 [n, 32], nodes i32 [n] per-feature node ids, flags u8 [n],
        points f64 [n, 3], ids i32 [n], point_desc u8 [n, 32], min_dist / max_dist f32 [n]); no synchronisation"""
        idx = C.c_int32(-1)
        check(lib().vo_kfstore_insert_dev(self._h, int(k["flags"].numel()), int(bool(k.get("bad", False))), _p(k["angle"]), _p(k["desc"]),
                                          _p(k["nodes"]), _p(k["flags"]), _p(k["points"]), _p(k["ids"]), _p(k["point_desc"]),
                                          _p(k["min_dist"]), _p(k["max_dist"]), C.byref(idx)), "vo_kfstore_insert_dev")
        return int(idx.value)

    def set_bad(self, keyframe, bad=True):
        check(lib().vo_kfstore_set_bad(self._h, int(keyframe), int(bool(bad))), "vo_kfstore_set_bad")

    def update_points(self, keyframe, flags, points, ids, point_desc, min_dist, max_dist):
        """the map side of a key-frame replaced (numpy arrays [n], n as inserted)"""
        a = lambda x, dt: np.ascontiguousarray(x, dt)
        check(lib().vo_kfstore_update_points(self._h, int(keyframe), _p(a(flags, np.uint8)), _p(a(points, np.float64)), _p(a(ids, np.int32)),
                                             _p(a(point_desc, np.uint8)), _p(a(min_dist, np.float32)), _p(a(max_dist, np.float32))),
              "vo_kfstore_update_points")

    MAX_NEIGHBORS, MAX_CHILDREN = 10, 64

    def set_graph(self, keyframe, neighbors, children, parent=-1):
        """the links build_local_map walks: neighbors = getBestCovisibleKFs(10) in its order, children in ascending
        key-frame number (at most MAX_CHILDREN), parent a key-frame number or -1"""
        nb, ch = np.ascontiguousarray(neighbors, np.int32), np.ascontiguousarray(children, np.int32)
        check(lib().vo_kfstore_set_graph(self._h, int(keyframe), len(nb), _p(nb), len(ch), _p(ch), int(parent)), "vo_kfstore_set_graph")

    def set_graph_batch(self, first, neighbors, children, parents):
        """set_graph for the key-frames first, first + 1, ... in one call (lists of lists, a list of parents)"""
        count = len(parents)
        for name, lists, cap in (("neighbours", neighbors, self.MAX_NEIGHBORS), ("children", children, self.MAX_CHILDREN)):
            if any(len(x) > cap for x in lists):
                raise VoError(f"vo_kfstore_set_graph_batch failed with status -4: more than {cap} {name} for a key-frame")
        n_nb = np.array([len(x) for x in neighbors], np.int32)
        n_ch = np.array([len(x) for x in children], np.int32)
        nb = np.full((count, self.MAX_NEIGHBORS), -1, np.int32)
        ch = np.full((count, self.MAX_CHILDREN), -1, np.int32)
        for k in range(count):
            nb[k, :n_nb[k]] = neighbors[k]
            ch[k, :n_ch[k]] = children[k]
        par = np.ascontiguousarray(parents, np.int32)   # (named: the array must outlive the call)
        check(lib().vo_kfstore_set_graph_batch(self._h, int(first), count, _p(n_nb), _p(nb), _p(n_ch), _p(ch), _p(par)),
              "vo_kfstore_set_graph_batch")

    def set_normals(self, keyframe, normals):
        """MapPoint::normalVector_ per feature [n, 3] (n as inserted); zero until set, and a zero normal fails isInFrame"""
        nrm = np.ascontiguousarray(normals, np.float64)
        check(lib().vo_kfstore_set_normals(self._h, int(keyframe), _p(nrm)), "vo_kfstore_set_normals")

    CONNECTIONS_INVALID, CONNECTIONS_CAPACITY = 1, 2

    def enable_connections(self):
        """the covisibility graph and spanning tree maintained on the device from now on; valid on
        an empty store only, and set_graph / set_graph_batch are invalid afterwards"""
        check(lib().vo_kfstore_enable_connections(self._h), "vo_kfstore_enable_connections")

    def update_connections(self, keyframes):
        """KeyFrame::updateConnections for the listed key-frames in list order (repeats allowed).  A list / numpy array is
        validated and synchronises once; a device tensor (int32) is enqueued only and must stay untouched until the
        store's stream has passed the call"""
        if hasattr(keyframes, "data_ptr"):
            check(lib().vo_kfstore_update_connections_dev(self._h, int(keyframes.numel()), _p(keyframes)), "vo_kfstore_update_connections_dev")
            return
        kf = np.ascontiguousarray(keyframes, np.int32).reshape(-1)
        check(lib().vo_kfstore_update_connections(self._h, len(kf), _p(kf)), "vo_kfstore_update_connections")

    def connections_status(self):
        """the sticky word of update_connections (CONNECTIONS_INVALID | CONNECTIONS_CAPACITY), cleared by the read"""
        w = C.c_int32(0)
        check(lib().vo_kfstore_connections_status(self._h, C.byref(w)), "vo_kfstore_connections_status")
        return int(w.value)

    def connections(self, keyframe):
        """-> dict(n_connected, weights [size] (0: not connected), ordered, ordered_weights (orderedConnectKFs_ /
        orderedWTs_), parent, children (ascending, at most MAX_CHILDREN)) as plain lists and ints"""
        size = len(self)
        w, o, ow = (np.zeros(max(size, 1), np.int32) for _ in range(3))
        ch = np.zeros(self.MAX_CHILDREN, np.int32)
        nc, no, par, nch = (C.c_int32(0) for _ in range(4))
        check(lib().vo_kfstore_get_connections(self._h, int(keyframe), C.byref(nc), _p(w), C.byref(no), _p(o), _p(ow), C.byref(par),
                                               C.byref(nch), _p(ch)), "vo_kfstore_get_connections")
        return dict(n_connected=int(nc.value), weights=[int(x) for x in w[:size]], ordered=[int(x) for x in o[:no.value]],
                    ordered_weights=[int(x) for x in ow[:no.value]], parent=int(par.value), children=[int(x) for x in ch[:nch.value]])

    CULL_KEPT, CULL_ERASED, CULL_PENDING, CULL_SKIPPED = 0, 1, 2, 3

    def enable_culling(self):
        """cullingKeyFrames / eraseKeyFrame on the device from now on; valid on an empty store after
        enable_connections only"""
        check(lib().vo_kfstore_enable_culling(self._h), "vo_kfstore_enable_culling")

    def set_keypoints(self, keyframe, octave, depth, u_right):
        """octave (int32), depth and u_right (float32; < 0: none) per feature [n], n as inserted.  numpy arrays are copied and
        synchronise once; device tensors (all three) are enqueued only"""
        if hasattr(octave, "data_ptr"):
            check(lib().vo_kfstore_set_keypoints_dev(self._h, int(keyframe), _p(octave), _p(depth), _p(u_right)), "vo_kfstore_set_keypoints_dev")
            return
        o, d, u = np.ascontiguousarray(octave, np.int32), np.ascontiguousarray(depth, np.float32), np.ascontiguousarray(u_right, np.float32)
        check(lib().vo_kfstore_set_keypoints(self._h, int(keyframe), _p(o), _p(d), _p(u)), "vo_kfstore_set_keypoints")

    def set_erase_lock(self, keyframe, on=True):
        """notEraseLoopDetecting_: a locked key-frame is marked pending instead of being erased"""
        check(lib().vo_kfstore_set_erase_lock(self._h, int(keyframe), int(bool(on))), "vo_kfstore_set_erase_lock")

    def cull_keyframes(self, current, th_depth):
        """LocalMapping::cullingKeyFrames for the current key-frame; enqueued only"""
        check(lib().vo_kfstore_cull_keyframes(self._h, int(current), C.c_float(th_depth)), "vo_kfstore_cull_keyframes")

    def erase_keyframe(self, keyframe):
        """KeyFrame::eraseKeyFrame; enqueued only"""
        check(lib().vo_kfstore_erase_keyframe(self._h, int(keyframe)), "vo_kfstore_erase_keyframe")

    def cull_result(self):
        """the last cull call -> [(key-frame, mp_cnt, re_obs, decision)] per candidate in list order"""
        size = max(len(self), 1)
        kf, mp, re, de = (np.zeros(size, np.int32) for _ in range(4))
        n = C.c_int32(0)
        check(lib().vo_kfstore_cull_result(self._h, C.byref(n), _p(kf), _p(mp), _p(re), _p(de)), "vo_kfstore_cull_result")
        return [(int(kf[t]), int(mp[t]), int(re[t]), int(de[t])) for t in range(n.value)]

    def cull_state(self, keyframe):
        """-> dict(erased, locked, pending) of a key-frame"""
        e, l, p = (C.c_int32(0) for _ in range(3))
        check(lib().vo_kfstore_cull_state(self._h, int(keyframe), C.byref(e), C.byref(l), C.byref(p)), "vo_kfstore_cull_state")
        return dict(erased=int(e.value), locked=int(l.value), pending=int(p.value))

    def flags(self, keyframe, n=None):
        """-> (flags bytes as a list, bad) of a key-frame as the store holds them"""
        f = np.zeros(self.max_features, np.uint8)
        bad = C.c_int32(0)
        check(lib().vo_kfstore_get_flags(self._h, int(keyframe), _p(f), C.byref(bad)), "vo_kfstore_get_flags")
        return [int(x) for x in (f if n is None else f[:n])], int(bad.value)

    NP_SEARCHED, NP_SKIPPED_BAD, NP_SKIPPED_BASELINE, NP_SKIPPED_NO_POSE, NP_NOT_REACHED = 0, 1, 2, 3, 4

    def enable_mapping(self, cam6, scale_factors, first_point_id=0):
        """createNewMapPoints on the device from now on; valid on an empty store after enable_culling
        only.  cam6 = fx, fy, cx, cy, bf, b; scale_factors = scaleFactors_ (at most 16 levels)"""
        cam, sf = np.ascontiguousarray(cam6, np.float32).reshape(6), np.ascontiguousarray(scale_factors, np.float32).reshape(-1)
        check(lib().vo_kfstore_enable_mapping(self._h, _p(cam), len(sf), _p(sf), int(first_point_id)), "vo_kfstore_enable_mapping")

    def set_pose(self, keyframe, Tcw12):
        """Tcw as 12 doubles, R row-major then t.  A numpy array is copied and synchronises once; a device tensor (float64) is
        enqueued only"""
        if hasattr(Tcw12, "data_ptr"):
            _need_tensor(Tcw12, "float64", 12, "set_pose")
            check(lib().vo_kfstore_set_pose_dev(self._h, int(keyframe), _p(Tcw12)), "vo_kfstore_set_pose_dev")
            return
        T = np.ascontiguousarray(Tcw12, np.float64).reshape(12)
        check(lib().vo_kfstore_set_pose(self._h, int(keyframe), _p(T)), "vo_kfstore_set_pose")

    def set_keypoint_xy(self, keyframe, xy):
        """unKeypoints_[i].pt per feature [n, 2] (float32, n as inserted); numpy: copied, synchronises once; a device tensor:
        enqueued only"""
        if hasattr(xy, "data_ptr"):
            _need_tensor(xy, "float32", None, "set_keypoint_xy")
            check(lib().vo_kfstore_set_keypoint_xy_dev(self._h, int(keyframe), _p(xy)), "vo_kfstore_set_keypoint_xy_dev")
            return
        a = np.ascontiguousarray(xy, np.float32)
        check(lib().vo_kfstore_set_keypoint_xy(self._h, int(keyframe), _p(a)), "vo_kfstore_set_keypoint_xy")

    def next_point_id(self):
        """the id the next created map point gets (MapPoint::factory_id_); synchronises"""
        v = C.c_int32(0)
        check(lib().vo_kfstore_next_point_id(self._h, C.byref(v)), "vo_kfstore_next_point_id")
        return int(v.value)

    def create_map_points(self, current, max_neighbors=10):
        """LocalMapping::createNewMapPoints for the current key-frame against the first max_neighbors of its neighbours;
        enqueued only"""
        check(lib().vo_kfstore_create_map_points(self._h, int(current), int(max_neighbors)), "vo_kfstore_create_map_points")

    def new_points_result(self):
        """the last create_map_points call -> dict(neighbors [(key-frame, status, n_matches, n_created)] per entry of the
        current key-frame's list the call saw, created [(neighbour key-frame, idx1, idx2, id)] in creation order)"""
        kf, st, nm, nc = (np.zeros(self.MAX_NEIGHBORS, np.int32) for _ in range(4))
        created = np.zeros((self.MAX_NEIGHBORS * self.max_features, 4), np.int32)
        n = C.c_int32(0)
        check(lib().vo_kfstore_new_points_result(self._h, C.byref(n), _p(kf), _p(st), _p(nm), _p(nc), _p(created), len(created)),
              "vo_kfstore_new_points_result")
        total = int(nc[:n.value].sum())
        return dict(neighbors=[(int(kf[i]), int(st[i]), int(nm[i]), int(nc[i])) for i in range(n.value)],
                    created=[tuple(int(x) for x in row) for row in created[:total]])

    def points(self, keyframe, n):
        """the map side of a key-frame as the store holds it (n as inserted) -> dict(flags, ids, points, point_desc, min_dist,
        max_dist, normals) of numpy arrays"""
        n = int(n)
        out = dict(flags=np.zeros(n, np.uint8), ids=np.zeros(n, np.int32), points=np.zeros((n, 3)), point_desc=np.zeros((n, 32), np.uint8),
                   min_dist=np.zeros(n, np.float32), max_dist=np.zeros(n, np.float32), normals=np.zeros((n, 3)))
        check(lib().vo_kfstore_get_points(self._h, int(keyframe), *(_p(out[k]) for k in ("flags", "ids", "points", "point_desc", "min_dist",
                                                                                         "max_dist", "normals"))), "vo_kfstore_get_points")
        return out

    def pose(self, keyframe):
        """-> (Tcw12 as the store holds it, whether it has been set)"""
        T, on = np.zeros(12), C.c_int32(0)
        check(lib().vo_kfstore_get_pose(self._h, int(keyframe), _p(T), C.byref(on)), "vo_kfstore_get_pose")
        return T, bool(on.value)

    CONNECTIONS_LOCAL_BA_CAPACITY = 4
    BA_WINDOW_OK, BA_WINDOW_EMPTY, BA_WINDOW_OVERFLOW = 0, 1, 2
    BA_RECORD = ("n_cams", "n_local", "n_fixed", "n_points", "n_edges", "n_dropped", "status", "current", "n_erased", "n_feature0", "n_dead")

    def enable_local_ba(self, max_cams, max_points, max_edges):
        """solveLocalBAPoseAndPoint's window and write-back on the device from now on; valid on an
        empty store after enable_mapping only"""
        check(lib().vo_kfstore_enable_local_ba(self._h, int(max_cams), int(max_points), int(max_edges)), "vo_kfstore_enable_local_ba")
        self._ba_caps = (int(max_cams), int(max_points), int(max_edges))

    def set_point_refs(self, keyframe, ref_kf):
        """MapPoint::keyFrame_ref_ per feature [n] as a key-frame number, -1: unknown.  numpy: validated, copied, synchronises
        once; a device tensor (int32): enqueued only"""
        if hasattr(ref_kf, "data_ptr"):
            _need_tensor(ref_kf, "int32", None, "set_point_refs")
            check(lib().vo_kfstore_set_point_refs_dev(self._h, int(keyframe), _p(ref_kf)), "vo_kfstore_set_point_refs_dev")
            return
        r = np.ascontiguousarray(ref_kf, np.int32)
        check(lib().vo_kfstore_set_point_refs(self._h, int(keyframe), _p(r)), "vo_kfstore_set_point_refs")

    def point_refs(self, keyframe, n):
        r = np.zeros(int(n), np.int32)
        check(lib().vo_kfstore_get_point_refs(self._h, int(keyframe), _p(r)), "vo_kfstore_get_point_refs")
        return r

    def local_ba_window(self, current):
        """the window of Optimizer::solveLocalBAPoseAndPoint for the current key-frame; enqueued only"""
        check(lib().vo_kfstore_local_ba_window(self._h, int(current)), "vo_kfstore_local_ba_window")

    def local_ba_window_result(self):
        """the last window -> dict(record (dict over BA_RECORD), cam_keyframe, fixed, poses, point_id, points, e_cam, e_pt,
        e_feature, e_obs, e_inv_sigma) cut to the record's counts; the solver's names, so that dict(w, cam=...) is a problem
        of BundleAdjuster"""
        nc, npt, ne = self._ba_caps
        rec = np.zeros(16, np.int32)
        a = dict(cam_keyframe=np.zeros(nc, np.int32), fixed=np.zeros(nc, np.uint8), poses=np.zeros((nc, 6)), point_id=np.zeros(npt, np.int32),
                 points=np.zeros((npt, 3)), e_cam=np.zeros(ne, np.int32), e_pt=np.zeros(ne, np.int32), e_feature=np.zeros(ne, np.int32),
                 e_obs=np.zeros((ne, 3)), e_inv_sigma=np.zeros(ne))
        check(lib().vo_kfstore_local_ba_window_result(self._h, _p(rec), *(_p(v) for v in a.values())), "vo_kfstore_local_ba_window_result")
        r = {k: int(rec[i]) for i, k in enumerate(self.BA_RECORD)}
        ok = r["status"] == self.BA_WINDOW_OK
        cut = dict(cam_keyframe="n_cams", fixed="n_cams", poses="n_cams", point_id="n_points", points="n_points")
        return dict({k: v[:r[cut.get(k, "n_edges")] if ok else 0].copy() for k, v in a.items()}, record=r)

    def local_ba_apply(self, poses6, points, edge_erase):
        """a solver's result for the last window written back (host arrays in the window's order)"""
        po, pt, er = np.ascontiguousarray(poses6, np.float64), np.ascontiguousarray(points, np.float64), np.ascontiguousarray(edge_erase, np.uint8)
        check(lib().vo_kfstore_local_ba_apply(self._h, _p(po), _p(pt), _p(er)), "vo_kfstore_local_ba_apply")

    def refresh_points(self, ids):
        """MapPoint::updateNormalAndDepth for the listed map-point ids"""
        a = np.ascontiguousarray(ids, np.int32).reshape(-1)
        check(lib().vo_kfstore_refresh_points(self._h, len(a), _p(a)), "vo_kfstore_refresh_points")

    def local_ba(self, ba, current, stop=None):
        """window, solve on the caller's BundleAdjuster (its problem is replaced), write-back -> (summaries, status): status 0,
        or -5 when the stop flag (a ctypes.c_ubyte, or None) was set before the first solve; other failures raise"""
        sums = (LmSummary * 2)()
        rc = lib().vo_kfstore_local_ba(self._h, ba._h, int(current), None if stop is None else C.byref(stop), C.byref(sums))
        if rc not in (0, -5):
            check(rc, "vo_kfstore_local_ba")
        return sums, rc

    CONNECTIONS_UPKEEP_CAPACITY = 8
    DESC_MAX_HOLDERS = 1024
    UPKEEP_PROCESS, UPKEEP_CULL, UPKEEP_CREATED = 1, 2, 3
    UPKEEP_RECORD = ("kind", "current", "n_tracked", "n_new", "n_appended", "n_dead", "n_ratio", "n_few_obs", "n_matured", "n_kept",
                     "n_erased", "n_recent")

    def enable_point_upkeep(self, max_recent):
        """processNewKeyFrame / cullingMapPoints on the device from now on; valid on an empty store after
        enable_local_ba only.  max_recent: the entries addedMapPoints_ may hold"""
        check(lib().vo_kfstore_enable_point_upkeep(self._h, int(max_recent)), "vo_kfstore_enable_point_upkeep")
        self._max_recent = int(max_recent)

    def compute_descriptors(self, ids):
        """MapPoint::computeDescriptor for the listed map-point ids.  A list / numpy array is validated, copied and synchronises
        once; a device tensor (int32; negative entries are skipped) is enqueued only"""
        if hasattr(ids, "data_ptr"):
            _need_tensor(ids, "int32", None, "compute_descriptors")
            check(lib().vo_kfstore_compute_descriptors_dev(self._h, int(ids.numel()), _p(ids)), "vo_kfstore_compute_descriptors_dev")
            return
        a = np.ascontiguousarray(ids, np.int32).reshape(-1)
        check(lib().vo_kfstore_compute_descriptors(self._h, len(a), _p(a)), "vo_kfstore_compute_descriptors")

    def process_new_keyframe(self, current):
        """LocalMapping::processNewKeyFrame for the key-frame just inserted; enqueued only"""
        check(lib().vo_kfstore_process_new_keyframe(self._h, int(current)), "vo_kfstore_process_new_keyframe")

    def add_point_stats(self, ids, visible, found):
        """visible_cnt_ / found_cnt_ of the listed recent points grown by the increments.  Lists / numpy arrays are validated,
        copied and synchronise once; device tensors (int32, all three) are enqueued only"""
        if hasattr(ids, "data_ptr"):
            n = int(ids.numel())
            for t in (ids, visible, found):
                _need_tensor(t, "int32", n, "add_point_stats")
            check(lib().vo_kfstore_add_point_stats_dev(self._h, n, _p(ids), _p(visible), _p(found)), "vo_kfstore_add_point_stats_dev")
            return
        a, v, f = (np.ascontiguousarray(x, np.int32).reshape(-1) for x in (ids, visible, found))
        if not len(a) == len(v) == len(f):
            raise VoError("add_point_stats: ids, visible and found differ in length")
        check(lib().vo_kfstore_add_point_stats(self._h, len(a), _p(a), _p(v), _p(f)), "vo_kfstore_add_point_stats")

    def cull_map_points(self, current):
        """LocalMapping::cullingMapPoints for the current key-frame; enqueued only"""
        check(lib().vo_kfstore_cull_map_points(self._h, int(current)), "vo_kfstore_cull_map_points")

    def recent_points(self):
        """addedMapPoints_ -> [(id, first_kf, found, visible)] in ascending id; synchronises"""
        r = getattr(self, "_max_recent", 1)
        cols = [np.zeros(r, np.int32) for _ in range(4)]
        n = C.c_int32(0)
        check(lib().vo_kfstore_recent_points(self._h, C.byref(n), *(_p(c) for c in cols)), "vo_kfstore_recent_points")
        return [tuple(int(c[i]) for c in cols) for i in range(n.value)]

    def upkeep_result(self):
        """the last upkeep call -> dict over UPKEEP_RECORD plus erased (the ids a cull call erased, ascending); synchronises"""
        rec, er = np.zeros(16, np.int32), np.zeros(getattr(self, "_max_recent", 1), np.int32)
        check(lib().vo_kfstore_upkeep_result(self._h, _p(rec), _p(er)), "vo_kfstore_upkeep_result")
        out = {k: int(rec[i]) for i, k in enumerate(self.UPKEEP_RECORD)}
        out["erased"] = [int(x) for x in er[:out["n_erased"] if out["kind"] == self.UPKEEP_CULL else 0]]
        return out

    CONNECTIONS_FUSE_CAPACITY = 16
    FUSE_MAX_CARRIERS, FUSE_MAX_STEPS = 1024, 61
    FUSE_COLUMNS = ("passed", "matches", "adds", "kept_org", "kept_candidate", "cleared")

    def enable_fuse(self, bounds, max_candidates):
        """searchInNeighbors / fuseMapPoints on the device from now on; valid on an empty store after
        enable_point_upkeep only.  bounds: xMin, xMax, yMin, yMax of the undistorted image; max_candidates: the matches a call
        may make"""
        b = np.ascontiguousarray(bounds, np.float32).reshape(4)
        check(lib().vo_kfstore_enable_fuse(self._h, _p(b), int(max_candidates)), "vo_kfstore_enable_fuse")

    def fuse_map_points(self, target, ids, threshold=3.0):
        """Matcher::fuseMapPoints(target, ids, threshold): one fuse call on its own.  A list / numpy array is copied and
        synchronises once; a device tensor (int32; negative entries are skipped) is enqueued only"""
        if hasattr(ids, "data_ptr"):
            _need_tensor(ids, "int32", None, "fuse_map_points")
            check(lib().vo_kfstore_fuse_map_points_dev(self._h, int(target), int(ids.numel()), _p(ids), C.c_float(threshold)),
                  "vo_kfstore_fuse_map_points_dev")
            return
        a = np.ascontiguousarray(ids, np.int32).reshape(-1)
        check(lib().vo_kfstore_fuse_map_points(self._h, int(target), len(a), _p(a), C.c_float(threshold)), "vo_kfstore_fuse_map_points")

    def search_in_neighbors(self, current):
        """LocalMapping::searchInNeighbors for the current key-frame; enqueued only"""
        check(lib().vo_kfstore_search_in_neighbors(self._h, int(current)), "vo_kfstore_search_in_neighbors")

    def fuse_result(self):
        """the last fuse call -> dict(targets, per_target [(passed, matches, adds, kept_org, kept_candidate, cleared)], totals);
        synchronises"""
        rec, tg, per = np.zeros(8, np.int32), np.zeros(self.FUSE_MAX_STEPS, np.int32), np.zeros((self.FUSE_MAX_STEPS, 6), np.int32)
        check(lib().vo_kfstore_fuse_result(self._h, _p(rec), _p(tg), _p(per)), "vo_kfstore_fuse_result")
        n = int(rec[0])
        return dict(targets=[int(t) for t in tg[:n]], per_target=[tuple(int(x) for x in row) for row in per[:n]],
                    totals=tuple(int(x) for x in rec[1:7]))

    LOOP_MAX_CANDIDATES, CONNECTIONS_LOOP_RAND_SHORT, CONNECTIONS_LOOP_CAPACITY = 16, 32, 64
    LOOP_UNDECIDED, LOOP_NO_MATCH, LOOP_REJECTED, LOOP_ACCEPTED = 0, 1, 2, 3
    LOOP_RECORD = ("state", "match_pos", "match_kf", "rounds", "verifications", "rand_used", "refine_inliers", "match_cnt", "n_loop_points")
    LOOP_PER_CANDIDATE = ("kf", "reason", "bow_matches", "n", "max_iters", "iterations", "inliers_best", "verifications")

    def enable_loop(self, max_candidates, max_loop_points, max_rand):
        """LoopClosing::computeSim3 on the device from now on; valid on an empty store after enable_fuse
        only.  max_candidates <= LOOP_MAX_CANDIDATES; max_loop_points: the loop points a match may collect; max_rand: the
        rand() values a call may bring (3 * 300 * candidates always suffice)"""
        check(lib().vo_kfstore_enable_loop(self._h, int(max_candidates), int(max_loop_points), int(max_rand)), "vo_kfstore_enable_loop")
        self._loop_caps = (int(max_candidates), int(max_loop_points))

    def compute_sim3(self, current, candidates, rand_values, rand_max, fix_scale=True, max_rounds=8):
        """computeSim3 for the current key-frame over the candidates in their order, drawing from rand_values.  Lists / numpy
        arrays are copied and the call synchronises once; device tensors (int32, both) are enqueued only"""
        if hasattr(candidates, "data_ptr"):
            _need_tensor(candidates, "int32", None, "compute_sim3")
            _need_tensor(rand_values, "int32", None, "compute_sim3")
            check(lib().vo_kfstore_compute_sim3_dev(self._h, int(current), int(candidates.numel()), _p(candidates), int(bool(fix_scale)),
                                                    int(rand_values.numel()), _p(rand_values), int(rand_max), int(max_rounds)),
                  "vo_kfstore_compute_sim3_dev")
            return
        c, r = np.ascontiguousarray(candidates, np.int32).reshape(-1), np.ascontiguousarray(rand_values, np.int32).reshape(-1)
        check(lib().vo_kfstore_compute_sim3(self._h, int(current), len(c), _p(c), int(bool(fix_scale)), len(r), _p(r), int(rand_max),
                                            int(max_rounds)), "vo_kfstore_compute_sim3")

    def compute_sim3_continue(self, max_rounds):
        """more rounds on the state the last compute_sim3 left; enqueued only"""
        check(lib().vo_kfstore_compute_sim3_continue(self._h, int(max_rounds)), "vo_kfstore_compute_sim3_continue")

    def loop_result(self, n_current=None):
        """the last compute_sim3 -> dict over LOOP_RECORD plus per_candidate (dicts over LOOP_PER_CANDIDATE), Scm, Scw [13],
        match_ids [n_current] and loop_point_ids; synchronises"""
        C_, P = getattr(self, "_loop_caps", (1, 1))
        rec, per = np.zeros(16, np.int32), np.zeros((C_, 8), np.int32)
        Scm, Scw = np.zeros(13), np.zeros(13)
        mids = np.full(self.max_features, -1, np.int32)
        nlp, lids = C.c_int32(0), np.zeros(P, np.int32)
        check(lib().vo_kfstore_loop_result(self._h, _p(rec), _p(per), _p(Scm), _p(Scw), _p(mids), C.byref(nlp), _p(lids)), "vo_kfstore_loop_result")
        out = {k: int(rec[i]) for i, k in enumerate(self.LOOP_RECORD)}
        out["per_candidate"] = [{k: int(row[i]) for i, k in enumerate(self.LOOP_PER_CANDIDATE)} for row in per]
        out.update(Scm=Scm, Scw=Scw, match_ids=mids if n_current is None else mids[:n_current], loop_point_ids=lids[:nlp.value].copy())
        return out

    def loop_solver_inputs(self, position):
        """Sim3Solver's arrays of candidate `position` of the last compute_sim3 -> dict(pc1, pc2 [N, 3], px1, px2 [N, 2], me1, me2,
        index [N]); synchronises"""
        n, NK = C.c_int32(0), self.max_features
        pc1, pc2, px1, px2 = np.zeros((NK, 3)), np.zeros((NK, 3)), np.zeros((NK, 2)), np.zeros((NK, 2))
        me1, me2, idx = np.zeros(NK, np.int32), np.zeros(NK, np.int32), np.zeros(NK, np.int32)
        check(lib().vo_kfstore_loop_solver_inputs(self._h, int(position), C.byref(n), _p(pc1), _p(pc2), _p(px1), _p(px2), _p(me1), _p(me2),
                                                  _p(idx)), "vo_kfstore_loop_solver_inputs")
        N = n.value
        return dict(pc1=pc1[:N], pc2=pc2[:N], px1=px1[:N], px2=px2[:N], me1=me1[:N], me2=me2[:N], index=idx[:N])

    MAX_LOOP_EDGES = 8
    CONNECTIONS_POSE_GRAPH_CAPACITY = 128
    POSE_GRAPH_MAX_NODES = 683
    PG_RECORD = ("n_nodes", "n_edges", "n_a", "n_b", "n_c", "n_d", "status", "curr", "match", "fixed_node", "n_points_moved", "n_unanchored")

    def enable_pose_graph(self, max_edges, max_corrected, max_corrected_points):
        """solvePoseGraphLoop's gather and write-back on the device from now on; valid on an empty store
        after enable_local_ba only"""
        check(lib().vo_kfstore_enable_pose_graph(self._h, int(max_edges), int(max_corrected), int(max_corrected_points)),
              "vo_kfstore_enable_pose_graph")
        self._pg_edges = int(max_edges)

    def add_loop_edge(self, a, b):
        """KeyFrame::addLoopEdge both ways, with both erase locks; enqueued only"""
        check(lib().vo_kfstore_add_loop_edge(self._h, int(a), int(b)), "vo_kfstore_add_loop_edge")

    def loop_edges(self, keyframe):
        """-> the loop edges of a key-frame, ascending"""
        n, e = C.c_int32(0), np.zeros(self.MAX_LOOP_EDGES, np.int32)
        check(lib().vo_kfstore_get_loop_edges(self._h, int(keyframe), C.byref(n), _p(e)), "vo_kfstore_get_loop_edges")
        return [int(x) for x in e[:n.value]]

    @staticmethod
    def _pg_inputs(inp, dev):
        """inp: dict(corr_kf, S_corr, S_uncorr, lc_start, lc_kf, cp_id, cp_ref) -> the seven arrays as the entry points take them"""
        if dev:
            for k, dt in (("corr_kf", "int32"), ("S_corr", "float64"), ("S_uncorr", "float64"), ("lc_start", "int32"), ("lc_kf", "int32"),
                          ("cp_id", "int32"), ("cp_ref", "int32")):
                _need_tensor(inp[k], dt, None, "pose_graph_window")
            return [inp[k] for k in ("corr_kf", "S_corr", "S_uncorr", "lc_start", "lc_kf", "cp_id", "cp_ref")]
        i32, f64 = (lambda x: np.ascontiguousarray(x, np.int32).reshape(-1)), (lambda x: np.ascontiguousarray(x, np.float64).reshape(-1, 8))
        return [i32(inp["corr_kf"]), f64(inp["S_corr"]), f64(inp["S_uncorr"]), i32(inp["lc_start"]), i32(inp["lc_kf"]), i32(inp["cp_id"]),
                i32(inp["cp_ref"])]

    def pose_graph_window(self, curr, match, inp):
        """the pose graph of a loop closure curr - match from correctLoop's outputs (inp: see _pg_inputs).  numpy arrays / lists
        are validated, copied once and the call synchronises once; device tensors (all seven) are enqueued only"""
        dev = hasattr(inp["corr_kf"], "data_ptr")
        ck, sc, su, ls, lk, ci, cr = self._pg_inputs(inp, dev)   # (named: the arrays must outlive the call)
        if dev:
            check(lib().vo_kfstore_pose_graph_window_dev(self._h, int(curr), int(match), int(ck.numel()), _p(ck), _p(sc), _p(su), _p(ls),
                                                         int(lk.numel()), _p(lk), int(ci.numel()), _p(ci), _p(cr)),
                  "vo_kfstore_pose_graph_window_dev")
            return
        if len(ls) != len(ck) + 1 or len(sc) != len(ck) or len(su) != len(ck) or len(cr) != len(ci) or len(lk) < (int(ls[-1]) if len(ls) else 0):
            raise VoError("vo_kfstore_pose_graph_window failed with status -1: the arrays' lengths do not fit each other")
        check(lib().vo_kfstore_pose_graph_window(self._h, int(curr), int(match), len(ck), _p(ck), _p(sc), _p(su), _p(ls), _p(lk), len(ci),
                                                 _p(ci), _p(cr)), "vo_kfstore_pose_graph_window")

    def pose_graph_window_result(self):
        """the last window -> dict(record (dict over PG_RECORD), node_kf, quats, trans, scales, e_i, e_j, q_meas, t_meas, s_meas) cut
        to the record's counts; with fixed = record['fixed_node'] it is a graph Optimizer.solvePoseGraphLoop takes"""
        nn, ne = self.POSE_GRAPH_MAX_NODES, getattr(self, "_pg_edges", 1)
        rec = np.zeros(16, np.int32)
        a = dict(node_kf=np.zeros(nn, np.int32), quats=np.zeros((nn, 4)), trans=np.zeros((nn, 3)), scales=np.zeros(nn), e_i=np.zeros(ne, np.int32),
                 e_j=np.zeros(ne, np.int32), q_meas=np.zeros((ne, 4)), t_meas=np.zeros((ne, 3)), s_meas=np.zeros(ne))
        check(lib().vo_kfstore_pose_graph_window_result(self._h, _p(rec), *(_p(v) for v in a.values())), "vo_kfstore_pose_graph_window_result")
        r = {k: int(rec[i]) for i, k in enumerate(self.PG_RECORD)}
        ok = r["status"] == self.BA_WINDOW_OK
        cut = dict(node_kf="n_nodes", quats="n_nodes", trans="n_nodes", scales="n_nodes")
        return dict({k: v[:r[cut.get(k, "n_edges")] if ok else 0].copy() for k, v in a.items()}, record=r, fixed=r["fixed_node"])

    def pose_graph_apply(self, quats, trans):
        """a solver's result for the last window written back (host arrays in node order)"""
        q, t = np.ascontiguousarray(quats, np.float64), np.ascontiguousarray(trans, np.float64)
        check(lib().vo_kfstore_pose_graph_apply(self._h, _p(q), _p(t)), "vo_kfstore_pose_graph_apply")

    def pose_graph(self, curr, match, inp, max_iterations=20):
        """window, vo_pose_graph_solve with match's node fixed, write-back -> summary; a refusal of the solver raises and nothing
        has been written back"""
        ck, sc, su, ls, lk, ci, cr = self._pg_inputs(inp, False)   # (named: the arrays must outlive the call)
        if len(ls) != len(ck) + 1 or len(sc) != len(ck) or len(su) != len(ck) or len(cr) != len(ci) or len(lk) < (int(ls[-1]) if len(ls) else 0):
            raise VoError("vo_kfstore_pose_graph failed with status -1: the arrays' lengths do not fit each other")
        s = LmSummary()
        check(lib().vo_kfstore_pose_graph(self._h, int(curr), int(match), len(ck), _p(ck), _p(sc), _p(su), _p(ls), _p(lk), len(ci), _p(ci),
                                          _p(cr), int(max_iterations), C.byref(s)), "vo_kfstore_pose_graph")
        return s

    LOOP_FUSE_COLUMNS = ("passed", "matches", "adds", "replaces", "moved", "cleared")

    def enable_loop_fuse(self, max_corrected, max_loop_points):
        """LoopClosing::searchAndFuse on the device from now on; valid on an empty store after enable_fuse
        only.  max_corrected: the corrected key-frames (passes) of a call; max_loop_points: the loop points of a call"""
        check(lib().vo_kfstore_enable_loop_fuse(self._h, int(max_corrected), int(max_loop_points)), "vo_kfstore_enable_loop_fuse")
        self._lf_corrected = int(max_corrected)

    def search_and_fuse(self, corr_kf, S_corr, ids=None, threshold=4.0):
        """searchAndFuse(correctPose) over the loop points `ids`: corr_kf ascending, S_corr [n, 8] (quaternion x y z w,
        translation, scale) as pose_graph_window takes them.  numpy arrays / lists are validated, copied once and the call
        synchronises once; device tensors (all three) are enqueued only.  ids = None (corr_kf and S_corr device tensors): the
        loop points the last compute_sim3 left on the device, enqueued only"""
        th = C.c_float(threshold)
        if hasattr(corr_kf, "data_ptr"):
            _need_tensor(corr_kf, "int32", None, "search_and_fuse")
            _need_tensor(S_corr, "float64", int(corr_kf.numel()) * 8, "search_and_fuse")
            if ids is None:
                check(lib().vo_kfstore_search_and_fuse_loop(self._h, int(corr_kf.numel()), _p(corr_kf), _p(S_corr), th),
                      "vo_kfstore_search_and_fuse_loop")
                return
            _need_tensor(ids, "int32", None, "search_and_fuse")
            check(lib().vo_kfstore_search_and_fuse_dev(self._h, int(corr_kf.numel()), _p(corr_kf), _p(S_corr), int(ids.numel()), _p(ids), th),
                  "vo_kfstore_search_and_fuse_dev")
            return
        ck, sc = np.ascontiguousarray(corr_kf, np.int32).reshape(-1), np.ascontiguousarray(S_corr, np.float64).reshape(-1, 8)
        a = np.ascontiguousarray(ids, np.int32).reshape(-1)
        if len(sc) != len(ck):
            raise VoError("vo_kfstore_search_and_fuse failed with status -1: corr_kf and S_corr differ in length")
        check(lib().vo_kfstore_search_and_fuse(self._h, len(ck), _p(ck), _p(sc), len(a), _p(a), th), "vo_kfstore_search_and_fuse")

    def loop_fuse_result(self):
        """the last search_and_fuse -> dict(passes, per_pass [(passed, matches, adds, replaces, moved, cleared)], totals);
        synchronises"""
        rec, per = np.zeros(8, np.int32), np.zeros((getattr(self, "_lf_corrected", 1), 6), np.int32)
        check(lib().vo_kfstore_loop_fuse_result(self._h, _p(rec), _p(per)), "vo_kfstore_loop_fuse_result")
        n = int(rec[0])
        return dict(passes=n, per_pass=[tuple(int(x) for x in row) for row in per[:n]], totals=tuple(int(x) for x in rec[1:7]))

    CONNECTIONS_CORRECT_LOOP_CAPACITY = 256
    LC_RECORD = ("n_corr", "n_cp", "n_lc", "curr", "status", "n_rows_moved", "connections_status")

    def enable_loop_correct(self, max_corrected, max_corrected_points, max_loop_connections):
        """the propagation of the loop Sim3 and the loop connections on the device from now on; valid on an
        empty store after enable_pose_graph only"""
        check(lib().vo_kfstore_enable_loop_correct(self._h, int(max_corrected), int(max_corrected_points), int(max_loop_connections)),
              "vo_kfstore_enable_loop_correct")
        self._lc_caps = (int(max_corrected), int(max_corrected_points), int(max_loop_connections))

    def propagate_loop(self, curr=None, Scw=None):
        """loopClosing.cpp:364-437 for the current key-frame and the loop Sim3 Scw (8 doubles: quaternion x y z w, translation,
        scale).  A list / numpy array is copied and the call synchronises once; a device tensor (float64 [8]) is enqueued only;
        curr = None: curr and Scw where the last compute_sim3 left them, enqueued only"""
        if curr is None:
            check(lib().vo_kfstore_propagate_loop_sim3(self._h), "vo_kfstore_propagate_loop_sim3")
        elif hasattr(Scw, "data_ptr"):
            _need_tensor(Scw, "float64", 8, "propagate_loop")
            check(lib().vo_kfstore_propagate_loop_dev(self._h, int(curr), _p(Scw)), "vo_kfstore_propagate_loop_dev")
        else:
            S = np.ascontiguousarray(Scw, np.float64).reshape(-1)
            if len(S) != 8:
                raise VoError("vo_kfstore_propagate_loop failed with status -1: Scw is not 8 doubles")
            check(lib().vo_kfstore_propagate_loop(self._h, int(curr), _p(S)), "vo_kfstore_propagate_loop")

    def loop_connections(self):
        """loopClosing.cpp:461-479 on the lists the last propagate_loop left, after the caller's search_and_fuse; enqueued only"""
        check(lib().vo_kfstore_loop_connections(self._h), "vo_kfstore_loop_connections")

    def loop_correct_result(self):
        """the last propagate_loop / loop_connections -> dict(record (dict over LC_RECORD), list, corr_kf, S_corr, S_uncorr, cp_id,
        cp_ref, lc_start, lc_kf) cut to the record's counts; the last seven are what pose_graph_window takes.  Synchronises"""
        Cc, P, E = getattr(self, "_lc_caps", (1, 1, 1))
        rec = np.zeros(16, np.int32)
        a = dict(list=np.zeros(Cc, np.int32), corr_kf=np.zeros(Cc, np.int32), S_corr=np.zeros((Cc, 8)), S_uncorr=np.zeros((Cc, 8)),
                 cp_id=np.zeros(P, np.int32), cp_ref=np.zeros(P, np.int32), lc_start=np.zeros(Cc + 1, np.int32), lc_kf=np.zeros(E, np.int32))
        check(lib().vo_kfstore_loop_correct_result(self._h, _p(rec), *(_p(v) for v in a.values())), "vo_kfstore_loop_correct_result")
        r = {k: int(rec[i]) for i, k in enumerate(self.LC_RECORD)}
        ok = r["status"] == self.BA_WINDOW_OK
        conn_ok = ok and r["connections_status"] == self.BA_WINDOW_OK
        nc, ncp, nlc = (r["n_corr"] if ok else 0), (r["n_cp"] if ok else 0), (r["n_lc"] if conn_ok else 0)
        n = dict(list=nc, corr_kf=nc, S_corr=nc, S_uncorr=nc, cp_id=ncp, cp_ref=ncp, lc_start=nc + 1 if conn_ok else 0, lc_kf=nlc)
        return dict({k: v[:n[k]].copy() for k, v in a.items()}, record=r)

    def loop_correct_arrays(self):
        """-> dict(corr_kf, S_corr, S_uncorr, cp_id, cp_ref, lc_start, lc_kf) of DEVICE addresses (ints), as
        vo_kfstore_search_and_fuse_loop and vo_kfstore_pose_graph_window_dev take them; no synchronisation"""
        ptrs = [C.c_void_p() for _ in range(7)]
        check(lib().vo_kfstore_loop_correct_arrays(self._h, *(C.byref(p) for p in ptrs)), "vo_kfstore_loop_correct_arrays")
        return {k: int(p.value or 0) for k, p in zip(("corr_kf", "S_corr", "S_uncorr", "cp_id", "cp_ref", "lc_start", "lc_kf"), ptrs)}

    LM_RECORD = ("steps", "adds", "noops", "replaces", "moved", "cleared", "n_dead", "undone", "ordered", "curr")
    LM_NONE, LM_ADD, LM_NOOP, LM_REPLACE, LM_DEAD, LM_UNDONE = range(6)
    CL_RECORD = ("curr", "match", "n_corr", "n_cp", "n_lc", "merge_adds", "merge_replaces", "fuse_adds", "fuse_replaces", "n_nodes", "n_edges",
                 "n_points_moved", "stopped_at")

    def enable_loop_merge(self):
        """the merge of the loop matches (loopClosing.cpp:439-455) and the composed correct_loop on the device from now on
        (DESIGN.md section 4s); valid on an empty store after enable_loop_fuse only"""
        check(lib().vo_kfstore_enable_loop_merge(self._h), "vo_kfstore_enable_loop_merge")

    def merge_loop_matches(self, curr=None, match_ids=None):
        """the current key-frame takes the loop's map points: feature i replaces its point by match_ids[i] >= 0, or takes it when
        it has none.  A list / numpy array is copied and the call synchronises once; a device tensor (int32) is enqueued only;
        curr = None: curr and matchMapPoints_ where the last compute_sim3 left them, enqueued only"""
        if curr is None:
            check(lib().vo_kfstore_merge_loop_matches_loop(self._h), "vo_kfstore_merge_loop_matches_loop")
        elif hasattr(match_ids, "data_ptr"):
            _need_tensor(match_ids, "int32", None, "merge_loop_matches")
            check(lib().vo_kfstore_merge_loop_matches_dev(self._h, int(curr), int(match_ids.numel()), _p(match_ids)),
                  "vo_kfstore_merge_loop_matches_dev")
        else:
            a = np.ascontiguousarray(match_ids, np.int32).reshape(-1)
            check(lib().vo_kfstore_merge_loop_matches(self._h, int(curr), len(a), _p(a)), "vo_kfstore_merge_loop_matches")

    def loop_merge_result(self):
        """the last merge_loop_matches -> dict(record (dict over LM_RECORD), per_feature [max_features]: LM_NONE, LM_ADD, LM_NOOP,
        LM_REPLACE, LM_DEAD, LM_UNDONE); synchronises"""
        rec, per = np.zeros(16, np.int32), np.zeros(self.max_features, np.int32)
        check(lib().vo_kfstore_loop_merge_result(self._h, _p(rec), _p(per)), "vo_kfstore_loop_merge_result")
        return dict(record={k: int(rec[i]) for i, k in enumerate(self.LM_RECORD)}, per_feature=per)

    def correct_loop(self, threshold=4.0, max_iterations=20):
        """correctLoop (loopClosing.cpp:364-485) on the state the last compute_sim3 left: propagate_loop, merge_loop_matches,
        search_and_fuse, loop_connections, the pose graph (window, solve, write-back) and the loop edge in one call
        -> (summary, record: dict over CL_RECORD).  A refusal raises; self.correct_loop_record then holds the record"""
        s, rec = LmSummary(), np.zeros(16, np.int32)
        rc = lib().vo_kfstore_correct_loop(self._h, C.c_float(threshold), int(max_iterations), C.byref(s), _p(rec))
        self.correct_loop_record = {k: int(rec[i]) for i, k in enumerate(self.CL_RECORD)}
        check(rc, "vo_kfstore_correct_loop")
        return s, self.correct_loop_record

    CONNECTIONS_DETECT_CAPACITY = 512
    DETECT_MAX_GROUPS = 1024
    DETECT_NONE, DETECT_GATED, DETECT_NO_CANDIDATES, DETECT_NOT_CONSISTENT, DETECT_DETECTED, DETECT_OVERFLOW = range(6)
    DL_RECORD = ("outcome", "current", "n_excl", "n_conn", "min_score_bits", "n_candidates", "groups_before", "groups_after", "n_enough",
                 "locked", "pending")
    LCS_RECORD = ("outcome", "state", "correct_loop", "stopped_at", "n_enough", "match", "continue_passes", "last_loop_keyframe")

    def enable_detect_loop(self, max_detect_candidates, max_groups):
        """LoopClosing::detectLoop with its consistency groups, the loop thread's erase locks and the composed loop_closing_step
        on the device from now on; valid on an empty store after enable_loop and enable_pose_graph only"""
        check(lib().vo_kfstore_enable_detect_loop(self._h, int(max_detect_candidates), int(max_groups)), "vo_kfstore_enable_detect_loop")
        self._dl_caps = (int(max_detect_candidates), int(max_groups))

    def detect_loop(self, db, current, last_loop_keyframe=0):
        """detectLoop for key-frame `current`, which db (a KeyFrameDatabase with the store's numbering) holds already; enqueued
        only.  db's neighbour rows are overwritten from the store's graph rows"""
        check(lib().vo_kfstore_detect_loop(self._h, db._h, int(current), int(last_loop_keyframe)), "vo_kfstore_detect_loop")

    def detect_loop_result(self):
        """the last detect_loop -> dict over DL_RECORD plus min_score (float32), candidates and enough (lists); synchronises"""
        D, _ = getattr(self, "_dl_caps", (1, 1))
        rec, cand, en = np.zeros(16, np.int32), np.full(D, -1, np.int32), np.full(D, -1, np.int32)
        check(lib().vo_kfstore_detect_loop_result(self._h, _p(rec), _p(cand), _p(en)), "vo_kfstore_detect_loop_result")
        out = {k: int(rec[i]) for i, k in enumerate(self.DL_RECORD)}
        out.update(min_score=rec[4:5].view(np.float32)[0], candidates=[int(x) for x in cand[:min(max(out["n_candidates"], 0), D)]],
                   enough=[int(x) for x in en[:min(max(out["n_enough"], 0), D)]])
        return out

    def detect_loop_groups(self):
        """prevConsistentGroups_ as the layer holds it -> (counts list, members uint8 [n, size]); synchronises"""
        _, G = getattr(self, "_dl_caps", (1, 1))
        size = len(self)
        n, counts, members = C.c_int32(0), np.zeros(G, np.int32), np.zeros((G, max(size, 1)), np.uint8)
        check(lib().vo_kfstore_detect_loop_groups(self._h, C.byref(n), _p(counts), _p(members)), "vo_kfstore_detect_loop_groups")
        return [int(x) for x in counts[:n.value]], members.reshape(-1)[:n.value * size].reshape(n.value, size).copy()

    def compute_sim3_detected(self, rand_values, rand_max, fix_scale=True, max_rounds=8):
        """compute_sim3 for `current` and the enough list of the last detect_loop, read in place.  A list / numpy array of rand()
        values is copied and the call synchronises once; a device tensor (int32) is enqueued only"""
        if hasattr(rand_values, "data_ptr"):
            _need_tensor(rand_values, "int32", None, "compute_sim3_detected")
            check(lib().vo_kfstore_compute_sim3_detected_dev(self._h, int(bool(fix_scale)), int(rand_values.numel()), _p(rand_values),
                                                             int(rand_max), int(max_rounds)), "vo_kfstore_compute_sim3_detected_dev")
            return
        r = np.ascontiguousarray(rand_values, np.int32).reshape(-1)
        check(lib().vo_kfstore_compute_sim3_detected(self._h, int(bool(fix_scale)), len(r), _p(r), int(rand_max), int(max_rounds)),
              "vo_kfstore_compute_sim3_detected")

    def release_loop_locks(self):
        """computeSim3's lock releases by the state the last compute_sim3 ended in; enqueued only"""
        check(lib().vo_kfstore_release_loop_locks(self._h), "vo_kfstore_release_loop_locks")

    def loop_locks_result(self):
        """the last release_loop_locks -> (n_released, [released key-frames whose pending word is set]); synchronises"""
        nr, npend, pend = C.c_int32(0), C.c_int32(0), np.full(17, -1, np.int32)
        check(lib().vo_kfstore_loop_locks_result(self._h, C.byref(nr), C.byref(npend), _p(pend)), "vo_kfstore_loop_locks_result")
        return int(nr.value), [int(x) for x in pend[:npend.value]]

    @property
    def last_loop_keyframe(self):
        k = C.c_int32(0)
        check(lib().vo_kfstore_get_last_loop_keyframe(self._h, C.byref(k)), "vo_kfstore_get_last_loop_keyframe")
        return int(k.value)

    @last_loop_keyframe.setter
    def last_loop_keyframe(self, keyframe):
        check(lib().vo_kfstore_set_last_loop_keyframe(self._h, int(keyframe)), "vo_kfstore_set_last_loop_keyframe")

    def loop_closing_step(self, db, current, rand_values, rand_max, fix_scale=True, max_rounds=8, threshold=4.0, max_iterations=20):
        """one iteration of LoopClosing::run for key-frame `current`: detect_loop, compute_sim3_detected, ONE read, more rounds
        while undecided, release_loop_locks and, on an accepted loop, correct_loop -> (summary, record: dict over LCS_RECORD).  A
        refusal raises; self.loop_closing_record then holds the record"""
        r = np.ascontiguousarray(rand_values, np.int32).reshape(-1)
        s, rec = LmSummary(), np.zeros(16, np.int32)
        rc = lib().vo_kfstore_loop_closing_step(self._h, db._h, int(current), int(bool(fix_scale)), len(r), _p(r), int(rand_max),
                                                int(max_rounds), C.c_float(threshold), int(max_iterations), C.byref(s), _p(rec))
        self.loop_closing_record = {k: int(rec[i]) for i, k in enumerate(self.LCS_RECORD)}
        check(rc, "vo_kfstore_loop_closing_step")
        return s, self.loop_closing_record

    KC_RECORD = ("keyframe", "n", "n_pairs", "n_walked", "n_created", "n_tracked", "first_id", "next_id", "ended_early", "status")
    _KC_COLUMNS = (("x", "float32"), ("y", "float32"), ("octave", "int32"), ("angle", "float32"), ("depth", "float32"), ("u_right", "float32"))

    def enable_keyframe_create(self):
        """createNewKeyFrame / the first key-frame of initVisualOdometry on the device from now on; valid on
        an empty store after enable_local_ba only"""
        check(lib().vo_kfstore_enable_keyframe_create(self._h), "vo_kfstore_enable_keyframe_create")

    def create_keyframe(self, vocab, f, th_depth, initial=False):
        """a tracked frame written into the store as a key-frame -> its number.  f: dict(Tcw12 f64 [12], x, y, angle, depth, u_right
        f32 [n], octave i32 [n], desc u8 [n, 32], slot_ids i32 [n]: the frame's map-point slots as global ids, negative = null;
        ignored and optional with initial).  numpy arrays are validated, copied once and synchronise once; device tensors (all of
        them) are enqueued only and must stay untouched until the store's stream has passed the call"""
        idx = C.c_int32(-1)
        if hasattr(f["Tcw12"], "data_ptr"):
            n = int(f["depth"].numel())
            _need_tensor(f["Tcw12"], "float64", 12, "create_keyframe")
            for k, dt in self._KC_COLUMNS:
                _need_tensor(f[k], dt, n, "create_keyframe")
            _need_tensor(f["desc"], "uint8", n * 32, "create_keyframe")
            slot = None if initial else f["slot_ids"]
            if slot is not None:
                _need_tensor(slot, "int32", n, "create_keyframe")
            check(lib().vo_kfstore_create_keyframe_dev(self._h, vocab._h, n, _p(f["Tcw12"]), _p(f["x"]), _p(f["y"]), _p(f["octave"]), _p(f["angle"]),
                                                       _p(f["depth"]), _p(f["u_right"]), _p(f["desc"]), _p(slot), C.c_float(th_depth),
                                                       int(bool(initial)), C.byref(idx)), "vo_kfstore_create_keyframe_dev")
            return int(idx.value)
        T = np.ascontiguousarray(f["Tcw12"], np.float64).reshape(12)
        a = {k: np.ascontiguousarray(f[k], dt).reshape(-1) for k, dt in self._KC_COLUMNS}
        n = len(a["depth"])
        desc = np.ascontiguousarray(f["desc"], np.uint8).reshape(n, 32)
        slot = None if initial else np.ascontiguousarray(f["slot_ids"], np.int32).reshape(-1)
        if any(len(v) != n for v in a.values()) or (slot is not None and len(slot) != n):
            raise VoError("vo_kfstore_create_keyframe failed with status -1: the frame's arrays differ in length")
        check(lib().vo_kfstore_create_keyframe(self._h, vocab._h, n, _p(T), _p(a["x"]), _p(a["y"]), _p(a["octave"]), _p(a["angle"]), _p(a["depth"]),
                                               _p(a["u_right"]), _p(desc), _p(slot), C.c_float(th_depth), int(bool(initial)), C.byref(idx)),
              "vo_kfstore_create_keyframe")
        return int(idx.value)

    def create_keyframe_from_frames(self, vocab, frames, slot, n, Tcw12, slot_ids, th_depth, initial=False):
        """create_keyframe with the feature columns of `slot` of a Frames handle (Tracker.frames_handle() wrapped, or one of the
        caller's); n: the slot's feature count as the caller knows it; Tcw12 (f64 [12]) and slot_ids (i32 [n]) device tensors.
        Enqueued only; a wrong n shows as status 1 in keyframe_result() and raises the sticky CONNECTIONS_INVALID"""
        _need_tensor(Tcw12, "float64", 12, "create_keyframe_from_frames")
        if not initial:
            _need_tensor(slot_ids, "int32", int(n), "create_keyframe_from_frames")
        idx = C.c_int32(-1)
        h = frames._h if hasattr(frames, "_h") else C.c_void_p(frames)
        check(lib().vo_kfstore_create_keyframe_from_frames(self._h, vocab._h, h, int(slot), int(n), _p(Tcw12), _p(None if initial else slot_ids),
                                                           C.c_float(th_depth), int(bool(initial)), C.byref(idx)),
              "vo_kfstore_create_keyframe_from_frames")
        return int(idx.value)

    def features(self, keyframe, n):
        """the feature side of a key-frame as the store holds it (n as inserted) -> dict(angle, desc, octave, depth, u_right, xy of
        numpy arrays and feature_vector: [(node, [features])] in ascending node)"""
        n = int(n)
        out = dict(angle=np.zeros(n, np.float32), desc=np.zeros((n, 32), np.uint8), octave=np.zeros(n, np.int32), depth=np.zeros(n, np.float32),
                   u_right=np.zeros(n, np.float32), xy=np.zeros((n, 2), np.float32))
        nn, node, start, feat = C.c_int32(0), np.zeros(n, np.int32), np.zeros(n + 1, np.int32), np.zeros(n, np.int32)
        check(lib().vo_kfstore_get_features(self._h, int(keyframe), *(_p(v) for v in out.values()), C.byref(nn), _p(node), _p(start), _p(feat)),
              "vo_kfstore_get_features")
        k = min(max(int(nn.value), 0), n)
        out["feature_vector"] = [(int(node[j]), [int(x) for x in feat[start[j]:start[j + 1]]]) for j in range(k)]
        return out

    def keyframe_result(self):
        """the last create_keyframe -> dict over KC_RECORD plus created [(feature, id)] in walk order; synchronises"""
        rec = np.zeros(16, np.int32)
        feat, ids = np.zeros(self.max_features, np.int32), np.zeros(self.max_features, np.int32)
        check(lib().vo_kfstore_keyframe_result(self._h, _p(rec), _p(feat), _p(ids)), "vo_kfstore_keyframe_result")
        out = {k: int(rec[i]) for i, k in enumerate(self.KC_RECORD)}
        out["created"] = [(int(feat[i]), int(ids[i])) for i in range(out["n_created"])]
        return out

    def keyframe_need_stats(self, ref_kf, min_obs, depth, slot_ids, th_depth, out=None):
        """the three counts of needNewKeyFrame -> (trackedMapPoints(min_obs) of ref_kf, map_cnt, total_cnt).  numpy arrays: copied,
        synchronises once; device tensors (depth f32, slot_ids i32, out i32 [4]): enqueued only, the counts land in out"""
        if hasattr(depth, "data_ptr"):
            n = int(depth.numel())
            _need_tensor(depth, "float32", n, "keyframe_need_stats")
            _need_tensor(slot_ids, "int32", n, "keyframe_need_stats")
            _need_tensor(out, "int32", 4, "keyframe_need_stats")
            check(lib().vo_kfstore_keyframe_need_stats_dev(self._h, int(ref_kf), int(min_obs), n, _p(depth), _p(slot_ids), C.c_float(th_depth),
                                                           _p(out)), "vo_kfstore_keyframe_need_stats_dev")
            return None
        d, s = np.ascontiguousarray(depth, np.float32).reshape(-1), np.ascontiguousarray(slot_ids, np.int32).reshape(-1)
        if len(d) != len(s):
            raise VoError("vo_kfstore_keyframe_need_stats failed with status -1: depth and slot_ids differ in length")
        o = np.zeros(4, np.int32)
        check(lib().vo_kfstore_keyframe_need_stats(self._h, int(ref_kf), int(min_obs), len(d), _p(d), _p(s), C.c_float(th_depth), _p(o)),
              "vo_kfstore_keyframe_need_stats")
        return int(o[0]), int(o[1]), int(o[2])


def rgb_to_gray(img, first_is_red=True):
    img = np.ascontiguousarray(img, np.uint8)
    out = np.zeros(img.shape[:2], np.uint8)
    check(lib().vo_rgb_to_gray(_p(img), C.c_longlong(out.size), img.shape[2], int(first_is_red), _p(out)), "vo_rgb_to_gray")
    return out


def load_vocabulary(path):
    """DBoW3::Vocabulary(path) -> (Vocabulary handle wrapper, info dict)"""
    h = C.c_void_p()
    nn, nw, k, L = C.c_int(), C.c_int(), C.c_int(), C.c_int()
    check(lib().vo_vocab_load(str(path).encode(), C.byref(h), C.byref(nn), C.byref(nw), C.byref(k), C.byref(L)), "vo_vocab_load")
    v = Vocabulary.__new__(Vocabulary)
    v._h = h
    return v, dict(n_nodes=nn.value, n_words=nw.value, k=k.value, L=L.value)


class Dataset:
    """associate.txt of a TUM RGB-D sequence as test/vo_run.cpp:24-58 reads it."""

    def __init__(self, dataset_dir, max_frames):
        self._h = C.c_void_p()
        check(lib().vo_dataset_open(C.byref(self._h), str(dataset_dir).encode(), int(max_frames)), "vo_dataset_open")

    def __len__(self):
        return lib().vo_dataset_size(self._h)

    def __getitem__(self, i):
        s = [C.c_char_p() for _ in range(4)]
        check(lib().vo_dataset_entry(self._h, int(i), *[C.byref(x) for x in s]), "vo_dataset_entry")
        return tuple(x.value.decode() for x in s)

    def close(self):
        if getattr(self, "_h", None) and self._h.value and _lib is not None:
            _lib.vo_dataset_close(self._h)
            self._h = C.c_void_p()

    __del__ = close


def read_png(path, as_bgr=False):
    w, h, ch, bd = C.c_int(), C.c_int(), C.c_int(), C.c_int()
    check(lib().vo_png_info(str(path).encode(), C.byref(w), C.byref(h), C.byref(ch), C.byref(bd)), "vo_png_info")
    shape = (h.value, w.value) if ch.value == 1 else (h.value, w.value, ch.value)
    out = np.zeros(shape, np.uint16 if bd.value == 16 else np.uint8)
    check(lib().vo_png_read(str(path).encode(), int(as_bgr), _p(out), C.c_size_t(out.nbytes)), "vo_png_read")
    return out


def write_trajectory(path, timestamps, Twc7):
    T = np.ascontiguousarray(Twc7, np.float64).reshape(-1, 7)
    arr = (C.c_char_p * len(T))(*[str(t).encode() for t in timestamps])
    check(lib().vo_trajectory_write(str(path).encode(), len(T), arr, _p(T)), "vo_trajectory_write")


def tracking_time_stats(seconds):
    s = np.ascontiguousarray(seconds, np.float64)
    med, mean = C.c_double(), C.c_double()
    check(lib().vo_tracking_time_stats(_p(s), len(s), C.byref(med), C.byref(mean)), "vo_tracking_time_stats")
    return med.value, mean.value
