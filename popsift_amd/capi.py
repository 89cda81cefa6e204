"""ctypes binding of the C-ABI (include/popsift_hip.h) -> popsift_amd/lib/libpopsift_hip.so.

This is plumbing for tests and bench.py; the product host side is the C++14 library
(popsift_amd/csrc/host).  The binding fails loudly when the HIP library is missing: there is
no CPU fallback anywhere in the product path.
"""
import ctypes as C
import os

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("POPSIFT_HIP_LIB") or os.path.join(_HERE, "lib", "libpopsift_hip.so")

MAX_OCTAVES = 20
GAUSS_ALIGN = 32
GAUSS_LEVELS = 12
ORI_MAX = 4

GAUSS_VLFEAT_COMPUTE, GAUSS_VLFEAT_RELATIVE, GAUSS_VLFEAT_RELATIVE_ALL, GAUSS_OPENCV_COMPUTE, \
    GAUSS_FIXED9, GAUSS_FIXED15 = range(6)
MODE_POPSIFT, MODE_OPENCV, MODE_VLFEAT = 0, 1, 2
SCALE_DIRECT, SCALE_DEFAULT = 0, 1
DESC_LOOP, DESC_ILOOP, DESC_GRID, DESC_IGRID, DESC_NOTILE = range(5)
NORM_ROOTSIFT, NORM_CLASSIC = 0, 1
FILTER_RANDOM, FILTER_LARGEST_FIRST, FILTER_SMALLEST_FIRST = 0, 1, 2
PLANE_GAUSS, PLANE_DOG = 0, 1


class Config(C.Structure):
    """POD image of popsift::Config (psx_config)."""
    _fields_ = [
        ("octaves", C.c_int), ("levels", C.c_int), ("sigma", C.c_float), ("edge_limit", C.c_float),
        ("threshold", C.c_float), ("upscale_factor", C.c_float), ("gauss_mode", C.c_int),
        ("sift_mode", C.c_int), ("scaling_mode", C.c_int), ("desc_mode", C.c_int),
        ("norm_mode", C.c_int), ("norm_multi", C.c_int), ("max_extrema", C.c_int),
        ("assume_initial_blur", C.c_int), ("initial_blur", C.c_float),
        ("filter_max_extrema", C.c_int), ("filter_grid_size", C.c_int), ("grid_filter_mode", C.c_int),
    ]


FEATURE_DTYPE = np.dtype([("debug_octave", "<i4"), ("xpos", "<f4"), ("ypos", "<f4"), ("sigma", "<f4"),
                          ("num_ori", "<i4"), ("orientation", "<f4", (ORI_MAX,)),
                          ("desc_idx", "<i4", (ORI_MAX,))])
# popsift::Feature as stored in a FeaturesDev (psx_feature_dev, 72 bytes; desc[] are device addresses)
FEATURE_DEV_DTYPE = np.dtype([("debug_octave", "<i4"), ("xpos", "<f4"), ("ypos", "<f4"), ("sigma", "<f4"),
                              ("num_ori", "<i4"), ("orientation", "<f4", (ORI_MAX,)), ("pad", "<i4"),
                              ("desc", "<u8", (ORI_MAX,))])
IEXT_DTYPE = np.dtype([("xpos", "<f4"), ("ypos", "<f4"), ("lpos", "<i4"), ("sigma", "<f4"),
                       ("cell", "<i4"), ("ignore", "<i4")])
EXT_DTYPE = np.dtype([("xpos", "<f4"), ("ypos", "<f4"), ("lpos", "<i4"), ("sigma", "<f4"),
                      ("octave", "<i4"), ("num_ori", "<i4"), ("idx_ori", "<i4"),
                      ("orientation", "<f4", (ORI_MAX,))])
KP_AUTO = -1                     # PSX_KP_AUTO
DESCRIBE_REUSE_PYRAMID = 1       # PSX_DESCRIBE_REUSE_PYRAMID
# psx_keypoint (40 bytes): a caller-supplied keypoint in input-image units
KEYPOINT_DTYPE = np.dtype([("xpos", "<f4"), ("ypos", "<f4"), ("sigma", "<f4"), ("octave", "<i4"), ("lpos", "<i4"),
                           ("num_ori", "<i4"), ("orientation", "<f4", (ORI_MAX,))])


class Keypoint(C.Structure):
    """psx_keypoint as a ctypes structure (KEYPOINT_DTYPE is the same record for numpy arrays)."""
    _fields_ = [("xpos", C.c_float), ("ypos", C.c_float), ("sigma", C.c_float), ("octave", C.c_int), ("lpos", C.c_int),
                ("num_ori", C.c_int), ("orientation", C.c_float * ORI_MAX)]

    dtype = KEYPOINT_DTYPE


def keypoints_array(kps):
    """A C-contiguous KEYPOINT_DTYPE array of kps: such an array, a sequence of Keypoint structures, or None (empty)."""
    if kps is None:
        return np.zeros((0,), dtype=KEYPOINT_DTYPE)
    if isinstance(kps, np.ndarray):
        if kps.dtype != KEYPOINT_DTYPE:
            raise TypeError("keypoints must have capi.KEYPOINT_DTYPE")
        return np.ascontiguousarray(kps).reshape(-1)
    out = np.zeros((len(kps),), dtype=KEYPOINT_DTYPE)
    for i, k in enumerate(kps):
        out[i] = (k.xpos, k.ypos, k.sigma, k.octave, k.lpos, k.num_ori, tuple(k.orientation))
    return out

# every symbol include/popsift_hip.h declares
SYMBOLS = [
    "psx_version", "psx_config_default", "psx_peak_threshold", "psx_gauss_tables", "psx_create",
    "psx_destroy", "psx_last_error", "psx_resize", "psx_num_octaves", "psx_num_levels",
    "psx_octave_dims", "psx_upload_u8", "psx_upload_f32", "psx_set_input_dev", "psx_build_pyramid",
    "psx_find_extrema", "psx_orientation", "psx_descriptors", "psx_extract", "psx_sync", "psx_counts",
    "psx_download", "psx_attach_export", "psx_device_results", "psx_dump_plane", "psx_dump_iext", "psx_dump_extrema",
    "psx_set_wait_mode", "psx_enable_timers", "psx_stage_times", "psx_time_blur", "psx_stream",
    "psx_host_alloc", "psx_host_alloc_near", "psx_host_free", "psx_dev_alloc", "psx_dev_free", "psx_dev_read", "psx_dev_write", "psx_clone_results", "psx_match", "psx_match_release", "psx_device_count", "psx_device_info", "psx_device_pci",
    "psx_enable_blur_probe", "psx_blur_probe_times", "psx_copy_bench", "psx_upload_pinned", "psx_attach_export_mapped",
    "psx_print_gauss_tables", "psx_flow_trace", "psx_debug_cross_stream", "psx_probe_extra_times",
    "psx_set_descriptor_format", "psx_download_u8", "psx_attach_export_u8", "psx_attach_export_mapped_u8",
    "psx_quantize_desc", "psx_match_u8",
    "psx_keypoint_bounds", "psx_place_keypoints", "psx_set_keypoints", "psx_set_keypoints_dev", "psx_describe",
    "psx_keypoint_map",
    "psx_set_mask", "psx_set_mask_dev", "psx_mask_keep",
    "psx_match_opts_default", "psx_match_pairs", "psx_match_pairs_u8", "psx_match_pairs_dev", "psx_match_pairs_u8_dev",
    "psx_pairs_join", "psx_pairs_join_u8",
    "psx_match_pairs_many_u8", "psx_match_pairs_many_u8_dev", "psx_match_many_plan",
    "psx_match_pairs_graph_u8", "psx_match_pairs_graph_u8_dev", "psx_match_graph_plan",
    "psx_match_pairs_many", "psx_match_pairs_many_dev", "psx_match_many_f32_plan", "psx_match_many_f32_last",
    "psx_guide_allows", "psx_desc_positions", "psx_match_guided", "psx_match_guided_u8",
    "psx_match_pairs_guided", "psx_match_pairs_guided_u8", "psx_match_pairs_guided_dev", "psx_match_pairs_guided_u8_dev",
    "psx_match_pairs_guided_many_u8", "psx_match_pairs_guided_many_u8_dev", "psx_guides_from_ransac",
    "psx_ransac_opts_default", "psx_ransac_samples", "psx_homography_fit", "psx_ransac_homography_ref",
    "psx_ransac_homography", "psx_ransac_homography_dev",
    "psx_ransac_samples_k", "psx_fundamental_fit", "psx_ransac_fundamental_ref", "psx_ransac_fundamental", "psx_ransac_fundamental_dev",
    "psx_ransac_homography_many", "psx_ransac_homography_many_dev", "psx_ransac_homography_many_ref",
    "psx_ransac_fundamental_many", "psx_ransac_fundamental_many_dev", "psx_ransac_fundamental_many_ref", "psx_ransac_many_plan",
    "psx_affine_fit", "psx_ransac_affine_ref", "psx_ransac_affine", "psx_ransac_affine_dev",
    "psx_similarity_fit", "psx_ransac_similarity_ref", "psx_ransac_similarity", "psx_ransac_similarity_dev",
    "psx_ransac_affine_many", "psx_ransac_affine_many_dev", "psx_ransac_affine_many_ref",
    "psx_ransac_similarity_many", "psx_ransac_similarity_many_dev", "psx_ransac_similarity_many_ref",
    "psx_ransac_homography_graph", "psx_ransac_homography_graph_dev", "psx_ransac_homography_graph_ref",
    "psx_ransac_fundamental_graph", "psx_ransac_fundamental_graph_dev", "psx_ransac_fundamental_graph_ref",
    "psx_ransac_affine_graph", "psx_ransac_affine_graph_dev", "psx_ransac_affine_graph_ref",
    "psx_ransac_similarity_graph", "psx_ransac_similarity_graph_dev", "psx_ransac_similarity_graph_ref",
    "psx_match_pairs_guided_graph_u8", "psx_match_pairs_guided_graph_u8_dev",
    "psx_match_pairs_graph", "psx_match_pairs_graph_dev", "psx_match_graph_f32_plan", "psx_match_graph_f32_last",
    "psx_match_pairs_guided_many", "psx_match_pairs_guided_many_dev", "psx_match_pairs_guided_graph", "psx_match_pairs_guided_graph_dev",
    "psx_tracks_graph", "psx_tracks_graph_dev", "psx_tracks_graph_ref", "psx_tracks_plan",
    "psx_vocab_train_u8", "psx_vocab_train_u8_dev", "psx_vocab_train_u8_ref", "psx_bow_u8", "psx_bow_u8_dev", "psx_bow_u8_ref",
    "psx_shortlist_views", "psx_shortlist_views_dev", "psx_shortlist_views_ref", "psx_bow_weights",
    "psx_bow_quantize_dev", "psx_bow_quantize_ref", "psx_shortlist_query", "psx_shortlist_query_dev", "psx_shortlist_query_ref",
    "psx_shortlist_query_plan",
    "psx_pyramid_plan", "psx_blur_grid_of",
]

PAIRS_MUTUAL = 1     # PSX_PAIRS_MUTUAL
# psx_match_pair / psx_match_pair_u8 (16 bytes): one correspondence; byte distances are integers, INT_MAX = none
PAIR_DTYPE = np.dtype([("left", "<i4"), ("right", "<i4"), ("d1", "<f4"), ("d2", "<f4")])
PAIR_U8_DTYPE = np.dtype([("left", "<i4"), ("right", "<i4"), ("d1", "<i4"), ("d2", "<i4")])


class ManyF32Plan(C.Structure):
    """psx_many_f32_plan: what psx_match_pairs_many decides for the sizes of a call (path 1 scan, 2 prefilter, 0 nothing)"""
    _fields_ = [("path", C.c_int), ("fwd_groups", C.c_int), ("bwd_groups", C.c_int), ("launches", C.c_int), ("scratch_bytes", C.c_longlong)]


class GraphPlanInfo(C.Structure):
    """psx_graph_plan_info: what psx_match_pairs_graph_u8 plans for the sizes of a call"""
    _fields_ = [("referenced_sets", C.c_int), ("blocks", C.c_int), ("chunks", C.c_int), ("chunk_len", C.c_int),
                ("fwd_items", C.c_int), ("bwd_items", C.c_int), ("fwd_groups", C.c_int), ("bwd_groups", C.c_int),
                ("join_workgroups", C.c_int), ("launches", C.c_int), ("scratch_bytes", C.c_longlong)]


class GraphF32PlanInfo(C.Structure):
    """psx_graph_f32_plan_info: what psx_match_pairs_graph decides and plans for the sizes of a call"""
    _fields_ = [("path", C.c_int), ("referenced_sets", C.c_int), ("blocks", C.c_int), ("chunks", C.c_int), ("chunk_len", C.c_int),
                ("fwd_items", C.c_int), ("bwd_items", C.c_int), ("fwd_groups", C.c_int), ("bwd_groups", C.c_int),
                ("join_workgroups", C.c_int), ("launches", C.c_int), ("scratch_bytes", C.c_longlong)]


class ManyF32Info(C.Structure):
    """psx_many_f32_info: the calling thread's last psx_match_pairs_many call"""
    _fields_ = [("path", C.c_int), ("fell_back", C.c_int), ("launches", C.c_int), ("syncs", C.c_int)]


class MatchOpts(C.Structure):
    """psx_match_opts: {0.8, 0} is the accept flag of psx_match."""
    _fields_ = [("ratio", C.c_float), ("flags", C.c_int)]


GUIDE_HOMOGRAPHY = 1     # PSX_GUIDE_HOMOGRAPHY
GUIDE_EPIPOLAR = 2       # PSX_GUIDE_EPIPOLAR
GUIDE_NONE = 0           # PSX_GUIDE_NONE: in the *_many call only, this set is skipped


class Guide(C.Structure):
    """psx_guide: which (left, right) pairs guided matching may form, from their positions in input-image units.
    Guide.homography(H, tol): the right point lies within tol of H * left point (identity H: a search window);
    Guide.epipolar(F, tol): the right point lies within tol of the line F * left point.  Matrices row major."""
    _fields_ = [("kind", C.c_int), ("m", C.c_float * 9), ("tol", C.c_float)]

    @classmethod
    def make(cls, kind, m, tol):
        m = np.asarray(m, dtype=np.float32).reshape(9)
        return cls(kind, (C.c_float * 9)(*[float(v) for v in m]), float(np.float32(tol)))

    @classmethod
    def homography(cls, H, tol):
        return cls.make(GUIDE_HOMOGRAPHY, H, tol)

    @classmethod
    def epipolar(cls, F, tol):
        return cls.make(GUIDE_EPIPOLAR, F, tol)

    @classmethod
    def none(cls):
        """the guide of a set that match_pairs_guided_many_* skips (kind 0); the single-set calls refuse it"""
        return cls.make(GUIDE_NONE, np.zeros(9, np.float32), 0.0)


RANSAC_REFIT = 1         # PSX_RANSAC_REFIT
RANSAC_MODELS = ("homography", "fundamental", "affine", "similarity")


class RansacOpts(C.Structure):
    """psx_ransac_opts: inlier tolerance in pixels, number of hypotheses (1..65536), seed, flags (RANSAC_REFIT)."""
    _fields_ = [("tol", C.c_float), ("hypotheses", C.c_int), ("seed", C.c_uint), ("flags", C.c_int)]


class RansacResult(C.Structure):
    """psx_ransac_result: the kept model (row major, left -> right), the winning hypothesis (-1: no model), its inlier
    count, the inlier count under the kept model, and whether the refit replaced the sample model."""
    _fields_ = [("m", C.c_float * 9), ("best", C.c_int), ("sample_inliers", C.c_int), ("inliers", C.c_int), ("refit_kept", C.c_int)]

    def matrix(self):
        return np.array(list(self.m), np.float32)

    kind = GUIDE_HOMOGRAPHY      # the ransac_fundamental* wrappers set GUIDE_EPIPOLAR on the results they return

    def guide(self, tol):
        """the kept model as the psx_guide of a guided re-match: a homography guide from ransac_homography*, an epipolar
        one from ransac_fundamental*"""
        return Guide.make(self.kind, self.matrix(), tol)


TRACKS_KEEP_CONFLICTS = 1     # PSX_TRACKS_KEEP_CONFLICTS
TRACK_MEMBER_DTYPE = np.dtype([("view", "<i4"), ("row", "<i4")])     # psx_track_member (8 bytes)


class TrackOpts(C.Structure):
    """psx_track_opts: a track has members in at least min_views (>= 2) views; flags: TRACKS_KEEP_CONFLICTS"""
    _fields_ = [("min_views", C.c_int), ("flags", C.c_int)]


class TracksInfo(C.Structure):
    """psx_tracks_info: the totals of a tracks call, whatever the capacities were"""
    _fields_ = [("tracks", C.c_int), ("members", C.c_int), ("components", C.c_int), ("conflicts", C.c_int), ("too_few_views", C.c_int),
                ("joined_records", C.c_int)]


class TracksPlanInfo(C.Structure):
    """psx_tracks_plan_info: what psx_tracks_graph plans for the sizes of a call"""
    _fields_ = [("nodes", C.c_int), ("records", C.c_int), ("record_blocks", C.c_int), ("sort_bits", C.c_int), ("launches", C.c_int),
                ("scratch_bytes", C.c_longlong)]


SHORTLIST_MUTUAL = 1          # PSX_SHORTLIST_MUTUAL
VIEW_EDGE_DTYPE = np.dtype([("left", "<i4"), ("right", "<i4")])      # psx_view_edge (8 bytes)


class VocabOpts(C.Structure):
    """psx_vocab_opts: words (2..65536, at most the number of rows) and iterations (>= 1) of the integer k-means"""
    _fields_ = [("words", C.c_int), ("iterations", C.c_int)]


class VocabInfo(C.Structure):
    """psx_vocab_info: iterations run; changed rows, empty words and inertia of the last assignment"""
    _fields_ = [("iterations", C.c_int), ("changed", C.c_int), ("empty_words", C.c_int), ("reserved", C.c_int), ("inertia", C.c_ulonglong)]


class ShortlistOpts(C.Structure):
    """psx_shortlist_opts: the k most similar views per view; flags: SHORTLIST_MUTUAL"""
    _fields_ = [("k", C.c_int), ("flags", C.c_int)]


QUERY_MAX_VIEWS = 1 << 20     # PSX_QUERY_MAX_VIEWS
QUERY_MAX_WEIGHT = 1023       # PSX_QUERY_MAX_WEIGHT


class QueryOpts(C.Structure):
    """psx_query_opts: the k most similar stored views per query; flags and reserved must be 0; self_base >= 0: query i IS
    stored view self_base + i (-1: none); the left of query i's edges is edge_base + i; min_score: the least score listed"""
    _fields_ = [("k", C.c_int), ("flags", C.c_int), ("self_base", C.c_int), ("edge_base", C.c_int), ("min_score", C.c_uint),
                ("reserved", C.c_int)]


class QueryPlan(C.Structure):
    """psx_query_plan: database blocks of the score grid, keys per block list, keys between the two kernels, device scratch"""
    _fields_ = [("blocks", C.c_int), ("keys_per_block", C.c_int), ("partial_keys", C.c_longlong), ("scratch_bytes", C.c_longlong)]


DESCFMT_F32 = 0      # PSX_DESCFMT_F32
DESCFMT_U8 = 1       # PSX_DESCFMT_U8

_LIB = None


class PopSiftError(RuntimeError):
    pass


def lib():
    global _LIB
    if _LIB is None:
        if not os.path.exists(LIB_PATH):
            raise PopSiftError(
                "%s is missing: build it with `python -m popsift_amd.build` "
                "(there is no CPU fallback)" % LIB_PATH)
        L = C.CDLL(LIB_PATH)
        vp, ip, fp = C.c_void_p, C.POINTER(C.c_int), C.POINTER(C.c_float)
        L.psx_version.restype = C.c_char_p
        L.psx_config_default.argtypes = [C.POINTER(Config)]
        L.psx_peak_threshold.argtypes = [C.POINTER(Config)]
        L.psx_peak_threshold.restype = C.c_float
        L.psx_gauss_tables.argtypes = [C.POINTER(Config), fp, ip, fp, fp, ip, fp]
        L.psx_create.argtypes = [C.c_int, C.POINTER(Config), C.POINTER(vp)]
        L.psx_destroy.argtypes = [vp]
        L.psx_last_error.argtypes = [vp]
        L.psx_last_error.restype = C.c_char_p
        L.psx_resize.argtypes = [vp, C.c_int, C.c_int]
        L.psx_num_octaves.argtypes = [vp]
        L.psx_num_levels.argtypes = [vp]
        L.psx_octave_dims.argtypes = [vp, C.c_int, ip, ip]
        L.psx_upload_u8.argtypes = [vp, vp, C.c_int, C.c_int]
        L.psx_upload_f32.argtypes = [vp, vp, C.c_int, C.c_int]
        L.psx_set_input_dev.argtypes = [vp, vp, C.c_int, C.c_int, C.c_int]
        for n in ("psx_build_pyramid", "psx_find_extrema", "psx_orientation", "psx_descriptors",
                  "psx_extract", "psx_sync"):
            getattr(L, n).argtypes = [vp]
        L.psx_counts.argtypes = [vp, ip, ip]
        L.psx_download.argtypes = [vp, vp, C.c_int, vp, C.c_int]
        L.psx_attach_export.argtypes = [vp, vp, C.c_int, vp, C.c_int]
        L.psx_device_results.argtypes = [vp, C.POINTER(vp), C.POINTER(vp), C.POINTER(vp)]
        L.psx_dump_plane.argtypes = [vp, C.c_int, C.c_int, C.c_int, vp]
        L.psx_dump_iext.argtypes = [vp, C.c_int, vp, C.c_int, ip]
        L.psx_dump_extrema.argtypes = [vp, vp, C.c_int, ip]
        L.psx_enable_timers.argtypes = [vp, C.c_int]
        L.psx_stage_times.argtypes = [vp, fp]
        L.psx_time_blur.argtypes = [vp, C.c_int, C.c_int, C.c_int, fp, C.POINTER(C.c_double)]
        L.psx_stream.argtypes = [vp]
        L.psx_stream.restype = vp
        L.psx_enable_blur_probe.argtypes = [vp, C.c_int]
        L.psx_blur_probe_times.argtypes = [vp, fp, C.c_int, ip, C.POINTER(C.c_double)]
        L.psx_copy_bench.argtypes = [C.c_int, C.c_size_t, C.c_int, fp, C.POINTER(C.c_double)]
        L.psx_device_pci.argtypes = [C.c_int, C.c_char_p, C.c_int]
        L.psx_keypoint_bounds.argtypes = [C.POINTER(Config), fp, C.c_int, ip]
        L.psx_place_keypoints.argtypes = [C.POINTER(Config), C.c_int, C.c_int, vp, C.c_int, vp, vp]
        L.psx_set_keypoints.argtypes = [vp, vp, C.c_int]
        L.psx_set_keypoints_dev.argtypes = [vp, vp, C.c_int]
        L.psx_describe.argtypes = [vp, C.c_int]
        L.psx_keypoint_map.argtypes = [vp, vp, C.c_int, ip]
        L.psx_set_mask.argtypes = [vp, vp, C.c_int, C.c_int]
        L.psx_set_mask_dev.argtypes = [vp, vp, C.c_int, C.c_int]
        L.psx_mask_keep.argtypes = [vp, C.c_int, C.c_int, vp, vp, C.c_int, vp]
        L.psx_match_opts_default.argtypes = [C.POINTER(MatchOpts)]
        for n in ("psx_match_pairs", "psx_match_pairs_u8", "psx_match_pairs_dev", "psx_match_pairs_u8_dev"):
            getattr(L, n).argtypes = [C.c_int, vp, C.c_int, vp, C.c_int, C.POINTER(MatchOpts), vp, C.c_int, ip]
        for n in ("psx_pairs_join", "psx_pairs_join_u8"):
            getattr(L, n).argtypes = [vp, vp, C.c_int, vp, C.c_int, C.POINTER(MatchOpts), vp, C.c_int, ip]
        for n in ("psx_match_pairs_many_u8", "psx_match_pairs_many_u8_dev", "psx_match_pairs_many", "psx_match_pairs_many_dev"):
            getattr(L, n).argtypes = [C.c_int, vp, C.c_int, vp, vp, C.c_int, C.POINTER(MatchOpts), vp, C.c_int, vp, ip]
        L.psx_match_many_f32_plan.argtypes = [C.c_int, vp, C.c_int, C.c_int, C.c_int, C.POINTER(ManyF32Plan)]
        L.psx_match_many_f32_last.argtypes = [C.POINTER(ManyF32Info)]
        L.psx_match_many_plan.argtypes = [C.c_int, vp, C.c_int, C.c_int, vp, C.c_int, ip, vp, C.c_int, ip]
        for n in ("psx_match_pairs_graph_u8", "psx_match_pairs_graph_u8_dev", "psx_match_pairs_graph", "psx_match_pairs_graph_dev"):
            getattr(L, n).argtypes = [C.c_int, vp, vp, C.c_int, vp, C.c_int, C.POINTER(MatchOpts), vp, C.c_int, vp, ip]
        L.psx_match_graph_plan.argtypes = [vp, C.c_int, vp, C.c_int, C.c_int, C.POINTER(GraphPlanInfo)]
        L.psx_match_graph_f32_plan.argtypes = [vp, C.c_int, vp, C.c_int, C.c_int, C.c_int, C.POINTER(GraphF32PlanInfo)]
        L.psx_match_graph_f32_last.argtypes = [C.POINTER(ManyF32Info)]
        L.psx_guide_allows.argtypes = [C.POINTER(Guide), vp, C.c_int, vp, C.c_int, vp]
        L.psx_desc_positions.argtypes = [C.c_int, vp, vp, C.c_int, vp]
        for n in ("psx_match_guided", "psx_match_guided_u8"):
            getattr(L, n).argtypes = [C.c_int, vp, vp, C.c_int, vp, vp, C.c_int, C.POINTER(Guide), vp, vp]
        for n in ("psx_match_pairs_guided", "psx_match_pairs_guided_u8", "psx_match_pairs_guided_dev", "psx_match_pairs_guided_u8_dev"):
            getattr(L, n).argtypes = [C.c_int, vp, vp, C.c_int, vp, vp, C.c_int, C.POINTER(Guide), C.POINTER(MatchOpts), vp, C.c_int, ip]
        for n in ("psx_match_pairs_guided_many_u8", "psx_match_pairs_guided_many_u8_dev", "psx_match_pairs_guided_many",
                  "psx_match_pairs_guided_many_dev"):
            getattr(L, n).argtypes = [C.c_int, vp, vp, C.c_int, vp, vp, vp, C.c_int, vp, C.POINTER(MatchOpts), vp, C.c_int, vp, ip]
        L.psx_guides_from_ransac.argtypes = [vp, C.c_int, C.c_int, C.c_float, vp]
        L.psx_ransac_opts_default.argtypes = [C.POINTER(RansacOpts)]
        L.psx_ransac_samples.argtypes = [C.c_uint, C.c_int, C.c_int, C.c_int, vp]
        L.psx_homography_fit.argtypes = [vp, vp, C.c_int, vp]
        L.psx_ransac_samples_k.argtypes = [C.c_uint, C.c_int, C.c_int, C.c_int, C.c_int, vp]
        L.psx_fundamental_fit.argtypes = L.psx_affine_fit.argtypes = L.psx_similarity_fit.argtypes = [vp, vp, C.c_int, vp]
        L.psx_ransac_affine_ref.argtypes = L.psx_ransac_similarity_ref.argtypes = L.psx_ransac_fundamental_ref.argtypes = L.psx_ransac_homography_ref.argtypes = [vp, C.c_int, vp, C.c_int, vp, C.c_int, C.POINTER(RansacOpts), C.POINTER(RansacResult),
                                                vp, C.c_int, ip, vp, vp]
        for n in ("psx_ransac_homography", "psx_ransac_homography_dev", "psx_ransac_fundamental", "psx_ransac_fundamental_dev",
                  "psx_ransac_affine", "psx_ransac_affine_dev", "psx_ransac_similarity", "psx_ransac_similarity_dev"):
            getattr(L, n).argtypes = [C.c_int, vp, C.c_int, vp, C.c_int, vp, C.c_int, C.POINTER(RansacOpts), C.POINTER(RansacResult),
                                      vp, C.c_int, ip, vp, vp]
        for n in ("psx_ransac_homography_many", "psx_ransac_homography_many_dev", "psx_ransac_fundamental_many", "psx_ransac_fundamental_many_dev",
                  "psx_ransac_affine_many", "psx_ransac_affine_many_dev", "psx_ransac_similarity_many", "psx_ransac_similarity_many_dev"):
            getattr(L, n).argtypes = [C.c_int, vp, vp, C.c_int, vp, C.c_int, vp, vp, C.POINTER(RansacOpts), vp, vp, C.c_int, ip, vp, vp]
        for n in ("psx_ransac_homography_many_ref", "psx_ransac_fundamental_many_ref", "psx_ransac_affine_many_ref", "psx_ransac_similarity_many_ref"):
            getattr(L, n).argtypes = [vp, vp, C.c_int, vp, C.c_int, vp, vp, C.POINTER(RansacOpts), vp, vp, C.c_int, ip, vp, vp]
        L.psx_ransac_many_plan.argtypes = [vp, C.c_int, C.c_int, C.c_int, vp, C.c_int, ip]
        for m in RANSAC_MODELS:
            for n in ("psx_ransac_%s_graph" % m, "psx_ransac_%s_graph_dev" % m):
                getattr(L, n).argtypes = [C.c_int, vp, vp, vp, C.c_int, vp, vp, C.c_int, C.POINTER(RansacOpts), vp, vp, C.c_int, ip, vp, vp]
            getattr(L, "psx_ransac_%s_graph_ref" % m).argtypes = [vp, vp, vp, C.c_int, vp, vp, C.c_int, C.POINTER(RansacOpts), vp, vp, C.c_int, ip,
                                                                   vp, vp]
        for n in ("psx_match_pairs_guided_graph_u8", "psx_match_pairs_guided_graph_u8_dev", "psx_match_pairs_guided_graph",
                  "psx_match_pairs_guided_graph_dev"):
            getattr(L, n).argtypes = [C.c_int, vp, vp, vp, C.c_int, vp, C.c_int, vp, C.POINTER(MatchOpts), vp, C.c_int, vp, ip]
        for n in ("psx_tracks_graph", "psx_tracks_graph_dev"):
            getattr(L, n).argtypes = [C.c_int, vp, vp, vp, C.c_int, vp, C.c_int, C.POINTER(TrackOpts), vp, vp, C.c_int, vp, C.c_int,
                                      C.POINTER(TracksInfo)]
        L.psx_tracks_graph_ref.argtypes = [vp, vp, vp, C.c_int, vp, C.c_int, C.POINTER(TrackOpts), vp, vp, C.c_int, vp, C.c_int, C.POINTER(TracksInfo)]
        L.psx_tracks_plan.argtypes = [vp, C.c_int, vp, C.c_int, C.POINTER(TracksPlanInfo)]
        for n in ("psx_vocab_train_u8", "psx_vocab_train_u8_dev"):
            getattr(L, n).argtypes = [C.c_int, vp, vp, C.c_int, C.POINTER(VocabOpts), vp, C.POINTER(VocabInfo)]
        L.psx_vocab_train_u8_ref.argtypes = [vp, vp, C.c_int, C.POINTER(VocabOpts), vp, C.POINTER(VocabInfo)]
        for n in ("psx_bow_u8", "psx_bow_u8_dev"):
            getattr(L, n).argtypes = [C.c_int, vp, C.c_int, vp, vp, C.c_int, vp, vp]
        L.psx_bow_u8_ref.argtypes = [vp, C.c_int, vp, vp, C.c_int, vp, vp]
        for n in ("psx_shortlist_views", "psx_shortlist_views_dev"):
            getattr(L, n).argtypes = [C.c_int, vp, C.c_int, C.c_int, C.POINTER(ShortlistOpts), vp, vp, vp, C.c_int, ip]
        L.psx_shortlist_views_ref.argtypes = [vp, C.c_int, C.c_int, C.POINTER(ShortlistOpts), vp, vp, vp, C.c_int, ip]
        L.psx_bow_weights.argtypes = [vp, C.c_int, C.c_int, vp]
        L.psx_bow_quantize_dev.argtypes = [C.c_int, vp, C.c_int, C.c_int, vp, vp]
        L.psx_bow_quantize_ref.argtypes = [vp, C.c_int, C.c_int, vp, vp]
        for n in ("psx_shortlist_query", "psx_shortlist_query_dev"):
            getattr(L, n).argtypes = [C.c_int, vp, C.c_int, vp, C.c_int, C.c_int, vp, vp, C.POINTER(QueryOpts), vp, vp, vp, C.c_int, ip]
        L.psx_shortlist_query_ref.argtypes = [vp, C.c_int, vp, C.c_int, C.c_int, vp, vp, C.POINTER(QueryOpts), vp, vp, vp, C.c_int, ip]
        L.psx_shortlist_query_plan.argtypes = [C.c_int, C.c_int, C.c_int, C.c_int, C.POINTER(QueryPlan)]
        L.psx_pyramid_plan.argtypes = [C.c_int] * 4 + [vp] + [C.c_int] * 3 + [vp, C.c_int, ip]
        L.psx_blur_grid_of.argtypes = [C.c_int] * 3
        _LIB = L
    return _LIB


def default_config(**kw):
    c = Config()
    lib().psx_config_default(C.byref(c))
    for k, v in kw.items():
        if not hasattr(c, k):
            raise AttributeError(k)
        setattr(c, k, v)
    return c


def keypoint_bounds(cfg):
    """psx_keypoint_bounds: the levels + 1 float32 level boundaries of automatic keypoint placement."""
    out = (C.c_float * GAUSS_LEVELS)()
    n = C.c_int()
    rc = lib().psx_keypoint_bounds(C.byref(cfg), out, GAUSS_LEVELS, C.byref(n))
    if rc != 0:
        raise PopSiftError("psx_keypoint_bounds failed (%d)" % rc)
    return np.array(out[:n.value], dtype=np.float32)


def place_keypoints(cfg, w, h, kps):
    """psx_place_keypoints: (octave, lpos) int32 arrays for the records kps; octave = -1 where the rule drops one.
    Host only."""
    kps = keypoints_array(kps)
    octave = np.zeros((len(kps),), np.int32)
    lpos = np.zeros((len(kps),), np.int32)
    rc = lib().psx_place_keypoints(C.byref(cfg), w, h, kps.ctypes.data_as(C.c_void_p), len(kps),
                                   octave.ctypes.data_as(C.c_void_p), lpos.ctypes.data_as(C.c_void_p))
    if rc != 0:
        raise PopSiftError("psx_place_keypoints failed (%d)" % rc)
    return octave, lpos


def mask_array(mask):
    """A C-contiguous (h, w) uint8 array of a detection mask given as a 2-D uint8 or bool array (non-zero = allowed)."""
    m = np.asarray(mask)
    if m.ndim != 2 or m.dtype not in (np.dtype(np.uint8), np.dtype(np.bool_)):
        raise TypeError("a mask is a 2-D uint8 or bool array")
    return np.ascontiguousarray(m).view(np.uint8)


def mask_keep(mask, xpos, ypos):
    """psx_mask_keep: the detection mask's rule on the host.  mask: (h, w) uint8 / bool; xpos, ypos: reported positions
    (psx_feature.xpos / ypos).  Returns a bool array, True where a keypoint at that position is allowed.  No device."""
    m = mask_array(mask)
    x = np.ascontiguousarray(xpos, dtype=np.float32).reshape(-1)
    y = np.ascontiguousarray(ypos, dtype=np.float32).reshape(-1)
    if len(x) != len(y):
        raise ValueError("xpos and ypos differ in length")
    keep = np.zeros((len(x),), np.uint8)
    rc = lib().psx_mask_keep(m.ctypes.data_as(C.c_void_p), m.shape[1], m.shape[0], x.ctypes.data_as(C.c_void_p),
                             y.ctypes.data_as(C.c_void_p), len(x), keep.ctypes.data_as(C.c_void_p))
    if rc != 0:
        raise PopSiftError("psx_mask_keep failed (%d)" % rc)
    return keep.astype(bool)


def match(left, right, device=0):
    """psx_match on host arrays: left (n,128) / right (m,128) float32 go to the device through
    psx_dev_alloc / psx_dev_write.  Returns (match (n,3) int32 = best, second, accept; dist (n,2) float32
    squared distances)."""
    L = lib()
    L.psx_match.argtypes = [C.c_int, C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p]
    L.psx_dev_alloc.argtypes = [C.c_int, C.c_size_t, C.POINTER(C.c_void_p)]
    L.psx_dev_free.argtypes = [C.c_int, C.c_void_p]
    L.psx_dev_write.argtypes = [C.c_int, C.c_void_p, C.c_void_p, C.c_size_t]
    left = np.ascontiguousarray(left, dtype=np.float32).reshape(-1, 128)
    right = np.ascontiguousarray(right, dtype=np.float32).reshape(-1, 128)
    bufs = []
    try:
        ptrs = []
        for arr in (left, right):
            p = C.c_void_p()
            if len(arr):
                if L.psx_dev_alloc(device, arr.nbytes, C.byref(p)) != 0:
                    raise PopSiftError("psx_dev_alloc failed")
                bufs.append(p)
                if L.psx_dev_write(device, p, arr.ctypes.data_as(C.c_void_p), arr.nbytes) != 0:
                    raise PopSiftError("psx_dev_write failed")
            ptrs.append(p)
        mm = np.zeros((len(left), 3), np.int32)
        dd = np.zeros((len(left), 2), np.float32)
        rc = L.psx_match(device, ptrs[0], len(left), ptrs[1], len(right),
                         mm.ctypes.data_as(C.c_void_p), dd.ctypes.data_as(C.c_void_p))
        if rc != 0:
            raise PopSiftError("psx_match failed (%d)" % rc)
        return mm, dd
    finally:
        for p in bufs:
            L.psx_dev_free(device, p)


def quantize_rule(desc):
    """The byte rule of include/popsift_hip.h on the host: (uint8) min(255, max(0, roundf(d))), roundf = half away from zero."""
    d = np.asarray(desc, dtype=np.float32)
    # roundf(d) = sign(d) floor(|d| + 0.5) with an EXACT sum (in float32, 0.49999997 + 0.5 rounds to 1): float64 holds it
    exact = np.floor(np.abs(d).astype(np.float64) + 0.5)
    r = np.where(d >= 0, exact, -exact)
    return np.nan_to_num(np.clip(r, 0, 255), nan=0.0).astype(np.uint8)


def _to_device(L, device, arrays, bufs):
    L.psx_dev_alloc.argtypes = [C.c_int, C.c_size_t, C.POINTER(C.c_void_p)]
    L.psx_dev_free.argtypes = [C.c_int, C.c_void_p]
    L.psx_dev_write.argtypes = [C.c_int, C.c_void_p, C.c_void_p, C.c_size_t]
    ptrs = []
    for arr in arrays:
        p = C.c_void_p()
        if arr.nbytes:
            if L.psx_dev_alloc(device, arr.nbytes, C.byref(p)) != 0:
                raise PopSiftError("psx_dev_alloc failed")
            bufs.append(p)
            if L.psx_dev_write(device, p, arr.ctypes.data_as(C.c_void_p), arr.nbytes) != 0:
                raise PopSiftError("psx_dev_write failed")
        ptrs.append(p)
    return ptrs


def quantize(desc, device=0):
    """psx_quantize_desc on a host array of (n,128) float32 descriptors (through device buffers): (n,128) uint8."""
    L = lib()
    L.psx_quantize_desc.argtypes = [C.c_int, C.c_void_p, C.c_int, C.c_void_p]
    L.psx_dev_read.argtypes = [C.c_int, C.c_void_p, C.c_void_p, C.c_size_t]
    desc = np.ascontiguousarray(desc, dtype=np.float32).reshape(-1, 128)
    out = np.zeros(desc.shape, np.uint8)
    bufs = []
    try:
        (ps,) = _to_device(L, device, [desc], bufs)
        pd = C.c_void_p()
        if len(desc):
            if L.psx_dev_alloc(device, out.nbytes, C.byref(pd)) != 0:
                raise PopSiftError("psx_dev_alloc failed")
            bufs.append(pd)
        rc = L.psx_quantize_desc(device, ps, len(desc), pd)
        if rc != 0:
            raise PopSiftError("psx_quantize_desc failed (%d)" % rc)
        if len(desc) and L.psx_dev_read(device, out.ctypes.data_as(C.c_void_p), pd, out.nbytes) != 0:
            raise PopSiftError("psx_dev_read failed")
        return out
    finally:
        for p in bufs:
            L.psx_dev_free(device, p)


def match_u8(left, right, device=0):
    """psx_match_u8 on host arrays of (n,128) / (m,128) uint8 descriptors: (match (n,3) int32 = best, second, accept;
    dist (n,2) int32 squared distances, INT_MAX where there is no neighbour)."""
    L = lib()
    L.psx_match_u8.argtypes = [C.c_int, C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p]
    left = np.ascontiguousarray(left, dtype=np.uint8).reshape(-1, 128)
    right = np.ascontiguousarray(right, dtype=np.uint8).reshape(-1, 128)
    bufs = []
    try:
        pl, pr = _to_device(L, device, [left, right], bufs)
        mm = np.zeros((len(left), 3), np.int32)
        dd = np.zeros((len(left), 2), np.int32)
        rc = L.psx_match_u8(device, pl, len(left), pr, len(right), mm.ctypes.data_as(C.c_void_p), dd.ctypes.data_as(C.c_void_p))
        if rc != 0:
            raise PopSiftError("psx_match_u8 failed (%d)" % rc)
        return mm, dd
    finally:
        for p in bufs:
            L.psx_dev_free(device, p)


def match_opts(ratio=0.8, mutual=False):
    """psx_match_opts from the two keywords every pairs function takes"""
    return MatchOpts(ratio, PAIRS_MUTUAL if mutual else 0)


def _pairs_call(fn, name, device, pl, nl, pr, nr, ratio, mutual, dtype, capacity):
    """One host-output pairs call; capacity None: room for every left descriptor.  Returns (pairs, total count)."""
    cap = nl if capacity is None else capacity
    out = np.zeros((cap,), dtype)
    n = C.c_int(-1)
    o = match_opts(ratio, mutual)
    rc = fn(device, pl, nl, pr, nr, C.byref(o), out.ctypes.data_as(C.c_void_p) if cap else None, cap, C.byref(n))
    if rc != 0:
        raise PopSiftError("%s failed (%d)" % (name, rc))
    return out[:min(n.value, cap)], n.value


def match_pairs(left, right, ratio=0.8, mutual=False, device=0, capacity=None):
    """psx_match_pairs on host arrays of (n,128) / (m,128) float32 descriptors (through device buffers): the PAIR_DTYPE
    records of the pairs that pass the ratio test (and the cross-check, with mutual), in ascending left.  With a
    capacity: (the first min(count, capacity) records, count)."""
    L = lib()
    left = np.ascontiguousarray(left, dtype=np.float32).reshape(-1, 128)
    right = np.ascontiguousarray(right, dtype=np.float32).reshape(-1, 128)
    bufs = []
    try:
        pl, pr = _to_device(L, device, [left, right], bufs)
        got = _pairs_call(L.psx_match_pairs, "psx_match_pairs", device, pl, len(left), pr, len(right), ratio, mutual, PAIR_DTYPE, capacity)
        return got[0] if capacity is None else got
    finally:
        for p in bufs:
            L.psx_dev_free(device, p)


def match_pairs_u8(left, right, ratio=0.8, mutual=False, device=0, capacity=None):
    """psx_match_pairs_u8 on host arrays of (n,128) / (m,128) uint8 descriptors: PAIR_U8_DTYPE records, as match_pairs."""
    L = lib()
    left = np.ascontiguousarray(left, dtype=np.uint8).reshape(-1, 128)
    right = np.ascontiguousarray(right, dtype=np.uint8).reshape(-1, 128)
    bufs = []
    try:
        pl, pr = _to_device(L, device, [left, right], bufs)
        got = _pairs_call(L.psx_match_pairs_u8, "psx_match_pairs_u8", device, pl, len(left), pr, len(right), ratio, mutual, PAIR_U8_DTYPE, capacity)
        return got[0] if capacity is None else got
    finally:
        for p in bufs:
            L.psx_dev_free(device, p)


def match_pairs_dev(left_ptr, l_len, right_ptr, r_len, out_ptr, capacity, ratio=0.8, mutual=False, device=0, u8=False):
    """psx_match_pairs_dev / psx_match_pairs_u8_dev on DEVICE pointers (e.g. tensor.data_ptr()): the records go into
    the caller's device buffer at out_ptr (16-byte aligned, `capacity` records); returns the total count."""
    L = lib()
    fn = L.psx_match_pairs_u8_dev if u8 else L.psx_match_pairs_dev
    n = C.c_int(-1)
    o = match_opts(ratio, mutual)
    rc = fn(device, C.c_void_p(left_ptr), l_len, C.c_void_p(right_ptr), r_len, C.byref(o), C.c_void_p(out_ptr), capacity, C.byref(n))
    if rc != 0:
        raise PopSiftError("psx_match_pairs%s_dev failed (%d)" % ("_u8" if u8 else "", rc))
    return n.value


def _many_call(fn, name, device, left_ptr, l_len, right_ptrs, r_lens, out_ptr, capacity, ratio, mutual):
    """One one-to-many call on device pointers: (per-set counts (n_sets,) int32, total count)"""
    k = len(r_lens)
    ptrs = (C.c_void_p * max(k, 1))(*[p.value if isinstance(p, C.c_void_p) else p for p in right_ptrs])
    lens = np.ascontiguousarray(r_lens, dtype=np.int32)
    counts = np.full((k,), -1, np.int32)
    n = C.c_int(-1)
    o = match_opts(ratio, mutual)
    rc = fn(device, left_ptr, l_len, ptrs if k else None, lens.ctypes.data_as(C.c_void_p) if k else None, k, C.byref(o),
            out_ptr, capacity, counts.ctypes.data_as(C.c_void_p) if k else None, C.byref(n))
    if rc != 0:
        raise PopSiftError("%s failed (%d)" % (name, rc))
    return counts, n.value


def split_sets(records, set_counts, capacity=None):
    """The concatenated list of a one-to-many call as one array per set (a prefix sum of the counts); with a capacity
    the sets behind it are cut as the call cut them."""
    cap = len(records) if capacity is None else min(capacity, len(records))
    ends = np.minimum(np.cumsum(np.asarray(set_counts, np.int64)), cap)
    starts = np.concatenate([[0], ends[:-1]]) if len(ends) else ends
    return [records[int(a):int(b)] for a, b in zip(starts, ends)]


def match_pairs_many_u8(left, rights, ratio=0.8, mutual=False, device=0, capacity=None):
    """psx_match_pairs_many_u8 on host arrays: left (n,128) uint8 against every (m_k,128) uint8 array of `rights` in ONE
    call.  Returns (list of per-set PAIR_U8_DTYPE arrays -- set k's equals match_pairs_u8(left, rights[k]), `right`
    indexing rights[k] -- , per-set counts); with a capacity the list holds the first `capacity` records of the
    concatenation and the counts are still the totals."""
    L = lib()
    left = np.ascontiguousarray(left, dtype=np.uint8).reshape(-1, 128)
    rights = [np.ascontiguousarray(r, dtype=np.uint8).reshape(-1, 128) for r in rights]
    bufs = []
    try:
        ptrs = _to_device(L, device, [left] + rights, bufs)
        cap = len(left) * len(rights) if capacity is None else capacity
        out = np.zeros((cap,), PAIR_U8_DTYPE)
        counts, n = _many_call(L.psx_match_pairs_many_u8, "psx_match_pairs_many_u8", device, ptrs[0], len(left), ptrs[1:],
                               [len(r) for r in rights], out.ctypes.data_as(C.c_void_p) if cap else None, cap, ratio, mutual)
        return split_sets(out[:min(n, cap)], counts), counts
    finally:
        for p in bufs:
            L.psx_dev_free(device, p)


def match_pairs_many(left, rights, ratio=0.8, mutual=False, device=0, capacity=None):
    """psx_match_pairs_many on host arrays: left (n,128) float32 against every (m_k,128) float32 array of `rights` in ONE
    call.  Returns (list of per-set PAIR_DTYPE arrays -- set k's equals match_pairs(left, rights[k]), `right` indexing
    rights[k] -- , per-set counts); with a capacity the list holds the first `capacity` records of the concatenation and
    the counts are still the totals."""
    L = lib()
    left = np.ascontiguousarray(left, dtype=np.float32).reshape(-1, 128)
    rights = [np.ascontiguousarray(r, dtype=np.float32).reshape(-1, 128) for r in rights]
    bufs = []
    try:
        ptrs = _to_device(L, device, [left] + rights, bufs)
        cap = len(left) * len(rights) if capacity is None else capacity
        out = np.zeros((cap,), PAIR_DTYPE)
        counts, n = _many_call(L.psx_match_pairs_many, "psx_match_pairs_many", device, ptrs[0], len(left), ptrs[1:],
                               [len(r) for r in rights], out.ctypes.data_as(C.c_void_p) if cap else None, cap, ratio, mutual)
        return split_sets(out[:min(n, cap)], counts), counts
    finally:
        for p in bufs:
            L.psx_dev_free(device, p)


def match_pairs_many_dev(left_ptr, l_len, right_ptrs, r_lens, out_ptr, capacity, ratio=0.8, mutual=False, device=0, u8=True):
    """psx_match_pairs_many_u8_dev (u8=False: psx_match_pairs_many_dev, float descriptors) on DEVICE pointers (e.g.
    tensor.data_ptr()): the concatenated records go into the caller's device buffer at out_ptr (16-byte aligned,
    `capacity` records); returns (per-set counts, total count)."""
    name = "psx_match_pairs_many_u8_dev" if u8 else "psx_match_pairs_many_dev"
    return _many_call(getattr(lib(), name), name, device, C.c_void_p(left_ptr), l_len,
                      list(right_ptrs), r_lens, C.c_void_p(out_ptr), capacity, ratio, mutual)


def match_many_f32_plan(l_len, r_lens, mutual=False, mfma_enabled=True):
    """psx_match_many_f32_plan: what psx_match_pairs_many decides for these sizes, as a dict (path, fwd_groups, bwd_groups,
    launches, scratch_bytes).  No device."""
    lens = np.ascontiguousarray(r_lens, dtype=np.int32)
    out = ManyF32Plan()
    rc = lib().psx_match_many_f32_plan(l_len, lens.ctypes.data_as(C.c_void_p) if len(lens) else None, len(lens),
                                       PAIRS_MUTUAL if mutual else 0, 1 if mfma_enabled else 0, C.byref(out))
    if rc != 0:
        raise PopSiftError("psx_match_many_f32_plan failed (%d)" % rc)
    return {n: int(getattr(out, n)) for n, _ in ManyF32Plan._fields_}


def match_many_f32_last():
    """psx_match_many_f32_last: the calling thread's last match_pairs_many / match_pairs_many_dev(u8=False) call as a dict
    (path, fell_back, launches, syncs); zeros before any"""
    out = ManyF32Info()
    rc = lib().psx_match_many_f32_last(C.byref(out))
    if rc != 0:
        raise PopSiftError("psx_match_many_f32_last failed (%d)" % rc)
    return {n: int(getattr(out, n)) for n, _ in ManyF32Info._fields_}


def match_many_plan(l_len, r_lens, backward=False):
    """psx_match_many_plan: (chunks (n,3) int32 = set, r0, r1; blocks (m,2) int32 = set, row0) of one direction.  No device."""
    L = lib()
    lens = np.ascontiguousarray(r_lens, dtype=np.int32)
    nc, nb = C.c_int(-1), C.c_int(-1)
    args = (l_len, lens.ctypes.data_as(C.c_void_p) if len(lens) else None, len(lens), 1 if backward else 0)
    rc = L.psx_match_many_plan(*args, None, 0, C.byref(nc), None, 0, C.byref(nb))
    if rc != 0:
        raise PopSiftError("psx_match_many_plan failed (%d)" % rc)
    chunks, blocks = np.zeros((nc.value, 3), np.int32), np.zeros((nb.value, 2), np.int32)
    rc = L.psx_match_many_plan(*args, chunks.ctypes.data_as(C.c_void_p) if nc.value else None, nc.value, C.byref(nc),
                               blocks.ctypes.data_as(C.c_void_p) if nb.value else None, nb.value, C.byref(nb))
    if rc != 0:
        raise PopSiftError("psx_match_many_plan failed (%d)" % rc)
    return chunks, blocks


def _graph_edges(edges):
    """an edge list as the (n, 2) int32 array of psx_view_edge records"""
    e = np.ascontiguousarray(edges, dtype=np.int32)
    return e.reshape(-1, 2)


def _graph_call(fn, name, device, set_ptrs, lens, edges, out_ptr, capacity, ratio, mutual):
    """One edge-list call on device pointers: (per-edge counts (n_edges,) int32, total count)"""
    k = len(lens)
    ptrs = (C.c_void_p * max(k, 1))(*[p.value if isinstance(p, C.c_void_p) else p for p in set_ptrs])
    la = np.ascontiguousarray(lens, dtype=np.int32)
    ea = _graph_edges(edges)
    counts = np.full((len(ea),), -1, np.int32)
    n = C.c_int(-1)
    o = match_opts(ratio, mutual)
    rc = fn(device, ptrs if k else None, la.ctypes.data_as(C.c_void_p) if k else None, k,
            ea.ctypes.data_as(C.c_void_p) if len(ea) else None, len(ea), C.byref(o), out_ptr, capacity,
            counts.ctypes.data_as(C.c_void_p) if len(ea) else None, C.byref(n))
    if rc != 0:
        raise PopSiftError("%s failed (%d)" % (name, rc))
    return counts, n.value


def _match_pairs_graph(name, dtype, pair_dtype, sets, edges, ratio, mutual, device, capacity):
    L = lib()
    sets = [np.ascontiguousarray(s, dtype=dtype).reshape(-1, 128) for s in sets]
    ea = _graph_edges(edges)
    bufs = []
    try:
        ptrs = _to_device(L, device, sets, bufs) if sets else []
        lens = [len(s) for s in sets]
        ok = all(0 <= a < len(sets) and 0 <= b < len(sets) for a, b in ea)
        cap = (sum(lens[a] for a, _ in ea) if ok else 0) if capacity is None else capacity
        out = np.zeros((cap,), pair_dtype)
        counts, n = _graph_call(getattr(L, name), name, device, ptrs, lens, ea,
                                out.ctypes.data_as(C.c_void_p) if cap else None, cap, ratio, mutual)
        return split_sets(out[:min(n, cap)], counts), counts
    finally:
        for p in bufs:
            L.psx_dev_free(device, p)


def match_pairs_graph_u8(sets, edges, ratio=0.8, mutual=False, device=0, capacity=None):
    """psx_match_pairs_graph_u8 on host arrays: `sets` are (n_s,128) uint8 arrays, `edges` (left, right) index pairs into
    them, all matched in ONE call.  Returns (list of per-edge PAIR_U8_DTYPE arrays -- edge e's equals
    match_pairs_u8(sets[left], sets[right]), in the order of the edge list --, per-edge counts); with a capacity the list
    holds the first `capacity` records of the concatenation and the counts are still the totals."""
    return _match_pairs_graph("psx_match_pairs_graph_u8", np.uint8, PAIR_U8_DTYPE, sets, edges, ratio, mutual, device, capacity)


def match_pairs_graph(sets, edges, ratio=0.8, mutual=False, device=0, capacity=None):
    """psx_match_pairs_graph on host arrays, the float form of match_pairs_graph_u8: `sets` are (n_s,128) float32 arrays.
    Returns (list of per-edge PAIR_DTYPE arrays -- edge e's equals match_pairs(sets[left], sets[right]) --, per-edge
    counts); capacity as there."""
    return _match_pairs_graph("psx_match_pairs_graph", np.float32, PAIR_DTYPE, sets, edges, ratio, mutual, device, capacity)


def match_pairs_graph_dev(ptrs, lens, edges, out_ptr, capacity, ratio=0.8, mutual=False, device=0, u8=True):
    """psx_match_pairs_graph_u8_dev (u8=False: psx_match_pairs_graph_dev, float descriptors) on DEVICE pointers (e.g.
    tensor.data_ptr()): the concatenated records go into the caller's device buffer at out_ptr (16-byte aligned,
    `capacity` records); returns (per-edge counts, total count).  With the edge list grouped by left, a left view's slice
    of the buffer and of the counts is what match_pairs_many_dev leaves for that star: ransac_*_many_dev and
    match_pairs_guided_many_dev take it unchanged."""
    name = "psx_match_pairs_graph_u8_dev" if u8 else "psx_match_pairs_graph_dev"
    return _graph_call(getattr(lib(), name), name, device, list(ptrs), lens, edges, C.c_void_p(out_ptr), capacity, ratio, mutual)


def match_graph_f32_plan(lens, edges, mutual=False, mfma_enabled=True):
    """psx_match_graph_f32_plan: what psx_match_pairs_graph decides and plans for these sizes, as a dict (path,
    referenced_sets, blocks, chunks, chunk_len, fwd_items, bwd_items, fwd_groups, bwd_groups, join_workgroups, launches,
    scratch_bytes).  No device."""
    la = np.ascontiguousarray(lens, dtype=np.int32)
    ea = _graph_edges(edges)
    out = GraphF32PlanInfo()
    rc = lib().psx_match_graph_f32_plan(la.ctypes.data_as(C.c_void_p) if len(la) else None, len(la),
                                        ea.ctypes.data_as(C.c_void_p) if len(ea) else None, len(ea), PAIRS_MUTUAL if mutual else 0,
                                        1 if mfma_enabled else 0, C.byref(out))
    if rc != 0:
        raise PopSiftError("psx_match_graph_f32_plan failed (%d)" % rc)
    return {n: int(getattr(out, n)) for n, _ in GraphF32PlanInfo._fields_}


def match_graph_f32_last():
    """psx_match_graph_f32_last: the calling thread's last match_pairs_graph / match_pairs_graph_dev(u8=False) call as a
    dict (path, fell_back, launches, syncs); zeros before any"""
    out = ManyF32Info()
    rc = lib().psx_match_graph_f32_last(C.byref(out))
    if rc != 0:
        raise PopSiftError("psx_match_graph_f32_last failed (%d)" % rc)
    return {n: int(getattr(out, n)) for n, _ in ManyF32Info._fields_}


def match_graph_plan(lens, edges, mutual=False):
    """psx_match_graph_plan: what psx_match_pairs_graph_u8 plans for these sizes, as a dict (referenced_sets, blocks, chunks,
    chunk_len, fwd_items, bwd_items, fwd_groups, bwd_groups, join_workgroups, launches, scratch_bytes).  No device."""
    la = np.ascontiguousarray(lens, dtype=np.int32)
    ea = _graph_edges(edges)
    out = GraphPlanInfo()
    rc = lib().psx_match_graph_plan(la.ctypes.data_as(C.c_void_p) if len(la) else None, len(la),
                                    ea.ctypes.data_as(C.c_void_p) if len(ea) else None, len(ea), PAIRS_MUTUAL if mutual else 0, C.byref(out))
    if rc != 0:
        raise PopSiftError("psx_match_graph_plan failed (%d)" % rc)
    return {n: int(getattr(out, n)) for n, _ in GraphPlanInfo._fields_}


def pairs_join(fwd_match, fwd_dist, bwd_match, r_len, ratio=0.8, mutual=False, capacity=None):
    """psx_pairs_join / psx_pairs_join_u8 (chosen by fwd_dist.dtype: float32 or int32): the join alone, on directed
    results held on the host -- fwd_* = match(L, R), bwd_match = match(R, L)[0] or None without mutual.  No device.
    Returns the pair records; with a capacity (records, count)."""
    L = lib()
    fwd_dist = np.asarray(fwd_dist)
    if fwd_dist.dtype == np.float32:
        fn, name, dtype = L.psx_pairs_join, "psx_pairs_join", PAIR_DTYPE
    elif fwd_dist.dtype == np.int32:
        fn, name, dtype = L.psx_pairs_join_u8, "psx_pairs_join_u8", PAIR_U8_DTYPE
    else:
        raise TypeError("fwd_dist must be float32 (psx_match) or int32 (psx_match_u8)")
    fm = np.ascontiguousarray(fwd_match, dtype=np.int32).reshape(-1, 3)
    fd = np.ascontiguousarray(fwd_dist).reshape(-1, 2)
    if len(fm) != len(fd):
        raise ValueError("fwd_match and fwd_dist differ in length")
    bm = None if bwd_match is None else np.ascontiguousarray(bwd_match, dtype=np.int32).reshape(-1, 3)
    if bm is not None and len(bm) != r_len:
        raise ValueError("bwd_match must have r_len rows")
    ptr = lambda a: a.ctypes.data_as(C.c_void_p) if a is not None and a.size else None
    join = lambda dev, pm, nl, pb, nr, *rest: fn(pm, ptr(fd), nl, pb, nr, *rest)
    got = _pairs_call(join, name, 0, ptr(fm), len(fm), ptr(bm), r_len, ratio, mutual, dtype, capacity)
    return got[0] if capacity is None else got


def _xy(xy):
    """(n, 2) float32 positions, C-contiguous"""
    return np.ascontiguousarray(xy, dtype=np.float32).reshape(-1, 2)


def guide_allows(guide, left_xy, right_xy):
    """psx_guide_allows: the guide's rule on the host.  left_xy (nl, 2), right_xy (nr, 2): positions in input-image units.
    Returns the (nl, nr) bool relation, [i, j] True where (left i, right j) is admissible.  No device."""
    lx, rx = _xy(left_xy), _xy(right_xy)
    out = np.zeros((len(lx), len(rx)), np.uint8)
    ptr = lambda a: a.ctypes.data_as(C.c_void_p) if a.size else None
    rc = lib().psx_guide_allows(C.byref(guide), ptr(lx), len(lx), ptr(rx), len(rx), ptr(out))
    if rc != 0:
        raise PopSiftError("psx_guide_allows failed (%d)" % rc)
    return out.astype(bool)


def desc_positions(features_ptr, reverse_map_ptr, n_desc, xy_ptr, device=0):
    """psx_desc_positions on DEVICE pointers: xy[k] = (xpos, ypos) of the feature descriptor k belongs to, gathered from
    what psx_clone_results leaves; xy_ptr: 2 n_desc floats, 8-byte aligned."""
    rc = lib().psx_desc_positions(device, C.c_void_p(features_ptr), C.c_void_p(reverse_map_ptr), n_desc, C.c_void_p(xy_ptr))
    if rc != 0:
        raise PopSiftError("psx_desc_positions failed (%d)" % rc)


def _guided_sides(left, left_xy, right, right_xy, dtype):
    left = np.ascontiguousarray(left, dtype=dtype).reshape(-1, 128)
    right = np.ascontiguousarray(right, dtype=dtype).reshape(-1, 128)
    lx, rx = _xy(left_xy), _xy(right_xy)
    if len(lx) != len(left) or len(rx) != len(right):
        raise ValueError("one position per descriptor")
    return left, lx, right, rx


def _match_guided(name, dtype, ddtype, left, left_xy, right, right_xy, guide, device):
    L = lib()
    left, lx, right, rx = _guided_sides(left, left_xy, right, right_xy, dtype)
    bufs = []
    try:
        pl, plx, pr, prx = _to_device(L, device, [left, lx, right, rx], bufs)
        mm = np.zeros((len(left), 3), np.int32)
        dd = np.zeros((len(left), 2), ddtype)
        rc = getattr(L, name)(device, pl, plx, len(left), pr, prx, len(right), C.byref(guide),
                              mm.ctypes.data_as(C.c_void_p), dd.ctypes.data_as(C.c_void_p))
        if rc != 0:
            raise PopSiftError("%s failed (%d)" % (name, rc))
        return mm, dd
    finally:
        for p in bufs:
            L.psx_dev_free(device, p)


def match_guided(left, left_xy, right, right_xy, guide, device=0):
    """psx_match_guided on host arrays (through device buffers): as match(), every left descriptor's search restricted to
    the right descriptors the guide admits.  left_xy / right_xy: (n, 2) / (m, 2) float32 positions."""
    return _match_guided("psx_match_guided", np.float32, np.float32, left, left_xy, right, right_xy, guide, device)


def match_guided_u8(left, left_xy, right, right_xy, guide, device=0):
    """psx_match_guided_u8 on host arrays of uint8 descriptors: as match_u8(), restricted by the guide."""
    return _match_guided("psx_match_guided_u8", np.uint8, np.int32, left, left_xy, right, right_xy, guide, device)


def _guided_fn(fn, plx, prx, guide):
    """a guided pairs entry point with the argument order _pairs_call uses"""
    return lambda dev, pl, nl, pr, nr, *rest: fn(dev, pl, plx, nl, pr, prx, nr, C.byref(guide), *rest)


def _match_pairs_guided(name, dtype, pair_dtype, left, left_xy, right, right_xy, guide, ratio, mutual, device, capacity):
    L = lib()
    left, lx, right, rx = _guided_sides(left, left_xy, right, right_xy, dtype)
    bufs = []
    try:
        pl, plx, pr, prx = _to_device(L, device, [left, lx, right, rx], bufs)
        got = _pairs_call(_guided_fn(getattr(L, name), plx, prx, guide), name, device, pl, len(left), pr, len(right), ratio, mutual,
                          pair_dtype, capacity)
        return got[0] if capacity is None else got
    finally:
        for p in bufs:
            L.psx_dev_free(device, p)


def match_pairs_guided(left, left_xy, right, right_xy, guide, ratio=0.8, mutual=False, device=0, capacity=None):
    """psx_match_pairs_guided on host arrays (through device buffers): PAIR_DTYPE records as match_pairs(), from guided
    directed passes.  With a capacity: (the first min(count, capacity) records, count)."""
    return _match_pairs_guided("psx_match_pairs_guided", np.float32, PAIR_DTYPE, left, left_xy, right, right_xy, guide, ratio, mutual,
                               device, capacity)


def match_pairs_guided_u8(left, left_xy, right, right_xy, guide, ratio=0.8, mutual=False, device=0, capacity=None):
    """psx_match_pairs_guided_u8 on host arrays of uint8 descriptors: PAIR_U8_DTYPE records, as match_pairs_guided."""
    return _match_pairs_guided("psx_match_pairs_guided_u8", np.uint8, PAIR_U8_DTYPE, left, left_xy, right, right_xy, guide, ratio, mutual,
                               device, capacity)


def match_pairs_guided_dev(left_ptr, left_xy_ptr, l_len, right_ptr, right_xy_ptr, r_len, guide, out_ptr, capacity, ratio=0.8,
                           mutual=False, device=0, u8=False):
    """psx_match_pairs_guided_dev / psx_match_pairs_guided_u8_dev on DEVICE pointers: the records go into the caller's
    device buffer at out_ptr (16-byte aligned, `capacity` records); returns the total count."""
    L = lib()
    fn = L.psx_match_pairs_guided_u8_dev if u8 else L.psx_match_pairs_guided_dev
    n = C.c_int(-1)
    o = match_opts(ratio, mutual)
    rc = fn(device, C.c_void_p(left_ptr), C.c_void_p(left_xy_ptr), l_len, C.c_void_p(right_ptr), C.c_void_p(right_xy_ptr), r_len,
            C.byref(guide), C.byref(o), C.c_void_p(out_ptr), capacity, C.byref(n))
    if rc != 0:
        raise PopSiftError("psx_match_pairs_guided%s_dev failed (%d)" % ("_u8" if u8 else "", rc))
    return n.value


def _guide_array(guides):
    """a HOST array of psx_guide from a sequence of Guide (None stands for Guide.none())"""
    gs = [Guide.none() if g is None else g for g in guides]
    return (Guide * max(len(gs), 1))(*gs)


def _guided_many_call(fn, name, device, left_ptr, left_xy_ptr, l_len, right_ptrs, right_xy_ptrs, r_lens, guides, out_ptr, capacity,
                      ratio, mutual):
    """One guided one-to-many call on device pointers: (per-set counts (n_sets,) int32, total count)"""
    k = len(r_lens)
    if not (len(right_ptrs) == len(right_xy_ptrs) == len(guides) == k):
        raise ValueError("one descriptor pointer, one position pointer and one guide per set")
    val = lambda p: p.value if isinstance(p, C.c_void_p) else p
    ptrs = (C.c_void_p * max(k, 1))(*[val(p) for p in right_ptrs])
    xptrs = (C.c_void_p * max(k, 1))(*[val(p) for p in right_xy_ptrs])
    lens = np.ascontiguousarray(r_lens, dtype=np.int32)
    garr = _guide_array(guides)
    counts = np.full((k,), -1, np.int32)
    n = C.c_int(-1)
    o = match_opts(ratio, mutual)
    rc = fn(device, left_ptr, left_xy_ptr, l_len, ptrs if k else None, xptrs if k else None, lens.ctypes.data_as(C.c_void_p) if k else None,
            k, garr if k else None, C.byref(o), out_ptr, capacity, counts.ctypes.data_as(C.c_void_p) if k else None, C.byref(n))
    if rc != 0:
        raise PopSiftError("%s failed (%d)" % (name, rc))
    return counts, n.value


def match_pairs_guided_many(left, left_xy, rights, right_xys, guides, ratio=0.8, mutual=False, device=0, capacity=None):
    """psx_match_pairs_guided_many on host arrays, the float form of match_pairs_guided_many_u8: (n,128) float32 arrays,
    per-set PAIR_DTYPE arrays -- set k's equals match_pairs_guided(left, left_xy, rights[k], right_xys[k], guides[k])."""
    return _match_pairs_guided_many("psx_match_pairs_guided_many", np.float32, PAIR_DTYPE, left, left_xy, rights, right_xys, guides, ratio,
                                    mutual, device, capacity)


def match_pairs_guided_many_u8(left, left_xy, rights, right_xys, guides, ratio=0.8, mutual=False, device=0, capacity=None):
    """psx_match_pairs_guided_many_u8 on host arrays: left (n,128) uint8 with positions left_xy (n,2) against every
    (m_k,128) uint8 array of `rights` with positions right_xys[k], set k under guides[k], in ONE call.  A guide of kind
    GUIDE_NONE (Guide.none(), or None) skips its set; that set's arrays may be None.  Returns (list of per-set
    PAIR_U8_DTYPE arrays -- set k's equals match_pairs_guided_u8(left, left_xy, rights[k], right_xys[k], guides[k]) --,
    per-set counts); with a capacity the list holds the first `capacity` records of the concatenation and the counts are
    still the totals."""
    return _match_pairs_guided_many("psx_match_pairs_guided_many_u8", np.uint8, PAIR_U8_DTYPE, left, left_xy, rights, right_xys, guides, ratio,
                                    mutual, device, capacity)


def _match_pairs_guided_many(name, dtype, pair_dtype, left, left_xy, rights, right_xys, guides, ratio, mutual, device, capacity):
    L = lib()
    if not (len(rights) == len(right_xys) == len(guides)):
        raise ValueError("one descriptor array, one position array and one guide per set")
    empty, empty_xy = np.zeros((0, 128), dtype), np.zeros((0, 2), np.float32)
    sides = [_guided_sides(left, left_xy, empty if r is None else r, empty_xy if x is None else x, dtype) for r, x in zip(rights, right_xys)]
    left, lx = _guided_sides(left, left_xy, empty, empty_xy, dtype)[:2]
    bufs = []
    try:
        ptrs = _to_device(L, device, [left, lx] + [s[2] for s in sides] + [s[3] for s in sides], bufs)
        k = len(sides)
        cap = len(left) * k if capacity is None else capacity
        out = np.zeros((cap,), pair_dtype)
        counts, n = _guided_many_call(getattr(L, name), name, device, ptrs[0], ptrs[1], len(left),
                                      ptrs[2:2 + k], ptrs[2 + k:], [len(s[2]) for s in sides], guides,
                                      out.ctypes.data_as(C.c_void_p) if cap else None, cap, ratio, mutual)
        return split_sets(out[:min(n, cap)], counts), counts
    finally:
        for p in bufs:
            L.psx_dev_free(device, p)


def match_pairs_guided_many_dev(left_ptr, left_xy_ptr, l_len, right_ptrs, right_xy_ptrs, r_lens, guides, out_ptr, capacity, ratio=0.8,
                                mutual=False, device=0, u8=True):
    """psx_match_pairs_guided_many_u8_dev (u8=False: psx_match_pairs_guided_many_dev, float descriptors) on DEVICE pointers
    (e.g. tensor.data_ptr()): the concatenated records go into the caller's device buffer at out_ptr (16-byte aligned,
    `capacity` records); returns (per-set counts, total count)."""
    name = "psx_match_pairs_guided_many_u8_dev" if u8 else "psx_match_pairs_guided_many_dev"
    return _guided_many_call(getattr(lib(), name), name, device, C.c_void_p(left_ptr),
                             C.c_void_p(left_xy_ptr), l_len, list(right_ptrs), list(right_xy_ptrs), r_lens, guides, C.c_void_p(out_ptr),
                             capacity, ratio, mutual)


def guides_from_ransac(results, kind, tol):
    """psx_guides_from_ransac: the results of ransac_*_many* (RansacResult objects) as the guides of
    match_pairs_guided_many_*: a result without a model (best < 0) becomes Guide.none(), every other one
    Guide(kind, its matrix, tol).  kind: GUIDE_HOMOGRAPHY or GUIDE_EPIPOLAR.  No device."""
    k = len(results)
    res = (RansacResult * max(k, 1))(*results)
    out = (Guide * max(k, 1))()
    rc = lib().psx_guides_from_ransac(res if k else None, k, kind, float(np.float32(tol)), out if k else None)
    if rc != 0:
        raise PopSiftError("psx_guides_from_ransac failed (%d)" % rc)
    return [Guide(g.kind, g.m, g.tol) for g in out[:k]]


def ransac_opts(tol=2.0, hypotheses=1024, seed=0, refit=True):
    """psx_ransac_opts from keywords"""
    return RansacOpts(float(np.float32(tol)), int(hypotheses), int(seed) & 0xffffffff, RANSAC_REFIT if refit else 0)


def ransac_samples(seed, first, count, n, k=4):
    """psx_ransac_samples (k = 4, the homography's) / psx_ransac_samples_k (any other k; the fundamental matrix draws 8, the
    affine transform 3, the similarity 2): the
    (count, k) int32 pair indices of hypotheses first .. first + count - 1 among n pairs.  No device."""
    out = np.zeros((count, max(int(k), 0)), np.int32)
    po = out.ctypes.data_as(C.c_void_p) if out.size else None
    if k == 4:
        rc = lib().psx_ransac_samples(int(seed) & 0xffffffff, first, count, n, po)
    else:
        rc = lib().psx_ransac_samples_k(int(seed) & 0xffffffff, first, count, n, k, po)
    if rc != 0:
        raise PopSiftError("psx_ransac_samples%s failed (%d)" % ("" if k == 4 else "_k", rc))
    return out


def homography_fit(left_xy, right_xy):
    """psx_homography_fit: the 9 float32 entries (row major) of the model fitted to left_xy[i] -> right_xy[i], in the given
    order; a degenerate input gives non-finite entries.  No device."""
    lx, rx = _xy(left_xy), _xy(right_xy)
    if len(lx) != len(rx):
        raise ValueError("one right position per left position")
    m = np.zeros(9, np.float32)
    rc = lib().psx_homography_fit(lx.ctypes.data_as(C.c_void_p), rx.ctypes.data_as(C.c_void_p), len(lx), m.ctypes.data_as(C.c_void_p))
    if rc != 0:
        raise PopSiftError("psx_homography_fit failed (%d)" % rc)
    return m


def fundamental_fit(left_xy, right_xy):
    """psx_fundamental_fit: the 9 float32 entries (row major, (xr yr 1) F (xl yl 1)^T = 0) of the fundamental matrix fitted to
    n >= 8 correspondences left_xy[i] -> right_xy[i], in the given order.  No device."""
    lx, rx = _xy(left_xy), _xy(right_xy)
    if len(lx) != len(rx):
        raise ValueError("one right position per left position")
    m = np.zeros(9, np.float32)
    rc = lib().psx_fundamental_fit(lx.ctypes.data_as(C.c_void_p), rx.ctypes.data_as(C.c_void_p), len(lx), m.ctypes.data_as(C.c_void_p))
    if rc != 0:
        raise PopSiftError("psx_fundamental_fit failed (%d)" % rc)
    return m


def _fit_xy(name, left_xy, right_xy):
    lx, rx = _xy(left_xy), _xy(right_xy)
    if len(lx) != len(rx):
        raise ValueError("one right position per left position")
    m = np.zeros(9, np.float32)
    rc = getattr(lib(), name)(lx.ctypes.data_as(C.c_void_p), rx.ctypes.data_as(C.c_void_p), len(lx), m.ctypes.data_as(C.c_void_p))
    if rc != 0:
        raise PopSiftError("%s failed (%d)" % (name, rc))
    return m


def affine_fit(left_xy, right_xy):
    """psx_affine_fit: the 9 float32 entries (row major, last row exactly 0 0 1) of the 2-D affine transform fitted to n >= 3
    correspondences left_xy[i] -> right_xy[i], in the given order.  No device."""
    return _fit_xy("psx_affine_fit", left_xy, right_xy)


def similarity_fit(left_xy, right_xy):
    """psx_similarity_fit: as affine_fit for a similarity (rotation, uniform scale, translation) and n >= 2.  No device."""
    return _fit_xy("psx_similarity_fit", left_xy, right_xy)


def _pair_records(pairs):
    """16-byte pair records (PAIR_DTYPE or PAIR_U8_DTYPE), C-contiguous"""
    pairs = np.ascontiguousarray(pairs).reshape(-1)
    if pairs.dtype.itemsize != 16:
        raise TypeError("pairs must be PAIR_DTYPE or PAIR_U8_DTYPE records")
    return pairs


def _ransac_call(fn, name, pairs_ptr, n, dtype, plx, nl, prx, nr, opts, capacity, layers, out_ptr=None, kind=GUIDE_HOMOGRAPHY):
    """One RANSAC call.  out_ptr None: the inliers come back in a host array.  Returns a dict: result (RansacResult), count,
    inliers (host forms), and with layers models (N, 9) and counts (N).  kind: the guide the result's model is."""
    cap = n if capacity is None else capacity
    N = max(int(opts.hypotheses), 0)
    res, cnt = RansacResult(), C.c_int(-1)
    out = np.zeros((cap,), dtype) if out_ptr is None else None
    models = np.zeros((N, 9), np.float32) if layers else None
    counts = np.zeros((N,), np.int32) if layers else None
    ptr = lambda a: a.ctypes.data_as(C.c_void_p) if a is not None and a.size else None
    po = ptr(out) if out_ptr is None else (C.c_void_p(out_ptr) if cap else None)
    rc = fn(pairs_ptr, n, plx, nl, prx, nr, C.byref(opts), C.byref(res), po, cap, C.byref(cnt), ptr(models), ptr(counts))
    if rc != 0:
        raise PopSiftError("%s failed (%d)" % (name, rc))
    res.kind = kind
    got = dict(result=res, count=cnt.value)
    if out is not None:
        got["inliers"] = out[:min(cnt.value, cap)]
    if layers:
        got["models"], got["counts"] = models, counts
    return got


def _ransac_names(model):
    """(C name stem, guide kind) of the model "homography", "fundamental", "affine" or "similarity" that a ransac_* wrapper
    estimates"""
    return "psx_ransac_" + model, {"homography": GUIDE_HOMOGRAPHY, "fundamental": GUIDE_EPIPOLAR, "affine": GUIDE_HOMOGRAPHY,
                                   "similarity": GUIDE_HOMOGRAPHY}[model]


def ransac_homography_ref(pairs, left_xy, right_xy, opts=None, capacity=None, layers=False, model="homography"):
    """psx_ransac_homography_ref: the whole rule on host arrays, no device.  pairs: PAIR_DTYPE / PAIR_U8_DTYPE records;
    left_xy / right_xy: (nl, 2) / (nr, 2) positions.  Returns a dict: result, count, inliers, and with layers the
    per-hypothesis models and counts."""
    L = lib()
    pairs, lx, rx = _pair_records(pairs), _xy(left_xy), _xy(right_xy)
    opts = opts or ransac_opts()
    ptr = lambda a: a.ctypes.data_as(C.c_void_p) if a.size else None
    name, kind = _ransac_names(model)
    return _ransac_call(getattr(L, name + "_ref"), name + "_ref", ptr(pairs), len(pairs), pairs.dtype, ptr(lx), len(lx),
                        ptr(rx), len(rx), opts, capacity, layers, kind=kind)


def ransac_homography(pairs, left_xy, right_xy, opts=None, device=0, capacity=None, layers=False, model="homography"):
    """psx_ransac_homography on host arrays (the positions go through device buffers): as ransac_homography_ref, on the
    device."""
    L = lib()
    pairs, lx, rx = _pair_records(pairs), _xy(left_xy), _xy(right_xy)
    opts = opts or ransac_opts()
    bufs = []
    try:
        plx, prx = _to_device(L, device, [lx, rx], bufs)
        name, kind = _ransac_names(model)
        fn = lambda *a: getattr(L, name)(device, *a)
        return _ransac_call(fn, name, pairs.ctypes.data_as(C.c_void_p) if pairs.size else None, len(pairs), pairs.dtype,
                            plx, len(lx), prx, len(rx), opts, capacity, layers, kind=kind)
    finally:
        for p in bufs:
            L.psx_dev_free(device, p)


def ransac_homography_dev(pairs_ptr, n, left_xy_ptr, l_len, right_xy_ptr, r_len, out_ptr, capacity, opts=None, device=0, layers=False,
                          model="homography"):
    """psx_ransac_homography_dev on DEVICE pointers: the records at pairs_ptr (e.g. what match_pairs_dev left) are read and
    the inlier records written in device memory (16-byte aligned, `capacity` records).  Returns a dict: result, count, and
    with layers the per-hypothesis models and counts."""
    L = lib()
    opts = opts or ransac_opts()
    vp = lambda p: C.c_void_p(p) if p else None
    name, kind = _ransac_names(model)
    fn = lambda *a: getattr(L, name + "_dev")(device, *a)
    return _ransac_call(fn, name + "_dev", vp(pairs_ptr), n, None, vp(left_xy_ptr), l_len, vp(right_xy_ptr), r_len, opts,
                        capacity, layers, out_ptr=out_ptr or 0, kind=kind)


def ransac_fundamental_ref(pairs, left_xy, right_xy, opts=None, capacity=None, layers=False):
    """psx_ransac_fundamental_ref: as ransac_homography_ref for a fundamental matrix (n >= 8 pairs); result.guide(tol) is an
    epipolar Guide"""
    return ransac_homography_ref(pairs, left_xy, right_xy, opts, capacity, layers, model="fundamental")


def ransac_fundamental(pairs, left_xy, right_xy, opts=None, device=0, capacity=None, layers=False):
    """psx_ransac_fundamental on host arrays: as ransac_fundamental_ref, on the device"""
    return ransac_homography(pairs, left_xy, right_xy, opts, device, capacity, layers, model="fundamental")


def ransac_fundamental_dev(pairs_ptr, n, left_xy_ptr, l_len, right_xy_ptr, r_len, out_ptr, capacity, opts=None, device=0, layers=False):
    """psx_ransac_fundamental_dev on DEVICE pointers: as ransac_homography_dev"""
    return ransac_homography_dev(pairs_ptr, n, left_xy_ptr, l_len, right_xy_ptr, r_len, out_ptr, capacity, opts, device, layers,
                                 model="fundamental")


def _ransac_many_call(fn, name, pairs_ptr, set_counts, dtype, plx, nl, right_ptrs, r_lens, opts, capacity, layers, out_ptr=None,
                      kind=GUIDE_HOMOGRAPHY):
    """One batched RANSAC call on K pair lists behind one another.  out_ptr None: the inliers come back in a host array.
    Returns a dict: results (K RansacResult), count (all inliers), and for the host forms records (the concatenated inlier
    records) and inliers (one array per set, cut by split_sets); with layers models (K, N, 9) and counts (K, N)."""
    k = len(set_counts)
    sc = np.ascontiguousarray(set_counts, dtype=np.int32)
    lens = np.ascontiguousarray(r_lens, dtype=np.int32)
    ptrs = (C.c_void_p * max(k, 1))(*[p.value if isinstance(p, C.c_void_p) else p for p in right_ptrs])
    n = int(sc.sum())
    cap = n if capacity is None else capacity
    N = max(int(opts.hypotheses), 0)
    res, cnt = (RansacResult * max(k, 1))(), C.c_int(-1)
    out = np.zeros((cap,), dtype) if out_ptr is None else None
    models = np.zeros((k, N, 9), np.float32) if layers else None
    counts = np.zeros((k, N), np.int32) if layers else None
    ptr = lambda a: a.ctypes.data_as(C.c_void_p) if a is not None and a.size else None
    po = ptr(out) if out_ptr is None else (C.c_void_p(out_ptr) if cap else None)
    rc = fn(pairs_ptr, ptr(sc), k, plx, nl, ptrs if k else None, ptr(lens), C.byref(opts), res if k else None, po, cap, C.byref(cnt),
            ptr(models), ptr(counts))
    if rc != 0:
        raise PopSiftError("%s failed (%d)" % (name, rc))
    results = []
    for i in range(k):
        r = RansacResult.from_buffer_copy(res[i])
        r.kind = kind
        results.append(r)
    got = dict(results=results, count=cnt.value)
    if out is not None:
        got["records"] = out[:min(cnt.value, cap)]
        got["inliers"] = split_sets(got["records"], [r.inliers for r in results])
    if layers:
        got["models"], got["counts"] = models, counts
    return got


def _pair_lists(pair_lists):
    """per-set record arrays -> (the concatenation, the counts)"""
    lists = [_pair_records(p) for p in pair_lists]
    dtype = lists[0].dtype if lists else PAIR_DTYPE
    return (np.concatenate(lists) if lists else np.zeros((0,), dtype)), [len(p) for p in lists]


def ransac_homography_many_ref(pair_lists, left_xy, right_xys, opts=None, capacity=None, layers=False, model="homography"):
    """psx_ransac_homography_many_ref: the loop over the single-list rule on host arrays, no device.  pair_lists: one
    PAIR_DTYPE / PAIR_U8_DTYPE array per set (what match_pairs_many_u8 returns), `right` indexing right_xys[k]; left_xy: one
    (nl, 2) array.  Returns the dict of _ransac_many_call."""
    L = lib()
    pairs, set_counts = _pair_lists(pair_lists)
    lx, rxs = _xy(left_xy), [_xy(r) for r in right_xys]
    opts = opts or ransac_opts()
    ptr = lambda a: a.ctypes.data_as(C.c_void_p) if a.size else None
    name, kind = _ransac_names(model)
    return _ransac_many_call(getattr(L, name + "_many_ref"), name + "_many_ref", ptr(pairs), set_counts, pairs.dtype, ptr(lx), len(lx),
                             [r.ctypes.data if r.size else None for r in rxs], [len(r) for r in rxs], opts, capacity, layers, kind=kind)


def ransac_homography_many(pair_lists, left_xy, right_xys, opts=None, device=0, capacity=None, layers=False, model="homography"):
    """psx_ransac_homography_many on host arrays (the positions go through device buffers): K pair lists verified in ONE
    call; set k's result and inliers equal ransac_homography(pair_lists[k], left_xy, right_xys[k], opts)."""
    L = lib()
    pairs, set_counts = _pair_lists(pair_lists)
    lx, rxs = _xy(left_xy), [_xy(r) for r in right_xys]
    opts = opts or ransac_opts()
    bufs = []
    try:
        ptrs = _to_device(L, device, [lx] + rxs, bufs)
        name, kind = _ransac_names(model)
        fn = lambda *a: getattr(L, name + "_many")(device, *a)
        return _ransac_many_call(fn, name + "_many", pairs.ctypes.data_as(C.c_void_p) if pairs.size else None, set_counts, pairs.dtype,
                                 ptrs[0], len(lx), ptrs[1:], [len(r) for r in rxs], opts, capacity, layers, kind=kind)
    finally:
        for p in bufs:
            L.psx_dev_free(device, p)


def ransac_homography_many_dev(pairs_ptr, set_counts, left_xy_ptr, l_len, right_xy_ptrs, r_lens, out_ptr, capacity, opts=None, device=0,
                               layers=False, model="homography"):
    """psx_ransac_homography_many_dev on DEVICE pointers: pairs_ptr and set_counts are what match_pairs_many_dev left and
    returned; the concatenated inlier records are written in device memory (16-byte aligned, `capacity` records).  Returns
    a dict: results, count, and with layers the per-set models and counts."""
    L = lib()
    opts = opts or ransac_opts()
    vp = lambda p: C.c_void_p(p) if p else None
    name, kind = _ransac_names(model)
    fn = lambda *a: getattr(L, name + "_many_dev")(device, *a)
    return _ransac_many_call(fn, name + "_many_dev", vp(pairs_ptr), set_counts, None, vp(left_xy_ptr), l_len, list(right_xy_ptrs), r_lens,
                             opts, capacity, layers, out_ptr=out_ptr or 0, kind=kind)


def ransac_fundamental_many_ref(pair_lists, left_xy, right_xys, opts=None, capacity=None, layers=False):
    """psx_ransac_fundamental_many_ref: as ransac_homography_many_ref for fundamental matrices"""
    return ransac_homography_many_ref(pair_lists, left_xy, right_xys, opts, capacity, layers, model="fundamental")


def ransac_fundamental_many(pair_lists, left_xy, right_xys, opts=None, device=0, capacity=None, layers=False):
    """psx_ransac_fundamental_many on host arrays: as ransac_homography_many; every result's guide is an epipolar one"""
    return ransac_homography_many(pair_lists, left_xy, right_xys, opts, device, capacity, layers, model="fundamental")


def ransac_fundamental_many_dev(pairs_ptr, set_counts, left_xy_ptr, l_len, right_xy_ptrs, r_lens, out_ptr, capacity, opts=None, device=0,
                                layers=False):
    """psx_ransac_fundamental_many_dev on DEVICE pointers: as ransac_homography_many_dev"""
    return ransac_homography_many_dev(pairs_ptr, set_counts, left_xy_ptr, l_len, right_xy_ptrs, r_lens, out_ptr, capacity, opts, device,
                                      layers, model="fundamental")


def ransac_affine_ref(pairs, left_xy, right_xy, opts=None, capacity=None, layers=False):
    """psx_ransac_affine_ref: as ransac_homography_ref for the affine model; result.guide(tol) is a homography Guide"""
    return ransac_homography_ref(pairs, left_xy, right_xy, opts, capacity, layers, model="affine")


def ransac_affine(pairs, left_xy, right_xy, opts=None, device=0, capacity=None, layers=False):
    """psx_ransac_affine on host arrays: as ransac_affine_ref, on the device"""
    return ransac_homography(pairs, left_xy, right_xy, opts, device, capacity, layers, model="affine")


def ransac_affine_dev(pairs_ptr, n, left_xy_ptr, l_len, right_xy_ptr, r_len, out_ptr, capacity, opts=None, device=0, layers=False):
    """psx_ransac_affine_dev on DEVICE pointers: as ransac_homography_dev"""
    return ransac_homography_dev(pairs_ptr, n, left_xy_ptr, l_len, right_xy_ptr, r_len, out_ptr, capacity, opts, device, layers,
                                 model="affine")


def ransac_affine_many_ref(pair_lists, left_xy, right_xys, opts=None, capacity=None, layers=False):
    """psx_ransac_affine_many_ref: as ransac_homography_many_ref for the affine model"""
    return ransac_homography_many_ref(pair_lists, left_xy, right_xys, opts, capacity, layers, model="affine")


def ransac_affine_many(pair_lists, left_xy, right_xys, opts=None, device=0, capacity=None, layers=False):
    """psx_ransac_affine_many on host arrays: as ransac_homography_many"""
    return ransac_homography_many(pair_lists, left_xy, right_xys, opts, device, capacity, layers, model="affine")


def ransac_affine_many_dev(pairs_ptr, set_counts, left_xy_ptr, l_len, right_xy_ptrs, r_lens, out_ptr, capacity, opts=None, device=0,
                          layers=False):
    """psx_ransac_affine_many_dev on DEVICE pointers: as ransac_homography_many_dev"""
    return ransac_homography_many_dev(pairs_ptr, set_counts, left_xy_ptr, l_len, right_xy_ptrs, r_lens, out_ptr, capacity, opts, device,
                                      layers, model="affine")


def ransac_similarity_ref(pairs, left_xy, right_xy, opts=None, capacity=None, layers=False):
    """psx_ransac_similarity_ref: as ransac_homography_ref for the similarity model; result.guide(tol) is a homography Guide"""
    return ransac_homography_ref(pairs, left_xy, right_xy, opts, capacity, layers, model="similarity")


def ransac_similarity(pairs, left_xy, right_xy, opts=None, device=0, capacity=None, layers=False):
    """psx_ransac_similarity on host arrays: as ransac_similarity_ref, on the device"""
    return ransac_homography(pairs, left_xy, right_xy, opts, device, capacity, layers, model="similarity")


def ransac_similarity_dev(pairs_ptr, n, left_xy_ptr, l_len, right_xy_ptr, r_len, out_ptr, capacity, opts=None, device=0, layers=False):
    """psx_ransac_similarity_dev on DEVICE pointers: as ransac_homography_dev"""
    return ransac_homography_dev(pairs_ptr, n, left_xy_ptr, l_len, right_xy_ptr, r_len, out_ptr, capacity, opts, device, layers,
                                 model="similarity")


def ransac_similarity_many_ref(pair_lists, left_xy, right_xys, opts=None, capacity=None, layers=False):
    """psx_ransac_similarity_many_ref: as ransac_homography_many_ref for the similarity model"""
    return ransac_homography_many_ref(pair_lists, left_xy, right_xys, opts, capacity, layers, model="similarity")


def ransac_similarity_many(pair_lists, left_xy, right_xys, opts=None, device=0, capacity=None, layers=False):
    """psx_ransac_similarity_many on host arrays: as ransac_homography_many"""
    return ransac_homography_many(pair_lists, left_xy, right_xys, opts, device, capacity, layers, model="similarity")


def ransac_similarity_many_dev(pairs_ptr, set_counts, left_xy_ptr, l_len, right_xy_ptrs, r_lens, out_ptr, capacity, opts=None, device=0,
                          layers=False):
    """psx_ransac_similarity_many_dev on DEVICE pointers: as ransac_homography_many_dev"""
    return ransac_homography_many_dev(pairs_ptr, set_counts, left_xy_ptr, l_len, right_xy_ptrs, r_lens, out_ptr, capacity, opts, device,
                                      layers, model="similarity")


def ransac_many_plan(set_counts, min_pairs, block_rows):
    """psx_ransac_many_plan: the (n, 3) int32 blocks = set, first, end of the concatenated list.  No device."""
    L = lib()
    sc = np.ascontiguousarray(set_counts, dtype=np.int32)
    nb = C.c_int(-1)
    args = (sc.ctypes.data_as(C.c_void_p) if len(sc) else None, len(sc), min_pairs, block_rows)
    rc = L.psx_ransac_many_plan(*args, None, 0, C.byref(nb))
    if rc != 0:
        raise PopSiftError("psx_ransac_many_plan failed (%d)" % rc)
    blocks = np.zeros((nb.value, 3), np.int32)
    rc = L.psx_ransac_many_plan(*args, blocks.ctypes.data_as(C.c_void_p) if nb.value else None, nb.value, C.byref(nb))
    if rc != 0:
        raise PopSiftError("psx_ransac_many_plan failed (%d)" % rc)
    return blocks


def _ransac_graph_call(fn, name, pairs_ptr, edge_counts, edges, dtype, xy_ptrs, lens, opts, capacity, layers, out_ptr=None,
                       kind=GUIDE_HOMOGRAPHY):
    """One RANSAC call over an edge list: E pair lists behind one another, edge e on the position arrays xy_ptrs[left_e] and
    xy_ptrs[right_e].  out_ptr None: the inliers come back in a host array.  Returns the dict of _ransac_many_call with one
    entry per EDGE: results, count, for the host forms records and inliers, with layers models (E, N, 9) and counts (E, N)."""
    ea = _graph_edges(edges)
    E, k = len(ea), len(lens)
    if len(edge_counts) != E:
        raise ValueError("one pair list per edge")
    ec = np.ascontiguousarray(edge_counts, dtype=np.int32)
    la = np.ascontiguousarray(lens, dtype=np.int32)
    ptrs = (C.c_void_p * max(k, 1))(*[p.value if isinstance(p, C.c_void_p) else p for p in xy_ptrs])
    n = int(ec.sum())
    cap = n if capacity is None else capacity
    N = max(int(opts.hypotheses), 0)
    res, cnt = (RansacResult * max(E, 1))(), C.c_int(-1)
    out = np.zeros((cap,), dtype) if out_ptr is None else None
    models = np.zeros((E, N, 9), np.float32) if layers else None
    counts = np.zeros((E, N), np.int32) if layers else None
    ptr = lambda a: a.ctypes.data_as(C.c_void_p) if a is not None and a.size else None
    po = ptr(out) if out_ptr is None else (C.c_void_p(out_ptr) if cap else None)
    rc = fn(pairs_ptr, ptr(ec), ptr(ea), E, ptrs if k else None, ptr(la), k, C.byref(opts), res if E else None, po, cap, C.byref(cnt),
            ptr(models), ptr(counts))
    if rc != 0:
        raise PopSiftError("%s failed (%d)" % (name, rc))
    results = []
    for i in range(E):
        r = RansacResult.from_buffer_copy(res[i])
        r.kind = kind
        results.append(r)
    got = dict(results=results, count=cnt.value)
    if out is not None:
        got["records"] = out[:min(cnt.value, cap)]
        got["inliers"] = split_sets(got["records"], [r.inliers for r in results])
    if layers:
        got["models"], got["counts"] = models, counts
    return got


def ransac_graph_ref(pair_lists, edges, xys, opts=None, capacity=None, layers=False, model="homography"):
    """psx_ransac_<model>_graph_ref: the loop over the single-list rule on host arrays, no device.  pair_lists: one
    PAIR_DTYPE / PAIR_U8_DTYPE array per EDGE (what match_pairs_graph_u8 returns); edges: (left, right) indices into xys,
    the views' (n_s, 2) position arrays.  Edge e's result equals ransac_<model>_ref(pair_lists[e], xys[left], xys[right])."""
    L = lib()
    pairs, edge_counts = _pair_lists(pair_lists)
    xs = [_xy(x) for x in xys]
    opts = opts or ransac_opts()
    name, kind = _ransac_names(model)
    return _ransac_graph_call(getattr(L, name + "_graph_ref"), name + "_graph_ref", pairs.ctypes.data_as(C.c_void_p) if pairs.size else None,
                              edge_counts, edges, pairs.dtype, [x.ctypes.data if x.size else None for x in xs], [len(x) for x in xs], opts,
                              capacity, layers, kind=kind)


def ransac_graph(pair_lists, edges, xys, opts=None, device=0, capacity=None, layers=False, model="homography"):
    """psx_ransac_<model>_graph on host arrays (the positions go through device buffers): the E pair lists of an edge list
    verified in ONE call; edge e's result and inliers equal ransac_<model>(pair_lists[e], xys[left], xys[right], opts)."""
    L = lib()
    pairs, edge_counts = _pair_lists(pair_lists)
    xs = [_xy(x) for x in xys]
    opts = opts or ransac_opts()
    bufs = []
    try:
        ptrs = _to_device(L, device, xs, bufs) if xs else []
        name, kind = _ransac_names(model)
        fn = lambda *a: getattr(L, name + "_graph")(device, *a)
        return _ransac_graph_call(fn, name + "_graph", pairs.ctypes.data_as(C.c_void_p) if pairs.size else None, edge_counts, edges, pairs.dtype,
                                  ptrs, [len(x) for x in xs], opts, capacity, layers, kind=kind)
    finally:
        for p in bufs:
            L.psx_dev_free(device, p)


def ransac_graph_dev(pairs_ptr, edge_counts, edges, xy_ptrs, lens, out_ptr, capacity, opts=None, device=0, layers=False, model="homography"):
    """psx_ransac_<model>_graph_dev on DEVICE pointers: pairs_ptr and edge_counts are what match_pairs_graph_dev left and
    returned, xy_ptrs / lens the views' position arrays; the concatenated inlier records are written in device memory
    (16-byte aligned, `capacity` records).  Returns a dict: results, count, and with layers the per-edge models and counts."""
    L = lib()
    opts = opts or ransac_opts()
    name, kind = _ransac_names(model)
    fn = lambda *a: getattr(L, name + "_graph_dev")(device, *a)
    return _ransac_graph_call(fn, name + "_graph_dev", C.c_void_p(pairs_ptr) if pairs_ptr else None, edge_counts, edges, None, list(xy_ptrs),
                              lens, opts, capacity, layers, out_ptr=out_ptr or 0, kind=kind)


def _ransac_graph_forms(model):
    """ransac_<model>_graph, _graph_dev and _graph_ref: the three functions above with the model fixed"""
    def host(pair_lists, edges, xys, opts=None, device=0, capacity=None, layers=False):
        return ransac_graph(pair_lists, edges, xys, opts, device, capacity, layers, model=model)

    def dev(pairs_ptr, edge_counts, edges, xy_ptrs, lens, out_ptr, capacity, opts=None, device=0, layers=False):
        return ransac_graph_dev(pairs_ptr, edge_counts, edges, xy_ptrs, lens, out_ptr, capacity, opts, device, layers, model=model)

    def ref(pair_lists, edges, xys, opts=None, capacity=None, layers=False):
        return ransac_graph_ref(pair_lists, edges, xys, opts, capacity, layers, model=model)

    for f, suffix, base in ((host, "_graph", ransac_graph), (dev, "_graph_dev", ransac_graph_dev), (ref, "_graph_ref", ransac_graph_ref)):
        f.__name__ = f.__qualname__ = "ransac_%s%s" % (model, suffix)
        f.__doc__ = "psx_ransac_%s%s: %s(..., model=%r)" % (model, suffix, base.__name__, model)
        globals()[f.__name__] = f


for _m in RANSAC_MODELS:
    _ransac_graph_forms(_m)


def track_opts(min_views=2, keep_conflicts=False):
    return TrackOpts(int(min_views), TRACKS_KEEP_CONFLICTS if keep_conflicts else 0)


def _tracks_call(fn, name, pairs_ptr, edge_counts, edges, lens, opts, labels_ptr, starts_ptr, track_capacity, members_ptr, member_capacity):
    """One tracks call on raw pointers (host or device alike): the TracksInfo"""
    ea = _graph_edges(edges)
    E, k = len(ea), len(lens)
    if len(edge_counts) != E:
        raise ValueError("one record list per edge")
    ec = np.ascontiguousarray(edge_counts, dtype=np.int32)
    la = np.ascontiguousarray(lens, dtype=np.int32)
    info = TracksInfo()
    ptr = lambda a: a.ctypes.data_as(C.c_void_p) if a.size else None
    rc = fn(pairs_ptr, ptr(ec), ptr(ea), E, ptr(la), k, C.byref(opts), labels_ptr, starts_ptr, track_capacity, members_ptr, member_capacity,
            C.byref(info))
    if rc != 0:
        raise PopSiftError("%s failed (%d)" % (name, rc))
    return info


def _tracks_host(fn, name, pair_lists, edges, lens, opts, labels, track_capacity, member_capacity):
    """a host form: asks "how many?" unless both capacities are given, then fills arrays of that size"""
    pairs, edge_counts = _pair_lists(pair_lists)
    opts = opts or track_opts()
    pp = pairs.ctypes.data_as(C.c_void_p) if pairs.size else None
    if track_capacity is None or member_capacity is None:
        how = _tracks_call(fn, name, pp, edge_counts, edges, lens, opts, None, None, 0, None, 0)
        track_capacity = how.tracks if track_capacity is None else track_capacity
        member_capacity = how.members if member_capacity is None else member_capacity
    M = int(np.sum(np.asarray(lens, np.int64))) if len(lens) else 0
    lab = np.zeros((M,), np.int32) if labels else None
    starts = np.zeros((track_capacity + 1,), np.int32)
    mem = np.zeros((member_capacity,), TRACK_MEMBER_DTYPE)
    vp = lambda a: a.ctypes.data_as(C.c_void_p) if a is not None and a.size else None
    info = _tracks_call(fn, name, pp, edge_counts, edges, lens, opts, vp(lab), vp(starts), track_capacity, vp(mem), member_capacity)
    got = {n: int(getattr(info, n)) for n, _ in TracksInfo._fields_}
    got["starts"] = starts[:min(info.tracks, track_capacity) + 1]
    got["member_records"] = mem[:min(info.members, member_capacity)]
    if labels:
        got["labels"] = lab
    return got


def tracks_graph_ref(pair_lists, edges, lens, opts=None, labels=True, track_capacity=None, member_capacity=None):
    """psx_tracks_graph_ref: the sequential union-find on host arrays, no device.  pair_lists: one 16-byte record array per
    EDGE (what match_pairs_graph_u8, ransac_*_graph["inliers"] or match_pairs_guided_graph_u8 return); edges: (left, right)
    indices into lens, the views' row counts.  Returns a dict: the six totals of TracksInfo by name, starts (CSR, tracks + 1
    ints), member_records (TRACK_MEMBER_DTYPE; track t owns [starts[t], starts[t + 1])) and labels (sum(lens) ints, -1: in no
    track)."""
    L = lib()
    return _tracks_host(L.psx_tracks_graph_ref, "psx_tracks_graph_ref", pair_lists, edges, lens, opts, labels, track_capacity, member_capacity)


def tracks_graph(pair_lists, edges, lens, opts=None, device=0, labels=True, track_capacity=None, member_capacity=None):
    """psx_tracks_graph on host arrays: the tracks of the E record lists of an edge list in ONE device call; the dict of
    tracks_graph_ref, bit for bit."""
    L = lib()
    fn = lambda *a: L.psx_tracks_graph(device, *a)
    return _tracks_host(fn, "psx_tracks_graph", pair_lists, edges, lens, opts, labels, track_capacity, member_capacity)


def tracks_graph_dev(pairs_ptr, edge_counts, edges, lens, labels_ptr, starts_ptr, track_capacity, members_ptr, member_capacity, opts=None, device=0):
    """psx_tracks_graph_dev on DEVICE pointers: pairs_ptr and edge_counts are what match_pairs_graph_dev, ransac_*_graph_dev
    (counts: [r.inliers for r in results]) or match_pairs_guided_graph_dev left; labels (sum(lens) ints), track starts
    (track_capacity + 1 ints) and members (member_capacity 8-byte records) are written in device memory, any of them 0 /
    None with capacity 0.  Returns the totals as a dict."""
    L = lib()
    fn = lambda *a: L.psx_tracks_graph_dev(device, *a)
    vp = lambda p: C.c_void_p(p) if p else None
    info = _tracks_call(fn, "psx_tracks_graph_dev", vp(pairs_ptr), edge_counts, edges, lens, opts or track_opts(), vp(labels_ptr), vp(starts_ptr),
                        track_capacity, vp(members_ptr), member_capacity)
    return {n: int(getattr(info, n)) for n, _ in TracksInfo._fields_}


def tracks_plan(lens, edge_counts):
    """psx_tracks_plan: what psx_tracks_graph plans for these sizes, as a dict (nodes, records, record_blocks, sort_bits,
    launches, scratch_bytes).  No device."""
    la = np.ascontiguousarray(lens, dtype=np.int32)
    ec = np.ascontiguousarray(edge_counts, dtype=np.int32)
    out = TracksPlanInfo()
    rc = lib().psx_tracks_plan(la.ctypes.data_as(C.c_void_p) if len(la) else None, len(la), ec.ctypes.data_as(C.c_void_p) if len(ec) else None,
                               len(ec), C.byref(out))
    if rc != 0:
        raise PopSiftError("psx_tracks_plan failed (%d)" % rc)
    return {n: int(getattr(out, n)) for n, _ in TracksPlanInfo._fields_}


def _set_table(ptrs, lens):
    """(pointer array or None, lens array, lens pointer or None, n) of a list of sets given as addresses"""
    k = len(lens)
    val = lambda p: p.value if isinstance(p, C.c_void_p) else p
    arr = (C.c_void_p * max(k, 1))(*[val(p) for p in ptrs])
    la = np.ascontiguousarray(lens, dtype=np.int32)
    return (arr if k else None), la, (la.ctypes.data_as(C.c_void_p) if k else None), k


def _host_sets(sets):
    sets = [np.ascontiguousarray(s, dtype=np.uint8).reshape(-1, 128) for s in sets]
    return sets, [s.ctypes.data for s in sets], [len(s) for s in sets]


def _vocab_info(info):
    return {n: int(getattr(info, n)) for n, _ in VocabInfo._fields_ if n != "reserved"}


def _vocab_train(fn, name, ptrs, lens, words, iterations, vocab_ptr):
    arr, la, lp, k = _set_table(ptrs, lens)
    o, info = VocabOpts(int(words), int(iterations)), VocabInfo()
    rc = fn(arr, lp, k, C.byref(o), vocab_ptr, C.byref(info))
    if rc != 0:
        raise PopSiftError("%s failed (%d)" % (name, rc))
    return _vocab_info(info)


def vocab_train_u8_ref(sets, words, iterations):
    """psx_vocab_train_u8_ref: the sequential integer k-means on host arrays, no device.  sets: (n_v,128) uint8 arrays.
    Returns (vocabulary (words,128) uint8, dict iterations / changed / empty_words / inertia)."""
    sets, ptrs, lens = _host_sets(sets)
    vocab = np.zeros((max(int(words), 0), 128), np.uint8)
    info = _vocab_train(lib().psx_vocab_train_u8_ref, "psx_vocab_train_u8_ref", ptrs, lens, words, iterations, vocab.ctypes.data_as(C.c_void_p))
    return vocab, info


def vocab_train_u8(sets, words, iterations, device=0):
    """psx_vocab_train_u8 on host arrays (the sets go through device buffers): what vocab_train_u8_ref returns, bit for bit"""
    L = lib()
    sets, _, lens = _host_sets(sets)
    vocab = np.zeros((max(int(words), 0), 128), np.uint8)
    bufs = []
    try:
        ptrs = _to_device(L, device, sets, bufs) if sets else []
        fn = lambda *a: L.psx_vocab_train_u8(device, *a)
        return vocab, _vocab_train(fn, "psx_vocab_train_u8", ptrs, lens, words, iterations, vocab.ctypes.data_as(C.c_void_p))
    finally:
        for p in bufs:
            L.psx_dev_free(device, p)


def vocab_train_u8_dev(ptrs, lens, words, iterations, vocab_ptr, device=0):
    """psx_vocab_train_u8_dev on DEVICE pointers: the vocabulary (words x 128 bytes, 16-byte aligned) is written in device
    memory; returns the info dict"""
    L = lib()
    fn = lambda *a: L.psx_vocab_train_u8_dev(device, *a)
    return _vocab_train(fn, "psx_vocab_train_u8_dev", list(ptrs), lens, words, iterations, C.c_void_p(vocab_ptr) if vocab_ptr else None)


def _bow(fn, name, vocab_ptr, words, ptrs, lens, hist_ptr, words_ptr):
    arr, la, lp, k = _set_table(ptrs, lens)
    rc = fn(vocab_ptr, int(words), arr, lp, k, hist_ptr, words_ptr)
    if rc != 0:
        raise PopSiftError("%s failed (%d)" % (name, rc))


def _bow_host(fn, name, vocab, ptrs, lens, row_words):
    vocab = np.ascontiguousarray(vocab, dtype=np.uint8).reshape(-1, 128)
    hist = np.zeros((len(lens), len(vocab)), np.uint32)
    rw = np.zeros((int(sum(lens)),), np.int32) if row_words else None
    vp = lambda a: a.ctypes.data_as(C.c_void_p) if a is not None and a.size else None
    _bow(fn, name, vocab.ctypes.data_as(C.c_void_p), len(vocab), ptrs, lens, vp(hist), vp(rw))
    return (hist, rw) if row_words else hist


def bow_u8_ref(vocab, sets, row_words=False):
    """psx_bow_u8_ref: the bags of words of N views on host arrays, no device.  Returns hist (N, words) uint32; with row_words
    also the word of every row (sum of the lengths, int32)."""
    sets, ptrs, lens = _host_sets(sets)
    return _bow_host(lib().psx_bow_u8_ref, "psx_bow_u8_ref", vocab, ptrs, lens, row_words)


def bow_u8(vocab, sets, device=0, row_words=False):
    """psx_bow_u8 on host arrays (the sets go through device buffers): what bow_u8_ref returns, bit for bit, in ONE call"""
    L = lib()
    sets, _, lens = _host_sets(sets)
    bufs = []
    try:
        ptrs = _to_device(L, device, sets, bufs) if sets else []
        fn = lambda *a: L.psx_bow_u8(device, *a)
        return _bow_host(fn, "psx_bow_u8", vocab, ptrs, lens, row_words)
    finally:
        for p in bufs:
            L.psx_dev_free(device, p)


def bow_u8_dev(vocab_ptr, words, ptrs, lens, hist_ptr, words_ptr=0, device=0):
    """psx_bow_u8_dev on DEVICE pointers: the vocabulary is read and hist (N x words uint32) and, unless 0, the rows' words
    (int32) are written in device memory"""
    L = lib()
    vp = lambda p: C.c_void_p(p) if p else None
    fn = lambda *a: L.psx_bow_u8_dev(device, *a)
    _bow(fn, "psx_bow_u8_dev", vp(vocab_ptr), words, list(ptrs), lens, vp(hist_ptr), vp(words_ptr))


def shortlist_opts(k, mutual=False):
    return ShortlistOpts(int(k), SHORTLIST_MUTUAL if mutual else 0)


def _shortlist_call(fn, name, hist_ptr, n_views, words, opts, nb_ptr, sc_ptr, edges_ptr, capacity):
    n = C.c_int(-1)
    rc = fn(hist_ptr, n_views, words, C.byref(opts), nb_ptr, sc_ptr, edges_ptr, capacity, C.byref(n))
    if rc != 0:
        raise PopSiftError("%s failed (%d)" % (name, rc))
    return n.value


def _shortlist_host(fn, name, hist, k, mutual, capacity):
    """a host form: asks "how many?" unless the capacity is given, then fills arrays of that size"""
    hist = np.ascontiguousarray(hist, dtype=np.uint32)
    if hist.ndim != 2:
        raise ValueError("hist is an (n_views, words) array")
    N, W = hist.shape
    o = shortlist_opts(k, mutual)
    hp = hist.ctypes.data_as(C.c_void_p) if hist.size else None
    if capacity is None:
        capacity = _shortlist_call(fn, name, hp, N, W, o, None, None, None, 0)
    nb = np.zeros((N, int(k)), np.int32)
    sc = np.zeros((N, int(k)), np.uint32)
    ed = np.zeros((capacity,), VIEW_EDGE_DTYPE)
    vp = lambda a: a.ctypes.data_as(C.c_void_p) if a.size else None
    n = _shortlist_call(fn, name, hp, N, W, o, vp(nb), vp(sc), vp(ed), capacity)
    return {"neighbours": nb, "scores": sc, "edges": ed[:min(n, capacity)], "count": n}


def shortlist_views_ref(hist, k, mutual=False, capacity=None):
    """psx_shortlist_views_ref on a host (n_views, words) uint32 histogram, no device.  Returns a dict: neighbours and scores
    ((n_views, k), unused entries -1 and 0), edges (VIEW_EDGE_DTYPE, sorted by (left, right), each pair once; .tolist() is the
    edge list the graph calls take) and count, the total whatever the capacity."""
    return _shortlist_host(lib().psx_shortlist_views_ref, "psx_shortlist_views_ref", hist, k, mutual, capacity)


def shortlist_views(hist, k, mutual=False, device=0, capacity=None):
    """psx_shortlist_views on a host histogram: the dict of shortlist_views_ref, bit for bit"""
    L = lib()
    fn = lambda *a: L.psx_shortlist_views(device, *a)
    return _shortlist_host(fn, "psx_shortlist_views", hist, k, mutual, capacity)


def shortlist_views_dev(hist_ptr, n_views, words, k, nb_ptr, sc_ptr, edges_ptr, capacity, mutual=False, device=0):
    """psx_shortlist_views_dev on DEVICE pointers (what bow_u8_dev left at hist_ptr): neighbours and scores (n_views x k
    each, either 0 / None) and the first `capacity` edges are written in device memory; returns the total edge count"""
    L = lib()
    vp = lambda p: C.c_void_p(p) if p else None
    fn = lambda *a: L.psx_shortlist_views_dev(device, *a)
    return _shortlist_call(fn, "psx_shortlist_views_dev", vp(hist_ptr), n_views, words, shortlist_opts(k, mutual), vp(nb_ptr), vp(sc_ptr),
                           vp(edges_ptr), capacity)


def bow_weights(df, n_views):
    """psx_bow_weights: the idf weight of every word from its document frequency, int32; host only"""
    df = np.ascontiguousarray(df, dtype=np.int32).reshape(-1)
    out = np.zeros_like(df)
    rc = lib().psx_bow_weights(df.ctypes.data_as(C.c_void_p) if df.size else None, len(df), int(n_views),
                               out.ctypes.data_as(C.c_void_p) if df.size else None)
    if rc != 0:
        raise PopSiftError("psx_bow_weights failed (%d)" % rc)
    return out


def bow_quantize_ref(hist, df_accum=None):
    """psx_bow_quantize_ref: q (n_views, words) uint16 of a host (n_views, words) uint32 histogram, every row by its own sum;
    df_accum (words int32, or None) is added to IN PLACE"""
    hist = np.ascontiguousarray(hist, dtype=np.uint32)
    if hist.ndim != 2:
        raise ValueError("hist is an (n_views, words) array")
    q = np.zeros(hist.shape, np.uint16)
    vp = lambda a: a.ctypes.data_as(C.c_void_p) if a is not None and a.size else None
    rc = lib().psx_bow_quantize_ref(vp(hist), hist.shape[0], hist.shape[1], vp(q), _df_accum(df_accum, hist.shape[1]))
    if rc != 0:
        raise PopSiftError("psx_bow_quantize_ref failed (%d)" % rc)
    return q


def _df_accum(df_accum, words):
    if df_accum is None:
        return None
    if not (isinstance(df_accum, np.ndarray) and df_accum.dtype == np.int32 and df_accum.flags.c_contiguous and df_accum.size == words):
        raise ValueError("df_accum is a contiguous int32 array of `words` entries")
    return df_accum.ctypes.data_as(C.c_void_p)


def bow_quantize_dev(hist_ptr, n_views, words, q_ptr, df_accum=None, device=0):
    """psx_bow_quantize_dev on DEVICE pointers: hist (n_views x words uint32) is read, q (uint16) written -- at the end of a
    database's rows to grow it; df_accum (HOST int32 array of `words` entries, or None) is added to in place"""
    vp = lambda p: C.c_void_p(p) if p else None
    rc = lib().psx_bow_quantize_dev(device, vp(hist_ptr), int(n_views), int(words), vp(q_ptr), _df_accum(df_accum, words))
    if rc != 0:
        raise PopSiftError("psx_bow_quantize_dev failed (%d)" % rc)


def query_opts(k, self_base=-1, edge_base=0, min_score=0):
    return QueryOpts(int(k), 0, int(self_base), int(edge_base), int(min_score), 0)


def _query_tables(weights, db_limit, n_queries):
    w = np.ascontiguousarray(weights, dtype=np.int32).reshape(-1)
    lim = None if db_limit is None else np.ascontiguousarray(db_limit, dtype=np.int32).reshape(-1)
    if lim is not None and len(lim) != n_queries:
        raise ValueError("db_limit has one entry per query")
    return w, lim


def _query_call(fn, name, db_ptr, n_db, q_ptr, n_queries, words, weights, db_limit, opts, nb_ptr, sc_ptr, edges_ptr, capacity):
    """one query call on prepared pointers: the total edge count"""
    w, lim = _query_tables(weights, db_limit, n_queries)
    if len(w) != words:
        raise ValueError("one weight per word")
    n = C.c_int(-1)
    rc = fn(db_ptr, int(n_db), q_ptr, int(n_queries), int(words), w.ctypes.data_as(C.c_void_p),
            lim.ctypes.data_as(C.c_void_p) if lim is not None and lim.size else None, C.byref(opts), nb_ptr, sc_ptr, edges_ptr, int(capacity),
            C.byref(n))
    if rc != 0:
        raise PopSiftError("%s failed (%d)" % (name, rc))
    return n.value


def _query_host(fn, name, db_ptr, n_db, q_ptr, n_queries, words, weights, db_limit, opts, capacity):
    """a form with host outputs: asks "how many?" unless the capacity is given, then fills arrays of that size"""
    if capacity is None:
        capacity = _query_call(fn, name, db_ptr, n_db, q_ptr, n_queries, words, weights, db_limit, opts, None, None, None, 0)
    nb = np.zeros((n_queries, opts.k), np.int32)
    sc = np.zeros((n_queries, opts.k), np.uint32)
    ed = np.zeros((capacity,), VIEW_EDGE_DTYPE)
    vp = lambda a: a.ctypes.data_as(C.c_void_p) if a.size else None
    n = _query_call(fn, name, db_ptr, n_db, q_ptr, n_queries, words, weights, db_limit, opts, vp(nb), vp(sc), vp(ed), capacity)
    return {"neighbours": nb, "scores": sc, "edges": ed[:min(n, capacity)], "count": n}


def shortlist_query_ref(db_q, query_q, weights, k, db_limit=None, self_base=-1, edge_base=0, min_score=0, capacity=None):
    """psx_shortlist_query_ref on host (n, words) uint16 arrays, no device.  Returns a dict: neighbours and scores ((n_queries,
    k), unused entries -1 and 0), edges (VIEW_EDGE_DTYPE: {edge_base + i, neighbour}, grouped by left in list order) and count,
    the total whatever the capacity."""
    db_q, query_q = np.ascontiguousarray(db_q, dtype=np.uint16), np.ascontiguousarray(query_q, dtype=np.uint16)
    if db_q.ndim != 2 or query_q.ndim != 2 or db_q.shape[1] != query_q.shape[1]:
        raise ValueError("db_q and query_q are (n, words) arrays of one width")
    vp = lambda a: a.ctypes.data_as(C.c_void_p) if a.size else None
    return _query_host(lib().psx_shortlist_query_ref, "psx_shortlist_query_ref", vp(db_q), len(db_q), vp(query_q), len(query_q), db_q.shape[1],
                       weights, db_limit, query_opts(k, self_base, edge_base, min_score), capacity)


def shortlist_query(db_ptr, n_db, query_ptr, n_queries, words, weights, k, db_limit=None, self_base=-1, edge_base=0, min_score=0,
                    device=0, capacity=None):
    """psx_shortlist_query: the q arrays are DEVICE pointers, the dict of shortlist_query_ref comes back in host arrays"""
    L = lib()
    vp = lambda p: C.c_void_p(p) if p else None
    fn = lambda *a: L.psx_shortlist_query(device, *a)
    return _query_host(fn, "psx_shortlist_query", vp(db_ptr), n_db, vp(query_ptr), n_queries, words, weights, db_limit,
                       query_opts(k, self_base, edge_base, min_score), capacity)


def shortlist_query_dev(db_ptr, n_db, query_ptr, n_queries, words, weights, k, nb_ptr, sc_ptr, edges_ptr, capacity, db_limit=None,
                        self_base=-1, edge_base=0, min_score=0, device=0):
    """psx_shortlist_query_dev on DEVICE pointers: neighbours and scores (n_queries x k each, either 0 / None) and the first
    `capacity` edges are written in device memory; returns the total edge count"""
    L = lib()
    vp = lambda p: C.c_void_p(p) if p else None
    fn = lambda *a: L.psx_shortlist_query_dev(device, *a)
    return _query_call(fn, "psx_shortlist_query_dev", vp(db_ptr), n_db, vp(query_ptr), n_queries, words, weights, db_limit,
                       query_opts(k, self_base, edge_base, min_score), vp(nb_ptr), vp(sc_ptr), vp(edges_ptr), capacity)


def shortlist_query_plan(n_db, n_queries, words, k):
    """psx_shortlist_query_plan: dict blocks / keys_per_block / partial_keys / scratch_bytes of a query of these sizes; host only"""
    out = QueryPlan()
    rc = lib().psx_shortlist_query_plan(int(n_db), int(n_queries), int(words), int(k), C.byref(out))
    if rc != 0:
        raise PopSiftError("psx_shortlist_query_plan failed (%d)" % rc)
    return {n: int(getattr(out, n)) for n, _ in QueryPlan._fields_}


def _guided_graph_call(fn, name, device, set_ptrs, xy_ptrs, lens, edges, guides, out_ptr, capacity, ratio, mutual):
    """One guided edge-list call on device pointers: (per-edge counts (n_edges,) int32, total count)"""
    k = len(lens)
    ea = _graph_edges(edges)
    if not (len(set_ptrs) == len(xy_ptrs) == k) or len(guides) != len(ea):
        raise ValueError("one descriptor pointer and one position pointer per set, one guide per edge")
    val = lambda p: p.value if isinstance(p, C.c_void_p) else p
    ptrs = (C.c_void_p * max(k, 1))(*[val(p) for p in set_ptrs])
    xptrs = (C.c_void_p * max(k, 1))(*[val(p) for p in xy_ptrs])
    la = np.ascontiguousarray(lens, dtype=np.int32)
    garr = _guide_array(guides)
    counts = np.full((len(ea),), -1, np.int32)
    n = C.c_int(-1)
    o = match_opts(ratio, mutual)
    E = len(ea)
    rc = fn(device, ptrs if k else None, xptrs if k else None, la.ctypes.data_as(C.c_void_p) if k else None, k,
            ea.ctypes.data_as(C.c_void_p) if E else None, E, garr if E else None, C.byref(o), out_ptr, capacity,
            counts.ctypes.data_as(C.c_void_p) if E else None, C.byref(n))
    if rc != 0:
        raise PopSiftError("%s failed (%d)" % (name, rc))
    return counts, n.value


def match_pairs_guided_graph(sets, xys, edges, guides, ratio=0.8, mutual=False, device=0, capacity=None):
    """psx_match_pairs_guided_graph on host arrays, the float form of match_pairs_guided_graph_u8: (n_s,128) float32 sets,
    per-edge PAIR_DTYPE arrays -- edge e's equals match_pairs_guided(sets[left], xys[left], sets[right], xys[right],
    guides[e])."""
    return _match_pairs_guided_graph("psx_match_pairs_guided_graph", np.float32, PAIR_DTYPE, sets, xys, edges, guides, ratio, mutual, device,
                                     capacity)


def match_pairs_guided_graph_u8(sets, xys, edges, guides, ratio=0.8, mutual=False, device=0, capacity=None):
    """psx_match_pairs_guided_graph_u8 on host arrays: `sets` are (n_s,128) uint8 arrays with positions xys[s] (n_s,2),
    `edges` (left, right) index pairs into them, edge e re-matched under guides[e], all in ONE call.  A guide of kind
    GUIDE_NONE (Guide.none(), or None) skips its edge.  Returns (list of per-edge PAIR_U8_DTYPE arrays -- edge e's equals
    match_pairs_guided_u8(sets[left], xys[left], sets[right], xys[right], guides[e]) --, per-edge counts); with a capacity the
    list holds the first `capacity` records of the concatenation and the counts are still the totals."""
    return _match_pairs_guided_graph("psx_match_pairs_guided_graph_u8", np.uint8, PAIR_U8_DTYPE, sets, xys, edges, guides, ratio, mutual,
                                     device, capacity)


def _match_pairs_guided_graph(name, dtype, pair_dtype, sets, xys, edges, guides, ratio, mutual, device, capacity):
    L = lib()
    if len(sets) != len(xys):
        raise ValueError("one position array per descriptor set")
    empty, empty_xy = np.zeros((0, 128), dtype), np.zeros((0, 2), np.float32)
    sides = [_guided_sides(s, x, empty, empty_xy, dtype)[:2] for s, x in zip(sets, xys)]
    ea = _graph_edges(edges)
    bufs = []
    try:
        k = len(sides)
        ptrs = _to_device(L, device, [s[0] for s in sides] + [s[1] for s in sides], bufs) if k else []
        lens = [len(s[0]) for s in sides]
        ok = all(0 <= a < k and 0 <= b < k for a, b in ea)
        cap = (sum(lens[a] for a, _ in ea) if ok else 0) if capacity is None else capacity
        out = np.zeros((cap,), pair_dtype)
        counts, n = _guided_graph_call(getattr(L, name), name, device, ptrs[:k], ptrs[k:], lens, ea,
                                       guides, out.ctypes.data_as(C.c_void_p) if cap else None, cap, ratio, mutual)
        return split_sets(out[:min(n, cap)], counts), counts
    finally:
        for p in bufs:
            L.psx_dev_free(device, p)


def match_pairs_guided_graph_dev(set_ptrs, xy_ptrs, lens, edges, guides, out_ptr, capacity, ratio=0.8, mutual=False, device=0, u8=True):
    """psx_match_pairs_guided_graph_u8_dev (u8=False: psx_match_pairs_guided_graph_dev, float descriptors) on DEVICE
    pointers (e.g. tensor.data_ptr()): the concatenated records go into the caller's device buffer at out_ptr (16-byte
    aligned, `capacity` records); returns (per-edge counts, total count)."""
    name = "psx_match_pairs_guided_graph_u8_dev" if u8 else "psx_match_pairs_guided_graph_dev"
    return _guided_graph_call(getattr(lib(), name), name, device, list(set_ptrs),
                              list(xy_ptrs), lens, edges, guides, C.c_void_p(out_ptr), capacity, ratio, mutual)


# psx_step kinds and the schedules of psx_pyramid_plan
STEP_BLUR, STEP_BLUR2, STEP_TILE, STEP_FLOW, STEP_SCAN, STEP_SCAN_SET = 1, 2, 3, 4, 5, 6
PLAN_DIAGONAL, PLAN_TILE, PLAN_FLOW = 0, 1, 2
EXT_BATCH = 4                    # PSX_EXT_BATCH: octaves per batched extrema scan


def pyramid_plan(w0, h0, num_octaves, levels, spans, resident_blocks=1024, schedule=PLAN_DIAGONAL, first=0):
    """psx_pyramid_plan: the (n, 6) int32 steps = kind, n, a, b, c, d a context of this size issues per frame behind the
    level-0 launch.  No device.  None where the tile schedule is asked for and none exists."""
    L = lib()
    sp = np.ascontiguousarray(spans, dtype=np.int32)
    args = (w0, h0, num_octaves, levels, sp.ctypes.data_as(C.c_void_p), resident_blocks, schedule, first)
    n = C.c_int(-1)
    rc = L.psx_pyramid_plan(*args, None, 0, C.byref(n))
    if rc == -4 and schedule == PLAN_TILE:
        return None
    if rc != 0:
        raise PopSiftError("psx_pyramid_plan failed (%d)" % rc)
    steps = np.zeros((n.value, 6), np.int32)
    rc = L.psx_pyramid_plan(*args, steps.ctypes.data_as(C.c_void_p) if n.value else None, n.value, C.byref(n))
    if rc != 0:
        raise PopSiftError("psx_pyramid_plan failed (%d)" % rc)
    return steps


def blur_grid(w, h, span):
    """psx_blur_grid_of: workgroups of a plane-to-plane blur of a w x h plane at this span.  No device."""
    n = lib().psx_blur_grid_of(w, h, span)
    if n < 0:
        raise PopSiftError("psx_blur_grid_of failed (%d)" % n)
    return n


class DeviceDescriptors:
    """Descriptor sets resident on the device (what FeaturesDev holds, popsift.cpp:346-383): upload once, match many times."""

    def __init__(self, arr, device=0, xy=None):
        """xy: None, or one (x, y) position per descriptor in input-image units (needed by match_pairs_guided)"""
        L = lib()
        L.psx_dev_alloc.argtypes = [C.c_int, C.c_size_t, C.POINTER(C.c_void_p)]
        L.psx_dev_free.argtypes = [C.c_int, C.c_void_p]
        L.psx_dev_write.argtypes = [C.c_int, C.c_void_p, C.c_void_p, C.c_size_t]
        arr = np.ascontiguousarray(arr, dtype=np.float32).reshape(-1, 128)
        self.n, self.device, self.ptr, self.xy_ptr = len(arr), device, C.c_void_p(), C.c_void_p()
        if self.n:
            if L.psx_dev_alloc(device, arr.nbytes, C.byref(self.ptr)) != 0:
                raise PopSiftError("psx_dev_alloc failed")
            if L.psx_dev_write(device, self.ptr, arr.ctypes.data_as(C.c_void_p), arr.nbytes) != 0:
                raise PopSiftError("psx_dev_write failed")
        if xy is not None:
            xy = _xy(xy)
            if len(xy) != self.n:
                raise ValueError("one position per descriptor")
            if self.n:
                if L.psx_dev_alloc(device, xy.nbytes, C.byref(self.xy_ptr)) != 0:
                    raise PopSiftError("psx_dev_alloc failed")
                if L.psx_dev_write(device, self.xy_ptr, xy.ctypes.data_as(C.c_void_p), xy.nbytes) != 0:
                    raise PopSiftError("psx_dev_write failed")

    def match(self, right):
        """psx_match(self as left, right: DeviceDescriptors): (n,3) int32 and (n,2) float32 host arrays"""
        L = lib()
        L.psx_match.argtypes = [C.c_int, C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p]
        mm = np.zeros((self.n, 3), np.int32)
        dd = np.zeros((self.n, 2), np.float32)
        rc = L.psx_match(self.device, self.ptr, self.n, right.ptr, right.n, mm.ctypes.data_as(C.c_void_p), dd.ctypes.data_as(C.c_void_p))
        if rc != 0:
            raise PopSiftError("psx_match failed (%d)" % rc)
        return mm, dd

    def match_pairs(self, right, ratio=0.8, mutual=False, capacity=None):
        """psx_match_pairs(self as left, right: DeviceDescriptors): PAIR_DTYPE records; with a capacity (records, count)"""
        got = _pairs_call(lib().psx_match_pairs, "psx_match_pairs", self.device, self.ptr, self.n, right.ptr, right.n,
                          ratio, mutual, PAIR_DTYPE, capacity)
        return got[0] if capacity is None else got

    def match_pairs_guided(self, right, guide, ratio=0.8, mutual=False, capacity=None):
        """psx_match_pairs_guided(self as left, right: DeviceDescriptors, both built with positions): PAIR_DTYPE records;
        with a capacity (records, count)"""
        if (self.n and not self.xy_ptr) or (right.n and not right.xy_ptr):
            raise ValueError("both sides need positions (DeviceDescriptors(arr, xy=...))")
        fn = _guided_fn(lib().psx_match_pairs_guided, self.xy_ptr, right.xy_ptr, guide)
        got = _pairs_call(fn, "psx_match_pairs_guided", self.device, self.ptr, self.n, right.ptr, right.n, ratio, mutual, PAIR_DTYPE, capacity)
        return got[0] if capacity is None else got

    def ransac_homography(self, right, pairs, opts=None, capacity=None, layers=False, model="homography"):
        """psx_ransac_homography(pairs of self as left and right: DeviceDescriptors, both built with positions): the dict
        of capi.ransac_homography"""
        if (self.n and not self.xy_ptr) or (right.n and not right.xy_ptr):
            raise ValueError("both sides need positions (DeviceDescriptors(arr, xy=...))")
        pairs = _pair_records(pairs)
        name, kind = _ransac_names(model)
        fn = lambda *a: getattr(lib(), name)(self.device, *a)
        return _ransac_call(fn, name, pairs.ctypes.data_as(C.c_void_p) if pairs.size else None, len(pairs), pairs.dtype,
                            self.xy_ptr, self.n, right.xy_ptr, right.n, opts or ransac_opts(), capacity, layers, kind=kind)

    def ransac_fundamental(self, right, pairs, opts=None, capacity=None, layers=False):
        """psx_ransac_fundamental(pairs of self as left and right): the dict of capi.ransac_fundamental"""
        return self.ransac_homography(right, pairs, opts, capacity, layers, model="fundamental")

    def ransac_affine(self, right, pairs, opts=None, capacity=None, layers=False):
        """psx_ransac_affine(pairs of self as left and right): the dict of capi.ransac_affine"""
        return self.ransac_homography(right, pairs, opts, capacity, layers, model="affine")

    def ransac_similarity(self, right, pairs, opts=None, capacity=None, layers=False):
        """psx_ransac_similarity(pairs of self as left and right): the dict of capi.ransac_similarity"""
        return self.ransac_homography(right, pairs, opts, capacity, layers, model="similarity")

    def close(self):
        if self.ptr:
            lib().psx_dev_free(self.device, self.ptr)
            self.ptr = C.c_void_p()
        if self.xy_ptr:
            lib().psx_dev_free(self.device, self.xy_ptr)
            self.xy_ptr = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def gauss_tables(cfg):
    inc_f = (C.c_float * (GAUSS_LEVELS * GAUSS_ALIGN))()
    inc_sp = (C.c_int * GAUSS_LEVELS)()
    inc_sg = (C.c_float * GAUSS_LEVELS)()
    dd_f = (C.c_float * (MAX_OCTAVES * GAUSS_ALIGN))()
    dd_sp = (C.c_int * MAX_OCTAVES)()
    dd_sg = (C.c_float * MAX_OCTAVES)()
    rc = lib().psx_gauss_tables(C.byref(cfg), inc_f, inc_sp, inc_sg, dd_f, dd_sp, dd_sg)
    if rc != 0:
        raise PopSiftError("psx_gauss_tables failed (%d)" % rc)
    return {
        "inc_filter": np.array(inc_f, dtype=np.float32).reshape(GAUSS_LEVELS, GAUSS_ALIGN),
        "inc_sigma": np.array(inc_sg, dtype=np.float32),
        "inc_span": np.array(inc_sp, dtype=np.int32),
        "dd_filter": np.array(dd_f, dtype=np.float32).reshape(MAX_OCTAVES, GAUSS_ALIGN),
        "dd_sigma": np.array(dd_sg, dtype=np.float32),
        "dd_span": np.array(dd_sp, dtype=np.int32),
    }


class Context:
    """One extraction context (pyramid + buffers + HIP stream) on one device."""

    def __init__(self, cfg=None, device=0):
        self._h = C.c_void_p()
        self.cfg = cfg if cfg is not None else default_config()
        rc = lib().psx_create(device, C.byref(self.cfg), C.byref(self._h))
        if rc != 0:
            msg = lib().psx_last_error(None)
            raise PopSiftError("psx_create failed (%d): %s" % (rc, msg.decode() if msg else ""))
        self._keep = None
        self._keep_kps = None
        self._keep_mask = None

    def _chk(self, rc):
        if rc != 0:
            msg = lib().psx_last_error(self._h)
            raise PopSiftError("C-ABI call failed (%d): %s" % (rc, msg.decode() if msg else ""))

    def close(self):
        if self._h:
            lib().psx_destroy(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    # ---- input -------------------------------------------------------------------------------
    def upload(self, img):
        img = np.ascontiguousarray(img)
        h, w = img.shape
        if img.dtype == np.uint8:
            self._chk(lib().psx_upload_u8(self._h, img.ctypes.data_as(C.c_void_p), w, h))
        elif img.dtype == np.float32:
            self._chk(lib().psx_upload_f32(self._h, img.ctypes.data_as(C.c_void_p), w, h))
        else:
            raise TypeError("image must be uint8 or float32")
        self._keep = img

    def set_input_dev(self, dev_ptr, w, h, is_float):
        self._chk(lib().psx_set_input_dev(self._h, C.c_void_p(dev_ptr), w, h, 1 if is_float else 0))

    def set_input_tensor(self, t):
        """t: contiguous 2-D torch tensor (uint8 or float32) already on this context's device."""
        assert t.is_contiguous() and t.dim() == 2
        import torch
        is_float = t.dtype == torch.float32
        assert is_float or t.dtype == torch.uint8
        self._keep = t
        self.set_input_dev(t.data_ptr(), t.shape[1], t.shape[0], is_float)

    # ---- stages ------------------------------------------------------------------------------
    def resize(self, w, h):
        self._chk(lib().psx_resize(self._h, w, h))

    def build_pyramid(self):
        self._chk(lib().psx_build_pyramid(self._h))

    def find_extrema(self):
        self._chk(lib().psx_find_extrema(self._h))

    def orientation(self):
        self._chk(lib().psx_orientation(self._h))

    def descriptors(self):
        self._chk(lib().psx_descriptors(self._h))

    def extract(self):
        self._chk(lib().psx_extract(self._h))

    def sync(self):
        self._chk(lib().psx_sync(self._h))

    # ---- caller-supplied keypoints -------------------------------------------------------------
    def set_keypoints(self, kps):
        """The keypoints of the next describe(): a KEYPOINT_DTYPE numpy array / a sequence of Keypoint (copied in
        stream order), or a contiguous torch uint8 / int32 / float32 tensor on this context's device that holds such
        records (no copy: it is kept alive here until the next call)."""
        if hasattr(kps, "data_ptr"):
            assert kps.is_contiguous() and kps.is_cuda
            nbytes = kps.numel() * kps.element_size()
            assert nbytes % KEYPOINT_DTYPE.itemsize == 0
            self._keep_kps = kps
            self._chk(lib().psx_set_keypoints_dev(self._h, C.c_void_p(kps.data_ptr()), nbytes // KEYPOINT_DTYPE.itemsize))
            return
        arr = keypoints_array(kps)
        self._keep_kps = None
        self._chk(lib().psx_set_keypoints(self._h, arr.ctypes.data_as(C.c_void_p), len(arr)))

    # ---- detection mask -------------------------------------------------------------------------
    def set_mask(self, mask):
        """psx_set_mask: mask = (h, w) uint8 / bool numpy array, non-zero = keypoints allowed (copied in stream order),
        or None to clear.  Sticky: it holds for every later find_extrema / extract until replaced or cleared; its size
        is checked there against the input's.  describe() ignores it."""
        self._keep_mask = None
        if mask is None:
            self._chk(lib().psx_set_mask(self._h, None, 0, 0))
            return
        m = mask_array(mask)
        self._chk(lib().psx_set_mask(self._h, m.ctypes.data_as(C.c_void_p), m.shape[1], m.shape[0]))

    def set_mask_tensor(self, t):
        """psx_set_mask_dev: t = contiguous 2-D torch uint8 / bool tensor on this context's device (no copy: it is kept
        alive here until the mask is replaced or cleared).  Work that writes t on another stream must be ordered against
        the context's stream (Context.stream) by the caller, as for set_input_tensor."""
        import torch
        assert t.is_contiguous() and t.dim() == 2 and t.is_cuda
        assert t.dtype in (torch.uint8, torch.bool)
        self._chk(lib().psx_set_mask_dev(self._h, C.c_void_p(t.data_ptr()), t.shape[1], t.shape[0]))
        self._keep_mask = t

    def describe(self, reuse_pyramid=False):
        """psx_describe: orientation (where a record brings none) and descriptors at the keypoints set before."""
        self._chk(lib().psx_describe(self._h, DESCRIBE_REUSE_PYRAMID if reuse_pyramid else 0))

    def keypoint_map(self):
        """psx_keypoint_map: int32 array, entry i = index of the input record output feature i came from."""
        n = C.c_int()
        self._chk(lib().psx_keypoint_map(self._h, None, 0, C.byref(n)))
        out = np.zeros((n.value,), np.int32)
        if n.value:
            self._chk(lib().psx_keypoint_map(self._h, out.ctypes.data_as(C.c_void_p), n.value, C.byref(n)))
        return out

    # ---- results -----------------------------------------------------------------------------
    @property
    def num_octaves(self):
        return lib().psx_num_octaves(self._h)

    @property
    def num_levels(self):
        return lib().psx_num_levels(self._h)

    def octave_dims(self, o):
        w, h = C.c_int(), C.c_int()
        self._chk(lib().psx_octave_dims(self._h, o, C.byref(w), C.byref(h)))
        return w.value, h.value

    def counts(self):
        ne, no = C.c_int(), C.c_int()
        self._chk(lib().psx_counts(self._h, C.byref(ne), C.byref(no)))
        return ne.value, no.value

    def download(self):
        ne, no = self.counts()
        feats = np.zeros((ne,), dtype=FEATURE_DTYPE)
        desc = np.zeros((no, 128), dtype=np.float32)
        self._chk(lib().psx_download(self._h, feats.ctypes.data_as(C.c_void_p), ne,
                                     desc.ctypes.data_as(C.c_void_p), no))
        return feats, desc

    def set_descriptor_format(self, fmt):
        """psx_set_descriptor_format: DESCFMT_F32 (default) or DESCFMT_U8 (floats and their quantised bytes)."""
        lib().psx_set_descriptor_format.argtypes = [C.c_void_p, C.c_int]
        self._chk(lib().psx_set_descriptor_format(self._h, fmt))

    def download_u8(self):
        """psx_download_u8: (features, (n,128) uint8 descriptors) of the last extraction in byte mode."""
        lib().psx_download_u8.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_int]
        ne, no = self.counts()
        feats = np.zeros((ne,), dtype=FEATURE_DTYPE)
        desc = np.zeros((no, 128), dtype=np.uint8)
        self._chk(lib().psx_download_u8(self._h, feats.ctypes.data_as(C.c_void_p), ne,
                                        desc.ctypes.data_as(C.c_void_p), no))
        return feats, desc

    def attach_export_u8(self, feat_buf, desc_buf):
        """psx_attach_export_u8: as attach_export, desc_buf a uint8 buffer of m*128 bytes; exported() then returns bytes."""
        L = lib()
        L.psx_attach_export_u8.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_int]
        if feat_buf is None:
            self._chk(L.psx_attach_export_u8(self._h, None, 0, None, 0))
            self._export = None
            return

        def ptr_n(b, itemsize):
            if hasattr(b, "data_ptr"):
                return b.data_ptr(), b.numel() * b.element_size() // itemsize
            return b.ctypes.data, b.nbytes // itemsize
        fp_, fn = ptr_n(feat_buf, FEATURE_DTYPE.itemsize)
        dp_, dn = ptr_n(desc_buf, 128)
        self._chk(L.psx_attach_export_u8(self._h, C.c_void_p(fp_), fn, C.c_void_p(dp_), dn))
        self._export = (feat_buf, desc_buf, np.uint8)

    def clone_results(self, device=0):
        """psx_clone_results into caller-owned device buffers (what FeaturesDev holds), read back:
        (Feature records with device pointers, descriptors, descriptor->extremum map, device address of descriptor 0)."""
        L = lib()
        L.psx_dev_alloc.argtypes = [C.c_int, C.c_size_t, C.POINTER(C.c_void_p)]
        L.psx_dev_free.argtypes = [C.c_int, C.c_void_p]
        L.psx_dev_read.argtypes = [C.c_int, C.c_void_p, C.c_void_p, C.c_size_t]
        L.psx_clone_results.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
        ne, no = self.counts()
        pf, pd, pr = C.c_void_p(), C.c_void_p(), C.c_void_p()
        for p, n in ((pf, max(ne, 1) * FEATURE_DEV_DTYPE.itemsize), (pd, max(no, 1) * 512), (pr, max(no, 1) * 4)):
            if L.psx_dev_alloc(device, n, C.byref(p)) != 0:
                raise PopSiftError("psx_dev_alloc failed")
        try:
            self._chk(L.psx_clone_results(self._h, pf, pd, pr))
            feats = np.zeros((ne,), dtype=FEATURE_DEV_DTYPE)
            desc = np.zeros((no, 128), dtype=np.float32)
            rev = np.zeros((no,), dtype=np.int32)
            for arr, p in ((feats, pf), (desc, pd), (rev, pr)):
                if arr.nbytes and L.psx_dev_read(device, arr.ctypes.data_as(C.c_void_p), p, arr.nbytes) != 0:
                    raise PopSiftError("psx_dev_read failed")
            return feats, desc, rev, pd.value
        finally:
            for p in (pf, pd, pr):
                L.psx_dev_free(device, p)

    def attach_export(self, feat_buf, desc_buf):
        """Attach host buffers for zero-copy export.  feat_buf: uint8 buffer (numpy array or pinned
        torch tensor) of n*52 bytes, desc_buf: float32 buffer of m*128 floats.  None detaches."""
        if feat_buf is None:
            self._chk(lib().psx_attach_export(self._h, None, 0, None, 0))
            self._export = None
            return

        def ptr_n(b, itemsize):
            if hasattr(b, "data_ptr"):
                return b.data_ptr(), b.numel() * b.element_size() // itemsize
            return b.ctypes.data, b.nbytes // itemsize
        fp_, fn = ptr_n(feat_buf, FEATURE_DTYPE.itemsize)
        dp_, dn = ptr_n(desc_buf, 128 * 4)
        self._chk(lib().psx_attach_export(self._h, C.c_void_p(fp_), fn, C.c_void_p(dp_), dn))
        self._export = (feat_buf, desc_buf)

    def exported(self):
        """After counts(): numpy views (no copy) of the exported features / descriptors."""
        ne, no = self.counts()
        fb, db = self._export[:2]
        dt = self._export[2] if len(self._export) > 2 else np.float32
        fa = fb.numpy() if hasattr(fb, "numpy") else fb
        da = db.numpy() if hasattr(db, "numpy") else db
        feats = fa.view(np.uint8).reshape(-1)[: ne * FEATURE_DTYPE.itemsize].view(FEATURE_DTYPE)
        desc = da.view(dt).reshape(-1)[: no * 128].reshape(no, 128)
        return feats, desc

    def dump_plane(self, kind, octave, level):
        w, h = self.octave_dims(octave)
        out = np.zeros((h, w), dtype=np.float32)
        self._chk(lib().psx_dump_plane(self._h, kind, octave, level, out.ctypes.data_as(C.c_void_p)))
        return out

    def dump_iext(self, octave):
        n = C.c_int()
        self._chk(lib().psx_dump_iext(self._h, octave, None, 0, C.byref(n)))
        out = np.zeros((n.value,), dtype=IEXT_DTYPE)
        if n.value:
            self._chk(lib().psx_dump_iext(self._h, octave, out.ctypes.data_as(C.c_void_p), n.value, C.byref(n)))
        return out

    def dump_extrema(self):
        n = C.c_int()
        self._chk(lib().psx_dump_extrema(self._h, None, 0, C.byref(n)))
        out = np.zeros((n.value,), dtype=EXT_DTYPE)
        if n.value:
            self._chk(lib().psx_dump_extrema(self._h, out.ctypes.data_as(C.c_void_p), n.value, C.byref(n)))
        return out

    # ---- measurement -------------------------------------------------------------------------
    def enable_timers(self, on=True):
        self._chk(lib().psx_enable_timers(self._h, 1 if on else 0))

    def stage_times(self):
        ms = (C.c_float * 4)()
        self._chk(lib().psx_stage_times(self._h, ms))
        return [ms[i] for i in range(4)]

    def time_blur(self, octave, level, reps=20):
        ms, by = C.c_float(), C.c_double()
        self._chk(lib().psx_time_blur(self._h, octave, level, reps, C.byref(ms), C.byref(by)))
        return ms.value, by.value

    def enable_blur_probe(self, on=True):
        self._chk(lib().psx_enable_blur_probe(self._h, 1 if on else 0))

    def blur_probe_times(self):
        """Durations (ms) of the octave-0 blur launches of the last extraction, timed in the pipeline, and the
        algorithmic bytes of one launch."""
        ms = (C.c_float * GAUSS_LEVELS)()
        n, by = C.c_int(), C.c_double()
        self._chk(lib().psx_blur_probe_times(self._h, ms, GAUSS_LEVELS, C.byref(n), C.byref(by)))
        return [ms[i] for i in range(n.value)], by.value

    def probe_extra_times(self):
        """(level0 ms, level0 algorithmic bytes, octave-0 extrema ms, its bytes) of the last extraction (blur probe on)."""
        L = lib()
        L.psx_probe_extra_times.argtypes = [C.c_void_p, C.POINTER(C.c_float), C.POINTER(C.c_double), C.POINTER(C.c_float), C.POINTER(C.c_double)]
        a, b, c, d = C.c_float(), C.c_double(), C.c_float(), C.c_double()
        self._chk(L.psx_probe_extra_times(self._h, C.byref(a), C.byref(b), C.byref(c), C.byref(d)))
        return a.value, b.value, c.value, d.value

    @property
    def stream(self):
        return lib().psx_stream(self._h)


def device_info(device=0):
    """psx_device_info: dict(name, total_mem, compute_units, clock_khz) of a device."""
    L = lib()
    L.psx_device_info.argtypes = [C.c_int, C.c_char_p, C.c_int, C.POINTER(C.c_size_t), C.POINTER(C.c_int), C.POINTER(C.c_int)]
    name = C.create_string_buffer(256)
    mem, cus, khz = C.c_size_t(), C.c_int(), C.c_int()
    if L.psx_device_info(device, name, 256, C.byref(mem), C.byref(cus), C.byref(khz)) != 0:
        raise PopSiftError("psx_device_info failed")
    return dict(name=name.value.decode(), total_mem=mem.value, compute_units=cus.value, clock_khz=khz.value)


def copy_bench(device=0, nbytes=0, reps=10):
    """Measured HBM roofline: (GB/s, ms per launch) of the 16 B/lane streaming copy kernel (psx_copy_bench)."""
    ms, by = C.c_float(), C.c_double()
    rc = lib().psx_copy_bench(device, nbytes, reps, C.byref(ms), C.byref(by))
    if rc != 0:
        raise PopSiftError("psx_copy_bench failed (%d)" % rc)
    return by.value / (ms.value * 1e-3) / 1e9, ms.value


# ---- the C++ host library through its flat C binding (include/popsift_c.h) --------------------------
HOST_LIB_PATH = os.environ.get("POPSIFT_HOST_LIB") or os.path.join(_HERE, "lib", "libpopsift.so")
HOST_SYMBOLS = ["popsift_c_create", "popsift_c_destroy", "popsift_c_enqueue_u8", "popsift_c_enqueue_f32",
                "popsift_c_get", "popsift_c_feature_count", "popsift_c_descriptor_count", "popsift_c_copy",
                "popsift_c_descriptors", "popsift_c_free", "popsift_c_last_error", "popsift_c_pool_stats",
                "popsift_c_create_fmt", "popsift_c_descriptor_format", "popsift_c_copy_u8", "popsift_c_descriptor_bytes",
                "popsift_c_enqueue_u8_kp", "popsift_c_enqueue_f32_kp", "popsift_c_source_indices",
                "popsift_c_enqueue_u8_mask", "popsift_c_enqueue_f32_mask"]
_HOST = None


def host_lib():
    global _HOST
    if _HOST is None:
        if not os.path.exists(HOST_LIB_PATH):
            raise PopSiftError("%s is missing: build it with `python -m popsift_amd.build`" % HOST_LIB_PATH)
        lib()                                   # libpopsift.so links against libpopsift_hip.so
        H = C.CDLL(HOST_LIB_PATH)
        vp = C.c_void_p
        H.popsift_c_create.argtypes = [C.POINTER(Config), C.c_int, C.c_int]
        H.popsift_c_create.restype = vp
        H.popsift_c_create_fmt.argtypes = [C.POINTER(Config), C.c_int, C.c_int, C.c_int]
        H.popsift_c_create_fmt.restype = vp
        H.popsift_c_descriptor_format.argtypes = [vp]
        H.popsift_c_copy_u8.argtypes = [vp, vp, vp]
        H.popsift_c_descriptor_bytes.argtypes = [vp]
        H.popsift_c_descriptor_bytes.restype = vp
        H.popsift_c_destroy.argtypes = [vp]
        H.popsift_c_destroy.restype = None
        for n in ("popsift_c_enqueue_u8", "popsift_c_enqueue_f32"):
            getattr(H, n).argtypes = [vp, C.c_int, C.c_int, vp]
            getattr(H, n).restype = vp
        for n in ("popsift_c_enqueue_u8_kp", "popsift_c_enqueue_f32_kp"):
            getattr(H, n).argtypes = [vp, C.c_int, C.c_int, vp, vp, C.c_int]
            getattr(H, n).restype = vp
        for n in ("popsift_c_enqueue_u8_mask", "popsift_c_enqueue_f32_mask"):
            getattr(H, n).argtypes = [vp, C.c_int, C.c_int, vp, vp, C.c_int, C.c_int]
            getattr(H, n).restype = vp
        H.popsift_c_source_indices.argtypes = [vp, vp, C.c_int]
        H.popsift_c_get.argtypes = [vp]
        H.popsift_c_get.restype = vp
        H.popsift_c_feature_count.argtypes = [vp]
        H.popsift_c_descriptor_count.argtypes = [vp]
        H.popsift_c_copy.argtypes = [vp, vp, vp]
        H.popsift_c_descriptors.argtypes = [vp]
        H.popsift_c_descriptors.restype = vp
        H.popsift_c_free.argtypes = [vp]
        H.popsift_c_free.restype = None
        H.popsift_c_last_error.restype = C.c_char_p
        H.popsift_c_pool_stats.argtypes = [C.c_int, C.POINTER(C.c_longlong)]
        H.popsift_c_pool_stats.restype = None
        _HOST = H
    return _HOST


def pool_stats(device=-1):
    """Counters of libpopsift's pinned pool (popsift_c_pool_stats): dict(allocs, frees, hits, free_buffers, free_bytes, in_use)."""
    out = (C.c_longlong * 6)()
    host_lib().popsift_c_pool_stats(device, out)
    return dict(zip(("allocs", "frees", "hits", "free_buffers", "free_bytes", "in_use"), [int(v) for v in out]))


class PopSift:
    """PopSift / SiftJob / FeaturesHost of the C++ library (popsift/popsift.h), through popsift_c.h:
    enqueue(img) -> job handle, get(job) -> (features, descriptors) numpy arrays or just the counts."""

    def __init__(self, cfg=None, device=0, float_images=False, byte_descriptors=False):
        """byte_descriptors: Config::ByteDescriptors -- get() returns (n,128) uint8 descriptors."""
        self.cfg = cfg if cfg is not None else default_config()
        if byte_descriptors:
            self._h = host_lib().popsift_c_create_fmt(C.byref(self.cfg), 1 if float_images else 0, device, DESCFMT_U8)
        else:
            self._h = host_lib().popsift_c_create(C.byref(self.cfg), 1 if float_images else 0, device)
        if not self._h:
            raise PopSiftError("popsift_c_create failed: %s" % host_lib().popsift_c_last_error().decode())
        self._float = float_images
        self._bytes = byte_descriptors

    def enqueue(self, img, keypoints=None, mask=None):
        """img: C-contiguous (h, w) numpy array, uint8 or float32 (matching the image mode).  keypoints: None (the
        detector runs) or the records to describe instead (KEYPOINT_DTYPE array or a sequence of Keypoint, may be
        empty); get_sources() of the result then maps the features back to them.  mask: None or the detection mask of
        this job, a (h', w') uint8 / bool array (deep-copied; refused when its size is not the image's); a job without
        one runs unmasked.  Keypoint jobs take no mask (the caller chose those points)."""
        h, w = img.shape
        if mask is not None:
            if keypoints is not None:
                raise ValueError("a job takes keypoints or a mask, not both")
            m = mask_array(mask)
            f = host_lib().popsift_c_enqueue_f32_mask if self._float else host_lib().popsift_c_enqueue_u8_mask
            job = f(self._h, w, h, img.ctypes.data, m.ctypes.data, m.shape[1], m.shape[0])
        elif keypoints is not None:
            kps = keypoints_array(keypoints)
            f = host_lib().popsift_c_enqueue_f32_kp if self._float else host_lib().popsift_c_enqueue_u8_kp
            job = f(self._h, w, h, img.ctypes.data, kps.ctypes.data, len(kps))
        else:
            f = host_lib().popsift_c_enqueue_f32 if self._float else host_lib().popsift_c_enqueue_u8
            job = f(self._h, w, h, img.ctypes.data)
        if not job:
            raise PopSiftError("enqueue refused the image: %s" % host_lib().popsift_c_last_error().decode())
        return job

    def get_counts(self, job):
        """SiftJob::get, then only the two counts; the FeaturesHost is deleted."""
        H = host_lib()
        f = H.popsift_c_get(job)
        if not f:
            raise PopSiftError("SiftJob::get failed: %s" % H.popsift_c_last_error().decode())
        n = (H.popsift_c_feature_count(f), H.popsift_c_descriptor_count(f))
        H.popsift_c_free(f)
        return n

    def get(self, job, with_sources=False):
        """(features, descriptors) of a job; with_sources: also the int32 input-record index of every feature (a job
        enqueued with keypoints; empty for a detector job)."""
        H = host_lib()
        f = H.popsift_c_get(job)
        if not f:
            raise PopSiftError("SiftJob::get failed: %s" % H.popsift_c_last_error().decode())
        ne, no = H.popsift_c_feature_count(f), H.popsift_c_descriptor_count(f)
        feats = np.zeros((ne,), dtype=FEATURE_DTYPE)
        src = np.zeros((max(H.popsift_c_source_indices(f, None, 0), 0),), np.int32)
        if len(src):
            H.popsift_c_source_indices(f, src.ctypes.data, len(src))
        if H.popsift_c_descriptor_format(f) == DESCFMT_U8:
            desc = np.zeros((no, 128), dtype=np.uint8)
            rc = H.popsift_c_copy_u8(f, feats.ctypes.data, desc.ctypes.data)
        else:
            desc = np.zeros((no, 128), dtype=np.float32)
            rc = H.popsift_c_copy(f, feats.ctypes.data, desc.ctypes.data)
        H.popsift_c_free(f)
        if rc != 0:
            raise PopSiftError("popsift_c_copy failed: %s" % H.popsift_c_last_error().decode())
        if with_sources:
            return feats, desc, src
        return feats, desc

    def close(self):
        if self._h:
            host_lib().popsift_c_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass
