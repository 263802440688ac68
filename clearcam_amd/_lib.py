"""ctypes binding of libclearcam_hip.so (include/clearcam_hip.h).  Fails loudly when the library is absent."""
from __future__ import annotations

import ctypes as C
import os

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "libclearcam_hip.so")

# every symbol include/clearcam_hip.h declares
SYMBOLS = [
    "cc_last_error", "cc_version", "cc_device_count",
    "cc_yolo_create", "cc_yolo_load", "cc_yolo_calibrate", "cc_yolo_calibration_info", "cc_gptq_round_f16", "cc_yolo_finalize", "cc_yolo_detect", "cc_yolo_set_in_flight", "cc_yolo_submit", "cc_yolo_wait",
    "cc_yolo_detect_ragged", "cc_yolo_submit_ragged", "cc_letterbox_geometry", "cc_yolo_plans_built",
    "cc_yolo_get_tensor", "cc_yolo_get_tensor_frames", "cc_yolo_nonfinite",
    "cc_yolo_last_gpu_ms", "cc_yolo_profile", "cc_yolo_profile_graph", "cc_yolo_destroy", "cc_conv2d_nhwc", "cc_conv2d_ex", "cc_conv2d_ex_route", "cc_route_log_take", "cc_conv_bench", "cc_dev_set", "cc_round_weights", "cc_attn_bench",
    "cc_dev_decode", "cc_dev_head_tail", "cc_dev_topk_nms", "cc_dev_blaze_post",
    "cc_dev_pool", "cc_dev_pool_choice", "cc_dev_fuse", "cc_dev_conv_src", "cc_dev_conv_det", "cc_dev_conv_det_choice", "cc_dev_affine", "cc_dev_face_pre",
    "cc_dev_csp", "cc_dev_csp_choice", "cc_dev_stem",
    "cc_dev_attention", "cc_dev_layernorm", "cc_dev_assemble_ln", "cc_dev_patchify", "cc_dev_embed", "cc_dev_l2norm",
    "cc_clip_create", "cc_clip_load", "cc_clip_finalize", "cc_clip_encode_image", "cc_clip_encode_text",
    "cc_clip_set_in_flight", "cc_clip_submit_image", "cc_clip_wait",
    "cc_clip_last_gpu_ms", "cc_clip_destroy", "cc_crop_preprocess", "cc_cv_resize_linear_u8", "cc_cv_warp_affine_u8",
    "cc_blaze_create", "cc_blaze_load", "cc_blaze_finalize", "cc_blaze_detect", "cc_blaze_detect_batch", "cc_blaze_destroy",
    "cc_face_locate", "cc_face_align",
    "cc_face_create", "cc_face_load", "cc_face_finalize", "cc_face_embed", "cc_face_destroy",
    "cc_ocsort_create", "cc_ocsort_update", "cc_ocsort_update_many", "cc_ocsort_num_tracks", "cc_ocsort_destroy",
    "cc_index_create", "cc_index_create_ex", "cc_index_add", "cc_index_add_grouped", "cc_index_size", "cc_index_info", "cc_index_scores", "cc_index_last_path",
    "cc_index_search", "cc_index_search_groups", "cc_index_add_tracked", "cc_index_search_tracks", "cc_index_rank",
    "cc_index_add_described", "cc_index_row_info", "cc_index_rank_where", "cc_index_timeline", "cc_index_fetch_rows", "cc_index_rank_like",
    "cc_index_rank_terms", "cc_index_timeline_terms", "cc_index_rank_near", "cc_index_timeline_near",
    "cc_index_gram", "cc_index_distinct", "cc_index_digest", "cc_index_sightings",
    "cc_index_remove_rows", "cc_index_remove_groups", "cc_index_destroy",
    "cc_watch_create", "cc_watch_set", "cc_watch_size", "cc_watch_scores", "cc_watch_match", "cc_watch_destroy",
]


class ClipConfig(C.Structure):
    _fields_ = [(n, C.c_int) for n in ("image_size", "patch", "v_width", "v_layers", "v_heads", "v_mlp",
                                       "t_ctx", "t_vocab", "t_width", "t_layers", "t_heads", "t_mlp", "embed")]


class ConvDesc(C.Structure):
    """cc_conv_desc: the launch cc_conv2d_ex runs (include/clearcam_hip.h)."""
    _fields_ = [(n, C.c_int) for n in ("dtype", "B", "H", "W", "Cin", "Cout", "k", "stride", "groups", "act", "pad", "Ho", "Wo",
                                       "out_f32", "out_cstride", "out_coff", "res_f32", "res_cstride", "res_coff", "variant")]


class SrcDesc(C.Structure):
    """cc_src_desc: one source view of cc_dev_conv_src (include/clearcam_hip.h)."""
    _fields_ = [("ptr", C.c_void_p)] + [(n, C.c_int) for n in ("H", "W", "cstride", "coff", "C", "shift")]


DEV_CSP_LAYERS = 3                                    # CC_DEV_CSP_LAYERS: *choice of cc_dev_csp for the four conv launches
DEV_CONV_ADOWN = 100                                  # CC_DEV_CONV_ADOWN: choice[0] of cc_dev_conv_src for the averaging kernel
ROUTE_REC_INTS = 23                                   # ints per cc_route_log_take record
CONV_CHOICE_INTS = 8                                  # ints cc_conv2d_ex_route and cc_dev_conv_det write to `choice`: kernel, sched, bm, bn, simple, two, cprw, ns (cc_conv2d_ex: the first four)


class FaceAlignRec(C.Structure):
    """cc_face_align_rec: one face of cc_face_align (crop, cut rectangle, the two forward warpAffine matrices)."""
    _fields_ = [("offset", C.c_int64), ("h", C.c_int32), ("w", C.c_int32),
                ("cx1", C.c_int32), ("cy1", C.c_int32), ("cw", C.c_int32), ("ch", C.c_int32),
                ("out_w", C.c_int32), ("out_h", C.c_int32), ("rot", C.c_double * 6), ("place", C.c_double * 6)]


ROW_NO_TS = -(1 << 31)                                # CC_ROW_NO_TS: a row without a ts
RANK_TRACKS = 1                                       # CC_RANK_TRACKS
LIKE_MAX_ROWS = 64                                    # CC_LIKE_MAX_ROWS: the most query rows of one cc_index_rank_like
LIKE_EXCLUDE_ROWS, LIKE_EXCLUDE_TRACK = 2, 4          # CC_LIKE_EXCLUDE_ROWS / CC_LIKE_EXCLUDE_TRACK
TERMS_MAX = 64                                        # CC_TERMS_MAX: the most terms of one cc_index_rank_terms
TERM_RANK, TERM_REQUIRE, TERM_REJECT = 0, 1, 2        # CC_TERM_RANK / CC_TERM_REQUIRE / CC_TERM_REJECT
COMBINE_MAX, COMBINE_MIN, COMBINE_SUM = 0, 1, 2       # CC_COMBINE_MAX / CC_COMBINE_MIN / CC_COMBINE_SUM
NEAR_MAX_PARTNERS, NEAR_DEFAULT_PARTNERS = 16384, 4096   # CC_NEAR_MAX_PARTNERS / CC_NEAR_DEFAULT_PARTNERS
NEAR_VALUE = {"a": 0, "min": 1}                       # CC_NEAR_VALUE_A / CC_NEAR_VALUE_MIN
DISTINCT_MAX_DEPTH, DISTINCT_MAX_Q = 1024, 64        # CC_DISTINCT_MAX_DEPTH / CC_DISTINCT_MAX_Q
DIGEST_MAX_LEADERS = 1024                             # CC_DIGEST_MAX_LEADERS
DIGEST_BY_COUNT, DIGEST_BY_FIRST = 0, 1               # CC_DIGEST_BY_COUNT / CC_DIGEST_BY_FIRST
SIGHT_MAX_OBJECTS, SIGHT_MAX_GROUPS = 1024, 4096      # CC_SIGHT_MAX_OBJECTS / CC_SIGHT_MAX_GROUPS
SIGHT_SKIP_SELF = 1                                   # CC_SIGHT_SKIP_SELF


class RowFilter(C.Structure):
    """cc_row_filter: the row filter of cc_index_rank_where / cc_index_timeline (include/clearcam_hip.h)."""
    _fields_ = [("use_ts", C.c_int32), ("ts_min", C.c_int32), ("ts_max", C.c_int32), ("use_cls", C.c_int32), ("cls_mask", C.c_uint64 * 4)]


class Term(C.Structure):
    """cc_term: what one term of cc_index_rank_terms / cc_index_timeline_terms is (include/clearcam_hip.h)."""
    _fields_ = [("role", C.c_int32), ("weight", C.c_float), ("cut", C.c_float)]


class CCError(RuntimeError):
    pass


_lib = None


def lib() -> C.CDLL:
    """Load the HIP library (no CPU fallback: a missing .so is an error, not a slow path)."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise CCError(f"{LIB_PATH} not built: run `python -c 'import __graft_entry__ as g; g.build()'` "
                      "(hipcc --offload-arch=gfx950). There is no CPU fallback.")
    try:
        # PyTorch-ROCm ships its own libamdhip64/libhsa-runtime64.  Whichever copy is mapped first serves the whole
        # process (same SONAME), and torch fails to find the GPU on the system copy: let torch map its runtime first.
        import torch  # noqa: F401
    except ImportError:
        pass
    L = C.CDLL(LIB_PATH)
    L.cc_last_error.restype = C.c_char_p
    vp, ip, fp, i64p = C.c_void_p, C.POINTER(C.c_int), C.POINTER(C.c_float), C.POINTER(C.c_int64)
    sig = {
        "cc_version": [],
        "cc_device_count": [ip],
        "cc_yolo_create": [C.POINTER(vp), C.c_char_p, C.c_int, C.c_int, C.c_int],
        "cc_yolo_load": [vp, C.c_char_p, vp, i64p, C.c_int],
        "cc_yolo_finalize": [vp],
        "cc_yolo_calibrate": [vp, vp, C.c_int, C.c_int, C.c_int, C.c_int],
        "cc_yolo_calibration_info": [vp, ip, ip],
        "cc_gptq_round_f16": [vp, C.c_int64, C.c_int64, vp, C.c_double, vp],
        "cc_yolo_detect": [vp, vp, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, vp, C.c_int, vp],
        "cc_yolo_set_in_flight": [vp, C.c_int],
        "cc_yolo_submit": [vp, vp, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, vp, C.c_int, vp, C.POINTER(C.c_longlong)],
        "cc_yolo_wait": [vp, C.c_longlong, vp],
        "cc_yolo_detect_ragged": [vp, vp, i64p, C.POINTER(C.c_int32), C.POINTER(C.c_int32), C.c_int, C.c_int, C.c_int, vp, C.c_int, vp],
        "cc_yolo_submit_ragged": [vp, vp, i64p, C.POINTER(C.c_int32), C.POINTER(C.c_int32), C.c_int, C.c_int, C.c_int, vp, C.c_int, vp, C.POINTER(C.c_longlong)],
        "cc_letterbox_geometry": [C.c_int, C.c_int, C.c_int, ip, ip, ip, ip],
        "cc_yolo_plans_built": [vp, ip],
        "cc_yolo_get_tensor": [vp, C.c_char_p, vp, i64p, ip],
        "cc_yolo_get_tensor_frames": [vp, C.c_char_p, C.c_int, C.c_int, vp, i64p, ip],
        "cc_yolo_nonfinite": [vp, ip],
        "cc_yolo_last_gpu_ms": [vp, fp],
        "cc_yolo_profile": [vp, C.c_int, fp, C.POINTER(C.c_double), ip],
        "cc_yolo_profile_graph": [vp, C.c_int, C.c_int, fp],
        "cc_conv2d_nhwc": [C.c_int, vp, C.c_int, C.c_int, C.c_int, C.c_int, vp, vp, C.c_int, C.c_int, C.c_int, C.c_int,
                           C.c_int, vp, C.c_int, vp],
        "cc_conv2d_ex": [C.POINTER(ConvDesc), vp, vp, vp, vp, vp, vp, ip, vp],
        "cc_conv2d_ex_route": [C.POINTER(ConvDesc), vp, vp, vp, vp, vp, vp, ip, vp],
        "cc_route_log_take": [ip, C.c_int, ip],
        "cc_dev_decode": [vp, ip, ip, C.c_int, vp, C.c_float, vp, ip, vp],
        "cc_dev_head_tail": [C.c_int, C.c_int, vp, vp, vp, vp, vp, vp, ip, ip, C.c_int, vp, C.c_float, vp, ip, vp],
        "cc_dev_topk_nms": [vp, C.c_int, C.c_int, C.c_float, vp, C.c_int, vp, vp],
        "cc_dev_blaze_post": [vp, vp, vp, vp, C.c_int, vp, C.c_float, C.c_int, C.c_int, vp, vp, vp, vp],
        "cc_dev_pool": [C.c_int, vp, C.c_int, C.c_int, vp] + [C.c_int] * 12 + [ip, vp],
        "cc_dev_pool_choice": [C.c_int, vp, C.c_int, C.c_int, vp] + [C.c_int] * 12 + [ip],
        "cc_dev_fuse": [C.c_int, C.c_int, vp, ip, ip, ip, ip, ip, vp, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, vp],
        "cc_dev_conv_src": [C.POINTER(ConvDesc), C.POINTER(SrcDesc), C.POINTER(SrcDesc), vp, vp, vp, ip, vp],
        "cc_dev_conv_det": [C.POINTER(ConvDesc), C.POINTER(SrcDesc), C.POINTER(SrcDesc), vp, vp, vp, vp, ip, vp],
        "cc_dev_conv_det_choice": [C.POINTER(ConvDesc), C.POINTER(SrcDesc), C.POINTER(SrcDesc), vp, vp, ip],
        "cc_dev_affine": [C.c_int, vp, vp, vp, vp, C.c_longlong, C.c_int, vp],
        "cc_dev_face_pre": [C.c_int, vp, C.c_int, vp, C.c_int, C.c_int, vp],
        "cc_dev_csp": [C.c_int, C.c_int, C.c_int, vp, C.c_int, C.c_int, vp, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.POINTER(vp), C.POINTER(vp),
                       C.c_int, C.c_int, ip, vp],
        "cc_dev_csp_choice": [C.c_int] * 8 + [ip],
        "cc_dev_stem": [C.c_int, C.c_int, vp, C.c_int, i64p, C.POINTER(C.c_int32), C.POINTER(C.c_int32), C.c_int, C.c_int, C.c_int, vp, vp, C.c_int,
                        vp, C.c_int, C.c_int, ip, vp],
        "cc_dev_attention": [C.c_int, vp, C.c_int, C.c_int, C.c_int, C.c_int, C.c_float, vp, vp],
        "cc_dev_layernorm": [C.c_int, vp, C.c_longlong, vp, vp, vp, vp, C.c_int, C.c_int, C.c_int, vp],
        "cc_dev_assemble_ln": [C.c_int, vp, vp, vp, vp, vp, vp, C.c_int, C.c_int, C.c_int, vp],
        "cc_dev_patchify": [C.c_int, vp, vp, C.c_int, C.c_int, C.c_int, C.c_int, vp],
        "cc_dev_embed": [vp, C.c_int, vp, vp, vp, C.c_int, C.c_int, C.c_int, vp],
        "cc_dev_l2norm": [vp, C.c_int, C.c_int, C.c_float, vp],
        "cc_conv_bench": [C.c_int] * 11 + [fp],
        "cc_dev_set": [C.c_char_p, C.c_int],
        "cc_round_weights": [C.c_int, vp, C.c_int64, C.c_int64, C.c_int64, vp],
        "cc_attn_bench": [C.c_int] * 7 + [fp],
        "cc_clip_create": [C.POINTER(vp), C.POINTER(ClipConfig), C.c_int, C.c_int],
        "cc_clip_load": [vp, C.c_char_p, vp, i64p, C.c_int],
        "cc_clip_finalize": [vp],
        "cc_clip_encode_image": [vp, vp, C.c_int, C.c_int, vp, C.c_int, vp],
        "cc_clip_encode_text": [vp, vp, C.c_int, vp, C.c_int, vp],
        "cc_clip_set_in_flight": [vp, C.c_int],
        "cc_clip_submit_image": [vp, vp, C.c_int, C.c_int, vp, C.c_int, vp, C.POINTER(C.c_longlong)],
        "cc_clip_wait": [vp, C.c_longlong, vp],
        "cc_clip_last_gpu_ms": [vp, fp],
        "cc_crop_preprocess": [vp, vp, vp, vp, C.c_int, C.c_int, C.c_int, vp, C.c_int, vp],
        "cc_cv_resize_linear_u8": [vp, C.c_int, C.c_int, vp, C.c_int, C.c_int, C.c_int],
        "cc_cv_warp_affine_u8": [vp, C.c_int, C.c_int, vp, vp, C.c_int, C.c_int, C.c_int],
        "cc_blaze_create": [C.POINTER(vp), C.c_int, C.c_int],
        "cc_blaze_load": [vp, C.c_char_p, vp, i64p, C.c_int],
        "cc_blaze_finalize": [vp],
        "cc_blaze_detect": [vp, vp, C.c_int, C.c_int, C.c_int, C.c_int, vp, C.c_int, vp],
        "cc_blaze_detect_batch": [vp, vp, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, vp, C.c_int, vp],
        "cc_face_locate": [vp, vp, C.c_int64, vp, vp, vp, C.c_int, C.c_int, vp, vp, vp],
        "cc_face_align": [vp, C.c_int64, C.c_int, vp, C.c_int, vp, C.c_int, vp],
        "cc_face_create": [C.POINTER(vp), C.c_int, C.c_int],
        "cc_face_load": [vp, C.c_char_p, vp, i64p, C.c_int],
        "cc_face_finalize": [vp],
        "cc_face_embed": [vp, vp, C.c_int, C.c_int, C.c_int, vp, C.c_int, vp],
        "cc_ocsort_create": [C.POINTER(vp), C.c_int, C.c_int, C.c_double, C.c_int, C.c_double, C.c_int],
        "cc_ocsort_update": [vp, vp, C.c_int, C.c_double, vp, C.c_int, ip],
        "cc_ocsort_update_many": [vp, C.c_int, vp, C.c_int, C.c_double, vp, C.c_int, vp, C.c_int],
        "cc_ocsort_num_tracks": [vp, ip],
        "cc_index_create": [C.POINTER(vp), C.c_int, C.c_int64, C.c_int],
        "cc_index_create_ex": [C.POINTER(vp), C.c_int, C.c_int64, C.c_int, C.c_int],
        "cc_index_add": [vp, vp, C.c_int64, C.c_int],
        "cc_index_add_grouped": [vp, vp, C.c_int64, C.c_int, vp],
        "cc_index_add_tracked": [vp, vp, C.c_int64, C.c_int, vp, vp],
        "cc_index_info": [vp, i64p, C.POINTER(C.c_int), C.POINTER(C.c_int)],
        "cc_index_search_groups": [vp, vp, C.c_int, C.c_int, vp, C.c_int, vp, vp, C.c_int, vp],
        "cc_index_search_tracks": [vp, vp, C.c_int, C.c_int, vp, C.c_int, vp, vp, C.c_int, vp],
        "cc_index_rank": [vp, vp, C.c_int, C.c_int64, C.c_int64, C.c_float, C.c_int, vp, C.c_int, vp, vp, vp, C.c_int, vp],
        "cc_index_add_described": [vp, vp, C.c_int64, C.c_int, vp, vp, vp, vp],
        "cc_index_row_info": [vp, C.c_int64, C.c_int64, vp, vp],
        "cc_index_rank_where": [vp, vp, C.c_int, C.c_int64, C.c_int64, C.c_float, C.c_int, vp, C.c_int, C.POINTER(RowFilter), vp, vp, vp, C.c_int, vp],
        "cc_index_timeline": [vp, vp, C.c_int, C.c_float, C.c_int, vp, C.c_int, C.POINTER(RowFilter), C.c_int32, C.c_int32, C.c_int, vp, vp, C.c_int, vp],
        "cc_index_fetch_rows": [vp, i64p, C.c_int, vp, C.c_int, vp],
        "cc_index_rank_like": [vp, i64p, C.c_int, C.c_int64, C.c_int64, C.c_float, C.c_int, vp, C.c_int, C.POINTER(RowFilter), vp, vp, vp, C.c_int, vp],
        "cc_index_rank_terms": [vp, vp, C.c_int, i64p, C.c_int, C.POINTER(Term), C.c_int, C.c_int64, C.c_int64, C.c_float, C.c_int, vp, C.c_int,
                                C.POINTER(RowFilter), vp, vp, vp, vp, C.c_int, vp],
        "cc_index_timeline_terms": [vp, vp, C.c_int, i64p, C.c_int, C.POINTER(Term), C.c_int, C.c_float, C.c_int, vp, C.c_int, C.POINTER(RowFilter),
                                    C.c_int32, C.c_int32, C.c_int, vp, vp, C.c_int, vp],
        "cc_index_rank_near": [vp, vp, C.c_int64, vp, C.c_int64, C.c_int32, C.c_int, C.c_float, C.c_int, C.c_int64, C.c_int64, C.c_float, C.c_int, vp, C.c_int,
                               C.POINTER(RowFilter), C.POINTER(RowFilter), vp, vp, vp, vp, vp, vp, C.c_int, vp],
        "cc_index_timeline_near": [vp, vp, C.c_int64, vp, C.c_int64, C.c_int32, C.c_int, C.c_float, C.c_int, C.c_float, C.c_int, vp, C.c_int,
                                   C.POINTER(RowFilter), C.POINTER(RowFilter), C.c_int32, C.c_int32, C.c_int, vp, vp, vp, C.c_int, vp],
        "cc_index_gram": [vp, i64p, C.c_int, vp, C.c_int, vp],
        "cc_index_distinct": [vp, vp, vp, C.c_int, C.c_int, C.c_float, C.c_int64, C.c_int64, vp, vp, vp, vp, C.c_int, vp],
        "cc_index_digest": [vp, C.c_float, C.c_int, C.c_int, vp, C.c_int, C.POINTER(RowFilter), C.c_int64, C.c_int64, vp, vp, vp, vp, vp, vp, C.c_int, vp],
        "cc_index_sightings": [vp, i64p, C.c_int, C.c_float, C.c_int, vp, C.c_int, C.POINTER(RowFilter), vp, vp, vp, vp, C.c_int, vp, C.c_int, vp],
        "cc_index_remove_rows": [vp, vp, C.c_int64, i64p],
        "cc_index_remove_groups": [vp, vp, C.c_int, i64p],
        "cc_index_size": [vp, i64p],
        "cc_index_scores": [vp, vp, C.c_int, vp, C.c_int, vp],
        "cc_index_last_path": [vp, ip],
        "cc_index_search": [vp, vp, C.c_int, C.c_int, vp, vp, C.c_int, vp],
        "cc_watch_create": [C.POINTER(vp), C.c_int, C.c_int],
        "cc_watch_set": [vp, vp, vp, vp, C.c_int],
        "cc_watch_size": [vp, ip],
        "cc_watch_scores": [vp, vp, C.c_int, C.c_int, vp, C.c_int, vp],
        "cc_watch_match": [vp, vp, C.c_int, C.c_int, vp, vp, vp, vp, C.c_int, vp],
    }
    for name, args in sig.items():
        fn = getattr(L, name)
        fn.argtypes = args
        fn.restype = C.c_int
    for name in ("cc_yolo_destroy", "cc_clip_destroy", "cc_index_destroy", "cc_ocsort_destroy", "cc_face_destroy", "cc_blaze_destroy", "cc_watch_destroy"):
        getattr(L, name).argtypes = [vp]
        getattr(L, name).restype = None
    _lib = L
    return L


def check(rc: int) -> None:
    if rc != 0:
        raise CCError(f"libclearcam_hip error {rc}: {lib().cc_last_error().decode(errors='replace')}")


def ptr(x):
    """Raw address of a numpy array / torch tensor / int."""
    if x is None:
        return None
    if isinstance(x, int):
        return C.c_void_p(x)
    if hasattr(x, "data_ptr"):
        return C.c_void_p(x.data_ptr())
    return C.c_void_p(x.ctypes.data)
