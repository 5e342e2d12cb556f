"""ctypes binding of libhsefr.so (include/hsefr.h).  No fallback: if the library is missing the
import of anything that needs it raises, and every non-zero status becomes a Python exception
in the reference's error style (ValueError for shape errors, NotImplementedError for unsupported
graphs, RuntimeError otherwise)."""
from __future__ import annotations

import ctypes
import os
from ctypes import POINTER, c_char_p, c_float, c_int, c_longlong, c_size_t, c_void_p

_HERE = os.path.dirname(os.path.abspath(__file__))
# HSEFR_LIB selects another build of the library (e.g. libhsefr_dev.so for tools/kbench.py); the product is libhsefr.so
LIB_PATH = os.path.join(_HERE, os.environ.get("HSEFR_LIB", "libhsefr.so"))

OK, ERR_INVALID, ERR_UNSUPPORTED, ERR_HIP, ERR_NOMEM, ERR_SHAPE = 0, -1, -2, -3, -4, -5

_lib = None

# name -> (restype, argtypes); one row per declaration in include/hsefr.h
_fp = c_void_p   # device pointers travel as integers (tensor.data_ptr())
SIGNATURES = {
    "hsefr_version": (c_int, []),
    "hsefr_last_error_string": (c_char_p, []),
    "hsefr_engine_set_graph_batch": (c_int, [c_void_p, c_int]),
    "hsefr_engine_graph_launches": (c_longlong, [c_void_p]),
    "hsefr_engine_create": (c_int, [c_void_p, c_size_t, c_int, POINTER(c_void_p)]),
    "hsefr_plan_validate": (c_int, [c_void_p, c_size_t]),
    "hsefr_plan_describe": (c_int, [c_void_p, c_size_t, c_int, c_char_p, c_size_t]),
    "hsefr_engine_workspace_bytes": (c_size_t, [c_void_p]),
    "hsefr_engine_max_batch": (c_int, [c_void_p]),
    "hsefr_engine_forward": (c_int, [c_void_p, _fp, c_int, _fp, _fp, _fp, c_void_p]),
    "hsefr_engine_buffer": (c_void_p, [c_void_p, c_int]),
    "hsefr_engine_copy_buffer": (c_int, [c_void_p, c_int, _fp, c_size_t, c_void_p]),
    "hsefr_engine_set_profiling": (c_int, [c_void_p, c_int]),
    "hsefr_engine_profiled_calls": (c_longlong, [c_void_p]),
    "hsefr_engine_op_times_ms": (c_int, [c_void_p, c_int, POINTER(c_float), c_int]),
    "hsefr_engine_destroy": (c_int, [c_void_p]),
    "hsefr_conv_c3_bias_act": (c_int, [_fp, _fp, _fp, _fp] + [c_int] * 12 + [c_void_p]),
    "hsefr_dwconv3x3_bn_relu6": (c_int, [_fp, _fp, _fp, _fp, _fp] + [c_int] * 10 + [c_void_p]),
    "hsefr_dwconv3x3_bn_relu6_split": (c_int, [_fp, _fp, _fp, _fp, _fp] + [c_int] * 11 + [c_void_p]),
    "hsefr_pwconv1x1_presplit_gap": (c_int, [_fp, c_void_p, _fp, _fp, _fp, c_longlong, c_int, c_int, c_int, c_int, c_void_p]),
    "hsefr_pwconv1x1_presplit_dw": (c_int, [_fp, c_void_p, _fp, _fp, _fp, _fp, c_longlong] + [c_int] * 7 + [c_void_p]),
    "hsefr_pwconv1x1_presplit": (c_int, [_fp, c_void_p, _fp, _fp, _fp, c_longlong, c_int, c_int, c_int, c_void_p]),
    "hsefr_pwconv1x1_bias_relu6": (c_int, [_fp, _fp, _fp, _fp, c_longlong, c_int, c_int, c_int, c_void_p]),
    "hsefr_stem2_fused": (c_int, [_fp] * 6 + [c_void_p] + [_fp] * 6 + [c_int] * 13 + [c_void_p]),
    "hsefr_stem3_fused": (c_int, [_fp, c_void_p] + [_fp] * 5 + [c_void_p] + [_fp] * 7 + [c_int] * 14 + [c_void_p]),
    "hsefr_stem4_fused": (c_int, [_fp, c_int, c_void_p] + [_fp] * 5 + [c_void_p] + [_fp] * 7 + [c_int] * 6 + [c_void_p]),
    "hsefr_stem5_stream": (c_int, [_fp, c_int, c_void_p] + [_fp] * 5 + [c_void_p] + [_fp] * 7 + [c_int] * 6 + [c_void_p]),
    "hsefr_engine_accepts_u8": (c_int, [c_void_p]),
    "hsefr_engine_forward_u8": (c_int, [c_void_p, _fp, c_int, _fp, _fp, _fp, c_void_p]),
    "hsefr_engine_input_overflow": (c_int, [c_void_p, POINTER(c_int), c_void_p]),
    "hsefr_engine_input_overflow_async": (c_int, [c_void_p, POINTER(c_int), c_void_p]),
    "hsefr_dwpw_f16split": (c_int, [_fp, _fp, _fp, _fp, c_void_p, _fp, _fp, _fp] + [c_int] * 12 + [c_void_p]),
    "hsefr_pwblk_f16split": (c_int, [_fp, c_void_p, _fp, _fp, _fp, _fp, _fp, c_void_p, _fp, _fp, _fp, _fp] + [c_int] * 10 + [c_void_p]),
    "hsefr_pwconv1x1_f16split": (c_int, [_fp, c_void_p, _fp, _fp, _fp, c_longlong, c_int, c_int, c_int, c_int, c_void_p]),
    "hsefr_dwpw_fused": (c_int, [_fp] * 7 + [c_int] * 10 + [c_void_p]),
    "hsefr_gap": (c_int, [_fp, _fp, c_int, c_int, c_int, c_void_p]),
    "hsefr_dense": (c_int, [_fp, _fp, _fp, _fp, c_int, c_int, c_int, c_int, c_void_p]),
    "hsefr_softmax": (c_int, [_fp, _fp, c_int, c_int, c_void_p]),
    "hsefr_heads_fused": (c_int, [_fp] * 11 + [c_int] * 3 + [c_void_p]),
    "hsefr_conv_bf16": (c_int, [_fp, _fp, _fp, _fp, _fp, _fp] + [c_int] * 13 + [c_void_p]),
    "hsefr_conv1x1_proj_bf16": (c_int, [_fp] * 9 + [c_int] * 10 + [c_void_p]),
    "hsefr_conv1x1_sres_bf16": (c_int, [_fp] * 6 + [c_int] * 9 + [c_void_p]),
    "hsefr_conv1x1_pair_bf16": (c_int, [_fp] * 14 + [c_longlong] + [c_int] * 6 + [c_void_p]),
    "hsefr_conv1x1_pair_sub2_bf16": (c_int, [_fp] * 14 + [c_int] * 9 + [c_void_p]),
    "hsefr_stem7x7_bf16": (c_int, [_fp, _fp, _fp, _fp, _fp] + [c_int] * 6 + [c_void_p]),
    "hsefr_stem7x7_pool_bf16": (c_int, [_fp, c_void_p, _fp, _fp, c_void_p] + [c_int] * 7 + [c_void_p]),
    "hsefr_maxpool3x3s2_bf16": (c_int, [_fp, _fp] + [c_int] * 8 + [c_void_p]),
    "hsefr_gap_bf16": (c_int, [_fp, _fp, c_int, c_int, c_int, c_void_p]),
    "hsefr_preprocess_pil_u8": (c_int, [_fp, _fp, _fp] + [c_int] * 5 + [_fp, _fp, _fp, c_int, _fp, _fp, _fp, c_int, c_int,
                                        POINTER(ctypes.c_double), c_void_p]),
    "hsefr_preprocess_cv_u8": (c_int, [_fp, _fp] + [c_int] * 5 + [_fp] * 6 + [c_int, POINTER(ctypes.c_double), c_void_p]),
    "hsefr_l2_normalize": (c_int, [_fp, _fp, c_int, c_int, c_void_p]),
    "hsefr_conv2d_direct": (c_int, [_fp] * 5 + [c_int] * 12 + [c_void_p]),
    "hsefr_conv2d_f32": (c_int, [_fp] * 6 + [c_int] * 13 + [c_void_p]),
    "hsefr_conv2d_f32_mfma": (c_int, [_fp] * 6 + [c_int] * 13 + [c_void_p]),
    "hsefr_maxpool_f32": (c_int, [_fp, _fp] + [c_int] * 10 + [c_void_p]),
    "hsefr_mtcnn_pyramid_level": (c_int, [_fp, _fp, c_int, c_int, c_int, c_int, c_void_p]),
    "hsefr_mtcnn_post_capacity": (c_int, []),
    "hsefr_mtcnn_stage1_level": (c_int, [_fp, _fp, c_int, c_int, ctypes.c_double, ctypes.c_float, _fp, _fp, c_void_p]),
    "hsefr_mtcnn_stage1_finish": (c_int, [_fp, _fp, _fp, _fp, c_int, c_int, c_void_p]),
    "hsefr_mtcnn_stage_finish": (c_int, [c_int, _fp, c_int, _fp, _fp, _fp, ctypes.c_float, _fp, _fp, _fp, _fp, c_int, c_int, c_void_p]),
    "hsefr_mtcnn_nms": (c_int, [_fp, c_int, ctypes.c_double, c_int, _fp, _fp, c_void_p]),
    "hsefr_mtcnn_crops": (c_int, [_fp, _fp, _fp, c_int, c_int, c_int, c_int, c_void_p]),
    "hsefr_mtcnn_pyramid_level_batch": (c_int, [_fp, _fp] + [c_int] * 5 + [c_void_p]),
    "hsefr_mtcnn_stage1_level_batch": (c_int, [_fp, _fp, c_int, c_int, c_int, ctypes.c_double, ctypes.c_float, _fp, _fp, c_void_p]),
    "hsefr_mtcnn_stage1_finish_batch": (c_int, [_fp, _fp, _fp, _fp, c_int, c_int, c_int, c_void_p]),
    "hsefr_mtcnn_crops_batch": (c_int, [_fp, _fp, _fp, _fp] + [c_int] * 5 + [c_void_p]),
    "hsefr_mtcnn_stage_finish_batch": (c_int, [c_int, _fp, _fp, c_int, _fp, _fp, _fp, ctypes.c_float, _fp, _fp, _fp, _fp, c_int, c_int, c_int, c_void_p]),
    "hsefr_pairwise_dist": (c_int, [_fp, _fp, c_int, c_int, c_int, _fp, c_void_p]),
    "hsefr_single_linkage": (c_int, [_fp, c_int, c_int, _fp, _fp, _fp, _fp, _fp, _fp, c_void_p]),
    "hsefr_hier_linkage": (c_int, [_fp, c_int, c_int, _fp, _fp, _fp, c_int, _fp, _fp, _fp, _fp, c_void_p]),
    "hsefr_dbscan": (c_int, [_fp, c_int, c_int, _fp, _fp, _fp, ctypes.c_double, c_int, _fp, _fp, c_void_p]),
    "hsefr_rank_order": (c_int, [_fp, c_int, c_int, _fp, _fp, _fp, ctypes.c_double, ctypes.c_double, _fp, POINTER(c_int), c_void_p]),
    "hsefr_rank_order_sweep": (c_int, [_fp, c_int, c_int, _fp, _fp, _fp, POINTER(ctypes.c_double), c_int, _fp, POINTER(c_int), c_void_p]),
    "hsefr_flat_cuts": (c_int, [_fp, _fp, c_int, _fp, c_int, _fp, c_void_p]),
    "hsefr_partition_scores": (c_int, [_fp, _fp, c_int, c_int, _fp, _fp, c_void_p]),
    "hsefr_nn1": (c_int, [_fp, _fp, c_int, c_int, c_int, _fp, _fp, c_void_p]),
    "hsefr_knn": (c_int, [_fp, _fp, c_int, c_int, c_int, c_int, _fp, _fp, _fp, _fp, c_void_p]),
    "hsefr_nn1_fallbacks": (c_longlong, []),
    "hsefr_metric_dist": (c_int, [_fp, _fp, c_int, c_int, c_int, c_int, _fp, c_void_p]),
    "hsefr_knn_metric": (c_int, [_fp, _fp, c_int, c_int, c_int, c_int, c_int, _fp, _fp, _fp, _fp, c_void_p]),
    "hsefr_pca_fit": (c_int, [_fp, c_int, c_int, c_int, c_int, _fp, _fp, _fp, _fp, c_void_p]),
    "hsefr_pca_transform": (c_int, [_fp, c_int, c_int, c_int, _fp, _fp, _fp, c_int, c_void_p]),
    "hsefr_linear_svm_fit": (c_int, [_fp, c_int, c_int, _fp, c_int, ctypes.c_double, ctypes.c_double, c_int, _fp, _fp, _fp, c_void_p]),
    "hsefr_linear_svm_decision": (c_int, [_fp, c_int, c_int, _fp, _fp, c_int, _fp, c_void_p]),
    "hsefr_linear_svm_predict": (c_int, [_fp, c_int, c_int, _fp, c_void_p]),
    "hsefr_rbf_svm_gamma_scale": (c_int, [_fp, c_int, c_int, c_int, _fp, c_void_p]),
    "hsefr_rbf_svm_fit": (c_int, [_fp, c_int, c_int, _fp, c_int, ctypes.c_double, ctypes.c_double, ctypes.c_double, c_int, _fp, _fp, _fp,
                                  c_void_p]),
    "hsefr_rbf_svm_decision": (c_int, [_fp, c_int, _fp, c_int, c_int, _fp, c_int, ctypes.c_double, _fp, _fp, _fp, c_void_p]),
    "hsefr_rbf_svm_predict": (c_int, [_fp, c_int, _fp, c_int, c_int, _fp, c_int, ctypes.c_double, _fp, _fp, _fp, _fp, c_void_p]),
}

# development builds only (csrc/hsefr_dev.h; build.sh with HSEFR_DEV=1): bound when the loaded library has them
DEV_SIGNATURES = {
    "hsefr_debug_set": (c_int, [c_char_p, c_int]),
    "hsefr_debug_read_stamps": (c_int, [c_int, c_void_p, ctypes.c_size_t]),
    "hsefr_debug_clock_probe": (c_int, [_fp, c_int, c_int, c_void_p]),
    "hsefr_debug_copy": (c_int, [_fp, _fp, c_size_t, c_void_p]),
    "hsefr_stem_fused": (c_int, [_fp] * 6 + [c_void_p, _fp, _fp, _fp] + [c_int] * 9 + [c_void_p]),     # round 1's stem: dev builds only since round 6
}


# libhsefr_album.so (include/hsefr_album.h): the album organiser's device code, a library of its own.  HSEFR_ALBUM_LIB selects another build
ALBUM_LIB_PATH = os.path.join(_HERE, os.environ.get("HSEFR_ALBUM_LIB", "libhsefr_album.so"))
_album_lib = None
ALBUM_SIGNATURES = {
    "hsefr_album_version": (c_int, []),
    "hsefr_album_last_error_string": (c_char_p, []),
    "hsefr_album_face_crops": (c_int, [_fp, c_int, c_int, c_int, c_void_p, c_int, _fp, c_int, c_int, c_void_p]),
}

# libhsefr_frames.so (include/hsefr_frames.h): the frame stack's channel swap and quarter turns, a third library.  HSEFR_FRAMES_LIB selects
# another build
FRAMES_LIB_PATH = os.path.join(_HERE, os.environ.get("HSEFR_FRAMES_LIB", "libhsefr_frames.so"))
_frames_lib = None
FRAMES_SIGNATURES = {
    "hsefr_frames_version": (c_int, []),
    "hsefr_frames_last_error_string": (c_char_p, []),
    "hsefr_frames_prepare": (c_int, [_fp, _fp, c_int, c_int, c_int, c_int, c_int, c_void_p]),
}

# libhsefr_forest.so (include/hsefr_forest.h): the random forest classifier, a fourth library.  HSEFR_FOREST_LIB selects another build
FOREST_LIB_PATH = os.path.join(_HERE, os.environ.get("HSEFR_FOREST_LIB", "libhsefr_forest.so"))
_forest_lib = None
FOREST_SIGNATURES = {
    "hsefr_forest_version": (c_int, []),
    "hsefr_forest_last_error_string": (c_char_p, []),
    "hsefr_forest_workspace_bytes": (c_size_t, [c_int] * 5),
    "hsefr_forest_fit": (c_int, [_fp, c_int, c_int, _fp] + [c_int] * 5 + [c_longlong, c_int] + [_fp] * 12 + [c_size_t, c_void_p]),
    "hsefr_forest_predict": (c_int, [_fp] + [c_int] * 6 + [_fp] * 11 + [c_void_p]),
}

# libhsefr_ragged.so (include/hsefr_ragged.h): one detector pass over frames of different sizes, a fifth library.  HSEFR_RAGGED_LIB selects
# another build
RAGGED_LIB_PATH = os.path.join(_HERE, os.environ.get("HSEFR_RAGGED_LIB", "libhsefr_ragged.so"))
_ragged_lib = None
_i64 = ctypes.c_int64
RAGGED_SIGNATURES = {
    "hsefr_ragged_version": (c_int, []),
    "hsefr_ragged_last_error_string": (c_char_p, []),
    "hsefr_ragged_capacity": (c_int, []),
    "hsefr_ragged_pyramid": (c_int, [_fp, _i64, _fp, c_int, _fp, c_int, _fp, c_int, _fp, _i64, c_int, c_void_p]),
    "hsefr_ragged_conv2d": (c_int, [_fp, _i64, _fp, _fp, _fp, _fp, _i64, _fp, c_int, _fp, c_int] + [c_int] * 8 + [c_void_p]),
    "hsefr_ragged_maxpool": (c_int, [_fp, _i64, _fp, _i64, _fp, c_int, _fp, c_int, c_int, c_int, c_int, c_void_p]),
    "hsefr_ragged_stage1": (c_int, [_fp, _fp, _i64, _fp, c_int, _fp, c_int, ctypes.c_float, _fp, _fp, _fp, _fp, c_void_p]),
    "hsefr_ragged_crops": (c_int, [_fp, _i64, _fp, c_int, _fp, _fp, _fp, c_int, c_int, c_int, c_void_p]),
    "hsefr_ragged_stage_finish": (c_int, [c_int, _fp, _fp, c_int, _fp, _fp, _fp, ctypes.c_float, _fp, _fp, _fp, _fp, _fp, c_int, c_void_p]),
}

# libhsefr_mixed.so (include/hsefr_mixed.h): a mixed-size pass's frames turned, converted and cropped on the device, a sixth library.
# HSEFR_MIXED_LIB selects another build.  The two tables are HOST pointers (c_void_p: a NumPy array's ctypes.data)
MIXED_LIB_PATH = os.path.join(_HERE, os.environ.get("HSEFR_MIXED_LIB", "libhsefr_mixed.so"))
_mixed_lib = None
MIXED_SIGNATURES = {
    "hsefr_mixed_version": (c_int, []),
    "hsefr_mixed_last_error_string": (c_char_p, []),
    "hsefr_mixed_frames_prepare": (c_int, [_fp, _fp, _i64, c_void_p, c_int, c_int, c_int, c_void_p]),
    "hsefr_mixed_face_crops": (c_int, [_fp, _i64, c_void_p, c_int, c_void_p, c_int, _fp, c_int, c_int, c_void_p]),
}

# libhsefr_split.so (include/hsefr_split.h): the same-photo split of every cluster of a clustering in one pass, a seventh library.
# HSEFR_SPLIT_LIB selects another build.  The offset table is a HOST pointer (c_void_p: a NumPy array's ctypes.data)
SPLIT_LIB_PATH = os.path.join(_HERE, os.environ.get("HSEFR_SPLIT_LIB", "libhsefr_split.so"))
_split_lib = None
SPLIT_SIGNATURES = {
    "hsefr_split_version": (c_int, []),
    "hsefr_split_last_error": (c_char_p, []),
    "hsefr_split_groups": (c_int, [_fp, c_int, c_int, _fp, _fp, _fp, _fp, c_void_p, c_int, _fp, ctypes.c_double, ctypes.c_double, _fp, _fp,
                                   _fp, c_void_p]),
}

# libhsefr_geom.so (include/hsefr_geom.h): centroid, median and Ward linkage, an eighth library.  HSEFR_GEOM_LIB selects another build
GEOM_LIB_PATH = os.path.join(_HERE, os.environ.get("HSEFR_GEOM_LIB", "libhsefr_geom.so"))
_geom_lib = None
GEOM_SIGNATURES = {
    "hsefr_geom_version": (c_int, []),
    "hsefr_geom_last_error": (c_char_p, []),
    "hsefr_geom_linkage": (c_int, [_fp, c_int, c_int, _fp, _fp, _fp, c_int, _fp, _fp, _fp, _fp, _fp, _fp, c_void_p]),
}


class HsefrError(RuntimeError):
    pass


def lib() -> ctypes.CDLL:
    """Load libhsefr.so once.  torch is imported first on purpose: the library's DT_NEEDED
    libamdhip64.so.7 must resolve to the HIP runtime PyTorch already mapped, so that torch
    streams and ``data_ptr()`` addresses belong to the same runtime instance."""
    global _lib
    if _lib is None:
        import torch  # noqa: F401  (side effect: maps torch's libamdhip64)
        if not os.path.exists(LIB_PATH):
            raise ImportError("%s is missing: build it with `python -c 'import __graft_entry__ as g; g.build()'` "
                              "(hipcc --offload-arch=gfx950). There is no CPU fallback." % LIB_PATH)
        L = ctypes.CDLL(LIB_PATH)
        for name, (res, args) in SIGNATURES.items():
            fn = getattr(L, name)
            fn.restype = res
            fn.argtypes = args
        for name, (res, args) in DEV_SIGNATURES.items():
            if hasattr(L, name):
                fn = getattr(L, name)
                fn.restype = res
                fn.argtypes = args
        _lib = L
    return _lib


def album_lib() -> ctypes.CDLL:
    """Load libhsefr_album.so once (torch first, as lib() does and for the same reason).  Missing is an error: there is no fallback."""
    global _album_lib
    if _album_lib is None:
        import torch  # noqa: F401
        if not os.path.exists(ALBUM_LIB_PATH):
            raise ImportError("%s is missing: build it with `python -c 'import __graft_entry__ as g; g.build()'` "
                              "(hipcc --offload-arch=gfx950). There is no CPU fallback." % ALBUM_LIB_PATH)
        L = ctypes.CDLL(ALBUM_LIB_PATH)
        for name, (res, args) in ALBUM_SIGNATURES.items():
            fn = getattr(L, name)
            fn.restype = res
            fn.argtypes = args
        _album_lib = L
    return _album_lib


def album_last_error() -> str:
    s = album_lib().hsefr_album_last_error_string()
    return s.decode("utf-8", "replace") if s else ""


def album_check(status: int, what: str = "") -> None:
    """check() for a status of libhsefr_album.so (its own error string)."""
    if status != OK:
        _raise(status, "%s%s (hsefr_album status %d)" % (what + ": " if what else "", album_last_error(), status))


def frames_lib() -> ctypes.CDLL:
    """Load libhsefr_frames.so once (torch first, as lib() does and for the same reason).  Missing is an error: there is no fallback."""
    global _frames_lib
    if _frames_lib is None:
        import torch  # noqa: F401
        if not os.path.exists(FRAMES_LIB_PATH):
            raise ImportError("%s is missing: build it with `python -c 'import __graft_entry__ as g; g.build()'` "
                              "(hipcc --offload-arch=gfx950). There is no CPU fallback." % FRAMES_LIB_PATH)
        L = ctypes.CDLL(FRAMES_LIB_PATH)
        for name, (res, args) in FRAMES_SIGNATURES.items():
            fn = getattr(L, name)
            fn.restype = res
            fn.argtypes = args
        _frames_lib = L
    return _frames_lib


def frames_last_error() -> str:
    s = frames_lib().hsefr_frames_last_error_string()
    return s.decode("utf-8", "replace") if s else ""


def frames_check(status: int, what: str = "") -> None:
    """check() for a status of libhsefr_frames.so (its own error string)."""
    if status != OK:
        _raise(status, "%s%s (hsefr_frames status %d)" % (what + ": " if what else "", frames_last_error(), status))


def forest_lib() -> ctypes.CDLL:
    """Load libhsefr_forest.so once (torch first, as lib() does and for the same reason).  Missing is an error: there is no fallback."""
    global _forest_lib
    if _forest_lib is None:
        import torch  # noqa: F401
        if not os.path.exists(FOREST_LIB_PATH):
            raise ImportError("%s is missing: build it with `python -c 'import __graft_entry__ as g; g.build()'` "
                              "(hipcc --offload-arch=gfx950). There is no CPU fallback." % FOREST_LIB_PATH)
        L = ctypes.CDLL(FOREST_LIB_PATH)
        for name, (res, args) in FOREST_SIGNATURES.items():
            fn = getattr(L, name)
            fn.restype = res
            fn.argtypes = args
        _forest_lib = L
    return _forest_lib


def forest_last_error() -> str:
    s = forest_lib().hsefr_forest_last_error_string()
    return s.decode("utf-8", "replace") if s else ""


def forest_check(status: int, what: str = "") -> None:
    """check() for a status of libhsefr_forest.so (its own error string)."""
    if status != OK:
        _raise(status, "%s%s (hsefr_forest status %d)" % (what + ": " if what else "", forest_last_error(), status))


def ragged_lib() -> ctypes.CDLL:
    """Load libhsefr_ragged.so once (torch first, as lib() does and for the same reason).  Missing is an error: there is no fallback."""
    global _ragged_lib
    if _ragged_lib is None:
        import torch  # noqa: F401
        if not os.path.exists(RAGGED_LIB_PATH):
            raise ImportError("%s is missing: build it with `python -c 'import __graft_entry__ as g; g.build()'` "
                              "(hipcc --offload-arch=gfx950). There is no CPU fallback." % RAGGED_LIB_PATH)
        L = ctypes.CDLL(RAGGED_LIB_PATH)
        for name, (res, args) in RAGGED_SIGNATURES.items():
            fn = getattr(L, name)
            fn.restype = res
            fn.argtypes = args
        _ragged_lib = L
    return _ragged_lib


def ragged_last_error() -> str:
    s = ragged_lib().hsefr_ragged_last_error_string()
    return s.decode("utf-8", "replace") if s else ""


def ragged_check(status: int, what: str = "") -> None:
    """check() for a status of libhsefr_ragged.so (its own error string)."""
    if status != OK:
        _raise(status, "%s%s (hsefr_ragged status %d)" % (what + ": " if what else "", ragged_last_error(), status))


def mixed_lib() -> ctypes.CDLL:
    """Load libhsefr_mixed.so once (torch first, as lib() does and for the same reason).  Missing is an error: there is no fallback."""
    global _mixed_lib
    if _mixed_lib is None:
        import torch  # noqa: F401
        if not os.path.exists(MIXED_LIB_PATH):
            raise ImportError("%s is missing: build it with `python -c 'import __graft_entry__ as g; g.build()'` "
                              "(hipcc --offload-arch=gfx950). There is no CPU fallback." % MIXED_LIB_PATH)
        L = ctypes.CDLL(MIXED_LIB_PATH)
        for name, (res, args) in MIXED_SIGNATURES.items():
            fn = getattr(L, name)
            fn.restype = res
            fn.argtypes = args
        _mixed_lib = L
    return _mixed_lib


def mixed_last_error() -> str:
    s = mixed_lib().hsefr_mixed_last_error_string()
    return s.decode("utf-8", "replace") if s else ""


def mixed_check(status: int, what: str = "") -> None:
    """check() for a status of libhsefr_mixed.so (its own error string)."""
    if status != OK:
        _raise(status, "%s%s (hsefr_mixed status %d)" % (what + ": " if what else "", mixed_last_error(), status))


def split_lib() -> ctypes.CDLL:
    """Load libhsefr_split.so once (torch first, as lib() does and for the same reason).  Missing is an error: there is no fallback."""
    global _split_lib
    if _split_lib is None:
        import torch  # noqa: F401
        if not os.path.exists(SPLIT_LIB_PATH):
            raise ImportError("%s is missing: build it with `python -c 'import __graft_entry__ as g; g.build()'` "
                              "(hipcc --offload-arch=gfx950). There is no CPU fallback." % SPLIT_LIB_PATH)
        L = ctypes.CDLL(SPLIT_LIB_PATH)
        for name, (res, args) in SPLIT_SIGNATURES.items():
            fn = getattr(L, name)
            fn.restype = res
            fn.argtypes = args
        _split_lib = L
    return _split_lib


def split_last_error() -> str:
    s = split_lib().hsefr_split_last_error()
    return s.decode("utf-8", "replace") if s else ""


def split_check(status: int, what: str = "") -> None:
    """check() for a status of libhsefr_split.so (its own error string)."""
    if status != OK:
        _raise(status, "%s%s (hsefr_split status %d)" % (what + ": " if what else "", split_last_error(), status))


def geom_lib() -> ctypes.CDLL:
    """Load libhsefr_geom.so once (torch first, as lib() does and for the same reason).  Missing is an error: there is no fallback."""
    global _geom_lib
    if _geom_lib is None:
        import torch  # noqa: F401
        if not os.path.exists(GEOM_LIB_PATH):
            raise ImportError("%s is missing: build it with `python -c 'import __graft_entry__ as g; g.build()'` "
                              "(hipcc --offload-arch=gfx950). There is no CPU fallback." % GEOM_LIB_PATH)
        L = ctypes.CDLL(GEOM_LIB_PATH)
        for name, (res, args) in GEOM_SIGNATURES.items():
            fn = getattr(L, name)
            fn.restype = res
            fn.argtypes = args
        _geom_lib = L
    return _geom_lib


def geom_last_error() -> str:
    s = geom_lib().hsefr_geom_last_error()
    return s.decode("utf-8", "replace") if s else ""


def geom_check(status: int, what: str = "") -> None:
    """check() for a status of libhsefr_geom.so (its own error string)."""
    if status != OK:
        _raise(status, "%s%s (hsefr_geom status %d)" % (what + ": " if what else "", geom_last_error(), status))


def last_error() -> str:
    s = lib().hsefr_last_error_string()
    return s.decode("utf-8", "replace") if s else ""


def check(status: int, what: str = "") -> None:
    if status == OK:
        return
    _raise(status, "%s%s (hsefr status %d)" % (what + ": " if what else "", last_error(), status))


def _raise(status: int, msg: str) -> None:
    if status == ERR_SHAPE or status == ERR_INVALID:
        raise ValueError(msg)
    if status == ERR_UNSUPPORTED:
        raise NotImplementedError(msg)
    if status == ERR_NOMEM:
        raise MemoryError(msg)
    raise HsefrError(msg)


_torch_gpu = None      # torch, once a GPU has been seen (torch.cuda.is_available() re-reads the environment on every call: the
                       # small-net paths make ~100 launches per frame and spent a tenth of their host time asking)


def require_gpu():
    """The product path runs on an MI355X or not at all."""
    global _torch_gpu
    if _torch_gpu is None:
        import torch
        if not torch.cuda.is_available():
            raise RuntimeError("hse_facerec_tf_amd needs a ROCm GPU (gfx950); torch.cuda.is_available() is False "
                               "and there is no CPU fallback")
        _torch_gpu = torch
    return _torch_gpu


def current_stream_ptr() -> int:
    """The current torch stream OF THE CURRENT DEVICE: callers launch under ``on_device(tensor)`` so that the
    current device is the one that owns the pointers they pass."""
    import torch
    try:        # the raw handle without building a torch.cuda.Stream object (what torch's own compiled code paths call)
        return torch._C._cuda_getCurrentRawStream(torch._C._cuda_getDevice())
    except AttributeError:
        return torch.cuda.current_stream().cuda_stream


def cuda_device(device=None):
    """None -> the current device; an index, 'cuda:1' or torch.device -> torch.device('cuda', index)."""
    torch = require_gpu()
    if device is None:
        return torch.device("cuda", torch.cuda.current_device())
    d = torch.device("cuda", device) if isinstance(device, int) else torch.device(device)
    if d.type != "cuda":
        raise ValueError("hse_facerec_tf_amd runs on a ROCm GPU, not on %r" % (device,))
    return torch.device("cuda", torch.cuda.current_device() if d.index is None else d.index)


def on_device(t):
    """Context manager: make the device that owns tensor ``t`` (or the given torch.device) current, so that the
    stream handed to libhsefr and the HIP launch target match the pointers (a launch under device 0
    on device-1 pointers is a memory fault, not an exception)."""
    import torch
    dev = t.device if hasattr(t, "device") else t
    try:        # already current (the usual case): nothing to switch, nothing to restore
        if isinstance(dev, torch.device) and dev.index is not None and dev.index == torch._C._cuda_getDevice():
            return _NO_SWITCH
    except AttributeError:
        pass
    return torch.cuda.device(dev)


class _NoSwitch:
    def __enter__(self):
        return self

    def __exit__(self, *exc):
        return False


_NO_SWITCH = _NoSwitch()
