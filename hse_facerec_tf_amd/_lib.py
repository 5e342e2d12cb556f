"""ctypes binding of libhsefr.so (include/hsefr.h) and of the libraries built beside it (include/hsefr_<name>.h), each described by
one Library record in LIBRARIES.  No fallback: if a library is missing the import of anything that needs it raises, and every non-zero
status becomes a Python exception in the reference's error style (ValueError for shape errors, NotImplementedError for unsupported
graphs, RuntimeError otherwise).

A new library is a record in LIBRARIES with its line of module-level names, a row of csrc/build.sh's table at the same place, a header
under include/ and a row of FLOORS in tests/test_libraries_cpu.py."""
from __future__ import annotations

import ctypes
import os
from ctypes import POINTER, c_char_p, c_float, c_int, c_longlong, c_size_t, c_void_p

_HERE = os.path.dirname(os.path.abspath(__file__))

OK, ERR_INVALID, ERR_UNSUPPORTED, ERR_HIP, ERR_NOMEM, ERR_SHAPE = 0, -1, -2, -3, -4, -5


class HsefrError(RuntimeError):
    pass


class Library:
    """One shared library of the package: where it lies, what it exports and how it reports an error.

    ``tag`` stands in messages ("... (hsefr_album status -1)"), ``env`` names the variable that selects another build of the file,
    ``signatures`` is name -> (restype, argtypes) with one row per declaration in the public header, ``optional`` the same for names
    bound only when the loaded file has them, ``error_fn`` and ``version_fn`` name the error-string and version functions, and
    ``version`` is what the latter must return."""

    def __init__(self, tag, file, env, signatures, error_fn, version_fn, version, optional=None):
        self.tag, self.file, self.env, self.signatures, self.optional = tag, file, env, signatures, optional or {}
        self.error_fn, self.version_fn, self.version = error_fn, version_fn, version
        self.path = os.path.join(_HERE, os.environ.get(env, file))
        self._handle = None

    def load(self) -> ctypes.CDLL:
        """Load the library once.  torch is imported first on purpose: the library's DT_NEEDED libamdhip64.so.7 must resolve to the
        HIP runtime PyTorch already mapped, so that torch streams and ``data_ptr()`` addresses belong to the same runtime instance.
        Missing is an error: there is no fallback."""
        if self._handle is None:
            import torch  # noqa: F401  (side effect: maps torch's libamdhip64)
            if not os.path.exists(self.path):
                raise ImportError("%s is missing: build it with `python -c 'import __graft_entry__ as g; g.build()'` "
                                  "(hipcc --offload-arch=gfx950). There is no CPU fallback." % self.path)
            L = ctypes.CDLL(self.path)
            for table, required in ((self.signatures, True), (self.optional, False)):
                for name, (res, args) in table.items():
                    if required or hasattr(L, name):
                        fn = getattr(L, name)
                        fn.restype = res
                        fn.argtypes = args
            self._handle = L
        return self._handle

    def last_error(self) -> str:
        s = getattr(self.load(), self.error_fn)()
        return s.decode("utf-8", "replace") if s else ""

    def check(self, status: int, what: str = "") -> None:
        """Raise for a non-zero status of this library, with its own error string."""
        if status != OK:
            _raise(status, "%s%s (%s status %d)" % (what + ": " if what else "", self.last_error(), self.tag, status))


def _raise(status: int, msg: str) -> None:
    if status == ERR_SHAPE or status == ERR_INVALID:
        raise ValueError(msg)
    if status == ERR_UNSUPPORTED:
        raise NotImplementedError(msg)
    if status == ERR_NOMEM:
        raise MemoryError(msg)
    raise HsefrError(msg)


# ---- libhsefr.so.  HSEFR_LIB selects another build of it (e.g. libhsefr_dev.so for tools/kbench.py)
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

# ---- the later libraries, each with its own header, version and error string; HSEFR_<NAME>_LIB selects another build of one
# libhsefr_album.so (include/hsefr_album.h): the album organiser's device code
ALBUM_SIGNATURES = {
    "hsefr_album_version": (c_int, []),
    "hsefr_album_last_error_string": (c_char_p, []),
    "hsefr_album_face_crops": (c_int, [_fp, c_int, c_int, c_int, c_void_p, c_int, _fp, c_int, c_int, c_void_p]),
}

# libhsefr_frames.so (include/hsefr_frames.h): the frame stack's channel swap and quarter turns
FRAMES_SIGNATURES = {
    "hsefr_frames_version": (c_int, []),
    "hsefr_frames_last_error_string": (c_char_p, []),
    "hsefr_frames_prepare": (c_int, [_fp, _fp, c_int, c_int, c_int, c_int, c_int, c_void_p]),
}

# libhsefr_forest.so (include/hsefr_forest.h): the random forest classifier
FOREST_SIGNATURES = {
    "hsefr_forest_version": (c_int, []),
    "hsefr_forest_last_error_string": (c_char_p, []),
    "hsefr_forest_workspace_bytes": (c_size_t, [c_int] * 5),
    "hsefr_forest_fit": (c_int, [_fp, c_int, c_int, _fp] + [c_int] * 5 + [c_longlong, c_int] + [_fp] * 12 + [c_size_t, c_void_p]),
    "hsefr_forest_predict": (c_int, [_fp] + [c_int] * 6 + [_fp] * 11 + [c_void_p]),
}

# libhsefr_ragged.so (include/hsefr_ragged.h): one detector pass over frames of different sizes
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

# libhsefr_mixed.so (include/hsefr_mixed.h): a mixed-size pass's frames turned, converted and cropped on the device.  The two tables
# are HOST pointers (c_void_p: a NumPy array's ctypes.data)
MIXED_SIGNATURES = {
    "hsefr_mixed_version": (c_int, []),
    "hsefr_mixed_last_error_string": (c_char_p, []),
    "hsefr_mixed_frames_prepare": (c_int, [_fp, _fp, _i64, c_void_p, c_int, c_int, c_int, c_void_p]),
    "hsefr_mixed_face_crops": (c_int, [_fp, _i64, c_void_p, c_int, c_void_p, c_int, _fp, c_int, c_int, c_void_p]),
}

# libhsefr_split.so (include/hsefr_split.h): the same-photo split of every cluster of a clustering in one pass.  The offset table is
# a HOST pointer (c_void_p: a NumPy array's ctypes.data)
SPLIT_SIGNATURES = {
    "hsefr_split_version": (c_int, []),
    "hsefr_split_last_error": (c_char_p, []),
    "hsefr_split_groups": (c_int, [_fp, c_int, c_int, _fp, _fp, _fp, _fp, c_void_p, c_int, _fp, ctypes.c_double, ctypes.c_double, _fp, _fp,
                                   _fp, c_void_p]),
}

# libhsefr_geom.so (include/hsefr_geom.h): centroid, median and Ward linkage
GEOM_SIGNATURES = {
    "hsefr_geom_version": (c_int, []),
    "hsefr_geom_last_error": (c_char_p, []),
    "hsefr_geom_linkage": (c_int, [_fp, c_int, c_int, _fp, _fp, _fp, c_int, _fp, _fp, _fp, _fp, _fp, _fp, c_void_p]),
}

# libhsefr_shift.so (include/hsefr_shift.h): mean-shift clustering
_i32p = _fp
SHIFT_SIGNATURES = {
    "hsefr_shift_version": (c_int, []),
    "hsefr_shift_last_error": (c_char_p, []),
    "hsefr_shift_workspace_bytes": (c_size_t, [c_int, c_int]),
    "hsefr_shift_fit": (c_int, [_fp, c_int, c_int, ctypes.c_double, c_int, _fp, _i32p, _i32p, _fp, _i32p, _fp, c_size_t, c_void_p]),
    "hsefr_shift_assign": (c_int, [_fp, c_int, c_int, _fp, c_int, _i32p, _fp, c_void_p]),
}

# libhsefr_affinity.so (include/hsefr_affinity.h): affinity-propagation clustering
_f64, _ll = ctypes.c_double, c_longlong
_AFFINITY_TAIL = [_f64, c_int, c_int, _f64, _ll, _i32p, _i32p, _fp, _fp, _i32p, _fp, c_size_t, c_void_p]
AFFINITY_SIGNATURES = {
    "hsefr_affinity_version": (c_int, []),
    "hsefr_affinity_last_error": (c_char_p, []),
    "hsefr_affinity_workspace_bytes": (c_size_t, [c_int, c_int]),
    "hsefr_affinity_fit": (c_int, [_fp, c_int, c_int] + _AFFINITY_TAIL),
    "hsefr_affinity_fit_dense": (c_int, [_fp, c_int] + _AFFINITY_TAIL),
}


def _later(name, signatures, error_fn):
    return Library("hsefr_" + name, "libhsefr_%s.so" % name, "HSEFR_%s_LIB" % name.upper(), signatures, error_fn, "hsefr_%s_version" % name, 100)


# every library, in build order (csrc/build.sh's table has the same rows; tests/test_libraries_cpu.py holds the two together)
LIBRARIES = (
    Library("hsefr", "libhsefr.so", "HSEFR_LIB", SIGNATURES, "hsefr_last_error_string", "hsefr_version", 141, optional=DEV_SIGNATURES),
    _later("album", ALBUM_SIGNATURES, "hsefr_album_last_error_string"),
    _later("frames", FRAMES_SIGNATURES, "hsefr_frames_last_error_string"),
    _later("forest", FOREST_SIGNATURES, "hsefr_forest_last_error_string"),
    _later("ragged", RAGGED_SIGNATURES, "hsefr_ragged_last_error_string"),
    _later("mixed", MIXED_SIGNATURES, "hsefr_mixed_last_error_string"),
    _later("split", SPLIT_SIGNATURES, "hsefr_split_last_error"),
    _later("geom", GEOM_SIGNATURES, "hsefr_geom_last_error"),
    _later("shift", SHIFT_SIGNATURES, "hsefr_shift_last_error"),
    _later("affinity", AFFINITY_SIGNATURES, "hsefr_affinity_last_error"),
)
_MAIN, _ALBUM, _FRAMES, _FOREST, _RAGGED, _MIXED, _SPLIT, _GEOM, _SHIFT, _AFFINITY = LIBRARIES

# the module-level names of each library.  Callers go through the module attribute at call time (_lib.frames_lib()), so a test can put
# another function in its place
LIB_PATH, lib, last_error, check = _MAIN.path, _MAIN.load, _MAIN.last_error, _MAIN.check
ALBUM_LIB_PATH, album_lib, album_last_error, album_check = _ALBUM.path, _ALBUM.load, _ALBUM.last_error, _ALBUM.check
FRAMES_LIB_PATH, frames_lib, frames_last_error, frames_check = _FRAMES.path, _FRAMES.load, _FRAMES.last_error, _FRAMES.check
FOREST_LIB_PATH, forest_lib, forest_last_error, forest_check = _FOREST.path, _FOREST.load, _FOREST.last_error, _FOREST.check
RAGGED_LIB_PATH, ragged_lib, ragged_last_error, ragged_check = _RAGGED.path, _RAGGED.load, _RAGGED.last_error, _RAGGED.check
MIXED_LIB_PATH, mixed_lib, mixed_last_error, mixed_check = _MIXED.path, _MIXED.load, _MIXED.last_error, _MIXED.check
SPLIT_LIB_PATH, split_lib, split_last_error, split_check = _SPLIT.path, _SPLIT.load, _SPLIT.last_error, _SPLIT.check
GEOM_LIB_PATH, geom_lib, geom_last_error, geom_check = _GEOM.path, _GEOM.load, _GEOM.last_error, _GEOM.check
SHIFT_LIB_PATH, shift_lib, shift_last_error, shift_check = _SHIFT.path, _SHIFT.load, _SHIFT.last_error, _SHIFT.check
AFFINITY_LIB_PATH, affinity_lib, affinity_last_error, affinity_check = _AFFINITY.path, _AFFINITY.load, _AFFINITY.last_error, _AFFINITY.check


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
