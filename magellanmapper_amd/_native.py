"""ctypes binding of ``libmmx_hip.so`` (the C ABI declared in ``include/mmx.h``).

There is NO CPU fallback: if the shared library is missing or a call fails the
functions raise.  Build the library with ``python -c "import __graft_entry__ as g; g.build()"``
or ``make -C magellanmapper_amd/csrc -j8``.
"""
from __future__ import annotations

import ctypes
import os
from ctypes import (POINTER, Structure, c_char_p, c_double, c_float, c_int, c_int32, c_int64,
                    c_uint8, c_uint32, c_void_p)

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
#: ``MMX_LIB_PATH`` selects an experimental build of the same ABI (kernel tuning only)
LIB_PATH = os.environ.get("MMX_LIB_PATH") or os.path.join(_HERE, "libmmx_hip.so")

MMX_ABI_VERSION = 21
MMX_U8, MMX_U16, MMX_F32, MMX_F64, MMX_I16 = 0, 1, 2, 3, 4
#: THE voxel-type table (``mmx_voxel_table`` of csrc/mmx_voxel.h states the same for the kernels), in code order:
#: (mmx_dtype code, NumPy dtype, name of the torch dtype -- this module does not import torch --, integer, signed).
#: Every dtype map and every tuple of accepted dtypes in the package is a view of it.
VOXEL_TYPES = (
    (MMX_U8, np.dtype(np.uint8), "uint8", True, False),
    (MMX_U16, np.dtype(np.uint16), "uint16", True, False),
    (MMX_F32, np.dtype(np.float32), "float32", False, True),
    (MMX_F64, np.dtype(np.float64), "float64", False, True),
    (MMX_I16, np.dtype(np.int16), "int16", True, True),
)
NP_TO_MMX = {v[1]: v[0] for v in VOXEL_TYPES}
MMX_TO_NP = {v[0]: v[1] for v in VOXEL_TYPES}
MMX_TO_TORCH_NAME = {v[0]: v[2] for v in VOXEL_TYPES}


def voxel_dtypes(integer):
    """The NumPy dtypes of the integer (``True``) or the float (``False``) voxel types, in code order."""
    return tuple(v[1] for v in VOXEL_TYPES if v[3] == integer)


MMX_MAX_RADIUS_FAST = 24
MMX_MAX_RADIUS_WIDE = 64
MMX_MAX_RADIUS_GENERIC = 255
MMX_CAND_CONTESTED = 1
MMX_CAND_BAND = 2
MMX_CAND_PROBE = 4
#: ``mmx_zx_mode``: how mmx_log_batch_f32 runs its Z and X passes (a per-call argument)
MMX_ZX_AUTO, MMX_ZX_SEPARATE, MMX_ZX_PACKED, MMX_ZX_MFMA_F32, MMX_ZX_MFMA_F16, MMX_ZX_MFMA_F16_LDS = -1, 0, 2, 3, 4, 5
MMX_ZX_TILED, MMX_ZX_TILED_Q16, MMX_ZX_PREPACKED, MMX_ZX_Y_VALU = 6, 7, 0x100, 0x200
MMX_ZX_EDGE_GLOBAL = 0x400
MMX_ZX_ROWS_SHIFT = 12
MMX_ZX_ROWS_MASK = 0xF000


def MMX_ZX_ROWS(n):
    """zx flag field: n rows per wave of the Z+X row march in every block (0: chosen per block of the launch)."""
    return int(n) << MMX_ZX_ROWS_SHIFT


MMX_ZX_WIDE = 8
#: by name only: the separate passes with the folded-reflection pass where a block is shorter than the kernel
MMX_ZX_THIN = 9
#: longest extent the folded passes fold (``MMX_FOLD_MAX_N``); a longer axis runs the generic tap loop
MMX_FOLD_MAX_N = 68
#: NMS entry layouts ``mmx_log_batch_f32`` reports and ``mmx_peaks_batch`` takes
MMX_MASK_ROWS, MMX_MASK_QUADS = 1, 2
MMX_MAX_BLOCKS = 65535
MMX_COLOC_BALL = 33
#: largest patch size ``mmx_extract_patches`` takes
MMX_PATCH_MAX_SIZE = 4096

#: NumPy mirror of ``mmx_block`` (32 bytes).
BLOCK_DTYPE = np.dtype([("src_off", "<i8"), ("nz", "<i4"), ("ny", "<i4"), ("nx", "<i4"),
                        ("slot", "<i4"), ("px", "<i4"), ("_pad", "<i4")], align=True)
MMX_ROW_ALIGN = 32
#: NumPy mirror of ``mmx_cand`` (48 bytes).
CAND_DTYPE = np.dtype([("slot", "<i4"), ("s", "<i4"), ("z", "<i4"), ("y", "<i4"), ("x", "<i4"),
                       ("flags", "<u4"), ("v", "<f4"), ("nbr_max", "<f4"), ("v64", "<f8"),
                       ("band", "<u8")], align=True)
assert BLOCK_DTYPE.itemsize == 32 and CAND_DTYPE.itemsize == 48
#: NumPy mirror of ``mmx_part`` (40 bytes): one part of a block that is detected as several (``mmx_fold_parts``)
PART_DTYPE = np.dtype([("parent", "<i4"), ("off", "<i4", (3,)), ("core_lo", "<i4", (3,)), ("core_hi", "<i4", (3,))],
                      align=True)
assert PART_DTYPE.itemsize == 40
#: NumPy mirrors of ``mmx_subblock`` (40 bytes), ``mmx_quantile_class`` (32), ``mmx_subblock_info`` (32)
SUBBLOCK_DTYPE = np.dtype([("src_off", "<i8"), ("dst_off", "<i8"), ("scratch_off", "<i8"),
                           ("nz", "<i4"), ("ny", "<i4"), ("nx", "<i4"), ("qclass", "<i4")], align=True)
QCLASS_DTYPE = np.dtype([("lo_prev", "<i4"), ("lo_next", "<i4"), ("hi_prev", "<i4"), ("hi_next", "<i4"),
                         ("lo_gamma", "<f8"), ("hi_gamma", "<f8")], align=True)
SUBINFO_DTYPE = np.dtype([("vmin", "<f8"), ("vmax", "<f8"), ("mean", "<f8"), ("flags", "<i4"),
                          ("_pad", "<i4")], align=True)
assert SUBBLOCK_DTYPE.itemsize == 40 and QCLASS_DTYPE.itemsize == 32 and SUBINFO_DTYPE.itemsize == 32
MMX_PP_IDENTITY, MMX_PP_ERODED, MMX_PP_EXACT_MEAN = 1, 2, 4
MMX_PP_AUTO, MMX_PP_SINGLE, MMX_PP_PIPELINED = 0, 1, 2     # kernel choice of mmx_preprocess_batch_mode
#: NumPy mirror of ``mmx_resize_block`` (48 bytes)
RESIZE_DTYPE = np.dtype([("src_off", "<i8"), ("in_nz", "<i4"), ("in_ny", "<i4"), ("in_nx", "<i4"),
                         ("out_nz", "<i4"), ("out_ny", "<i4"), ("out_nx", "<i4"), ("slot", "<i4"),
                         ("tz", "<i4"), ("ty", "<i4"), ("tx", "<i4")], align=True)
assert RESIZE_DTYPE.itemsize == 48
#: NumPy mirror of ``mmx_rank_group`` (40 bytes): planes ``[z0, z1)`` and four 0-based ranks into their sorted voxels
RANK_GROUP_DTYPE = np.dtype([("z0", "<i4"), ("z1", "<i4"), ("rank", "<i8", (4,))], align=True)
assert RANK_GROUP_DTYPE.itemsize == 40
#: NumPy mirror of ``mmx_ds_chunk`` (64 bytes): one chunk of a down-sampling batch
DS_CHUNK_DTYPE = np.dtype([("src_off", "<i8"), ("dst_off", "<i8"), ("in_nz", "<i4"), ("in_ny", "<i4"), ("in_nx", "<i4"),
                           ("out_nz", "<i4"), ("out_ny", "<i4"), ("out_nx", "<i4"), ("slot", "<i4"),
                           ("tz", "<i4"), ("ty", "<i4"), ("tx", "<i4"), ("_pad", "<i4", (2,))], align=True)
assert DS_CHUNK_DTYPE.itemsize == 64


class Volume(Structure):
    """``mmx_volume``."""
    _fields_ = [("d_data", c_void_p), ("dtype", c_int32), ("value_range", c_float),
                ("stride_z", c_int64), ("stride_y", c_int64), ("stride_x", c_int64)]


class DsView(Structure):
    """``mmx_ds_view``: one channel of the source or the destination of a down-sampling batch."""
    _fields_ = [("d_data", c_void_p), ("dtype", c_int32), ("_pad", c_int32),
                ("stride_z", c_int64), ("stride_y", c_int64), ("stride_x", c_int64)]


class EqGeom(Structure):
    """``mmx_eq_geom``: extent, kernel size, histogram tiles per axis and bins of one equalisation."""
    _fields_ = [("n", c_int32 * 3), ("k", c_int32 * 3), ("nt", c_int32 * 3), ("nbins", c_int32), ("_pad", c_int32 * 2)]


class DetectArgs(Structure):
    """``mmx_detect_args`` (one batch from voxels to the re-scored candidate table: ``mmx_detect_batch``)."""
    _fields_ = [("vol32", POINTER(Volume)), ("vol_exact", POINTER(Volume)), ("d_blocks", c_void_p),
                ("h_blocks", c_void_p), ("n_blocks", c_int32), ("n_sigma", c_int32), ("slot_elems", c_int64),
                ("h_w0", c_void_p), ("h_w2", c_void_p), ("d_w0", c_void_p), ("d_w2", c_void_p),
                ("h_radius", c_void_p), ("h_norm", c_void_p), ("d_work", c_void_p), ("work_bytes", ctypes.c_size_t),
                ("thr", c_float), ("eps", c_float), ("d_cands", c_void_p), ("cap", c_uint32), ("h_prefix", c_uint32),
                ("d_count", c_void_p), ("h_count", c_void_p), ("h_cands", c_void_p),
                ("zx_mode", c_int32), ("zx_flags", c_int32), ("store_f32", c_int32), ("exact", c_int32),
                ("expand", c_int32), ("_pad", c_int32),
                ("stream", c_void_p), ("tail_stream", c_void_p), ("pack_stream", c_void_p),
                ("ev_work_free", c_void_p), ("ev_work_read", c_void_p), ("ev_done", c_void_p),
                ("d_parts", c_void_p), ("d_parents", c_void_p), ("h_parents", c_void_p),
                ("n_parts", c_int32), ("n_parents", c_int32), ("d_block_f32", c_void_p)]


class FinishStackArgs(Structure):
    """``mmx_finish_stack_args`` (a one-batch stack from the re-scored candidates to its final table: ``mmx_host_finish_stack``)."""
    _fields_ = [("cands", c_void_p), ("n_cands", c_uint32), ("n_total", c_uint32),
                ("blocks", c_void_p), ("n_blocks", c_int32), ("n_sigma", c_int32),
                ("thr", c_double), ("eps", c_double),
                ("sigmas", c_void_p), ("overlap", c_double), ("overlap_band", c_double),
                ("channel", c_double),
                ("block_offsets", c_void_p), ("block_tags", c_void_p), ("interior", c_void_p),
                ("store", c_void_p), ("ld", c_int64), ("zyx", c_void_p), ("tag", c_void_p), ("abs_zyx", c_void_p),
                ("capacity", c_int64), ("rows_per_block", c_void_p), ("any_before", c_void_p),
                ("n_sections", c_void_p), ("bounds", c_void_p), ("last_end", c_void_p), ("tol", c_void_p),
                ("nxt_lo", c_void_p), ("nxt_hi", c_void_p),
                ("n_slab", c_void_p), ("n_after", c_void_p), ("n_next", c_void_p), ("stat_ld", c_int64),
                ("src_cols", c_void_p), ("n_out", c_int32), ("abs_dst0", c_int32),
                ("out", c_void_p), ("out_capacity", c_int64), ("out_rows", c_void_p),
                ("stats", c_void_p)]


MMX_DEFERRED = 6


class RowLayout(Structure):
    """``mmx_row_layout``: the columns in which rows leave the merged table (``mmx_host_take_rows``,
    ``mmx_host_gather_parts_by_key``, ``mmx_host_emit_parts``)."""
    _fields_ = [("src_cols", POINTER(c_int32)), ("n_out", c_int64), ("n_main", c_int64), ("abs_dst", c_int32 * 3)]


class DetectInfo(Structure):
    """``mmx_detect_info``."""
    _fields_ = [("zx_path", c_int32), ("mask_layout", c_int32), ("n_pass_rounds", c_int32), ("_pad", c_int32),
                ("q16_bound", c_double)]


class PreprocParams(Structure):
    """``mmx_preproc_params``."""
    _fields_ = [("clip_min", c_double), ("clip_max", c_double), ("max_thresh", c_double),
                ("unsharp_strength", c_double), ("erosion_threshold", c_double),
                ("radius", c_int32), ("rgb_guess", c_int32), ("tv_weight", c_double), ("tv_factor", c_double)]


class MmxError(RuntimeError):
    """A C-ABI call returned a non-zero status."""


_lib = None

#: every symbol ``include/mmx.h`` declares
SYMBOLS = (
    "mmx_abi_version", "mmx_strerror", "mmx_last_hip_error", "mmx_device_count",
    "mmx_detect_batch", "mmx_log_scales_f32", "mmx_detect_batch_capture", "mmx_graph_launch", "mmx_graph_destroy", "mmx_detect_last_error",
    "mmx_event_synchronize", "mmx_stream_wait_event", "mmx_timing_is_enabled",
    "mmx_log_batch_f32", "mmx_log_batch_f32_generic", "mmx_zx_pack", "mmx_fold_matrix", "mmx_col_prefetch", "mmx_tiled_q16_error_bound", "mmx_workspace_bytes", "mmx_peaks_batch", "mmx_rescore_f64",
    "mmx_overlap_pairs", "mmx_close_pairs", "mmx_event_create", "mmx_event_destroy",
    "mmx_event_record", "mmx_event_elapsed_ms", "mmx_timing_enable", "mmx_timing_read",
    "mmx_calib_stream", "mmx_host_prune_axis",
    "mmx_preprocess_fast_lds", "mmx_preprocess_batch", "mmx_preprocess_batch_mode", "mmx_preprocess_work_bytes", "mmx_preprocess_batch_generic", "mmx_preprocess_block_dtypes",
    "mmx_coloc_means", "mmx_coloc_voxels", "mmx_host_take_rows", "mmx_host_map_columns", "mmx_resize_batch_as", "mmx_gauss_axis_batch", "mmx_unmix_batch", "mmx_minmax_batch", "mmx_resize_batch",
    "mmx_cdist_f64", "mmx_host_lsap", "mmx_expand_probes", "mmx_fold_parts", "mmx_host_resolve_peaks", "mmx_host_overlap_prune",
    "mmx_host_emit_tables", "mmx_host_prune_region", "mmx_host_prune_parts", "mmx_host_rows_in_boxes", "mmx_host_append_rows", "mmx_host_emit_parts", "mmx_host_merge_parts_by_key", "mmx_host_gather_parts_by_key", "mmx_host_emit_tables_multi", "mmx_host_coloc_flags", "mmx_host_finish_stack", "mmx_copy_rect_h2d", "mmx_host_stage_upload", "mmx_host_stage_upload_pitched", "mmx_event_query",
    "mmx_order_stats_workspace", "mmx_order_stats", "mmx_extract_patches",
    "mmx_ds_zoom_batch", "mmx_ds_gauss_pick_batch",
    "mmx_eq_hist", "mmx_host_eq_maps", "mmx_eq_apply", "mmx_eq_output", "mmx_stretch",
    "mmx_rotate_minmax", "mmx_rotate_warp",
    "mmx_dn_sum", "mmx_dn_clip", "mmx_dn_blur", "mmx_dn_erode",
)
KERNEL_KINDS = ("zpass", "ypass", "xpass", "generic", "peaks", "rescore", "overlap_pairs",
                "close_pairs", "zxpass", "y2pass", "preproc", "coloc", "zxpack", "widepass")
#: families behind the ``MMX_K_COUNT`` counted ones (``MMX_K_THIN``): timed and read with them
MORE_KERNEL_KINDS = ("thinpass",)
_ALL_KINDS = KERNEL_KINDS + MORE_KERNEL_KINDS


def lib() -> ctypes.CDLL:
    """Load the library once; raise loudly when it is not there."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise MmxError(
            f"{LIB_PATH} not found: the HIP extension has not been built "
            "(run __graft_entry__.build() or make -C magellanmapper_amd/csrc). "
            "There is no CPU fallback for this path.")
    # PyTorch-ROCm wheels bundle their own libamdhip64: when this library is loaded first, the loader binds it to the
    # system's copy and a process that imports torch afterwards ends up with two HIP runtimes -- every launch on a torch
    # stream then fails with "HIP runtime error" (seen with __graft_entry__.build() followed by smoke() in one
    # process).  With torch imported first the runtime already in the process satisfies the dependency.
    try:
        import torch  # noqa: F401
    except ImportError:
        pass
    L = ctypes.CDLL(LIB_PATH)
    # (entry points added without a new version number -- mmx_fold_parts and the fields it appended to mmx_detect_args --
    #  are told by their symbols: a library built before them must not be handed the longer record)
    missing = [name for name in SYMBOLS if not hasattr(L, name)]
    if missing:
        raise MmxError(f"{LIB_PATH} lacks {', '.join(missing)}: it was built from older sources; rebuild it")
    vp = c_void_p
    L.mmx_abi_version.restype = c_int
    L.mmx_strerror.restype = c_char_p
    L.mmx_strerror.argtypes = [c_int]
    L.mmx_last_hip_error.restype = c_char_p
    L.mmx_device_count.restype = c_int
    log_args = [POINTER(Volume), vp, vp, c_int, c_int64, POINTER(c_double), POINTER(c_double),
                c_int, c_double, vp, vp]
    L.mmx_log_batch_f32.argtypes = log_args + [vp, c_float, c_float, POINTER(c_int), c_int, POINTER(c_int), vp]
    L.mmx_log_batch_f32_generic.argtypes = log_args + [vp]
    L.mmx_workspace_bytes.argtypes = [c_int, c_int64, c_int, c_int]
    L.mmx_workspace_bytes.restype = ctypes.c_size_t
    L.mmx_zx_pack.argtypes = [POINTER(Volume), vp, vp, c_int, c_int64, vp, vp]
    L.mmx_tiled_q16_error_bound.argtypes = [POINTER(c_double), POINTER(c_double), c_int, c_double]
    L.mmx_tiled_q16_error_bound.restype = c_double
    L.mmx_fold_matrix.argtypes = [POINTER(c_float), c_int, c_int, POINTER(c_float)]
    L.mmx_fold_matrix.restype = c_int
    L.mmx_col_prefetch.argtypes = []
    L.mmx_col_prefetch.restype = c_int
    L.mmx_peaks_batch.argtypes = [vp, vp, c_int, c_int, vp, vp, c_int, c_int64, c_float, c_float, vp,
                                  c_uint32, vp, vp]
    L.mmx_rescore_f64.argtypes = [POINTER(Volume), vp, c_int, vp, c_uint32, vp, vp, vp,
                                  POINTER(c_int32), POINTER(c_double), c_int, c_int, vp]
    L.mmx_overlap_pairs.argtypes = [vp, vp, c_int, c_double, c_double, c_double, vp, vp, c_uint32, vp, vp]
    L.mmx_close_pairs.argtypes = [vp, c_int, vp, c_int, POINTER(c_int32), vp, vp, vp]
    L.mmx_detect_batch.argtypes = [POINTER(DetectArgs), POINTER(DetectInfo)]
    L.mmx_log_scales_f32.argtypes = [POINTER(DetectArgs), POINTER(DetectInfo)]
    L.mmx_detect_batch_capture.argtypes = [POINTER(DetectArgs), POINTER(DetectInfo), POINTER(vp)]
    L.mmx_graph_launch.argtypes = [vp, vp, vp, POINTER(DetectInfo)]
    L.mmx_graph_destroy.argtypes = [vp]
    L.mmx_detect_last_error.restype = c_char_p
    L.mmx_event_synchronize.argtypes = [vp]
    L.mmx_stream_wait_event.argtypes = [vp, vp]
    L.mmx_event_create.argtypes = [POINTER(vp)]
    L.mmx_event_destroy.argtypes = [vp]
    L.mmx_event_record.argtypes = [vp, vp]
    L.mmx_event_elapsed_ms.argtypes = [vp, vp, POINTER(c_float)]
    L.mmx_timing_enable.argtypes = [c_int]
    L.mmx_timing_read.argtypes = [POINTER(c_double), POINTER(c_int64), c_int]
    L.mmx_calib_stream.argtypes = [c_int, vp, vp, c_int64, vp]
    L.mmx_host_prune_axis.argtypes = [vp, vp, vp, vp, c_int64, c_int, c_int, vp, c_double,
                                      POINTER(c_int32), vp, vp, vp, POINTER(c_int64), vp, vp, vp]
    L.mmx_preprocess_fast_lds.argtypes = [c_int, c_int, c_int]
    L.mmx_preprocess_fast_lds.restype = c_int64
    pre_args = [POINTER(Volume), vp, vp, c_int, vp, c_int, POINTER(PreprocParams), vp,
                c_int64, c_int64, vp, vp, vp]
    L.mmx_preprocess_batch.argtypes = pre_args + [vp]
    L.mmx_preprocess_batch_mode.argtypes = pre_args + [c_int, c_int, vp, c_int64, vp]
    L.mmx_preprocess_work_bytes.argtypes = [vp, c_int]
    L.mmx_preprocess_work_bytes.restype = c_int64
    L.mmx_preprocess_batch_generic.argtypes = pre_args + [vp, c_int64, vp]
    L.mmx_preprocess_block_dtypes.argtypes = [vp, vp, c_int, vp, vp, c_int, vp, c_int64, c_int64, vp, c_int64, vp, vp]
    L.mmx_minmax_batch.argtypes = [POINTER(Volume), vp, vp, c_int, vp, vp]
    L.mmx_minmax_batch.restype = c_int
    L.mmx_resize_batch.argtypes = [POINTER(Volume), vp, vp, c_int, vp, vp, vp, c_int64, c_int64, c_int64,
                                   vp, vp, vp]
    L.mmx_resize_batch.restype = c_int
    L.mmx_resize_batch_as.argtypes = [POINTER(Volume), vp, vp, c_int, vp, vp, vp, c_int64, c_int64, c_int64,
                                      c_int, vp, vp, vp]
    L.mmx_resize_batch_as.restype = c_int
    L.mmx_gauss_axis_batch.argtypes = [POINTER(Volume), vp, vp, c_int, c_int, vp, vp, c_int, c_int,
                                       c_int64, c_int64, c_int64, vp, vp]
    L.mmx_gauss_axis_batch.restype = c_int
    L.mmx_unmix_batch.argtypes = [POINTER(Volume), POINTER(Volume), POINTER(c_double), c_int, vp, vp, c_int,
                                  c_int64, c_int64, c_int64, vp, vp, vp]
    L.mmx_unmix_batch.restype = c_int
    L.mmx_host_take_rows.argtypes = [vp, c_int64, vp, c_int64, vp, POINTER(RowLayout), vp, vp]
    L.mmx_host_map_columns.argtypes = [vp, c_int64, c_int64, POINTER(c_int32), c_int32, vp, c_int64, c_int32]
    L.mmx_cdist_f64.argtypes = [vp, c_int64, vp, c_int64, c_int, vp, vp]
    L.mmx_cdist_f64.restype = c_int
    L.mmx_host_lsap.argtypes = [vp, c_int64, c_int64, vp, vp]
    L.mmx_host_lsap.restype = c_int
    L.mmx_coloc_means.argtypes = [POINTER(Volume), vp, c_int, vp, vp, c_int, vp, vp, vp]
    L.mmx_coloc_means.restype = c_int
    L.mmx_coloc_voxels.argtypes = [POINTER(Volume), vp, c_int, vp, vp, c_int, vp, vp, vp, vp]
    L.mmx_coloc_voxels.restype = c_int
    L.mmx_expand_probes.argtypes = [vp, c_uint32, vp, vp, vp, c_int, c_int, vp]
    L.mmx_expand_probes.restype = c_int
    L.mmx_fold_parts.argtypes = [vp, c_uint32, vp, vp, c_int, vp]
    L.mmx_fold_parts.restype = c_int
    L.mmx_host_resolve_peaks.argtypes = [vp, c_uint32, c_uint32, vp, c_int, c_int, c_double, vp, vp, vp, vp, vp, vp, vp]
    L.mmx_host_overlap_prune.argtypes = [vp, vp, c_int, vp, c_int, c_double, c_double, vp, vp, vp, vp, c_int64,
                                         POINTER(c_int64), POINTER(c_int64)]
    L.mmx_host_prune_region.argtypes = [vp, vp, vp, vp, c_int64, c_int64, c_int64, POINTER(c_int32), POINTER(vp),
                                        POINTER(c_double), POINTER(c_int32), POINTER(vp), POINTER(vp), vp, vp,
                                        POINTER(c_int64), vp, vp, vp, c_int64]
    L.mmx_host_prune_parts.argtypes = [vp, vp, vp, vp, c_int64, vp, c_int, c_int, POINTER(c_int32), POINTER(c_int32),
                                       vp, c_int, POINTER(c_int32), POINTER(vp), POINTER(c_double), POINTER(c_int32),
                                       POINTER(vp), POINTER(vp), c_int64, vp, vp, vp, POINTER(c_int64), vp, vp, vp,
                                       c_int64]
    L.mmx_host_rows_in_boxes.argtypes = [vp, vp, vp, vp, c_int64, c_int64, vp, vp, c_int, vp, c_int64, POINTER(c_int64)]
    L.mmx_host_append_rows.argtypes = [vp, c_int64, POINTER(c_int32), POINTER(c_int32), vp, vp, vp, vp, c_int64,
                                       c_int64, c_int64, POINTER(c_int64)]
    L.mmx_host_gather_parts_by_key.argtypes = [vp, c_int64, c_int32, vp, vp, vp, vp, c_int64, POINTER(RowLayout), vp, c_int64, vp]
    L.mmx_host_emit_parts.argtypes = [vp, c_int64, c_int32, vp, vp, vp, vp, POINTER(RowLayout), vp, c_int64]
    L.mmx_host_merge_parts_by_key.argtypes = [vp, vp, c_int32, c_int64, c_int64, c_int64, vp, c_int64]
    L.mmx_host_emit_tables_multi.argtypes = [c_int32, vp, vp, vp, c_int, vp, vp, vp, vp, vp, vp, vp, c_int64, c_int32, vp, vp,
                                             vp, c_int64, c_int64, vp, vp, vp]
    L.mmx_host_coloc_flags.argtypes = [vp, vp, c_int32, c_int64, vp, vp, c_int, vp, c_int32, vp, c_int64]
    L.mmx_host_finish_stack.argtypes = [POINTER(FinishStackArgs)]
    L.mmx_host_stage_upload.argtypes = [vp, vp, vp, c_int32, c_int64, c_int64, c_int64, vp, c_int64, c_int32, vp, vp, c_int32,
                                        vp, vp, c_int32]
    L.mmx_host_stage_upload_pitched.argtypes = [vp, c_int64, vp, vp, c_int32, c_int64, c_int64, c_int64, vp, c_int64, c_int32,
                                                vp, vp, c_int32, vp, vp, c_int32]
    L.mmx_event_query.argtypes = [vp]
    L.mmx_copy_rect_h2d.argtypes = [vp, ctypes.c_size_t, vp, ctypes.c_size_t, ctypes.c_size_t, ctypes.c_size_t, vp]
    L.mmx_host_emit_tables.argtypes = [vp, vp, vp, c_int, vp, c_int, c_double, vp, vp, vp, vp, c_int64, vp, vp, vp,
                                       c_int64, c_int64, vp]
    L.mmx_order_stats_workspace.argtypes = [c_int]
    L.mmx_order_stats_workspace.restype = ctypes.c_size_t
    L.mmx_order_stats.argtypes = [POINTER(Volume), c_int64, c_int64, c_int64, vp, vp, c_int, vp, vp, vp, ctypes.c_size_t, vp]
    L.mmx_order_stats.restype = c_int
    L.mmx_extract_patches.argtypes = [POINTER(Volume), vp, c_int64, c_int, vp, vp, vp]
    L.mmx_extract_patches.restype = c_int
    L.mmx_ds_zoom_batch.argtypes = [POINTER(DsView), POINTER(DsView), c_int64, vp, vp, c_int, vp, vp, c_int64, vp, vp,
                                    c_int, vp]
    L.mmx_ds_zoom_batch.restype = c_int
    L.mmx_ds_gauss_pick_batch.argtypes = [POINTER(DsView), vp, vp, c_int, c_int, vp, vp, vp, c_int, vp, vp, c_int64,
                                          c_int64, c_int64, c_int64, vp, vp]
    L.mmx_ds_gauss_pick_batch.restype = c_int
    L.mmx_eq_hist.argtypes = [POINTER(DsView), POINTER(EqGeom), vp, vp, vp]
    L.mmx_eq_hist.restype = c_int
    L.mmx_host_eq_maps.argtypes = [vp, c_int64, c_int, c_int64, c_int64, vp, vp]
    L.mmx_eq_apply.argtypes = [POINTER(DsView), POINTER(EqGeom), vp, vp, vp, vp, vp, vp, vp, vp]
    L.mmx_eq_apply.restype = c_int
    L.mmx_eq_output.argtypes = [vp, c_int64, vp, vp, vp]
    L.mmx_eq_output.restype = c_int
    L.mmx_stretch.argtypes = [POINTER(DsView), c_int, c_int, c_int, c_double, c_double, vp, vp]
    L.mmx_stretch.restype = c_int
    L.mmx_rotate_minmax.argtypes = [POINTER(DsView), c_int64, c_int, c_int, c_int, c_int, c_int, vp, vp]
    L.mmx_rotate_minmax.restype = c_int
    L.mmx_rotate_warp.argtypes = [POINTER(DsView), c_int64, POINTER(DsView), c_int64, c_int, c_int, c_int, c_int, c_int,
                                  POINTER(c_double), c_int, vp, vp]
    L.mmx_rotate_warp.restype = c_int
    L.mmx_dn_sum.argtypes = [POINTER(DsView), c_int, c_int, c_int, vp, vp]
    L.mmx_dn_sum.restype = c_int
    L.mmx_dn_clip.argtypes = [POINTER(DsView), c_int, c_int, c_int, c_double, c_double, vp, vp]
    L.mmx_dn_clip.restype = c_int
    L.mmx_dn_blur.argtypes = [POINTER(DsView), c_int, c_int, c_int, c_int, vp, c_double, c_double, vp, vp, c_int,
                              c_double, vp]
    L.mmx_dn_blur.restype = c_int
    L.mmx_dn_erode.argtypes = [vp, c_int, c_int, c_int, c_int, c_int, vp, vp]
    L.mmx_dn_erode.restype = c_int
    L.mmx_preprocess_batch.restype = c_int
    L.mmx_preprocess_batch_mode.restype = c_int
    L.mmx_preprocess_batch_generic.restype = c_int
    L.mmx_preprocess_block_dtypes.restype = c_int
    for name in SYMBOLS:
        fn = getattr(L, name)
        if name in ("mmx_preprocess_fast_lds", "mmx_workspace_bytes", "mmx_preprocess_work_bytes",
                    "mmx_order_stats_workspace"):
            continue
        if fn.restype is None or name.startswith(("mmx_log", "mmx_peaks", "mmx_rescore",
                                                  "mmx_overlap", "mmx_close", "mmx_event", "mmx_timing", "mmx_calib", "mmx_host")):
            fn.restype = c_int
    if L.mmx_abi_version() != MMX_ABI_VERSION:
        raise MmxError("libmmx_hip.so ABI version mismatch")
    _lib = L
    return L


def check(status: int, what: str) -> None:
    if status != 0:
        L = lib()
        msg = L.mmx_strerror(status).decode()
        hip = L.mmx_last_hip_error().decode()
        raise MmxError(f"{what}: {msg}" + (f" ({hip})" if hip else ""))


def as_double_ptr(a: np.ndarray):
    assert a.dtype == np.float64 and a.flags.c_contiguous
    return a.ctypes.data_as(POINTER(c_double))


def as_int32_ptr(a: np.ndarray):
    assert a.dtype == np.int32 and a.flags.c_contiguous
    return a.ctypes.data_as(POINTER(c_int32))


def timing_enable(on: bool = True, kinds=None) -> None:
    """Per-kernel HIP-event timing on / off; ``kinds`` (names from ``KERNEL_KINDS``): only those families."""
    mask = 1 if on else 0
    if on and kinds is not None:
        mask = 0
        for k in kinds:
            mask |= 1 << (_ALL_KINDS.index(k) + 1)
    check(lib().mmx_timing_enable(mask), "mmx_timing_enable")


def timing_read() -> dict:
    """``{kind: (milliseconds, launches)}`` since the last read (synchronises the events)."""
    ms = (c_double * len(_ALL_KINDS))()
    n = (c_int64 * len(_ALL_KINDS))()
    check(lib().mmx_timing_read(ms, n, len(_ALL_KINDS)), "mmx_timing_read")
    return {k: (ms[i], n[i]) for i, k in enumerate(_ALL_KINDS)}


def col_prefetch() -> int:
    """``MMX_COL_PREFETCH``, from the library: a block shorter than kernel radius + this along an axis is thin there."""
    return int(lib().mmx_col_prefetch())


def fold_matrix(w: np.ndarray, n: int) -> np.ndarray:
    """``mmx_fold_matrix``: the ``(n, n)`` float32 operator SciPy's "reflect" folds the symmetric kernel of half
    weights ``w[0 .. radius]`` (float32) into on an axis of ``n`` voxels."""
    w = np.ascontiguousarray(w, dtype=np.float32)
    out = np.empty((int(n), int(n)), dtype=np.float32)
    check(lib().mmx_fold_matrix(w.ctypes.data_as(POINTER(c_float)), len(w) - 1, int(n),
                                out.ctypes.data_as(POINTER(c_float))), "mmx_fold_matrix")
    return out


def keep_host_heap(mmap_threshold: int = 1 << 30, trim_threshold: int = (1 << 31) - 1) -> bool:
    """glibc ``mallopt``: serve large host arrays from the heap and keep freed heap memory mapped.

    A whole-volume detection builds tables of tens of MB per call (the merged blob table, its compact
    columns, the pruned output).  By default glibc ``mmap``s every allocation above 32 MiB: each call then pays
    page faults for fresh zero pages and an ``munmap`` when the arrays die -- ~8 ms per 2048 x 2048 x 1024 volume.
    Long-running detection processes (and ``bench.py``) call this once; it changes the allocator of the WHOLE
    process (memory is returned to the OS later), which is why importing the package does not do it.
    Returns False where ``mallopt`` is not available (non-glibc)."""
    try:
        libc = ctypes.CDLL("libc.so.6")
        ok1 = libc.mallopt(-3, int(mmap_threshold))      # M_MMAP_THRESHOLD
        ok2 = libc.mallopt(-1, int(trim_threshold))      # M_TRIM_THRESHOLD
        return bool(ok1 and ok2)
    except (OSError, AttributeError):
        return False
