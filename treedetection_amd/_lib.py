"""ctypes binding of libtreedet_hip.so (C ABI declared in include/treedet.h).

The library is built in-tree by ``__graft_entry__.build()`` / ``make -C treedetection_amd/csrc``.
There is no CPU fallback: if the shared object is missing, or a call is made without a GPU, the
product path raises (SURVEY.md §8b — the oracle under ``oracle/`` is test infrastructure only).
"""
from __future__ import annotations

import ctypes as C
import os
import threading
from typing import Optional

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "libtreedet_hip.so")

_lib: Optional[C.CDLL] = None
ERR_INVALID = -1    # TD_ERR_INVALID
ERR_CAPACITY = -4   # TD_ERR_CAPACITY
ERR_STATE = -5      # TD_ERR_STATE
ERR_UNSUPPORTED = -6  # TD_ERR_UNSUPPORTED
JPEG_TABSET_BYTES = 11904  # TD_JPEG_TABSET_BYTES: one table set of td_tiff_jpeg_plan
SAMPLE_U8, SAMPLE_F32, SAMPLE_U16 = 0, 1, 2           # TD_SAMPLE_*: source of td_resample_gdal_dev (U16: td_seam_first_dev only)
RESAMPLE_MODES = {"f32": 0, "u8": 1, "ndvi": 2}       # TD_RESAMPLE_*: its output modes
ZSTD_STATS = ("frames block_raw block_rle block_comp max_blocks_per_frame lit_raw lit_rle lit_huff lit_treeless lit_streams_1 lit_streams_4 "
              "hufw_direct hufw_fse seq0 LL_predef LL_rle LL_fse LL_repeat OF_predef OF_rle OF_fse OF_repeat ML_predef ML_rle ML_fse ML_repeat "
              "window_desc single_segment checksum seq_long seq_2byte skippable").split()   # TD_ZSTD_STATS counters of td_zstd_stream_stats, in order
RING_PAIR_CAP, RING_PAIR_WPB, RING_PAIR_GRID = 1024, 4, 2048   # ringiou.hip: vertices of a pair in LDS, waves per workgroup, workgroups per launch
# TD_RELATE_*_CAP (regionrelate.hip): points of a query ring, meeting parameters of one query edge, distinct region rings a query meets
RELATE_QUERY_CAP, RELATE_MEET_CAP, RELATE_RING_CAP = 256, 254, 64
ZONAL_RING_CAP = 512   # TD_ZONAL_RING_CAP (crownzonal.hip): vertices of an open crown ring the kernel holds
TREETOP_RADIUS_CAP, TREETOP_WINDOW_CAP = 8, 15   # TD_TREETOP_*_CAP (treetops.hip): the smoothing radius and the window the kernel holds


class TdError(RuntimeError):
    """A libtreedet_hip call returned a negative status (message from td_last_error)."""


class ModelDesc(C.Structure):
    _fields_ = [("num_classes", C.c_int32), ("precision", C.c_int32), ("pre_nms_topk", C.c_int32),
                ("post_nms_topk", C.c_int32), ("detections_per_image", C.c_int32),
                ("rpn_nms_thresh", C.c_float), ("score_thresh", C.c_float), ("nms_thresh", C.c_float),
                ("mask_thresh", C.c_float)]


class TensorDesc(C.Structure):
    _fields_ = [("name", C.c_char_p), ("data", C.c_void_p), ("ndim", C.c_int32), ("shape", C.c_int64 * 4)]


class SeamSource(C.Structure):
    """td_seam_source: one source buffer of td_seam_first_dev."""
    _fields_ = [("data", C.c_void_p), ("pitch", C.c_int64), ("rows", C.c_int32), ("row0", C.c_int32), ("col0", C.c_int32),
                ("r_lo", C.c_int32), ("c_lo", C.c_int32), ("r_hi", C.c_int32), ("c_hi", C.c_int32), ("has_own", C.c_int32),
                ("own", C.c_double)]


class WorkspaceRow(C.Structure):
    """td_workspace_row: one buffer of td_workspace_plan."""
    _fields_ = [("name", C.c_char * 32), ("public_name", C.c_char * 32), ("kind", C.c_int32), ("elem_size", C.c_int32),
                ("phase", C.c_int32), ("pad_", C.c_int32), ("dims", C.c_int64 * 4), ("alloc_bytes", C.c_int64)]


class Detections(C.Structure):
    _fields_ = [("boxes", C.c_void_p), ("scores", C.c_void_p), ("classes", C.c_void_p), ("count", C.c_void_p),
                ("mask_probs", C.c_void_p), ("mask_region", C.c_void_p), ("mask_offset", C.c_void_p),
                ("mask_bits", C.c_void_p), ("mask_words_per_image", C.c_int64)]


# name -> (restype, argtypes); every symbol include/treedet.h declares
SIGNATURES = {
    "td_model_desc_default": (None, [C.POINTER(ModelDesc)]),
    "td_engine_create": (C.c_int, [C.POINTER(ModelDesc), C.c_int, C.POINTER(C.c_void_p)]),
    "td_engine_load_weights": (C.c_int, [C.c_void_p, C.POINTER(TensorDesc), C.c_size_t]),
    "td_engine_reserve": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_int]),
    "td_engine_forward": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.POINTER(C.c_int32), C.POINTER(C.c_int32),
                                    C.c_int, C.c_int, C.c_int, C.c_void_p, C.POINTER(Detections)]),
    "td_engine_forward_phase": (C.c_int, [C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.POINTER(C.c_int32), C.POINTER(C.c_int32),
                                          C.c_int, C.c_int, C.c_int, C.c_void_p, C.POINTER(Detections)]),
    "td_engine_tensor": (C.c_int, [C.c_void_p, C.c_char_p, C.POINTER(C.c_void_p), C.POINTER(C.c_int64),
                                   C.POINTER(C.c_int)]),
    "td_engine_read_tensor": (C.c_int, [C.c_void_p, C.c_char_p, C.c_void_p, C.c_int64, C.c_void_p]),
    "td_engine_profile_enable": (C.c_int, [C.c_void_p, C.c_int]),
    "td_engine_profile_read": (C.c_int, [C.c_void_p, C.POINTER(C.c_double), C.POINTER(C.c_int64), C.POINTER(C.c_double),
                                         C.POINTER(C.c_double), C.c_int]),
    "td_engine_profile_classes": (C.c_int, [C.c_void_p, C.POINTER(C.c_double), C.POINTER(C.c_int64), C.POINTER(C.c_double),
                                            C.POINTER(C.c_double), C.POINTER(C.c_double), C.c_int]),
    "td_last_error": (C.c_char_p, []),
    "td_engine_destroy": (None, [C.c_void_p]),
    "td_resize_tile_u8": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_int, C.c_int, C.c_int,
                                    C.c_void_p, C.c_void_p]),
    "td_resize_batch_u8": (C.c_int, [C.POINTER(C.c_void_p), C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_int, C.c_int,
                                     C.c_int, C.c_int64, C.c_void_p, C.c_void_p]),
    "td_bottleneck_tail_nhwc": (C.c_int, [C.c_void_p] * 9 + [C.c_int] * 6 + [C.c_void_p]),
    "td_bottleneck_tail_split_nhwc": (C.c_int, [C.c_void_p] * 10 + [C.c_int] * 5 + [C.c_void_p]),
    "td_conv_split_pack": (C.c_int64, [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_int64]),
    "td_resize_bilinear_f64": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int64, C.c_void_p]),
    "td_windows_u16_to_input": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_int, C.c_int,
                                          C.c_int, C.c_int64, C.c_int64, C.c_void_p]),
    "td_resize_shape": (None, [C.c_int, C.c_int, C.c_int, C.c_int, C.POINTER(C.c_int), C.POINTER(C.c_int)]),
    "td_conv2d_nhwc": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p]
                       + [C.c_int] * 11 + [C.c_void_p]),
    "td_conv2d_rows_nhwc": (C.c_int, [C.c_void_p] * 5 + [C.c_int] * 10 + [C.c_void_p, C.c_int, C.c_int, C.c_void_p]),
    "td_conv2d_head_nhwc": (C.c_int, [C.c_void_p] * 6 + [C.c_int] * 9 + [C.c_void_p]),
    "td_conv2d_winograd_head_nhwc": (C.c_int, [C.c_void_p] * 6 + [C.c_int] * 5 + [C.c_void_p]),
    "td_conv2d_winograd_nhwc": (C.c_int, [C.c_void_p] * 5 + [C.c_int] * 6 + [C.c_void_p]),
    "td_conv_path": (C.c_int, [C.POINTER(C.c_int32), C.c_int64, C.POINTER(C.c_int32), C.POINTER(C.c_int32), C.POINTER(C.c_int32),
                               C.POINTER(C.c_int32)]),
    "td_workspace_plan": (C.c_int, [C.c_int] * 4 + [C.POINTER(C.c_int32)] + [C.c_int] * 3 + [C.POINTER(WorkspaceRow), C.c_int, C.POINTER(C.c_int)]),
    "td_nms": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_float, C.c_void_p, C.c_void_p, C.c_void_p]),
    "td_roi_align": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_int, C.c_float, C.c_int,
                               C.c_void_p, C.c_int, C.c_void_p]),
    "td_paste_masks": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_float, C.c_void_p,
                                 C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p]),
    "td_paste_masks_batch": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.POINTER(C.c_int32), C.c_int, C.c_int, C.c_float,
                                       C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p]),
    "td_crown_stats": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.POINTER(C.c_double), C.POINTER(C.c_int32), C.c_void_p, C.c_int,
                                 C.c_int, C.c_float, C.c_void_p, C.c_void_p]),
    "td_crown_zonal_dev": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.POINTER(C.c_double), C.c_void_p, C.c_int64, C.c_void_p, C.c_int,
                                     C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "td_crown_zonal": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.POINTER(C.c_double), C.c_void_p, C.c_int64, C.c_void_p, C.c_int,
                                 C.c_void_p, C.c_void_p, C.c_void_p]),
    "td_crown_labels_dev": (C.c_int, [C.c_int, C.c_int, C.POINTER(C.c_double), C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p, C.c_int,
                                      C.c_void_p, C.c_void_p, C.c_void_p]),
    "td_crown_labels": (C.c_int, [C.c_int, C.c_int, C.POINTER(C.c_double), C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p, C.c_int,
                                  C.c_void_p, C.c_void_p]),
    "td_treetops_dev": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_int, C.c_int, C.c_float, C.c_void_p, C.c_void_p, C.c_void_p,
                                  C.c_void_p]),
    "td_treetops": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_int, C.c_int, C.c_float, C.c_void_p, C.c_void_p, C.c_void_p]),
    "td_resample_gdal_dev": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.POINTER(C.c_int32), C.c_int]
                             + [C.c_void_p] * 4 + [C.c_int, C.c_int64] + [C.c_void_p] * 4 + [C.c_int, C.c_int64]
                             + [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p]),
    "td_seam_first_dev": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_double, C.POINTER(SeamSource), C.POINTER(SeamSource),
                                    C.c_void_p]),
    "td_crown_pairs_count": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_float, C.c_uint16, C.c_void_p, C.c_float, C.c_void_p, C.c_void_p,
                                       C.c_void_p]),
    "td_crown_pairs_fill": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_float, C.c_uint16, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "td_crown_pairs_greedy": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p]),
    "td_ring_pairs_area_dev": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_int64, C.c_void_p,
                                         C.c_void_p, C.c_void_p]),
    "td_ring_pairs_area": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_int64, C.c_void_p,
                                     C.c_void_p]),
    "td_box_pairs_ab_count": (C.c_int, [C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p]),
    "td_box_pairs_ab_fill": (C.c_int, [C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "td_box_pairs_ab": (C.c_int, [C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_int64]),
    "td_match_greedy": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_double, C.c_void_p, C.c_void_p,
                                  C.c_void_p]),
    "td_trace_contours_dev": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p, C.c_int, C.c_int, C.c_void_p,
                                        C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "td_find_contours": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_int, C.c_void_p, C.c_int]),
    "td_batch_prediction_files": (C.c_int, [C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p,
                                          C.c_void_p, C.c_void_p, C.c_void_p, C.c_char_p, C.POINTER(C.c_char_p), C.c_int, C.c_void_p, C.c_void_p]),
    "td_tiff_lzw_decode": (C.c_int64, [C.c_void_p, C.c_int64, C.c_void_p, C.c_int64]),
    "td_tiff_packbits_decode": (C.c_int64, [C.c_void_p, C.c_int64, C.c_void_p, C.c_int64]),
    "td_tiff_lzw_encode": (C.c_int64, [C.c_void_p, C.c_int64, C.c_void_p, C.c_int64]),
    "td_tiff_inflate": (C.c_int64, [C.c_void_p, C.c_int64, C.c_void_p, C.c_int64]),
    "td_tiff_inflate_dev": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p]),
    "td_tiff_inflate_verified": (C.c_int64, [C.c_void_p, C.c_int64, C.c_void_p, C.c_int64]),
    "td_tiff_inflate_verified_dev": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p,
                                               C.c_void_p]),
    "td_tiff_zstd_decode": (C.c_int64, [C.c_void_p, C.c_int64, C.c_void_p, C.c_int64]),
    "td_zstd_stream_stats": (C.c_int64, [C.c_void_p, C.c_int64, C.c_void_p]),
    "td_tiff_zstd_decode_dev": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p,
                                          C.c_int64, C.c_void_p]),
    "td_tiff_zstd_scratch_bytes": (C.c_int64, [C.c_int]),
    "td_tiff_adler32_blocks_dev": (C.c_int, [C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p,
                                             C.c_void_p]),
    "td_adler32_dev": (C.c_int, [C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p]),
    "td_tiff_lzw_decode_dev": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p]),
    "td_tiff_blocks_to_image_dev": (C.c_int, [C.c_void_p, C.c_int64, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_int, C.c_int, C.c_void_p]),
    "td_tiff_blocks_to_image_u16_dev": (C.c_int, [C.c_void_p, C.c_int64, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_int,
                                                  C.c_int, C.c_void_p]),
    "td_tiff_blocks_to_image_f32_dev": (C.c_int, [C.c_void_p, C.c_int64, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_int,
                                                  C.c_int, C.c_void_p]),
    "td_tiff_planes_to_image_dev": (C.c_int, [C.c_void_p, C.c_int64, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p,
                                              C.c_int, C.c_int, C.c_void_p]),
    "td_tiff_planes_to_image_u16_dev": (C.c_int, [C.c_void_p, C.c_int64, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p,
                                                  C.c_int, C.c_int, C.c_void_p]),
    "td_tiff_planes_to_image_f32_dev": (C.c_int, [C.c_void_p, C.c_int64, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p,
                                                  C.c_int, C.c_int, C.c_void_p]),
    "td_tiff_jpeg_plan": (C.c_int, [C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p,
                                    C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p, C.c_int64, C.c_void_p]),
    "td_tiff_jpeg_decode_dev": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64,
                                          C.c_void_p, C.c_void_p] + [C.c_int] * 6 + [C.c_void_p]),
    "td_jpeg_decode": (C.c_int64, [C.c_void_p, C.c_int64, C.c_void_p, C.c_int64, C.c_void_p]),
    "td_tiff_jpeg_decode_long_dev": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_int, C.c_void_p,
                                               C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p] + [C.c_int] * 6 + [C.c_void_p]),
    "td_jpeg_decode_sync": (C.c_int64, [C.c_void_p, C.c_int64, C.c_void_p, C.c_int64, C.c_void_p, C.c_int, C.c_int, C.c_void_p]),
    "td_read_windows": (C.c_int64, [C.c_int, C.c_int, C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int]),
    "td_tiff_unpredict": (C.c_int, [C.c_void_p, C.c_int64, C.c_int64, C.c_int, C.c_int]),
    "td_tiff_unpredict_float": (C.c_int, [C.c_void_p, C.c_int64, C.c_int64, C.c_int, C.c_int]),
    "td_region_relate": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p]),
    "td_region_relate_dev": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int64,
                                       C.c_double, C.c_double, C.c_double, C.c_void_p, C.c_void_p, C.c_int, C.c_int64, C.c_void_p, C.c_void_p,
                                       C.c_int, C.c_void_p]),
    "td_simplify_ring": (C.c_int, [C.c_void_p, C.c_int, C.c_double, C.c_void_p, C.c_int]),
    "td_ring_is_valid": (C.c_int, [C.c_void_p, C.c_int]),
    "td_stitch_tile_json": (C.c_int, [C.c_char_p, C.c_int64, C.POINTER(C.c_double), C.c_double, C.c_int32, C.c_void_p,
                                      C.c_int64, C.c_void_p, C.c_void_p, C.c_int, C.POINTER(C.c_int64), C.POINTER(C.c_int)]),
    "td_stitch_tile_files": (C.c_int, [C.c_char_p, C.c_void_p, C.c_int, C.c_void_p, C.c_double, C.c_void_p, C.c_int, C.c_void_p, C.c_int64,
                                       C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.POINTER(C.c_int64), C.POINTER(C.c_int)]),
    "td_tile_polygons_json_dev": (C.c_int, [C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64,
                                            C.c_void_p, C.c_void_p, C.c_int, C.POINTER(C.c_double), C.c_char_p, C.c_void_p, C.c_int64,
                                            C.POINTER(C.c_int64)]),
    "td_read_window": (C.c_int64, [C.c_int, C.c_int64, C.c_int64, C.c_int64, C.c_int64, C.c_void_p]),
    "td_tile_prediction_file": (C.c_int, [C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p,
                                          C.c_int, C.POINTER(C.c_double), C.c_char_p, C.c_char_p, C.POINTER(C.c_int64)]),
    "td_tile_polygons_json": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p, C.c_int,
                                        C.POINTER(C.c_double), C.c_char_p, C.c_void_p, C.c_int64, C.POINTER(C.c_int64)]),
}


def load() -> C.CDLL:
    """Load the shared object (after torch, so both share one HIP runtime) and bind signatures."""
    global _lib
    if _lib is not None:
        return _lib
    host_only = os.environ.get("TD_HOST_LIB")
    if host_only:
        # sanitizer runs of the CPU tests (make -C treedetection_amd/csrc asan-test): the host-side C++ built with
        # AddressSanitizer + UBSan and no device code. Only the symbols it exports are bound; anything that needs the
        # GPU library fails loudly on the missing attribute.
        lib = C.CDLL(host_only, mode=C.RTLD_GLOBAL)
        for name, (res, args) in SIGNATURES.items():
            fn = getattr(lib, name, None)
            if fn is not None:
                fn.restype = res
                fn.argtypes = args
        _lib = lib
        return lib
    if not os.path.exists(LIB_PATH):
        raise TdError(f"{LIB_PATH} not found — build it first: python -c 'import __graft_entry__ as g; g.build()' "
                      f"(or make -C treedetection_amd/csrc). There is no CPU fallback.")
    import torch  # noqa: F401  (loads libamdhip64 first; our .so then binds to the same runtime)

    lib = C.CDLL(LIB_PATH, mode=C.RTLD_GLOBAL)
    for name, (res, args) in SIGNATURES.items():
        fn = getattr(lib, name)
        fn.restype = res
        fn.argtypes = args
    _lib = lib
    return lib


def check(status: int, what: str = "") -> None:
    if status < 0:
        msg = load().td_last_error().decode("utf-8", "replace")
        raise TdError(f"{what or 'libtreedet_hip'} failed ({status}): {msg}")


def transform6(t):
    """The six coefficients of an affine transform as the ``const double*`` the library takes."""
    return (C.c_double * 6)(*[float(v) for v in t[:6]])


CONV_FORMS = ("direct", "split", "winograd F(2x2)", "winograd F(4x4)", "winograd F(4x4) folded")   # ConvForm (csrc/conv_path.h), in order
CONV_HEADS = ("own launch", "in the output transform", "if the tile owns 256 channels")            # ConvHead, in order


def conv_path(rules, wino_elems, layer, call, head=None) -> dict:
    """td_conv_path (include/treedet.h) on integer sequences: which form the engine gives one convolution. No engine, no GPU.
    → {"form", "head" (names above), "key" (the tune-key tuple, or None when nothing is measured), "slab_tiles", "fold_group"}"""
    arr = lambda v, n: (C.c_int32 * n)(*[int(x) for x in v])
    out = (C.c_int32 * 10)()
    check(load().td_conv_path(arr(rules, 8), int(wino_elems), arr(layer, 9), arr(call, 10), arr(head, 9) if head is not None else None, out),
          "td_conv_path")
    return {"form": CONV_FORMS[out[0]], "head": CONV_HEADS[out[1]], "key": tuple(out[3:8]) if out[2] else None,
            "slab_tiles": out[8], "fold_group": out[9]}


WORKSPACE_KINDS = ("act", "f32", "i32", "u32", "u64")   # WsKind (csrc/workspace.h), in order


def workspace_plan(precision, winograd, post_nms_topk, detections_per_image, widths, B, Hp, Wp) -> list:
    """td_workspace_plan (include/treedet.h): the rows of the engine's workspace plan at one shape. No engine, no GPU.
    widths: 16 integers (stem; conv1, conv2, conv3 of res2 .. res5; FPN; FC; mask deconv output)
    → [{"name", "public" ("" if none), "kind" (names above), "elem", "dims" (4, 0-padded), "alloc_bytes", "phase"}]"""
    rows, n = (WorkspaceRow * 128)(), C.c_int()
    check(load().td_workspace_plan(int(precision), int(winograd), int(post_nms_topk), int(detections_per_image),
                                   (C.c_int32 * 16)(*[int(x) for x in widths]), int(B), int(Hp), int(Wp), rows, 128, C.byref(n)), "td_workspace_plan")
    return [{"name": r.name.decode(), "public": r.public_name.decode(), "kind": WORKSPACE_KINDS[r.kind], "elem": r.elem_size,
             "dims": list(r.dims), "alloc_bytes": r.alloc_bytes, "phase": r.phase} for r in rows[:n.value]]


def stream_ptr() -> int:
    """Raw hipStream_t of torch's current stream on the current device."""
    import torch

    return int(torch.cuda.current_stream().cuda_stream)


_low_priority_streams: dict = {}
_low_priority_lock = threading.Lock()


def low_priority_stream(device_index: int):
    """→ a torch stream wrapping a HIP stream with the LOWEST priority the device offers (torch itself only creates normal and
    higher). Background work that shares the chip with the forwards — the raster decode of the NEXT image — goes there: HIP gives
    every priority level its own hardware queues, so the long decode kernel never sits in front of a model stream's kernels in
    one queue (with the default four queues and five or more streams it did: tools/probes/decode_overlap_probe.py, 763 vs 1 732
    tiles/s while a DEFLATE raster decodes), and the dispatcher serves the forwards' workgroups first. The HIP entry points are
    taken from the runtime libtreedet_hip.so is bound to — the one torch loaded. ONE stream per device for the life of the
    process, never destroyed: torch's allocators remember the streams a block was used on and record events on them when the
    block is freed, long after a Predictor is closed (destroying the stream at close() ended in a segmentation fault there)."""
    import torch

    with _low_priority_lock:
        if device_index in _low_priority_streams:
            return _low_priority_streams[device_index]
        lib = load()
        least, greatest, handle = C.c_int(0), C.c_int(0), C.c_void_p()
        with torch.cuda.device(device_index):
            torch.cuda.current_stream()                                    # the device's context exists before the raw calls
            err = lib.hipDeviceGetStreamPriorityRange(C.byref(least), C.byref(greatest))
            if err == 0:
                err = lib.hipStreamCreateWithPriority(C.byref(handle), C.c_uint(1), C.c_int(least.value))    # 1 = hipStreamNonBlocking
            if err != 0 or not handle.value:
                raise TdError(f"hipStreamCreateWithPriority(priority {least.value}) failed: hipError {err}")
            stream = torch.cuda.ExternalStream(handle.value, device=device_index)
        _low_priority_streams[device_index] = stream
        return stream
