"""ctypes binding of libdfd_hip.so (include/dfd_hip.h).

There is deliberately no fallback: if the shared library is missing, or no gfx950
device is visible, every compute entry point raises `DfdError`.
"""
from __future__ import annotations

import ctypes as C
import os
import threading
from typing import Optional

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("DFD_LIB_PATH") or os.path.join(_HERE, "libdfd_hip.so")   # DFD_LIB_PATH: diagnostic builds only

c_float_p = C.POINTER(C.c_float)
c_int32_p = C.POINTER(C.c_int32)
c_uint8_p = C.POINTER(C.c_uint8)


class DfdError(RuntimeError):
    def __init__(self, code: int, message: str):
        super().__init__(f"libdfd_hip: {message} (status {code})")
        self.code = code


# name -> (restype, argtypes); the single source of truth the symbol-export test walks
SIGNATURES = {
    "dfd_abi_version": (C.c_int, []),
    "dfd_create": (C.c_int, [C.c_int, C.c_void_p, C.c_size_t, C.c_int, C.POINTER(C.c_void_p)]),
    "dfd_destroy": (None, [C.c_void_p]),
    "dfd_last_error": (C.c_char_p, [C.c_void_p]),
    "dfd_max_batch": (C.c_int, [C.c_void_p]),
    "dfd_set_option": (C.c_int, [C.c_void_p, C.c_char_p, C.c_int]),
    "dfd_gemm_tile_count": (C.c_int, []),
    "dfd_warmup": (C.c_int, [C.c_void_p, C.c_int, C.c_int]),
    "dfd_tiles_export": (C.c_int, [C.c_void_p, C.c_void_p, C.c_size_t, C.POINTER(C.c_size_t)]),
    "dfd_tiles_import": (C.c_int, [C.c_void_p, C.c_char_p, C.c_size_t, C.POINTER(C.c_int)]),
    "dfd_gemm_chunk_rows": (C.c_longlong, [C.c_longlong, C.c_longlong, C.c_longlong]),
    "dfd_gemm_tap": (C.c_int, [C.c_void_p, C.c_void_p]),
    "dfd_device_alloc": (C.c_int, [C.c_void_p, C.c_size_t, C.POINTER(C.c_void_p)]),
    "dfd_device_free": (C.c_int, [C.c_void_p, C.c_void_p]),
    "dfd_memcpy_h2d": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t]),
    "dfd_memcpy_d2h": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t]),
    "dfd_sync": (C.c_int, [C.c_void_p]),
    "dfd_wait_for": (C.c_int, [C.c_void_p, C.c_void_p]),
    "dfd_frame_ptr": (C.c_void_p, [C.c_void_p]),
    "dfd_timer_begin": (C.c_int, [C.c_void_p]),
    "dfd_timer_end": (C.c_int, [C.c_void_p, c_float_p]),
    "dfd_classify_nchw": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p]),
    "dfd_classify_nchw_device": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p]),
    "dfd_extract_features": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p]),
    "dfd_b0_tap": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_char_p, C.c_void_p, C.c_size_t,
                              C.POINTER(C.c_size_t)]),
    "dfd_resize_bgr": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p]),
    "dfd_tta_augment": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_double, C.c_double,
                                  C.c_void_p]),
    "dfd_tta_augment_crops": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_int, C.c_int,
                                        C.c_void_p, C.c_void_p]),
    "dfd_classify_crops_tta": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_int, C.c_int,
                                         C.c_int, C.c_void_p, C.c_void_p]),
    "dfd_tta_arm": (C.c_int, [C.c_void_p, C.c_int, C.c_void_p, C.c_int]),
    "dfd_tta_logits": (C.c_int, [C.c_void_p, C.c_void_p, C.c_size_t, C.POINTER(C.c_int), C.POINTER(C.c_int)]),
    "dfd_preprocess_face_quality": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p]),
    "dfd_preprocess_crops": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_int,
                                       C.c_int, C.c_void_p]),
    "dfd_classify_crops": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_int,
                                     C.c_int, C.c_void_p]),
    "dfd_gradcam_nchw": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "dfd_gradcam_nchw_device": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p,
                                          C.c_void_p]),
    "dfd_gradcam_crops": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_int, C.c_int,
                                    C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "dfd_gradcam_tap": (C.c_int, [C.c_void_p, C.c_void_p]),
    "dfd_frequency_features": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p]),
    "dfd_frequency_domain": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_int, C.c_void_p]),
    "dfd_frequency_domain_device": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_int,
                                              C.c_void_p]),
    "dfd_frequency_domain_tap": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_char_p, C.c_void_p, C.c_size_t]),
    "dfd_frequency_features_sized": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p]),
    "dfd_frequency_features_tap": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_char_p,
                                             C.c_void_p, C.c_size_t]),
    "dfd_detect_faces": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_float, C.c_void_p,
                                   C.c_void_p, C.c_int, C.POINTER(C.c_int)]),
    "dfd_has_detector": (C.c_int, [C.c_void_p]),
    "dfd_last_detection_count": (C.c_int, [C.c_void_p]),
    "dfd_classifier_crop_count": (C.c_int, [C.c_void_p, C.POINTER(C.c_ulonglong)]),
    "dfd_ssd_tap": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_char_p, C.c_void_p,
                              C.c_size_t, C.POINTER(C.c_size_t)]),
    "dfd_ssd_detection_tap": (C.c_int, [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                        C.c_void_p, C.c_size_t, C.c_void_p]),
    "dfd_has_haar": (C.c_int, [C.c_void_p]),
    "dfd_detect_faces_haar": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_double, C.c_int, C.c_int,
                                        C.c_void_p, C.c_int, C.POINTER(C.c_int), C.POINTER(C.c_int)]),
    "dfd_haar_tap": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_double, C.c_int, C.c_char_p, C.c_void_p,
                               C.c_size_t, C.POINTER(C.c_size_t), C.c_void_p, C.POINTER(C.c_double)]),
    "dfd_has_mtcnn": (C.c_int, [C.c_void_p]),
    "dfd_mtcnn_align": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p,
                                  C.POINTER(C.c_int)]),
    "dfd_mtcnn_tap": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_char_p, C.c_void_p,
                                C.c_size_t, C.POINTER(C.c_size_t), C.c_void_p]),
    "dfd_mtcnn_tap_batch": (C.c_int, [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_char_p,
                                      C.c_void_p, C.c_size_t, C.c_void_p, C.c_void_p]),
    "dfd_mtcnn_net_tap": (C.c_int, [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_int, C.c_int,
                                    C.c_int, C.c_char_p, C.c_void_p, C.c_size_t, C.c_void_p, C.c_void_p]),
    "dfd_mtcnn_params_default": (None, [C.c_void_p]),
    "dfd_mtcnn_detect": (C.c_int, [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int,
                                   C.c_void_p, C.c_void_p, C.c_void_p]),
    "dfd_mtcnn_extract": (C.c_int, [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int,
                                    C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "dfd_analyze_frame": (C.c_int, [C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_float,
                                    C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.POINTER(C.c_int), C.c_void_p]),
    "dfd_jpeg_coefficients": (C.c_int, [C.c_void_p, C.c_size_t, C.POINTER(C.c_int), C.c_void_p, C.c_void_p, C.c_size_t,
                                        C.POINTER(C.c_size_t)]),
    "dfd_jpeg_coefficients_ex": (C.c_int, [C.c_void_p, C.c_size_t, C.c_uint, C.POINTER(C.c_int), C.c_void_p, C.c_void_p, C.c_size_t,
                                           C.POINTER(C.c_size_t)]),
    "dfd_decode_jpeg": (C.c_int, [C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p, C.c_size_t, C.POINTER(C.c_int),
                                  C.POINTER(C.c_int)]),
    "dfd_decode_jpeg_batch": (C.c_int, [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t, C.POINTER(C.c_int),
                                        C.POINTER(C.c_int)]),
    "dfd_encode_jpeg_bound": (C.c_size_t, [C.c_int, C.c_int, C.c_int]),
    "dfd_encode_jpeg": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int,
                                  C.c_void_p, C.c_size_t, C.POINTER(C.c_size_t)]),
    "dfd_encode_jpeg_batch": (C.c_int, [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p, C.c_void_p,
                                        C.POINTER(C.c_size_t)]),
    "dfd_encode_jpeg_device": (C.c_int, [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p, C.c_void_p,
                                         C.POINTER(C.c_size_t)]),
    "dfd_jpeg_decode_counts": (C.c_int, [C.c_void_p, C.POINTER(C.c_ulonglong), C.POINTER(C.c_ulonglong)]),
    "dfd_analyze_jpeg": (C.c_int, [C.c_void_p, C.c_int, C.c_void_p, C.c_size_t, C.c_int, C.c_float, C.c_int, C.c_int,
                                   C.c_void_p, C.c_void_p, C.c_void_p, C.POINTER(C.c_int), C.c_void_p, C.POINTER(C.c_int),
                                   C.POINTER(C.c_int)]),
    "dfd_analyze_stream_batch": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_void_p,
                                           C.c_float, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                           C.c_void_p, C.c_void_p, C.POINTER(C.c_int), C.POINTER(C.c_int)]),
    "dfd_analyze_batch_device": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_int,
                                           C.c_float, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p,
                                           C.c_void_p]),
    "dfd_forensics": (C.c_int, [C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int,
                                C.c_void_p, C.c_void_p, C.c_void_p]),
    "dfd_analyze_streams_batch": (C.c_int, [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                            C.c_void_p, C.c_float, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p,
                                            C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.POINTER(C.c_int)]),
    "dfd_forensics_reset": (C.c_int, [C.c_void_p, C.c_int]),
    "dfd_forensics_release": (C.c_int, [C.c_void_p, C.c_int]),
    "dfd_forensics_state": (C.c_int, [C.c_void_p, C.c_int, C.POINTER(C.c_int), C.POINTER(C.c_int),
                                      C.POINTER(C.c_int)]),
    "dfd_host_alloc": (C.c_int, [C.c_void_p, C.c_size_t, C.POINTER(C.c_void_p)]),
    "dfd_host_free": (C.c_int, [C.c_void_p, C.c_void_p]),
    "dfd_analyze_frames_host": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_int,
                                          C.c_float, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p,
                                          C.c_void_p]),
    "dfd_analyze_jpegs_host": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_int, C.c_float,
                                         C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                         C.POINTER(C.c_int), C.POINTER(C.c_int)]),
    "dfd_forensic_tap": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_char_p, C.c_void_p, C.c_char_p, C.c_int,
                                   C.c_void_p, C.c_size_t, C.POINTER(C.c_size_t)]),
    "dfd_forensics_sized": (C.c_int, [C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int,
                                      C.c_void_p, C.c_void_p, C.c_void_p]),
    "dfd_forensics_open": (C.c_int, [C.c_void_p, C.c_int, C.c_int]),
    "dfd_forensic_tap_sized": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_char_p, C.c_void_p, C.c_char_p,
                                         C.c_int, C.c_void_p, C.c_size_t, C.POINTER(C.c_size_t)]),
    "dfd_forensic_signals_device": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p,
                                              C.c_void_p, C.c_void_p]),
    "dfd_comm_unique_id": (C.c_int, [C.c_void_p]),
    "dfd_comm_init": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int]),
    "dfd_comm_destroy": (C.c_int, [C.c_void_p]),
    "dfd_comm_info": (C.c_int, [C.c_void_p, C.POINTER(C.c_int), C.POINTER(C.c_int)]),
    "dfd_vote_allgather": (C.c_int, [C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p]),
    "dfd_vote_allgather_waves": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_size_t, C.c_void_p]),
    "dfd_b0_profile_begin": (C.c_int, [C.c_void_p]),
    "dfd_b0_profile_end": (C.c_int, [C.c_void_p, c_float_p, C.POINTER(C.c_char_p), C.c_int,
                                      C.POINTER(C.c_int), C.POINTER(C.c_int)]),
    "dfd_head_config_default": (None, [C.c_void_p]),
    "dfd_head_train_begin": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p]),
    "dfd_head_train_accumulate": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_float, C.c_float,
                                            c_float_p, C.c_void_p]),
    "dfd_head_train_apply": (C.c_int, [C.c_void_p, C.c_float, c_float_p]),
    "dfd_head_train_eval": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_void_p]),
    "dfd_head_train_export": (C.c_int, [C.c_void_p, C.c_int, C.c_void_p]),
    "dfd_head_train_grads": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int]),
    "dfd_head_train_tap": (C.c_int, [C.c_void_p, C.c_char_p, C.c_void_p, C.c_size_t]),
    "dfd_head_train_commit": (C.c_int, [C.c_void_p, C.c_int]),
    "dfd_head_train_end": (C.c_int, [C.c_void_p]),
    "dfd_extract_trunk": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p]),
    "dfd_train_augment_trunk": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p,
                                          C.c_void_p]),
    "dfd_head_train_unfreeze_conv": (C.c_int, [C.c_void_p, C.c_void_p, C.c_float, C.c_float, C.c_float]),
    "dfd_head_train_accumulate_trunk": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_float, C.c_float,
                                                  c_float_p, C.c_void_p]),
    "dfd_head_train_eval_trunk": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_void_p]),
    "dfd_head_train_export_conv": (C.c_int, [C.c_void_p, C.c_int, C.c_void_p]),
    "dfd_head_train_conv_grads": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int]),
    "dfd_extract_trunk_at": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_void_p]),
    "dfd_train_augment_trunk_at": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p,
                                             C.c_int, C.c_void_p]),
    "dfd_head_train_unfreeze_block": (C.c_int, [C.c_void_p, C.c_int, C.c_void_p, C.c_float, C.c_float]),
    "dfd_head_train_accumulate_block": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_float, C.c_float,
                                                  c_float_p, C.c_void_p]),
    "dfd_head_train_eval_block": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_void_p]),
    "dfd_head_train_export_block": (C.c_int, [C.c_void_p, C.c_int, C.c_void_p]),
    "dfd_head_train_block_grads": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int]),
    "dfd_head_train_unfreeze_block_at": (C.c_int, [C.c_void_p, C.c_int, C.c_void_p, C.c_float, C.c_float, C.c_float]),
    "dfd_head_train_export_block_at": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_void_p]),
    "dfd_head_train_block_grads_at": (C.c_int, [C.c_void_p, C.c_int, C.c_void_p, C.c_int]),
    "dfd_extract_block_out": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_void_p]),
    "dfd_train_augment_block_out": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p,
                                              C.c_int, C.c_void_p]),
    "dfd_extract_block_input": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_void_p]),
    "dfd_extract_block_rows": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_void_p]),
    "dfd_train_augment_block_rows": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p,
                                               C.c_int, C.c_void_p]),
    "dfd_train_augment_block_input": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p,
                                              C.c_int, C.c_void_p]),
    "dfd_train_augment": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p]),
    "dfd_train_augment_features": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p,
                                             C.c_void_p]),
    "dfd_train_augment_gather": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_int, C.c_void_p]),
    "dfd_train_augment_noise_words": (C.c_int, [C.c_ulonglong, C.c_ulonglong, C.c_int, C.c_uint, C.c_uint, C.c_void_p, C.c_void_p]),
    "dfd_train_augment_tap": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p,
                                        C.c_char_p, C.c_void_p, C.c_size_t]),
}


GEMM_TAP_GUARD = 64                  # DFD_GEMM_TAP_GUARD: guard rows in front of and behind the result
GEMM_TAP_SENTINEL = 0x7FC5A5A5       # DFD_GEMM_TAP_SENTINEL (fp32 bits; bf16: the upper 16)
GEMM_TAP_UNSUPPORTED = -7            # DFD_ERR_UNSUPPORTED: a shape the launchers refuse
GEMM_ACTS = {None: 0, "none": 0, "swish": 1, "relu": 2, "prelu": 3}


class GemmTapParams(C.Structure):
    """`dfd_gemm_tap_params` (include/dfd_hip.h)"""
    _fields_ = ([(k, C.c_int32) for k in ("conv", "bf16", "planes", "act", "res_first", "reserved", "M", "K", "N", "HW", "n_img", "H",
                                          "W", "Cin", "ksize", "stride", "pad", "dil", "Ho", "Wo")] +
                [("x_rows", C.c_int64)] + [(k, C.c_void_p) for k in ("X", "Wt", "bias", "gate", "R", "Y")] +
                [("candidates", C.c_int32), ("launches", C.c_int32), ("tile", C.c_int32 * 6)] +
                [("n_ranges", C.c_int32), ("reserved2", C.c_int32), ("y_ranges", C.c_void_p), ("y_sentinels", C.c_uint64),
                 ("y_digest", C.c_uint64)])


GRADCAM_TAP_GUARD = 8                # DFD_GRADCAM_TAP_GUARD: guard rows behind D1, G and cam7
GRADCAM_TAP_SENTINEL = 0x7FC5A5A5    # DFD_GRADCAM_TAP_SENTINEL


class GradcamTapParams(C.Structure):
    """`dfd_gradcam_tap_params` (include/dfd_hip.h)"""
    _fields_ = ([(k, C.c_int32) for k in ("start", "n", "z_bf16", "reserved")] +
                [(k, C.c_void_p) for k in ("x", "z", "fc1", "fc2", "D1", "G", "cam7", "heat", "overlay")])


class MtcnnParams(C.Structure):
    """`dfd_mtcnn_params` (include/dfd_hip.h): the constructor arguments of facenet_pytorch.MTCNN."""
    _fields_ = [("image_size", C.c_int), ("margin", C.c_int), ("min_face_size", C.c_int), ("thresholds", C.c_float * 3),
                ("factor", C.c_double), ("selection", C.c_int), ("keep_all", C.c_int), ("post_process", C.c_int)]


class JpegSource(C.Structure):
    """`dfd_jpeg_source` (include/dfd_hip.h): one image of a batched JPEG encode."""
    _fields_ = [("pixels", C.c_void_p), ("height", C.c_int32), ("width", C.c_int32), ("stride", C.c_int32), ("rgb", C.c_int32),
                ("quality", C.c_int32), ("subsampling", C.c_int32), ("restart_blocks", C.c_int32)]


JPEG_GRAY = 3                 # DFD_JPEG_GRAY; 0 / 1 / 2 = 4:4:4 / 4:2:2 / 4:2:0 as in Pillow
JPEG_ENC_SCAN_TILE = 1024     # blocks one workgroup of the encoder's prefix sum covers in one pass (csrc/jpeg_encode.hip kEncScanTile)


HEAD_FIELDS = ("w1", "b1", "g1", "be1", "rm1", "rv1", "w2", "b2", "g2", "be2", "rm2", "rv2", "w3", "b3")
HEAD_SHAPES = {"w1": (512, 1280), "b1": (512,), "g1": (512,), "be1": (512,), "rm1": (512,), "rv1": (512,),
               "w2": (256, 512), "b2": (256,), "g2": (256,), "be2": (256,), "rm2": (256,), "rv2": (256,),
               "w3": (1, 256), "b3": (1,)}


class HeadParams(C.Structure):
    """`dfd_head_params` (include/dfd_hip.h): host arrays of the unfolded head, torch layouts."""
    _fields_ = [(k, C.c_void_p) for k in HEAD_FIELDS]


TRUNK_SHAPE = (7, 7, 320)     # block 15's output of one crop, NHWC (DFD_TRUNK_ROW floats)
TRUNK_ROW = 7 * 7 * 320
CONV_FIELDS = ("w", "g", "be", "rm", "rv")
CONV_SHAPES = {"w": (1280, 320), "g": (1280,), "be": (1280,), "rm": (1280,), "rv": (1280,)}


class HeadConvParams(C.Structure):
    """`dfd_headconv_params` (include/dfd_hip.h): host arrays of net._conv_head / net._bn1, torch layouts."""
    _fields_ = [(k, C.c_void_p) for k in CONV_FIELDS]


def _conv_arrays(arrays=None, skip=()):
    """(HeadConvParams, dict of the float32 arrays it points to); missing entries are allocated"""
    out, cp = {}, HeadConvParams()
    for k in CONV_FIELDS:
        if k in skip:
            continue
        if arrays is not None and k in arrays:
            a = np.ascontiguousarray(np.asarray(arrays[k], dtype=np.float32).reshape(CONV_SHAPES[k]))
        else:
            a = np.zeros(CONV_SHAPES[k], np.float32)
        out[k] = a
        setattr(cp, k, a.ctypes.data)
    return cp, out


BLOCK14_SHAPE = (7, 7, 192)   # block 14's output of one crop, NHWC (DFD_BLOCK14_ROW floats): the rows block 15's stage trains on
BLOCK14_ROW = 7 * 7 * 192
TRUNK_SHAPES = {14: BLOCK14_SHAPE, 15: TRUNK_SHAPE}
BLOCK_FIELDS = ("exp_w", "dw_w", "se_w1", "se_b1", "se_w2", "se_b2", "proj_w",
                "g0", "be0", "rm0", "rv0", "g1", "be1", "rm1", "rv1", "g2", "be2", "rm2", "rv2")
BLOCK_STAT_FIELDS = ("rm0", "rv0", "rm1", "rv1", "rm2", "rv2")
BLOCK_SHAPES = {"exp_w": (1152, 192), "dw_w": (1152, 3, 3), "se_w1": (48, 1152), "se_b1": (48,), "se_w2": (1152, 48),
                "se_b2": (1152,), "proj_w": (320, 1152)}
BLOCK_SHAPES.update({k + str(l): ((1152,) if l < 2 else (320,)) for l in range(3) for k in ("g", "be", "rm", "rv")})
# block 14 in the same struct (k5, 192 -> 1152 -> 192); blocks 13 and 12 have these shapes too
BLOCK14_SHAPES = dict(BLOCK_SHAPES, dw_w=(1152, 5, 5), proj_w=(192, 1152), g2=(192,), be2=(192,), rm2=(192,), rv2=(192,))
# block 11 in the same struct (k5 at stride 2, 112 -> 672 -> 192, squeeze-excite 28)
BLOCK11_SHAPES = {"exp_w": (672, 112), "dw_w": (672, 5, 5), "se_w1": (28, 672), "se_b1": (28,), "se_w2": (672, 28), "se_b2": (672,),
                  "proj_w": (192, 672)}
BLOCK11_SHAPES.update({k + str(l): ((672,) if l < 2 else (192,)) for l in range(3) for k in ("g", "be", "rm", "rv")})
BLOCK_SHAPES_AT = {15: BLOCK_SHAPES, 14: BLOCK14_SHAPES, 13: BLOCK14_SHAPES, 12: BLOCK14_SHAPES, 11: BLOCK11_SHAPES}
BLOCK11_INPUT_SHAPE = (14, 14, 112)   # block 10's output of one crop, NHWC (DFD_BLOCK11_INPUT_ROW floats): the rows block 11's stage trains on
BLOCK11_INPUT_ROW = 14 * 14 * 112
BLOCK_ROWS_SHAPES = {11: BLOCK11_INPUT_SHAPE, 12: BLOCK14_SHAPE, 13: BLOCK14_SHAPE, 14: BLOCK14_SHAPE, 15: BLOCK14_SHAPE}
BLOCK_OUT_SHAPES = {13: BLOCK14_SHAPE, 14: BLOCK14_SHAPE, 15: TRUNK_SHAPE}     # what `Handle.extract_block` returns per crop


class MBConvParams(C.Structure):
    """`dfd_mbconv_params` (include/dfd_hip.h): host arrays of net._blocks.15, torch layouts."""
    _fields_ = [(k, C.c_void_p) for k in BLOCK_FIELDS]


def _block_arrays(arrays=None, skip=(), block: int = 15):
    """(MBConvParams, dict of the float32 arrays it points to); missing entries are allocated; `block`: whose shapes"""
    out, bp = {}, MBConvParams()
    shapes = BLOCK_SHAPES_AT.get(int(block), BLOCK_SHAPES)
    for k in BLOCK_FIELDS:
        if k in skip:
            continue
        if arrays is not None and k in arrays:
            a = np.ascontiguousarray(np.asarray(arrays[k], dtype=np.float32).reshape(shapes[k]))
        else:
            a = np.zeros(shapes[k], np.float32)
        out[k] = a
        setattr(bp, k, a.ctypes.data)
    return bp, out


class HeadConfig(C.Structure):
    """`dfd_head_config` (include/dfd_hip.h)"""
    _fields_ = [("max_n", C.c_int), ("seed", C.c_ulonglong), ("dropout", C.c_float), ("beta1", C.c_float), ("beta2", C.c_float),
                ("eps", C.c_float), ("weight_decay", C.c_float), ("focal_gamma", C.c_float), ("focal_alpha", C.c_float),
                ("label_smoothing", C.c_float), ("clip_norm", C.c_float), ("ema_decay", C.c_float), ("bn_momentum", C.c_float)]


def head_config(**kw) -> HeadConfig:
    """The library's defaults (dfd_head_config_default: train.py's argparse defaults), then the given fields."""
    c = HeadConfig()
    load().dfd_head_config_default(C.byref(c))
    names = {f[0] for f in HeadConfig._fields_}
    for k, v in kw.items():
        if k not in names:
            raise TypeError(f"unknown head-training setting {k!r}")
        setattr(c, k, int(v) if k in ("max_n", "seed") else float(v))
    return c


def _head_arrays(arrays=None, skip=()):
    """(HeadParams, dict of the float32 arrays it points to); missing entries are allocated"""
    out, hp = {}, HeadParams()
    for k in HEAD_FIELDS:
        if k in skip:
            continue
        if arrays is not None and k in arrays:
            a = np.ascontiguousarray(np.asarray(arrays[k], dtype=np.float32).reshape(HEAD_SHAPES[k]))
        else:
            a = np.zeros(HEAD_SHAPES[k], np.float32)
        out[k] = a
        setattr(hp, k, a.ctypes.data)
    return hp, out


class TtaDraw(C.Structure):
    """`dfd_tta_draw` (include/dfd_hip.h): one augmented copy's flip, brightness and rotation angle."""
    _fields_ = [("flip", C.c_int32), ("reserved", C.c_int32), ("brightness", C.c_double), ("angle_deg", C.c_double)]


def tta_draws(draws, rows: int, copies: int):
    """[(flip, brightness, angle_deg), ...] (face-major, rows x copies of them) -> a `dfd_tta_draw` array"""
    draws = list(draws)
    if copies < 1 or len(draws) != rows * copies:
        raise ValueError(f"expected {rows} x {copies} draws, got {len(draws)}")
    arr = (TtaDraw * len(draws))()
    for d, (flip, brightness, angle) in zip(arr, draws):
        d.flip, d.brightness, d.angle_deg = int(bool(flip)), float(brightness), float(angle)
    return arr


MT_SELECT = {None: 0, "none": 0, "probability": 1, "largest": 2, "center_weighted_size": 3, "largest_over_threshold": 4}


def mtcnn_params(image_size=160, margin=0, min_face_size=20, thresholds=(0.6, 0.7, 0.7), factor=0.709, selection="largest",
                 keep_all=False, post_process=True) -> MtcnnParams:
    """The package's defaults from the library (dfd_mtcnn_params_default), then the given values."""
    p = MtcnnParams()
    load().dfd_mtcnn_params_default(C.byref(p))
    if selection not in MT_SELECT:
        raise ValueError(f"unknown selection {selection!r}")
    p.image_size, p.margin, p.min_face_size = int(image_size), int(margin), int(min_face_size)
    p.thresholds = (C.c_float * 3)(*[float(t) for t in thresholds])
    p.factor = float(factor)
    p.selection, p.keep_all, p.post_process = MT_SELECT[selection], int(bool(keep_all)), int(bool(post_process))
    return p


_lib: Optional[C.CDLL] = None
_lock = threading.Lock()


def load() -> C.CDLL:
    """Load the shared library and declare every prototype.  Raises if it is not built."""
    global _lib
    with _lock:
        if _lib is not None:
            return _lib
        if not os.path.exists(LIB_PATH):
            raise DfdError(-100, f"{LIB_PATH} not built; run `python -c 'import __graft_entry__ as g; g.build()'` "
                                 "or `make -C real-time-video-deepfake-detection_amd/csrc`")
        lib = C.CDLL(LIB_PATH)
        for name, (res, args) in SIGNATURES.items():
            fn = getattr(lib, name)      # AttributeError here = header/library drift
            fn.restype = res
            fn.argtypes = args
        _lib = lib
        return lib


def _ptr(a: np.ndarray):
    return a.ctypes.data_as(C.c_void_p)


JPEG_ALLOW_PROGRESSIVE = 1       # DFD_JPEG_ALLOW_PROGRESSIVE


def jpeg_coefficients(data: bytes, progressive: bool = False):
    """Host half of the JPEG decoder (no GPU): -> dict(width, height, components, hmax, vmax, comps=[(bw, bh, tq)],
    qtables (4,64) uint16, coef int16 flat).  Raises DfdError (code -7 = flavour not decoded on the device path).
    progressive: take complete progressive files too (dfd_jpeg_coefficients_ex with DFD_JPEG_ALLOW_PROGRESSIVE; what option
    "jpeg_progressive" is to a handle's calls)"""
    lib = load()
    buf = (C.c_char * len(data)).from_buffer_copy(data)
    info = (C.c_int * 16)()
    cnt = C.c_size_t()
    if progressive:
        def call(*a):
            return lib.dfd_jpeg_coefficients_ex(buf, len(data), JPEG_ALLOW_PROGRESSIVE, *a)
    else:
        def call(*a):
            return lib.dfd_jpeg_coefficients(buf, len(data), *a)
    rc = call(info, None, None, 0, C.byref(cnt))
    if rc != 0:
        raise DfdError(rc, (lib.dfd_last_error(None) or b"").decode())
    q = np.zeros((4, 64), np.uint16)
    coef = np.zeros(cnt.value, np.int16)
    rc = call(info, _ptr(q), _ptr(coef), coef.size, C.byref(cnt))
    if rc != 0:
        raise DfdError(rc, (lib.dfd_last_error(None) or b"").decode())
    n = info[2]
    return {"width": info[0], "height": info[1], "components": n, "hmax": info[3], "vmax": info[4],
            "comps": [(info[5 + 3 * c], info[6 + 3 * c], info[7 + 3 * c]) for c in range(n)], "qtables": q, "coef": coef}


def train_augment_noise_words(seed: int, counter: int, row: int, first: int, count: int):
    """the two uint32 words behind elements first .. first + count - 1 of image `row`, from the functions `aug_noise_kernel`
    calls (host side, no GPU): what train_augment.noise_words specifies"""
    u1, u2 = np.empty(count, np.uint32), np.empty(count, np.uint32)
    rc = load().dfd_train_augment_noise_words(int(seed) & (2 ** 64 - 1), int(counter) & (2 ** 64 - 1), int(row), int(first), int(count),
                                              _ptr(u1), _ptr(u2))
    if rc != 0:
        raise DfdError(rc, "train_augment_noise_words: bad arguments")
    return u1, u2


class DeviceBuffer:
    """A raw HBM allocation owned by a Handle."""

    def __init__(self, handle: "Handle", nbytes: int):
        self._h = handle
        self.nbytes = int(nbytes)
        p = C.c_void_p()
        handle._check(handle._lib.dfd_device_alloc(handle._p, self.nbytes, C.byref(p)))
        self.ptr = p.value

    def upload(self, a: np.ndarray, offset: int = 0) -> "DeviceBuffer":
        """host array -> the buffer, `offset` bytes in (a large buffer filled slab by slab)"""
        a = np.ascontiguousarray(a)
        if offset < 0 or offset + a.nbytes > self.nbytes:
            raise ValueError("upload larger than buffer")
        self._h._check(self._h._lib.dfd_memcpy_h2d(self._h._p, self.ptr + int(offset), _ptr(a), a.nbytes))
        return self

    def download(self, shape, dtype=np.float32, offset: int = 0) -> np.ndarray:
        out = np.empty(shape, dtype=dtype)
        if offset < 0 or offset + out.nbytes > self.nbytes:
            raise ValueError("download larger than buffer")
        self._h._check(self._h._lib.dfd_memcpy_d2h(self._h._p, _ptr(out), self.ptr + int(offset), out.nbytes))
        return out

    def free(self):
        if self.ptr:
            self._h._lib.dfd_device_free(self._h._p, self.ptr)
            self.ptr = None


class Handle:
    """One (device, stream) context of the library: weights + workspaces for `max_batch` crops."""

    def __init__(self, blob: bytes, device: int = 0, max_batch: int = 8):
        self._lib = load()
        self._blob = blob                      # keep alive during create
        p = C.c_void_p()
        buf = (C.c_char * len(blob)).from_buffer_copy(blob)
        rc = self._lib.dfd_create(int(device), buf, len(blob), int(max_batch), C.byref(p))
        if rc != 0:
            msg = self._lib.dfd_last_error(None)
            raise DfdError(rc, (msg or b"dfd_create failed").decode())
        self._p = p
        self.device = int(device)
        self.max_batch = int(max_batch)

    # -- plumbing
    def _check(self, rc: int):
        if rc != 0:
            raise DfdError(rc, (self._lib.dfd_last_error(self._p) or b"").decode())

    def close(self):
        if getattr(self, "_p", None):
            self._lib.dfd_destroy(self._p)
            self._p = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def set_option(self, name: str, value: int):
        self._check(self._lib.dfd_set_option(self._p, name.encode(), int(value)))

    def warmup(self, n_crops: int = 0, n_frames: int = 0):
        """Measure the split-GEMM tiles for these batch sizes (synchronises; serving calls never do).
        With DFD_TILE_CACHE=<file> in the environment the measured tiles are loaded from / saved to that file, so
        that e.g. a run under rocprofv3 launches no tuning candidates."""
        cache = os.environ.get("DFD_TILE_CACHE")
        if cache and os.path.exists(cache):
            self.tiles_import(open(cache).read())
        self._check(self._lib.dfd_warmup(self._p, int(n_crops), int(n_frames)))
        if cache:
            try:
                with open(cache, "w") as f:
                    f.write(self.tiles_export())
            except OSError:
                pass

    def tiles_export(self) -> str:
        n = C.c_size_t()
        self._check(self._lib.dfd_tiles_export(self._p, None, 0, C.byref(n)))
        buf = C.create_string_buffer(n.value + 1)
        self._check(self._lib.dfd_tiles_export(self._p, buf, n.value, C.byref(n)))
        return buf.raw[: n.value].decode()

    def tiles_import(self, text: str) -> int:
        acc = C.c_int()
        b = text.encode()
        self._check(self._lib.dfd_tiles_import(self._p, b, len(b), C.byref(acc)))
        return acc.value

    def alloc(self, nbytes: int) -> DeviceBuffer:
        return DeviceBuffer(self, nbytes)

    def sync(self):
        self._check(self._lib.dfd_sync(self._p))

    def wait_for(self, other: "Handle"):
        """work queued on this handle from now on starts after what `other` has queued so far (no host wait)"""
        self._check(self._lib.dfd_wait_for(self._p, other._p))

    def timer_begin(self):
        self._check(self._lib.dfd_timer_begin(self._p))

    def timer_end(self) -> float:
        ms = C.c_float()
        self._check(self._lib.dfd_timer_end(self._p, C.byref(ms)))
        return float(ms.value)

    # -- classifier
    @staticmethod
    def _as_nchw(x) -> np.ndarray:
        a = np.ascontiguousarray(np.asarray(x, dtype=np.float32))
        if a.ndim != 4 or a.shape[1:] != (3, 224, 224):
            raise ValueError(f"expected (B,3,224,224) float input, got {a.shape}")
        return a

    def classify(self, x) -> np.ndarray:
        a = self._as_nchw(x)
        out = np.empty((a.shape[0], 1), dtype=np.float32)
        self._check(self._lib.dfd_classify_nchw(self._p, _ptr(a), a.shape[0], _ptr(out)))
        return out

    def classify_device(self, x_dev: int, n: int, logits_dev: int):
        self._check(self._lib.dfd_classify_nchw_device(self._p, x_dev, int(n), logits_dev))

    def extract_features(self, x) -> np.ndarray:
        a = self._as_nchw(x)
        out = np.empty((a.shape[0], 1280), dtype=np.float32)
        self._check(self._lib.dfd_extract_features(self._p, _ptr(a), a.shape[0], _ptr(out)))
        return out

    def extract_trunk(self, x, block: int = 15) -> np.ndarray:
        """block 15's output, (n,7,7,320) float32 NHWC: the rows the head trainer's conv stage trains on; `block=14`:
        block 14's, (n,7,7,192), the rows block 15's stage trains on"""
        a = self._as_nchw(x)
        if block == 15:
            out = np.empty((a.shape[0],) + TRUNK_SHAPE, dtype=np.float32)
            self._check(self._lib.dfd_extract_trunk(self._p, _ptr(a), a.shape[0], _ptr(out)))
            return out
        out = np.empty((a.shape[0],) + TRUNK_SHAPES.get(int(block), TRUNK_SHAPE), dtype=np.float32)
        self._check(self._lib.dfd_extract_trunk_at(self._p, _ptr(a), a.shape[0], int(block), _ptr(out)))
        return out

    def extract_block(self, x, block: int) -> np.ndarray:
        """the output of block 13, 14 or 15, float32 NHWC (`dfd_extract_block_out`): (n,7,7,192) for 13 and 14 - block 13's
        are the rows block 14's stage trains on - and (n,7,7,320) for 15; any other block is refused"""
        a = self._as_nchw(x)
        out = np.empty((a.shape[0],) + BLOCK_OUT_SHAPES.get(int(block), TRUNK_SHAPE), dtype=np.float32)
        self._check(self._lib.dfd_extract_block_out(self._p, _ptr(a), a.shape[0], int(block), _ptr(out)))
        return out

    def extract_block_input(self, x, block: int) -> np.ndarray:
        """the input rows of block 12, 13, 14 or 15, (n,7,7,192) float32 NHWC (`dfd_extract_block_input`): the output of the
        block below, the rows a trainer whose deepest unfrozen block is `block` trains on; any other block is refused"""
        a = self._as_nchw(x)
        out = np.empty((a.shape[0],) + BLOCK14_SHAPE, dtype=np.float32)
        self._check(self._lib.dfd_extract_block_input(self._p, _ptr(a), a.shape[0], int(block), _ptr(out)))
        return out

    def extract_block_rows(self, x, block: int) -> np.ndarray:
        """`extract_block_input` with block 11 as well (`dfd_extract_block_rows`): (n,7,7,192) for 12..15 - the older entry's
        bits - and (n,14,14,112), block 10's output, for 11: the rows a trainer whose deepest unfrozen block is `block` trains
        on; any other block is refused"""
        a = self._as_nchw(x)
        out = np.empty((a.shape[0],) + BLOCK_ROWS_SHAPES.get(int(block), BLOCK14_SHAPE), dtype=np.float32)
        self._check(self._lib.dfd_extract_block_rows(self._p, _ptr(a), a.shape[0], int(block), _ptr(out)))
        return out

    # -- train-time augmentation (include/dfd_hip.h "train-time image augmentation"; train_augment.draw_batch makes the tables)
    @staticmethod
    def _aug_tables(n, rows, batch):
        """(rows array, batch record with its partner pointer set, the partner array) for `n` images - kept alive by the caller"""
        from . import train_augment as TA
        r = np.ascontiguousarray(np.asarray(rows, dtype=TA.ROW_DTYPE)).reshape(-1)
        if r.size != n:
            raise ValueError(f"{n} images but {r.size} parameter rows")
        b = np.array(batch, dtype=TA.BATCH_DTYPE).reshape(())
        partners = TA.batch_perm(batch)
        if partners is not None:
            partners = np.ascontiguousarray(np.asarray(partners, np.int32))
            if partners.size != n:
                raise ValueError("one mix partner per image")
        b["perm"] = partners.ctypes.data if partners is not None else 0
        return r, b, partners

    @classmethod
    def _aug_args(cls, rgb, rows, batch):
        """(uint8 (n,H,W,3) array, rows array, batch record, partner array)"""
        a = np.ascontiguousarray(np.asarray(rgb))
        if a.dtype != np.uint8 or a.ndim != 4 or a.shape[3] != 3:
            raise ValueError(f"expected (n,H,W,3) uint8 crops, got {a.dtype} {a.shape}")
        return (a,) + cls._aug_tables(a.shape[0], rows, batch)

    AUG_U8_STAGES = ("jpeg", "resize", "crop", "jitter0", "jitter1", "jitter2", "jitter3", "gray", "rotate", "affine", "perspective", "blur")
    AUG_F32_STAGES = ("norm", "erase", "noise", "mix")

    def train_augment(self, rgb, rows, batch, out_size: int = 224) -> np.ndarray:
        """the augmentation chain alone: (n,H,W,3) uint8 -> (n,3,T,T) float32"""
        a, r, b, _keep = self._aug_args(rgb, rows, batch)
        out = np.empty((a.shape[0], 3, int(out_size), int(out_size)), np.float32)
        self._check(self._lib.dfd_train_augment(self._p, _ptr(a), a.shape[0], a.shape[1], a.shape[2], int(out_size), _ptr(r), _ptr(b),
                                                _ptr(out)))
        return out

    def train_augment_tap(self, rgb, rows, batch, stage: str, out_size: int = 224) -> np.ndarray:
        """the images after `stage`: uint8 (n,T,T,3) ("jpeg": (n,H,W,3); "resize": (n,T+20,T+20,3) slots), float32 (n,3,T,T)
        from "norm" on"""
        a, r, b, _keep = self._aug_args(rgb, rows, batch)
        n, t = a.shape[0], int(out_size)
        if stage in self.AUG_F32_STAGES:
            out = np.empty((n, 3, t, t), np.float32)
        elif stage == "jpeg":
            out = np.empty(a.shape, np.uint8)
        elif stage == "resize":
            out = np.zeros((n, t + 20, t + 20, 3), np.uint8)
        else:
            out = np.empty((n, t, t, 3), np.uint8)
        self._check(self._lib.dfd_train_augment_tap(self._p, _ptr(a), n, a.shape[1], a.shape[2], t, _ptr(r), _ptr(b), stage.encode(),
                                                    _ptr(out), out.nbytes))
        return out

    def train_augment_gather(self, src: "DeviceBuffer", shape, idx, dst: "DeviceBuffer"):
        """crops `idx` of the resident (N,H,W,3) uint8 set in `src` (`shape` = (N,H,W)) -> contiguous in `dst` (device to device)"""
        n_src, hh, ww = (int(v) for v in shape)
        i = np.ascontiguousarray(np.asarray(idx, np.int32)).reshape(-1)
        if n_src * hh * ww * 3 > src.nbytes or i.size * hh * ww * 3 > dst.nbytes:
            raise ValueError("shape larger than the device buffer")
        self._check(self._lib.dfd_train_augment_gather(self._p, C.c_void_p(src.ptr), n_src, hh, ww, _ptr(i), i.size, C.c_void_p(dst.ptr)))

    def _train_augment_forward(self, fn, width, rgb, rows, batch, shape):
        if isinstance(rgb, DeviceBuffer):
            n, hh, ww = (int(v) for v in shape)
            if n * hh * ww * 3 > rgb.nbytes:
                raise ValueError("shape larger than the device buffer")
            r, b, _keep = self._aug_tables(n, rows, batch)
            src, on_device = C.c_void_p(rgb.ptr), 1
        else:
            a, r, b, _keep = self._aug_args(rgb, rows, batch)
            n, hh, ww = a.shape[:3]
            src, on_device = _ptr(a), 0
        out = np.empty((n,) + width, np.float32)
        self._check(fn(self._p, src, on_device, n, hh, ww, _ptr(r), _ptr(b), _ptr(out)))
        return out

    def train_augment_features(self, rgb, rows, batch, shape=None) -> np.ndarray:
        """chain at 224 + backbone -> (n,1280) pooled features.  `rgb`: (n,H,W,3) uint8, or a DeviceBuffer holding such an
        array with `shape` = (n,H,W) (a resident training set costs no upload)"""
        return self._train_augment_forward(self._lib.dfd_train_augment_features, (1280,), rgb, rows, batch, shape)

    def train_augment_trunk(self, rgb, rows, batch, shape=None, block: int = 15) -> np.ndarray:
        """`train_augment_features` with block 15's output in place of the pooled rows -> (n,7,7,320); `block=14`:
        block 14's -> (n,7,7,192)"""
        if block == 15:
            return self._train_augment_forward(self._lib.dfd_train_augment_trunk, TRUNK_SHAPE, rgb, rows, batch, shape)

        def fn(p, src, on_device, n, hh, ww, r, b, out):
            return self._lib.dfd_train_augment_trunk_at(p, src, on_device, n, hh, ww, r, b, int(block), out)

        return self._train_augment_forward(fn, TRUNK_SHAPES.get(int(block), TRUNK_SHAPE), rgb, rows, batch, shape)

    def train_augment_block14(self, rgb, rows, batch, shape=None) -> np.ndarray:
        """`train_augment_trunk(block=14)`: the extractor of a trainer with block 15 unfrozen"""
        return self.train_augment_trunk(rgb, rows, batch, shape, block=14)

    def train_augment_block(self, rgb, rows, batch, shape=None, block: int = 13) -> np.ndarray:
        """`train_augment_features` with the output of block 13, 14 or 15 in place of the pooled rows
        (`dfd_train_augment_block_out`)"""
        def fn(p, src, on_device, n, hh, ww, r, b, out):
            return self._lib.dfd_train_augment_block_out(p, src, on_device, n, hh, ww, r, b, int(block), out)

        return self._train_augment_forward(fn, BLOCK_OUT_SHAPES.get(int(block), TRUNK_SHAPE), rgb, rows, batch, shape)

    def train_augment_block13(self, rgb, rows, batch, shape=None) -> np.ndarray:
        """`train_augment_block(block=13)`: the extractor of a trainer with block 14 unfrozen"""
        return self.train_augment_block(rgb, rows, batch, shape, block=13)

    def train_augment_block_input(self, rgb, rows, batch, block: int = 12, shape=None) -> np.ndarray:
        """`train_augment_features` with the input rows of block 12, 13, 14 or 15 in place of the pooled rows -> (n,7,7,192)
        (`dfd_train_augment_block_input`)"""
        def fn(p, src, on_device, n, hh, ww, r, b, out):
            return self._lib.dfd_train_augment_block_input(p, src, on_device, n, hh, ww, r, b, int(block), out)

        return self._train_augment_forward(fn, BLOCK14_SHAPE, rgb, rows, batch, shape)

    def train_augment_block_rows(self, rgb, rows, batch, block: int = 11, shape=None) -> np.ndarray:
        """`train_augment_block_input` with block 11 as well -> (n,14,14,112) for 11, (n,7,7,192) for 12..15
        (`dfd_train_augment_block_rows`)"""
        def fn(p, src, on_device, n, hh, ww, r, b, out):
            return self._lib.dfd_train_augment_block_rows(p, src, on_device, n, hh, ww, r, b, int(block), out)

        return self._train_augment_forward(fn, BLOCK_ROWS_SHAPES.get(int(block), BLOCK14_SHAPE), rgb, rows, batch, shape)

    def train_augment_rows11(self, rgb, rows, batch, shape=None) -> np.ndarray:
        """`train_augment_block_rows(block=11)`: the extractor of a trainer with block 11 unfrozen"""
        return self.train_augment_block_rows(rgb, rows, batch, block=11, shape=shape)

    def train_augment_input13(self, rgb, rows, batch, shape=None) -> np.ndarray:
        """`train_augment_block_input(block=13)`: the extractor of a trainer with block 13 unfrozen"""
        return self.train_augment_block_input(rgb, rows, batch, block=13, shape=shape)

    def train_augment_input12(self, rgb, rows, batch, shape=None) -> np.ndarray:
        """`train_augment_block_input(block=12)`: the extractor of a trainer with block 12 unfrozen"""
        return self.train_augment_block_input(rgb, rows, batch, block=12, shape=shape)

    # -- head training (include/dfd_hip.h "classifier head training"; head_training.HeadTrainer is the front end)
    @staticmethod
    def _as_features(x) -> np.ndarray:
        a = np.ascontiguousarray(np.asarray(x, dtype=np.float32))
        if a.ndim != 2 or a.shape[1] != 1280:
            raise ValueError(f"expected (n,1280) features, got {a.shape}")
        return a

    def head_train_begin(self, params, config: "HeadConfig"):
        """params: dict of the 14 `HEAD_FIELDS` arrays"""
        missing = [k for k in HEAD_FIELDS if k not in params]
        if missing:
            raise KeyError(f"head parameters missing: {missing}")
        hp, _keep = _head_arrays(params)
        self._check(self._lib.dfd_head_train_begin(self._p, C.byref(hp), C.byref(config)))
        self._block_row = BLOCK14_ROW                           # floats of a row of the `_block` entries; block 11 widens it

    def head_train_accumulate(self, feat, labels_a, labels_b=None, lam: float = 1.0, loss_scale: float = 1.0):
        """-> (unscaled loss, logits (n,))"""
        a = self._as_features(feat)
        n = a.shape[0]
        ya = np.ascontiguousarray(np.asarray(labels_a, dtype=np.float32).reshape(-1))
        yb = None if labels_b is None else np.ascontiguousarray(np.asarray(labels_b, dtype=np.float32).reshape(-1))
        if ya.size != n or (yb is not None and yb.size != n):
            raise ValueError("one label per feature row")
        loss = C.c_float()
        logits = np.empty(max(n, 1), np.float32)
        self._check(self._lib.dfd_head_train_accumulate(self._p, _ptr(a), n, _ptr(ya), None if yb is None else _ptr(yb),
                                                        float(lam), float(loss_scale), C.byref(loss), _ptr(logits)))
        return float(loss.value), logits[:n]

    def head_train_apply(self, lr: float) -> float:
        """-> global gradient norm before clipping"""
        norm = C.c_float()
        self._check(self._lib.dfd_head_train_apply(self._p, float(lr), C.byref(norm)))
        return float(norm.value)

    def head_train_eval(self, feat, use_ema: bool = False) -> np.ndarray:
        a = self._as_features(feat)
        out = np.empty(max(a.shape[0], 1), np.float32)
        self._check(self._lib.dfd_head_train_eval(self._p, _ptr(a), a.shape[0], int(bool(use_ema)), _ptr(out)))
        return out[: a.shape[0]]

    def head_train_export(self, use_ema: bool = False):
        hp, out = _head_arrays()
        self._check(self._lib.dfd_head_train_export(self._p, int(bool(use_ema)), C.byref(hp)))
        return out

    def head_train_grads(self, set_to=None):
        """the accumulated gradients (dict without rm / rv); `set_to`: replace them first"""
        skip = ("rm1", "rv1", "rm2", "rv2")
        if set_to is not None:
            hp, _keep = _head_arrays(set_to, skip)
            self._check(self._lib.dfd_head_train_grads(self._p, C.byref(hp), 1))
        hp, out = _head_arrays(None, skip)
        self._check(self._lib.dfd_head_train_grads(self._p, C.byref(hp), 0))
        return out

    def head_train_tap(self, name: str, n: int) -> np.ndarray:
        width = {"mask0": 1280, "mask1": 512, "mask2": 256, "z1": 512, "z2": 256, "a1": 512, "a2": 256}.get(name, 1280)   # unknown names: the library refuses
        wide = {"cz": (49, 1280), "b15.out": (49, 320), "b15.dout": (49, 320), "b15.ad": (49, 1152), "b15.dae": (49, 1152),
                "b15.gate": (1152,)}
        for b in (14, 13, 12):                                  # the skip blocks share block 14's six taps
            wide.update({f"b{b}.out": (49, 192), f"b{b}.dout": (49, 192), f"b{b}.ad": (49, 1152), f"b{b}.dae": (49, 1152),
                         f"b{b}.gate": (1152,), f"b{b}.keep": ()})
        wide.update({"b11.out": (49, 192), "b11.dout": (49, 192), "b11.ad": (49, 672), "b11.dae": (196, 672), "b11.gate": (672,),
                     "b11.keep": ()})                           # block 11 has no skip: the library refuses "b11.keep"
        out = np.empty((int(n),) + wide.get(name, (width,)), np.float32)
        self._check(self._lib.dfd_head_train_tap(self._p, name.encode(), _ptr(out), out.size))
        return out

    def head_train_commit(self, use_ema: bool = True):
        self._check(self._lib.dfd_head_train_commit(self._p, int(bool(use_ema))))

    def head_train_end(self):
        self._check(self._lib.dfd_head_train_end(self._p))

    # -- the conv stage of the head trainer (include/dfd_hip.h "fine-tuning the head conv with the head")
    @staticmethod
    def _as_trunk(x) -> np.ndarray:
        a = np.ascontiguousarray(np.asarray(x, dtype=np.float32))
        if a.ndim < 2 or a.shape[1:] not in (TRUNK_SHAPE, (TRUNK_ROW,)):
            raise ValueError(f"expected (n,7,7,320) or (n,{TRUNK_ROW}) trunk rows, got {a.shape}")
        return a

    def head_train_unfreeze_conv(self, params, lr_scale: float = 0.1, bn_momentum: float = 0.01, bn_eps: float = 1e-3):
        """params: dict of the 5 `CONV_FIELDS` arrays (w (1280,320) or (1280,320,1,1))"""
        missing = [k for k in CONV_FIELDS if k not in params]
        if missing:
            raise KeyError(f"conv parameters missing: {missing}")
        cp, _keep = _conv_arrays(params)
        self._check(self._lib.dfd_head_train_unfreeze_conv(self._p, C.byref(cp), float(lr_scale), float(bn_momentum), float(bn_eps)))

    def head_train_accumulate_trunk(self, trunk, labels_a, labels_b=None, lam: float = 1.0, loss_scale: float = 1.0):
        """-> (unscaled loss, logits (n,))"""
        a = self._as_trunk(trunk)
        n = a.shape[0]
        ya = np.ascontiguousarray(np.asarray(labels_a, dtype=np.float32).reshape(-1))
        yb = None if labels_b is None else np.ascontiguousarray(np.asarray(labels_b, dtype=np.float32).reshape(-1))
        if ya.size != n or (yb is not None and yb.size != n):
            raise ValueError("one label per trunk row")
        loss = C.c_float()
        logits = np.empty(max(n, 1), np.float32)
        self._check(self._lib.dfd_head_train_accumulate_trunk(self._p, _ptr(a), n, _ptr(ya), None if yb is None else _ptr(yb),
                                                              float(lam), float(loss_scale), C.byref(loss), _ptr(logits)))
        return float(loss.value), logits[:n]

    def head_train_eval_trunk(self, trunk, use_ema: bool = False) -> np.ndarray:
        a = self._as_trunk(trunk)
        out = np.empty(max(a.shape[0], 1), np.float32)
        self._check(self._lib.dfd_head_train_eval_trunk(self._p, _ptr(a), a.shape[0], int(bool(use_ema)), _ptr(out)))
        return out[: a.shape[0]]

    def head_train_export_conv(self, use_ema: bool = False):
        cp, out = _conv_arrays()
        self._check(self._lib.dfd_head_train_export_conv(self._p, int(bool(use_ema)), C.byref(cp)))
        return out

    def head_train_conv_grads(self, set_to=None):
        """the accumulated gradients of w / g / be; `set_to`: replace them first"""
        skip = ("rm", "rv")
        if set_to is not None:
            cp, _keep = _conv_arrays(set_to, skip)
            self._check(self._lib.dfd_head_train_conv_grads(self._p, C.byref(cp), 1))
        cp, out = _conv_arrays(None, skip)
        self._check(self._lib.dfd_head_train_conv_grads(self._p, C.byref(cp), 0))
        return out

    # -- block 15 of the head trainer (include/dfd_hip.h "fine-tuning block 15 with the head conv and the head")
    @staticmethod
    def _as_block14(x, row: int = BLOCK14_ROW) -> np.ndarray:
        """rows of a block stage: (n,7,7,192) / (n,9408), or with block 11 unfrozen (`row` = 21952) its (n,14,14,112) /
        (n,21952): the library reads `row` floats a crop, so rows of the other kind are refused here"""
        a = np.ascontiguousarray(np.asarray(x, dtype=np.float32))
        ok = (BLOCK11_INPUT_SHAPE, (BLOCK11_INPUT_ROW,)) if row == BLOCK11_INPUT_ROW else (BLOCK14_SHAPE, (BLOCK14_ROW,))
        if a.ndim < 2 or a.shape[1:] not in ok:
            raise ValueError(f"expected (n,7,7,192) or (n,{BLOCK14_ROW}) rows of block 14's output (with block 11 unfrozen: "
                             f"(n,14,14,112) or (n,{BLOCK11_INPUT_ROW})), got {a.shape}")
        return a

    def head_train_unfreeze_block(self, params, block: int = 15, bn_momentum: float = 0.01, bn_eps: float = 1e-3):
        """params: dict of the 19 `BLOCK_FIELDS` arrays (torch layouts; conv kernels with or without their 1 x 1 axes)"""
        missing = [k for k in BLOCK_FIELDS if k not in params]
        if missing:
            raise KeyError(f"block parameters missing: {missing}")
        bp, _keep = _block_arrays(params)
        self._check(self._lib.dfd_head_train_unfreeze_block(self._p, int(block), C.byref(bp), float(bn_momentum), float(bn_eps)))

    def head_train_accumulate_block(self, rows, labels_a, labels_b=None, lam: float = 1.0, loss_scale: float = 1.0):
        """-> (unscaled loss, logits (n,))"""
        a = self._as_block14(rows, getattr(self, "_block_row", BLOCK14_ROW))
        n = a.shape[0]
        ya = np.ascontiguousarray(np.asarray(labels_a, dtype=np.float32).reshape(-1))
        yb = None if labels_b is None else np.ascontiguousarray(np.asarray(labels_b, dtype=np.float32).reshape(-1))
        if ya.size != n or (yb is not None and yb.size != n):
            raise ValueError("one label per row")
        loss = C.c_float()
        logits = np.empty(max(n, 1), np.float32)
        self._check(self._lib.dfd_head_train_accumulate_block(self._p, _ptr(a), n, _ptr(ya), None if yb is None else _ptr(yb),
                                                              float(lam), float(loss_scale), C.byref(loss), _ptr(logits)))
        return float(loss.value), logits[:n]

    def head_train_eval_block(self, rows, use_ema: bool = False) -> np.ndarray:
        a = self._as_block14(rows, getattr(self, "_block_row", BLOCK14_ROW))
        out = np.empty(max(a.shape[0], 1), np.float32)
        self._check(self._lib.dfd_head_train_eval_block(self._p, _ptr(a), a.shape[0], int(bool(use_ema)), _ptr(out)))
        return out[: a.shape[0]]

    def head_train_export_block(self, use_ema: bool = False):
        bp, out = _block_arrays()
        self._check(self._lib.dfd_head_train_export_block(self._p, int(bool(use_ema)), C.byref(bp)))
        return out

    def head_train_block_grads(self, set_to=None):
        """the accumulated gradients of the 13 trainable tensors; `set_to`: replace them first"""
        if set_to is not None:
            bp, _keep = _block_arrays(set_to, BLOCK_STAT_FIELDS)
            self._check(self._lib.dfd_head_train_block_grads(self._p, C.byref(bp), 1))
        bp, out = _block_arrays(None, BLOCK_STAT_FIELDS)
        self._check(self._lib.dfd_head_train_block_grads(self._p, C.byref(bp), 0))
        return out

    # -- block 14 of the head trainer (include/dfd_hip.h "fine-tuning block 14 with block 15, the head conv and the head");
    #    once it is unfrozen `head_train_accumulate_block` / `_eval_block` take rows of block 13's output (the same width);
    #    blocks 13 and 12 follow from the top down ("fine-tuning blocks 13 and 12 below block 14"), the rows are then the
    #    input rows of the deepest unfrozen block (`extract_block_input`)
    def head_train_unfreeze_block_at(self, params, block: int = 14, bn_momentum: float = 0.01, bn_eps: float = 1e-3,
                                     drop_connect: float = 0.2 * 14 / 16):
        """params: dict of the 19 `BLOCK_FIELDS` arrays in block 14's shapes (`BLOCK14_SHAPES`); `block` = 14, then 13, then
        12 (each with its own `drop_connect`; the reference's rates are 0.2 * block / 16)"""
        missing = [k for k in BLOCK_FIELDS if k not in params]
        if missing:
            raise KeyError(f"block parameters missing: {missing}")
        # block 11 has shapes of its own: the arrays are taken in the shapes their sizes name (block 11's or block 14's),
        # so that a call the library refuses by `block` or by the trainer's state reaches it and gets its code
        own = int(np.size(params["exp_w"])) == int(np.prod(BLOCK11_SHAPES["exp_w"]))
        bp, _keep = _block_arrays(params, block=11 if own else 14)
        self._check(self._lib.dfd_head_train_unfreeze_block_at(self._p, int(block), C.byref(bp), float(bn_momentum), float(bn_eps),
                                                               float(drop_connect)))
        if int(block) == 11:
            self._block_row = BLOCK11_INPUT_ROW                 # the rows are block 10's output from here on

    def head_train_export_block_at(self, block: int, use_ema: bool = False):
        bp, out = _block_arrays(block=block)
        self._check(self._lib.dfd_head_train_export_block_at(self._p, int(block), int(bool(use_ema)), C.byref(bp)))
        return out

    def head_train_block_grads_at(self, block: int, set_to=None):
        """`head_train_block_grads` of block 11 .. 15"""
        if set_to is not None:
            bp, _keep = _block_arrays(set_to, BLOCK_STAT_FIELDS, block)
            self._check(self._lib.dfd_head_train_block_grads_at(self._p, int(block), C.byref(bp), 1))
        bp, out = _block_arrays(None, BLOCK_STAT_FIELDS, block)
        self._check(self._lib.dfd_head_train_block_grads_at(self._p, int(block), C.byref(bp), 0))
        return out

    def tap(self, x_dev: int, n: int, name: str, capacity: int) -> np.ndarray:
        out = np.empty(int(capacity), dtype=np.float32)
        cnt = C.c_size_t()
        self._check(self._lib.dfd_b0_tap(self._p, x_dev, int(n), name.encode(), _ptr(out), out.size, C.byref(cnt)))
        return out[: cnt.value]

    def gemm_tap(self, x, w, bias, act=None, gate=None, res=None, res_first=False, hw=1, bf16=False, planes=3, conv=None,
                 rows=None, keep=None):
        """One split-GEMM call on host data (dfd_gemm_tap).  Pointwise: x (M, K), w (N, K), bias (N,) - (2N,) = bias then
        slopes with act "prelu" -, gate (ceil(M / hw), K), res (M, N); `rows` = M when x holds only a block of rows that the
        device operand repeats.  conv = dict(n_img, H, W, Cin, ksize, stride, pad, dil): x (n_img, H, W, Cin), w (N, ksize,
        ksize, Cin).  bf16: x, res and the result are uint16 bf16 bit patterns.
        keep = [(lo, hi), ...]: only these row ranges come back (a result too large to return whole); y then holds them
        one after the other.
        -> dict(rc (0, or GEMM_TAP_UNSUPPORTED for a refused shape), y (M, N), before / after (the guard rows), candidates,
        launches, tile (kind, wm, wn, mt, nt, ks), sentinels / digest (of the whole result, computed on the device))"""
        xt = np.uint16 if bf16 else np.float32
        x = np.ascontiguousarray(x, xt)
        w = np.ascontiguousarray(w, np.float32)
        b = np.ascontiguousarray(bias, np.float32).ravel()
        p = GemmTapParams()
        p.bf16, p.planes, p.act, p.res_first = int(bool(bf16)), int(planes), GEMM_ACTS[act], int(bool(res_first))
        n_out = w.shape[0]
        if conv is not None:
            p.conv = 1
            for k in ("n_img", "H", "W", "Cin", "ksize", "stride", "pad", "dil"):
                setattr(p, k, int(conv[k]))
            span = p.dil * (p.ksize - 1) + 1
            ho, wo = (p.H + 2 * p.pad - span) // p.stride + 1, (p.W + 2 * p.pad - span) // p.stride + 1
            m, k_in = p.n_img * ho * wo, p.ksize * p.ksize * p.Cin
            if x.size != p.n_img * p.H * p.W * p.Cin:
                raise ValueError("x does not hold n_img x H x W x Cin values")
        else:
            m, k_in = int(rows if rows is not None else x.shape[0]), x.shape[1]
            p.M, p.K, p.HW = m, k_in, int(hw)
            p.x_rows = x.shape[0] if rows is not None else 0
            if x.ndim != 2 or x.shape[0] > m:
                raise ValueError("x must be (M, K), or a block of at most `rows` rows")
        p.N = n_out
        if w.size != n_out * k_in or b.size != (2 * n_out if p.act == 3 else n_out) or m <= 0:
            raise ValueError("w must hold N x K values, bias N (2N with prelu)")
        keep_alive = [x, w, b]
        p.X, p.Wt, p.bias = x.ctypes.data, w.ctypes.data, b.ctypes.data
        if gate is not None:
            g = np.ascontiguousarray(gate, np.float32)
            if conv is not None or g.shape != (-(-m // p.HW), k_in):
                raise ValueError("gate must be (ceil(M / hw), K), pointwise only")
            keep_alive.append(g)
            p.gate = g.ctypes.data
        if res is not None:
            r = np.ascontiguousarray(res, xt)
            if r.size != m * n_out:
                raise ValueError("res must hold M x N values")
            keep_alive.append(r)
            p.R = r.ctypes.data
        back = m
        if keep is not None:
            rg = np.ascontiguousarray(keep, np.int64).reshape(-1, 2)
            keep_alive.append(rg)
            p.n_ranges, p.y_ranges = rg.shape[0], rg.ctypes.data
            back = int((rg[:, 1] - rg[:, 0]).sum())
        y = np.zeros((back + 2 * GEMM_TAP_GUARD, n_out), xt)
        p.Y = y.ctypes.data
        rc = self._lib.dfd_gemm_tap(self._p, C.byref(p))
        if rc not in (0, GEMM_TAP_UNSUPPORTED):
            self._check(rc)
        return {"rc": rc, "y": y[GEMM_TAP_GUARD:GEMM_TAP_GUARD + back], "before": y[:GEMM_TAP_GUARD], "after": y[GEMM_TAP_GUARD + back:],
                "candidates": int(p.candidates), "launches": int(p.launches), "tile": tuple(int(v) for v in p.tile),
                "sentinels": int(p.y_sentinels), "digest": int(p.y_digest)}

    def profile_begin(self):
        self._check(self._lib.dfd_b0_profile_begin(self._p))

    def profile_end(self, max_layers: int = 128):
        """-> (steps, [(launch name, summed ms over those steps), ...])"""
        ms = (C.c_float * max_layers)()
        names = (C.c_char_p * max_layers)()
        cnt, steps = C.c_int(), C.c_int()
        self._check(self._lib.dfd_b0_profile_end(self._p, ms, names, max_layers, C.byref(cnt), C.byref(steps)))
        return steps.value, [(names[i].decode(), float(ms[i])) for i in range(cnt.value)]

    # -- 8-bit image path
    @staticmethod
    def _as_bgr(frame) -> np.ndarray:
        a = np.asarray(frame)
        if a.dtype != np.uint8 or a.ndim != 3 or a.shape[2] != 3:
            raise ValueError(f"expected (H,W,3) uint8 BGR image, got {a.dtype} {a.shape}")
        # a one-row (or one-pixel) view counts as contiguous whatever its row stride, which the callers pass on
        if not a.flags["C_CONTIGUOUS"] or a.strides[0] != a.shape[1] * 3:
            a = np.array(a, order="C", copy=True)
        return a

    @staticmethod
    def _as_boxes(boxes) -> np.ndarray:
        b = np.ascontiguousarray(np.asarray(boxes, dtype=np.int32).reshape(-1, 4))
        if b.shape[0] == 0:
            raise ValueError("no boxes")
        return b

    def resize_bgr(self, frame, dw: int, dh: int) -> np.ndarray:
        a = self._as_bgr(frame)
        out = np.empty((dh, dw, 3), np.uint8)
        self._check(self._lib.dfd_resize_bgr(self._p, _ptr(a), a.shape[0], a.shape[1], a.strides[0], dh, dw, _ptr(out)))
        return out

    def preprocess_face_quality(self, face) -> np.ndarray:
        a = self._as_bgr(face)
        out = np.empty_like(a)
        self._check(self._lib.dfd_preprocess_face_quality(self._p, _ptr(a), a.shape[0], a.shape[1], a.strides[0], _ptr(out)))
        return out

    def tta_augment(self, face, flip: bool, brightness: float, angle_deg: float) -> np.ndarray:
        """cv2.flip / convertScaleAbs / warpAffine chain of the reference's test-time augmentation, on the device"""
        a = self._as_bgr(face)
        out = np.empty_like(a)
        self._check(self._lib.dfd_tta_augment(self._p, _ptr(a), a.shape[0], a.shape[1], a.strides[0], int(bool(flip)),
                                              float(brightness), float(angle_deg), _ptr(out)))
        return out

    def tta_augment_crops(self, frame, boxes, copies: int, draws):
        """`copies` augmented images of every box in ONE launch (dfd_tta_augment_crops; no CLAHE).  draws: (flip,
        brightness, angle_deg) per image, face-major.  -> [[image (h, w, 3) per copy] per box]"""
        a, b = self._as_bgr(frame), self._as_boxes(boxes)
        d = tta_draws(draws, b.shape[0], int(copies))
        out = np.empty(int(sum(int(w) * int(h) * 3 * copies for _, _, w, h in b)), np.uint8)
        self._check(self._lib.dfd_tta_augment_crops(self._p, _ptr(a), a.shape[0], a.shape[1], a.strides[0], _ptr(b), b.shape[0],
                                                    int(copies), d, _ptr(out)))
        res, at = [], 0
        for _, _, w, h in b:
            n = int(w) * int(h) * 3
            res.append([out[at + j * n: at + (j + 1) * n].reshape(int(h), int(w), 3) for j in range(copies)])
            at += n * copies
        return res

    def classify_crops_tta(self, frame, boxes, copies: int, draws, apply_clahe: bool = True) -> np.ndarray:
        """`classify_crops` with `copies` augmented images per box in the same pass -> logits (n, 1 + copies): column 0
        the un-augmented crop, NaN where the MTCNN stage found no face"""
        a, b = self._as_bgr(frame), self._as_boxes(boxes)
        d = tta_draws(draws, b.shape[0], int(copies))
        out = np.empty((b.shape[0], 1 + int(copies)), np.float32)
        self._check(self._lib.dfd_classify_crops_tta(self._p, _ptr(a), a.shape[0], a.shape[1], a.strides[0], _ptr(b), b.shape[0],
                                                     int(apply_clahe), int(copies), d, _ptr(out)))
        return out

    def tta_arm(self, copies: int, draws, capacity_faces: int):
        """arm the next fused analyze call (dfd_tta_arm): draws for `capacity_faces` faces, face-major"""
        d = tta_draws(draws, int(capacity_faces), int(copies))
        self._check(self._lib.dfd_tta_arm(self._p, int(copies), d, int(capacity_faces)))

    def tta_logits(self) -> np.ndarray:
        """(n_faces, 1 + copies) logits of the last armed call, faces in the order the call returned them"""
        n, c = C.c_int(), C.c_int()
        self._lib.dfd_tta_logits(self._p, None, 0, C.byref(n), C.byref(c))
        out = np.empty((n.value, 1 + c.value), np.float32)
        self._check(self._lib.dfd_tta_logits(self._p, _ptr(out), out.size, C.byref(n), C.byref(c)))
        return out

    def _tta_arm_for(self, tta, n_frames: int, max_faces: int):
        if tta is not None:
            copies, draws = tta
            self.tta_arm(copies, draws, n_frames * max_faces)

    def _tta_rows(self, counts):
        """per frame the (n, 1 + copies) logits of its faces (counts: faces per frame, call order)"""
        block = self.tta_logits()
        if block.shape[0] != sum(counts):
            raise DfdError(-5, f"armed call returned {sum(counts)} faces, dfd_tta_logits holds {block.shape[0]}")
        out, at = [], 0
        for k in counts:
            out.append(block[at:at + k].copy())
            at += k
        return out

    def preprocess_crops(self, frame, boxes, apply_clahe: bool = True) -> np.ndarray:
        a, b = self._as_bgr(frame), self._as_boxes(boxes)
        out = np.empty((b.shape[0], 3, 224, 224), np.float32)
        self._check(self._lib.dfd_preprocess_crops(self._p, _ptr(a), a.shape[0], a.shape[1], a.strides[0], _ptr(b),
                                                   b.shape[0], int(apply_clahe), _ptr(out)))
        return out

    def classify_crops(self, frame, boxes, apply_clahe: bool = True) -> np.ndarray:
        a, b = self._as_bgr(frame), self._as_boxes(boxes)
        out = np.empty((b.shape[0], 1), np.float32)
        self._check(self._lib.dfd_classify_crops(self._p, _ptr(a), a.shape[0], a.shape[1], a.strides[0], _ptr(b),
                                                 b.shape[0], int(apply_clahe), _ptr(out)))
        return out

    # -- Grad-CAM (include/dfd_hip.h, "Grad-CAM of the classifier")
    @staticmethod
    def _gradcam_outputs(n: int, overlay: bool, raw: bool):
        return (np.empty((n, 1), np.float32), np.empty((n, 224, 224), np.float32),
                np.empty((n, 224, 224, 3), np.uint8) if overlay else None,
                np.empty((n, 7, 7), np.float32) if raw else None)

    @staticmethod
    def _gradcam_result(logits, heat, ov, cam7):
        return (logits, heat) + ((ov,) if ov is not None else ()) + ((cam7,) if cam7 is not None else ())

    def gradcam(self, x, overlay: bool = False, raw: bool = False):
        """Grad-CAM of the head conv on (n,3,224,224) normalised input -> (logits (n,1), heat (n,224,224) float32
        [, overlay (n,224,224,3) BGR uint8 if `overlay`] [, cam7 (n,7,7) if `raw`]).  The logits are `classify`'s bits."""
        a = self._as_nchw(x)
        lg, heat, ov, c7 = self._gradcam_outputs(a.shape[0], overlay, raw)
        self._check(self._lib.dfd_gradcam_nchw(self._p, _ptr(a), a.shape[0], _ptr(lg), None if c7 is None else _ptr(c7),
                                               _ptr(heat), None if ov is None else _ptr(ov)))
        return self._gradcam_result(lg, heat, ov, c7)

    def gradcam_device(self, x_dev: int, n: int, logits_dev: int, cam7_dev: Optional[int] = None,
                       heat_dev: Optional[int] = None, overlay_dev: Optional[int] = None):
        """Enqueue Grad-CAM on device buffers (no host wait); any of the three map outputs may be None."""
        self._check(self._lib.dfd_gradcam_nchw_device(self._p, x_dev, int(n), logits_dev, cam7_dev, heat_dev, overlay_dev))

    def gradcam_crops(self, frame, boxes, apply_clahe: bool = True, overlay: bool = False, raw: bool = False):
        """`classify_crops` + Grad-CAM: as `gradcam`; a crop the MTCNN stage rejects has a NaN logit and zero maps."""
        a, b = self._as_bgr(frame), self._as_boxes(boxes)
        lg, heat, ov, c7 = self._gradcam_outputs(b.shape[0], overlay, raw)
        self._check(self._lib.dfd_gradcam_crops(self._p, _ptr(a), a.shape[0], a.shape[1], a.strides[0], _ptr(b), b.shape[0],
                                                int(apply_clahe), _ptr(lg), None if c7 is None else _ptr(c7), _ptr(heat),
                                                None if ov is None else _ptr(ov)))
        return self._gradcam_result(lg, heat, ov, c7)

    def gradcam_tap(self, x=None, z=None, fc1=None, fc2=None, heat: bool = True, overlay: bool = False, n: Optional[int] = None):
        """The three Grad-CAM launches with every stage returned (dfd_gradcam_tap).  Start "x" (z is None): x
        (n,3,224,224) runs through the forward as in `gradcam`.  Start "z": z (n,49,1280) float32, or uint16 bf16 bit
        patterns, with fc1 (n,512) and fc2 (n,256) injected, no forward; x only for the overlay.  `n` overrides the batch
        read from the arrays (the argument checks of the C entry).
        -> dict(z, z_bf16, fc1, fc2, D1 (n,512), G (n,1280), cam7 (n,49), guard_D1 / guard_G / guard_cam7 (the
        GRADCAM_TAP_GUARD rows behind them, uint32 bit patterns), heat, overlay (None when not asked for))"""
        from_z = z is not None or x is None
        p = GradcamTapParams()
        keep = []

        def arr(a, dtype, tail):
            if a is None:
                return None
            a = np.ascontiguousarray(a, dtype)
            if a.shape[1:] != tail:
                raise ValueError(f"expected (n,) + {tail}, got {a.shape}")
            keep.append(a)
            return a

        xa = arr(x, np.float32, (3, 224, 224))
        if from_z:
            zb = z is not None and np.asarray(z).dtype == np.uint16
            za, f1, f2 = arr(z, np.uint16 if zb else np.float32, (49, 1280)), arr(fc1, np.float32, (512,)), arr(fc2, np.float32, (256,))
            p.start, p.z_bf16 = 1, int(zb)
            first = next((a for a in (za, f1, f2, xa) if a is not None), None)
            m = int(n) if n is not None else (0 if first is None else first.shape[0])
            if any(a is not None and a.shape[0] < m for a in (za, f1, f2, xa)):
                raise ValueError("an input holds fewer than n rows")
        else:
            m = int(n) if n is not None else xa.shape[0]
            if xa.shape[0] < m:
                raise ValueError("x holds fewer than n crops")
            # room for either storage type; trimmed to the handle's below
            za, f1, f2 = np.zeros((max(m, 0), 49, 1280), np.float32), np.zeros((max(m, 0), 512), np.float32), np.zeros((max(m, 0), 256), np.float32)
        p.n = m
        rows = max(m, 0) + GRADCAM_TAP_GUARD
        out = {"D1": np.zeros((rows, 512), np.uint32), "G": np.zeros((rows, 1280), np.uint32), "cam7": np.zeros((rows, 49), np.uint32)}
        ht = np.zeros((max(m, 0), 224, 224), np.float32) if heat else None
        ov = np.zeros((max(m, 0), 224, 224, 3), np.uint8) if overlay else None
        for k, a in (("x", xa), ("z", za), ("fc1", f1), ("fc2", f2), ("D1", out["D1"]), ("G", out["G"]), ("cam7", out["cam7"]),
                     ("heat", ht), ("overlay", ov)):
            if a is not None:
                setattr(p, k, a.ctypes.data)
        self._check(self._lib.dfd_gradcam_tap(self._p, C.byref(p)))
        if not from_z and p.z_bf16:
            za = za.reshape(-1).view(np.uint16)[: m * 49 * 1280].reshape(m, 49, 1280).copy()
        res = {"z": za, "z_bf16": bool(p.z_bf16), "fc1": f1, "fc2": f2, "heat": ht, "overlay": ov}
        for k, a in out.items():
            res[k] = a[:m].view(np.float32)
            res["guard_" + k] = a[m:]
        return res

    # -- frame forensics
    FORENSIC_KEYS = ("frequency", "noise", "ela", "edge", "color", "temporal")
    FORENSIC_STAT_KEYS = ("freq_low", "freq_mid", "freq_high", "freq_high_ratio", "freq_mid_ratio", "freq_mid_cv",
                          "noise_mean", "noise_cv", "ela_mean", "ela_cv", "edge_density", "lap_var", "sat_std",
                          "val_std", "unique_hues", "mean_diff", "temporal_cv", "frame_count")

    def forensics(self, frame, full: bool = True, stream_id: int = 0):
        """-> (scores dict, fake_probability, stats dict)"""
        a = self._as_bgr(frame)
        sc = np.empty(6, np.float64)
        st = np.empty(len(self.FORENSIC_STAT_KEYS), np.float64)
        prob = C.c_double()
        self._check(self._lib.dfd_forensics(self._p, int(stream_id), _ptr(a), a.shape[0], a.shape[1], a.strides[0],
                                            int(bool(full)), _ptr(sc), C.byref(prob), _ptr(st)))
        scores = {k: float(v) for k, v in zip(self.FORENSIC_KEYS, sc) if not np.isnan(v)}
        return scores, float(prob.value), dict(zip(self.FORENSIC_STAT_KEYS, (float(v) for v in st)))

    def forensics_reset(self, stream_id: int = 0):
        self._check(self._lib.dfd_forensics_reset(self._p, int(stream_id)))

    def forensics_release(self, stream_id: int):
        """drop the stream's state; its device plane is reused by the next new stream (dfd_forensics_release)"""
        self._check(self._lib.dfd_forensics_release(self._p, int(stream_id)))

    def forensics_state(self, stream_id: int = 0):
        fc, nd, hp = C.c_int(), C.c_int(), C.c_int()
        self._check(self._lib.dfd_forensics_state(self._p, int(stream_id), C.byref(fc), C.byref(nd), C.byref(hp)))
        return fc.value, nd.value, bool(hp.value)

    # per-frame dtype and shape of every dfd_forensic_tap buffer ("stats": 6 entries unless full and start = "rs")
    FORENSIC_TAPS = {"rs": (np.uint8, (256, 256, 3)), "gray": (np.uint8, (256, 256)), "fft_tmp": (np.complex64, (256, 256)),
                     "spectrum": (np.complex64, (256, 256)), "logmag": (np.float32, (256, 256)),
                     "fft_part": (np.float64, (256, 7)), "grad": (np.int16, (256, 256, 2)), "lap_part": (np.float64, (256, 2)),
                     "map": (np.uint8, (256, 256)), "edges": (np.uint8, (256, 256)), "edge_count": (np.float64, (1,)),
                     "jy": (np.uint8, (256, 256)), "jcb": (np.uint8, (128, 128)), "jcr": (np.uint8, (128, 128)),
                     "stats_ela": (np.float64, (64,)), "stats_noise": (np.float64, (64,)), "hsv_part": (np.float64, (256, 4)),
                     "hue_bits": (np.uint32, (6,)), "stats": (np.float64, (9,)), "twiddle": (np.complex64, (128,))}
    FORENSIC_STARTS = {"rs": (np.uint8, (256, 256, 3)), "gray": (np.uint8, (256, 256)), "grad": (np.int16, (256, 256, 2)),
                       "map": (np.uint8, (256, 256))}

    def forensic_tap(self, data, name: str, full: bool = True, start: str = "rs", frame: int = -1) -> np.ndarray:
        """Test entry: the forensic kernel chain on `data` = n frames of the `start` buffer ("rs": 256x256 BGR; "gray",
        "grad", "map": that buffer injected, only the kernels downstream of it run) -> buffer `name` of all frames
        (n, ...) or of one `frame` (...).  "twiddle" is the FFT table, (128,) complex64."""
        dt, shp = self.FORENSIC_STARTS[start]
        a = np.ascontiguousarray(np.asarray(data))
        if a.dtype != dt or a.shape[1:] != shp:
            raise ValueError(f"start '{start}' takes (n,) + {shp} {np.dtype(dt).name}, got {a.shape} {a.dtype}")
        odt, oshp = self.FORENSIC_TAPS[name]
        if name == "stats" and not (full and start == "rs"):
            oshp = (6,)
        nout = 1 if (frame >= 0 or name == "twiddle") else a.shape[0]
        out = np.empty((nout,) + oshp, odt)
        cnt = C.c_size_t()
        self._check(self._lib.dfd_forensic_tap(self._p, _ptr(a) if start == "rs" else None, a.shape[0], int(bool(full)),
                                               start.encode(), None if start == "rs" else _ptr(a), name.encode(), int(frame),
                                               _ptr(out), out.nbytes, C.byref(cnt)))
        assert cnt.value == out.nbytes, (name, cnt.value, out.nbytes)
        return out[0] if (frame >= 0 or name == "twiddle") else out

    # ---- any square analysis size (dfd_forensics_sized / dfd_forensic_tap_sized)
    def forensics_sized(self, frame, size: int, full: bool = True, stream_id: int = 0):
        """`forensics` at analysis size (size, size), a multiple of 16 in 32..1024 -> (scores dict, fake_probability,
        stats dict).  A stream keeps the size of its first frame until it is released."""
        a = self._as_bgr(frame)
        sc = np.empty(6, np.float64)
        st = np.empty(len(self.FORENSIC_STAT_KEYS), np.float64)
        prob = C.c_double()
        self._check(self._lib.dfd_forensics_sized(self._p, int(stream_id), _ptr(a), a.shape[0], a.shape[1], a.strides[0],
                                                  int(size), int(bool(full)), _ptr(sc), C.byref(prob), _ptr(st)))
        scores = {k: float(v) for k, v in zip(self.FORENSIC_KEYS, sc) if not np.isnan(v)}
        return scores, float(prob.value), dict(zip(self.FORENSIC_STAT_KEYS, (float(v) for v in st)))

    def forensics_open(self, stream_id: int, size: int):
        """fix the analysis size of a stream that has not seen a frame (dfd_forensics_open): the fused entries
        (analyze_frame, analyze_jpeg, analyze_stream_batch, analyze_streams_batch) then run it at (size, size) on the
        general chain.  The same size again is a no-op; another size raises DfdError (-5) and changes nothing."""
        self._check(self._lib.dfd_forensics_open(self._p, int(stream_id), int(size)))

    @staticmethod
    def forensic_taps_sized(size: int):
        """per-frame dtype and shape of every dfd_forensic_tap_sized buffer, and of its four starts"""
        s, c, nb = int(size), int(size) // 2, (int(size) // 32) ** 2
        taps = {"rs": (np.uint8, (s, s, 3)), "gray": (np.uint8, (s, s)), "fft_tmp": (np.complex64, (s, s)),
                "spectrum": (np.complex64, (s, s)), "logmag": (np.float32, (s, s)), "fft_part": (np.float64, (s, 7)),
                "grad": (np.int16, (s, s, 2)), "lap_part": (np.float64, (s, 2)), "map": (np.uint8, (s, s)),
                "edges": (np.uint8, (s, s)), "edge_count": (np.float64, (1,)), "jy": (np.uint8, (s, s)),
                "jcb": (np.uint8, (c, c)), "jcr": (np.uint8, (c, c)), "stats_ela": (np.float64, (nb,)),
                "stats_noise": (np.float64, (nb,)), "hsv_part": (np.float64, (s, 4)), "hue_bits": (np.uint32, (6,)),
                "stats": (np.float64, (9,)), "twiddle": (np.complex64, (s,))}
        return taps, {k: taps[k] for k in ("rs", "gray", "grad", "map")}

    def forensic_tap_sized(self, data, size: int, name: str, full: bool = True, start: str = "rs", frame: int = -1) -> np.ndarray:
        """Test entry: `forensic_tap` for the general chain at analysis size (size, size); `data` = n <= 16 frames of the
        `start` buffer at that size."""
        taps, starts = self.forensic_taps_sized(size)
        dt, shp = starts[start]
        a = np.ascontiguousarray(np.asarray(data))
        if a.dtype != dt or a.shape[1:] != shp:
            raise ValueError(f"start '{start}' takes (n,) + {shp} {np.dtype(dt).name}, got {a.shape} {a.dtype}")
        odt, oshp = taps[name]
        if name == "stats" and not (full and start == "rs"):
            oshp = (6,)
        nout = 1 if (frame >= 0 or name == "twiddle") else a.shape[0]
        out = np.empty((nout,) + oshp, odt)
        cnt = C.c_size_t()
        self._check(self._lib.dfd_forensic_tap_sized(self._p, _ptr(a) if start == "rs" else None, a.shape[0], int(size),
                                                     int(bool(full)), start.encode(), None if start == "rs" else _ptr(a),
                                                     name.encode(), int(frame), _ptr(out), out.nbytes, C.byref(cnt)))
        assert cnt.value == out.nbytes, (name, cnt.value, out.nbytes)
        return out[0] if (frame >= 0 or name == "twiddle") else out

    @staticmethod
    def _as_gray_or_bgr(image) -> np.ndarray:
        a = np.ascontiguousarray(np.asarray(image))
        if a.dtype != np.uint8 or a.ndim not in (2, 3) or (a.ndim == 3 and a.shape[2] != 3):
            raise ValueError(f"expected (H,W,3) or (H,W) uint8 image, got {a.dtype} {a.shape}")
        return a

    def frequency_features(self, image, size: int = 224, *, sized: bool = False) -> np.ndarray:
        """(2, size, size) float32: size 224 on its own kernels (dfd_frequency_features); any other size - and 224 too
        with `sized` - on the any-size kernels (dfd_frequency_features_sized: even sizes in 2..1024)"""
        a = self._as_gray_or_bgr(image)
        size = int(size)
        if size == 224 and not sized:
            out = np.empty((2, 224, 224), np.float32)
            self._check(self._lib.dfd_frequency_features(self._p, _ptr(a), a.shape[0], a.shape[1], a.strides[0],
                                                         3 if a.ndim == 3 else 1, _ptr(out)))
            return out
        out = np.empty((2, max(size, 0), max(size, 0)), np.float32)
        self._check(self._lib.dfd_frequency_features_sized(self._p, _ptr(a), a.shape[0], a.shape[1], a.strides[0],
                                                           3 if a.ndim == 3 else 1, size, _ptr(out)))
        return out

    def frequency_features_tap(self, image, size: int, name: str) -> np.ndarray:
        """Test entry: a buffer of the dfd_frequency_features_sized launches - "gray" (size, size) uint8 after the resize,
        "spectrum" (size, size) complex64 [kx][ky], unshifted, "dct" (size, size) float32 [ky][kx] before log1p"""
        a = self._as_gray_or_bgr(image)
        size = int(size)
        dt = {"gray": np.uint8, "spectrum": np.complex64, "dct": np.float32}.get(name, np.uint8)
        out = np.empty((max(size, 0), max(size, 0)), dt)
        self._check(self._lib.dfd_frequency_features_tap(self._p, _ptr(a), a.shape[0], a.shape[1], a.strides[0],
                                                         3 if a.ndim == 3 else 1, size, name.encode(), _ptr(out), out.nbytes))
        return out

    # -- the frequency-domain check on face windows (reference deepfake_detection.py:457-487)
    @staticmethod
    def _freq_boxes(boxes):
        if boxes is None:
            return None, 1
        b = np.ascontiguousarray(np.asarray(boxes, np.int64).reshape(-1, 4))
        if b.shape[0] < 1:
            raise ValueError("boxes is empty")
        if (np.abs(b) >= 2 ** 31).any():
            raise ValueError("box coordinates do not fit 32 bits")
        return np.ascontiguousarray(b.astype(np.int32)), b.shape[0]

    def frequency_domain(self, image, boxes=None) -> np.ndarray:
        """(n, 2) float64 = (high, total) per window (x, y, w, h) of `image` ((H,W,3) BGR or (H,W) gray uint8; boxes None:
        the whole image): the sum of |fft2(gray window)| outside the reference's central mask, and over the whole
        spectrum.  ONE library call for all windows (dfd_frequency_domain)."""
        a = self._as_gray_or_bgr(image)
        b, n = self._freq_boxes(boxes)
        out = np.empty((n, 2), np.float64)
        self._check(self._lib.dfd_frequency_domain(self._p, _ptr(a), a.shape[0], a.shape[1], a.strides[0],
                                                   3 if a.ndim == 3 else 1, None if b is None else _ptr(b), n, _ptr(out)))
        return out

    def frequency_domain_device(self, frame_ptr: int, height: int, width: int, stride: int, channels: int, boxes=None) -> np.ndarray:
        """`frequency_domain` on a frame that is resident on this handle's device (a DeviceBuffer's `ptr`)"""
        b, n = self._freq_boxes(boxes)
        out = np.empty((n, 2), np.float64)
        self._check(self._lib.dfd_frequency_domain_device(self._p, C.c_void_p(frame_ptr), int(height), int(width), int(stride),
                                                          int(channels), None if b is None else _ptr(b), n, _ptr(out)))
        return out

    def frequency_domain_tap(self, gray, name: str) -> np.ndarray:
        """Test entry: a buffer of the dfd_frequency_domain launches on one (h, w) uint8 gray window - "rows" (w, h)
        complex64 (pass 1: the transform along x, transposed), "spectrum" (w, h) complex64 [kx][ky], "mag" (w, h)
        float32, "sums" (2,) float64 (high, total)"""
        a = np.ascontiguousarray(np.asarray(gray))
        if a.dtype != np.uint8 or a.ndim != 2:
            raise ValueError(f"expected (H,W) uint8 gray window, got {a.dtype} {a.shape}")
        hh, ww = a.shape
        out = np.empty(2, np.float64) if name == "sums" else np.empty((ww, hh), np.float32 if name == "mag" else np.complex64)
        self._check(self._lib.dfd_frequency_domain_tap(self._p, _ptr(a), hh, ww, name.encode(), _ptr(out), out.nbytes))
        return out

    # -- face detector
    @property
    def has_detector(self) -> bool:
        return bool(self._lib.dfd_has_detector(self._p))

    def detect_faces(self, frame, confidence_threshold: float = 0.5, max_out: int = 200, with_conf: bool = False):
        """-> [(x, y, w, h), ...] in descending-confidence order (reference face_detection.py:71-105)."""
        a = self._as_bgr(frame)
        boxes = np.zeros((max_out, 4), np.int32)
        conf = np.zeros(max_out, np.float32)
        n = C.c_int()
        self._check(self._lib.dfd_detect_faces(self._p, _ptr(a), a.shape[0], a.shape[1], a.strides[0],
                                               float(confidence_threshold), _ptr(boxes), _ptr(conf), max_out, C.byref(n)))
        out = [tuple(int(v) for v in boxes[i]) for i in range(n.value)]
        return (out, conf[: n.value].copy()) if with_conf else out

    @property
    def has_haar(self) -> bool:
        return bool(self._lib.dfd_has_haar(self._p))

    def detect_faces_haar(self, frame, scale_factor: float = 1.1, min_neighbors: int = 5, min_size: int = 30,
                          max_out: int = 256, with_candidates: bool = False):
        """cv2 detectMultiScale on the blob's Haar cascade -> [(x, y, w, h), ...] (reference face_detection.py:108-123)"""
        a = self._as_bgr_rows(frame)
        boxes = np.zeros((max(int(max_out), 1), 4), np.int32)
        n, nc = C.c_int(), C.c_int()
        self._check(self._lib.dfd_detect_faces_haar(self._p, _ptr(a), a.shape[0], a.shape[1], a.strides[0], float(scale_factor),
                                                    int(min_neighbors), int(min_size), _ptr(boxes), int(max_out), C.byref(n),
                                                    C.byref(nc)))
        out = [tuple(int(v) for v in boxes[i]) for i in range(n.value)]
        return (out, nc.value) if with_candidates else out

    @classmethod
    def _as_bgr_rows(cls, frame) -> np.ndarray:
        """_as_bgr, but a view whose rows are padded (packed pixels, row stride >= 3 * width, every row backed by a whole
        stride of the buffer it views) is passed on as it is: the Haar entries take the stride"""
        a = np.asarray(frame)
        if (a.dtype == np.uint8 and a.ndim == 3 and a.shape[2] == 3 and a.strides[1:] == (3, 1) and a.strides[0] >= a.shape[1] * 3
                and isinstance(a.base, np.ndarray) and a.base.flags["C_CONTIGUOUS"] and a.base.ndim == 2
                and a.base.shape == (a.shape[0], a.strides[0]) and a.base.dtype == np.uint8
                and a.__array_interface__["data"][0] == a.base.__array_interface__["data"][0]):
            return a
        return cls._as_bgr(frame)

    _HAAR_TAPS = {"gray": np.uint8, "scaled": np.uint8, "sum": np.uint32, "sqsum": np.uint64, "result": np.int32}

    def haar_tap(self, frame, scale_factor: float = 1.1, scale_index: int = 0, names=("gray", "scaled", "sum", "sqsum", "result")):
        """dfd_haar_tap: the named buffers of one scale of detectMultiScale's loop, shaped, with the geometry: {"gray": u8
        (h, w), "scaled": u8 (sh, sw), "sum": u32 (sh + 1, sw + 1), "sqsum": u64, "result": i32 (ny, nx), "factor", "step",
        "window": (w, h) as reported, "n_scales"}.  DfdError (DFD_ERR_ARG) for a scale index past the last scale."""
        a = self._as_bgr_rows(frame)
        dims = np.zeros(8, np.int32)
        factor = C.c_double()
        nb = C.c_size_t()

        def call(name, out, cap):
            self._check(self._lib.dfd_haar_tap(self._p, _ptr(a), a.shape[0], a.shape[1], a.strides[0], float(scale_factor),
                                               int(scale_index), name, out, cap, C.byref(nb), _ptr(dims), C.byref(factor)))
        call(None, None, 0)
        sh, sw, ny, nx, step, ww, wh, n_scales = (int(v) for v in dims)
        shapes = {"gray": a.shape[:2], "scaled": (sh, sw), "sum": (sh + 1, sw + 1), "sqsum": (sh + 1, sw + 1), "result": (ny, nx)}
        res = {"factor": factor.value, "step": step, "window": (ww, wh), "n_scales": n_scales}
        for name in names:
            out = np.empty(shapes[name], self._HAAR_TAPS[name])
            call(name.encode(), _ptr(out), out.nbytes)
            assert nb.value == out.nbytes, (name, nb.value, out.nbytes)
            res[name] = out
        return res

    def analyze_frame(self, frame, full_forensics: bool, stream_id: int = 0, confidence_threshold: float = 0.5,
                      max_faces: int = 16, apply_clahe: bool = True, tta=None):
        """One upload: forensics + detect + crop/CLAHE + classify.
        -> (scores dict, forensic probability, [(x,y,w,h)...], logits (n,))
        tta = (copies, draws for max_faces faces): the call is armed (dfd_tta_arm) and logits are (n, 1 + copies)"""
        a = self._as_bgr(frame)
        max_faces = max(1, int(max_faces))
        self._tta_arm_for(tta, 1, max_faces)
        sc = np.empty(6, np.float64)
        prob = C.c_double()
        boxes = np.zeros((max_faces, 4), np.int32)
        logits = np.zeros(max_faces, np.float32)
        n = C.c_int()
        self._check(self._lib.dfd_analyze_frame(self._p, int(stream_id), _ptr(a), a.shape[0], a.shape[1], a.strides[0],
                                                int(bool(full_forensics)), float(confidence_threshold), max_faces,
                                                int(bool(apply_clahe)), _ptr(sc), C.byref(prob), _ptr(boxes), C.byref(n),
                                                _ptr(logits)))
        scores = {k: float(v) for k, v in zip(self.FORENSIC_KEYS, sc) if not np.isnan(v)}
        lg = logits[: n.value].copy() if tta is None else self._tta_rows([n.value])[0]
        return scores, float(prob.value), [tuple(int(v) for v in boxes[i]) for i in range(n.value)], lg

    UNSUPPORTED = -7

    def decode_jpeg(self, data: bytes) -> np.ndarray:
        """cv2.imdecode(IMREAD_COLOR) for a sequential-Huffman JPEG -> (H,W,3) uint8 BGR.  DfdError with
        .code == Handle.UNSUPPORTED for flavours the device path does not decode."""
        buf = (C.c_char * len(data)).from_buffer_copy(data)
        hh, ww = C.c_int(), C.c_int()
        self._check(self._lib.dfd_decode_jpeg(self._p, buf, len(data), None, 0, C.byref(hh), C.byref(ww)))
        out = np.empty((hh.value, ww.value, 3), np.uint8)
        self._check(self._lib.dfd_memcpy_d2h(self._p, _ptr(out), self.frame_ptr(), out.nbytes))
        return out

    def decode_jpeg_batch(self, datas) -> np.ndarray:
        """n JPEGs of one size -> (n,H,W,3) uint8 BGR through the batch path (device entropy decoding where it applies)"""
        n = len(datas)
        bufs = [(C.c_char * len(d)).from_buffer_copy(d) for d in datas]
        ptrs = (C.c_void_p * n)(*[C.addressof(b) for b in bufs])
        lens = (C.c_size_t * n)(*[len(d) for d in datas])
        hh, ww = C.c_int(), C.c_int()
        self._check(self._lib.dfd_decode_jpeg_batch(self._p, n, ptrs, lens, None, 0, C.byref(hh), C.byref(ww)))
        out = np.empty((n, hh.value, ww.value, 3), np.uint8)
        self._check(self._lib.dfd_memcpy_d2h(self._p, _ptr(out), self.frame_ptr(), out.nbytes))
        return out

    # -- JPEG encode (csrc/jpeg_encode.hip)
    @staticmethod
    def _jpeg_source(img, quality, subsampling, restart_blocks, rgb, ptr=None) -> "JpegSource":
        """img: (H, W) gray or (H, W, 3) u8 array; or with `ptr` a (height, width, stride, channels) tuple of an image in HBM"""
        if ptr is None:
            if img.dtype != np.uint8 or img.ndim not in (2, 3) or (img.ndim == 3 and img.shape[2] != 3) or not img.flags.c_contiguous:
                raise ValueError("encode_jpeg expects a contiguous (H, W) or (H, W, 3) uint8 array")
            ch = 1 if img.ndim == 2 else 3
            hh, ww, stride, ptr = img.shape[0], img.shape[1], img.shape[1] * ch, img.ctypes.data
        else:
            hh, ww, stride, ch = img
        return JpegSource(ptr, hh, ww, stride, int(bool(rgb)), int(quality), JPEG_GRAY if ch == 1 else int(subsampling),
                          int(restart_blocks))

    def _encode_call(self, fn, srcs, guess: int):
        n = len(srcs)
        arr = (JpegSource * n)(*srcs)
        offs, lens = np.zeros(n, np.uintp), np.zeros(n, np.uintp)
        total = C.c_size_t()
        out = np.empty(max(int(guess), 1), np.uint8)
        rc = fn(self._p, n, arr, _ptr(out), out.size, _ptr(offs), _ptr(lens), C.byref(total))
        if rc == -1 and total.value > out.size:       # sizes are exact once the passes before the scatter have run: once more, with room
            out = np.empty(total.value, np.uint8)
            rc = fn(self._p, n, arr, _ptr(out), out.size, _ptr(offs), _ptr(lens), C.byref(total))
        self._check(rc)
        return [out[int(o):int(o) + int(k)].tobytes() for o, k in zip(offs, lens)]

    def encode_jpegs(self, images, quality=75, subsampling=2, restart_blocks=0, rgb=False):
        """A list of (H, W, 3) BGR (rgb=True: RGB) or (H, W) gray uint8 images of any sizes -> a list of JPEG files, encoded in
        one device pass (dfd_encode_jpeg_batch); each file's bytes equal Pillow's `save(quality=, subsampling=, optimize=False)`.
        quality / subsampling / restart_blocks / rgb: one value for all, or a list with one per image."""
        imgs = [np.ascontiguousarray(a) for a in images]
        n = len(imgs)
        if n == 0:
            return []
        per = [v if isinstance(v, (list, tuple)) else [v] * n for v in (quality, subsampling, restart_blocks, rgb)]
        srcs = [self._jpeg_source(a, per[0][i], per[1][i], per[2][i], per[3][i]) for i, a in enumerate(imgs)]
        return self._encode_call(self._lib.dfd_encode_jpeg_batch, srcs, sum(a.size // 2 + 4096 for a in imgs))

    def encode_jpeg(self, img, quality=75, subsampling=2, restart_blocks=0, rgb=False) -> bytes:
        """One image -> the bytes of its JPEG file (see encode_jpegs)."""
        return self.encode_jpegs([img], quality, subsampling, restart_blocks, rgb)[0]

    def encode_jpegs_device(self, sources, quality=75, subsampling=2, restart_blocks=0, rgb=False):
        """encode_jpegs for images already in HBM: sources = [(device address, height, width, stride in bytes, channels 1 or 3)];
        only the JPEG bytes cross to the host (dfd_encode_jpeg_device)."""
        n = len(sources)
        if n == 0:
            return []
        per = [v if isinstance(v, (list, tuple)) else [v] * n for v in (quality, subsampling, restart_blocks, rgb)]
        srcs = [self._jpeg_source(tuple(int(v) for v in s[1:]), per[0][i], per[1][i], per[2][i], per[3][i], ptr=int(s[0]))
                for i, s in enumerate(sources)]
        return self._encode_call(self._lib.dfd_encode_jpeg_device, srcs, sum(s[1] * s[2] * s[4] // 2 + 4096 for s in sources))

    def jpeg_decode_counts(self):
        """(frames of batch calls entropy-decoded on the device, frames decoded by the host decoder)"""
        a, b = C.c_ulonglong(), C.c_ulonglong()
        self._check(self._lib.dfd_jpeg_decode_counts(self._p, C.byref(a), C.byref(b)))
        return int(a.value), int(b.value)

    def frame_ptr(self) -> int:
        """device address of the last uploaded / decoded frame"""
        return self._lib.dfd_frame_ptr(self._p)

    def analyze_jpeg(self, data: bytes, full_forensics: bool, stream_id: int = 0, confidence_threshold: float = 0.5,
                     max_faces: int = 16, apply_clahe: bool = True, tta=None):
        """analyze_frame from JPEG bytes, decoded on the device -> (scores, forensic prob, boxes, logits, (H, W))"""
        buf = (C.c_char * len(data)).from_buffer_copy(data)
        max_faces = max(1, int(max_faces))
        self._tta_arm_for(tta, 1, max_faces)
        sc = np.empty(6, np.float64)
        prob = C.c_double()
        boxes = np.zeros((max_faces, 4), np.int32)
        logits = np.zeros(max_faces, np.float32)
        n, hh, ww = C.c_int(), C.c_int(), C.c_int()
        self._check(self._lib.dfd_analyze_jpeg(self._p, int(stream_id), buf, len(data), int(bool(full_forensics)),
                                               float(confidence_threshold), max_faces, int(bool(apply_clahe)), _ptr(sc),
                                               C.byref(prob), _ptr(boxes), C.byref(n), _ptr(logits), C.byref(hh), C.byref(ww)))
        scores = {k: float(v) for k, v in zip(self.FORENSIC_KEYS, sc) if not np.isnan(v)}
        lg = logits[: n.value].copy() if tta is None else self._tta_rows([n.value])[0]
        return (scores, float(prob.value), [tuple(int(v) for v in boxes[i]) for i in range(n.value)], lg, (hh.value, ww.value))

    def analyze_stream_batch(self, items, full_flags, stream_id: int = 0, confidence_threshold: float = 0.5,
                             max_faces: int = 1, apply_clahe: bool = True, tta=None):
        """n consecutive frames of one stream in ONE call (dfd_analyze_stream_batch).  items: JPEG `bytes` and / or BGR
        uint8 arrays of one size.  -> list of (scores dict, forensic prob, boxes, logits, n_detected) per frame, (H, W)"""
        n = len(items)
        if n == 0 or len(full_flags) != n:
            raise ValueError("analyze_stream_batch: one full / fast flag per frame")
        keep, ptrs, lens = [], (C.c_void_p * n)(), (C.c_size_t * n)()
        hh = ww = 0
        for i, it in enumerate(items):
            if isinstance(it, (bytes, bytearray, memoryview)):
                b = (C.c_char * len(it)).from_buffer_copy(it)
                keep.append(b)
                ptrs[i], lens[i] = C.addressof(b), len(it)
            else:
                a = np.ascontiguousarray(it, dtype=np.uint8)
                if a.ndim != 3 or a.shape[2] != 3 or (hh and a.shape[:2] != (hh, ww)):
                    raise ValueError("analyze_stream_batch: raw frames are (H, W, 3) uint8 of one size")
                hh, ww = a.shape[:2]
                keep.append(a)
                ptrs[i], lens[i] = a.ctypes.data, 0
        max_faces = max(1, int(max_faces))
        full = np.ascontiguousarray([int(bool(f)) for f in full_flags], dtype=np.int32)
        sc = np.empty((n, 6), np.float64)
        prob = np.empty(n, np.float64)
        boxes = np.zeros((n, max_faces, 4), np.int32)
        nf = np.zeros(n, np.int32)
        nd = np.zeros(n, np.int32)
        logits = np.zeros((n, max_faces), np.float32)
        oh, ow = C.c_int(), C.c_int()
        self._tta_arm_for(tta, n, max_faces)
        self._check(self._lib.dfd_analyze_stream_batch(self._p, int(stream_id), n, ptrs, lens, int(hh), int(ww), _ptr(full),
                                                       float(confidence_threshold), max_faces, int(bool(apply_clahe)), _ptr(sc),
                                                       _ptr(prob), _ptr(boxes), _ptr(nf), _ptr(nd), _ptr(logits),
                                                       C.byref(oh), C.byref(ow)))
        rows = None if tta is None else self._tta_rows([int(k) for k in nf])
        out = []
        for i in range(n):
            scores = {k: float(v) for k, v in zip(self.FORENSIC_KEYS, sc[i]) if not np.isnan(v)}
            out.append((scores, float(prob[i]), [tuple(int(v) for v in boxes[i, j]) for j in range(nf[i])],
                        logits[i, : nf[i]].copy() if rows is None else rows[i], int(nd[i])))
        return out, (oh.value, ow.value)

    def analyze_streams_batch(self, items, stream_ids, full_flags, confidence_threshold: float = 0.5, max_faces: int = 1,
                              apply_clahe: bool = True, tta=None):
        """frames of MANY streams and sizes in ONE call (dfd_analyze_streams_batch).  items: JPEG `bytes` and / or BGR
        uint8 arrays; stream_ids / full_flags: one per item (a stream's frames in stream order).  -> list of (scores dict,
        forensic prob, boxes, logits, n_detected, (H, W)) per frame.  A refused part raises DfdError with
        `.bad_index` = its index (-1: the call as a whole), before anything has moved."""
        n = len(items)
        if n == 0 or len(full_flags) != n or len(stream_ids) != n:
            raise ValueError("analyze_streams_batch: one stream id and one full / fast flag per frame")
        keep, ptrs, lens = [], (C.c_void_p * n)(), (C.c_size_t * n)()
        hs, ws = np.zeros(n, np.int32), np.zeros(n, np.int32)
        for i, it in enumerate(items):
            if isinstance(it, (bytes, bytearray, memoryview)):
                b = (C.c_char * len(it)).from_buffer_copy(it)
                keep.append(b)
                ptrs[i], lens[i] = C.addressof(b), len(it)
            else:
                a = np.ascontiguousarray(it, dtype=np.uint8)
                if a.ndim != 3 or a.shape[2] != 3:
                    raise ValueError("analyze_streams_batch: raw frames are (H, W, 3) uint8")
                hs[i], ws[i] = a.shape[:2]
                keep.append(a)
                ptrs[i], lens[i] = a.ctypes.data, 0
        max_faces = max(1, int(max_faces))
        ids = np.ascontiguousarray(stream_ids, dtype=np.int32)
        full = np.ascontiguousarray([int(bool(f)) for f in full_flags], dtype=np.int32)
        sc = np.empty((n, 6), np.float64)
        prob = np.empty(n, np.float64)
        boxes = np.zeros((n, max_faces, 4), np.int32)
        nf = np.zeros(n, np.int32)
        nd = np.zeros(n, np.int32)
        logits = np.zeros((n, max_faces), np.float32)
        oh, ow = np.zeros(n, np.int32), np.zeros(n, np.int32)
        bad = C.c_int(-1)
        self._tta_arm_for(tta, n, max_faces)
        rc = self._lib.dfd_analyze_streams_batch(self._p, n, ptrs, lens, _ptr(hs), _ptr(ws), _ptr(ids), _ptr(full),
                                                 float(confidence_threshold), max_faces, int(bool(apply_clahe)), _ptr(sc),
                                                 _ptr(prob), _ptr(boxes), _ptr(nf), _ptr(nd), _ptr(logits), _ptr(oh), _ptr(ow),
                                                 C.byref(bad))
        if rc != 0:
            err = DfdError(rc, (self._lib.dfd_last_error(self._p) or b"").decode())
            err.bad_index = bad.value
            raise err
        rows = None if tta is None else self._tta_rows([int(k) for k in nf])
        out = []
        for i in range(n):
            scores = {k: float(v) for k, v in zip(self.FORENSIC_KEYS, sc[i]) if not np.isnan(v)}
            out.append((scores, float(prob[i]), [tuple(int(v) for v in boxes[i, j]) for j in range(nf[i])],
                        logits[i, : nf[i]].copy() if rows is None else rows[i], int(nd[i]), (int(oh[i]), int(ow[i]))))
        return out

    def host_alloc(self, shape, dtype=np.uint8) -> np.ndarray:
        """A numpy array over pinned host memory (hipHostMalloc); release with host_free(arr)."""
        nbytes = int(np.prod(shape)) * np.dtype(dtype).itemsize
        p = C.c_void_p()
        self._check(self._lib.dfd_host_alloc(self._p, nbytes, C.byref(p)))
        buf = (C.c_char * nbytes).from_address(p.value)
        arr = np.frombuffer(buf, dtype=dtype).reshape(shape)
        self._pinned = getattr(self, "_pinned", {})
        self._pinned[arr.ctypes.data] = p.value
        return arr

    def host_free(self, arr: np.ndarray):
        p = getattr(self, "_pinned", {}).pop(arr.ctypes.data, None)
        if p:
            self._check(self._lib.dfd_host_free(self._p, p))

    def analyze_frames_host(self, frames: np.ndarray, batch: int, forced_boxes=None, confidence_threshold: float = 0.5,
                            max_faces: int = 4, apply_clahe: bool = True, with_forensics: bool = False):
        """frames: (n, H, W, 3) uint8 in host memory (pinned: host_alloc) -> as analyze_batch_device, PCIe included."""
        if frames.dtype != np.uint8 or frames.ndim != 4 or frames.shape[3] != 3 or not frames.flags["C_CONTIGUOUS"]:
            raise ValueError("expected a contiguous (n,H,W,3) uint8 array")
        n, height, width = frames.shape[:3]
        forced, forced_k = None, 0
        if forced_boxes is not None:
            forced = np.ascontiguousarray(np.asarray(forced_boxes, np.int32).reshape(n, -1, 4))
            forced_k = forced.shape[1]
        xy = np.zeros((n, max_faces, 4), np.int32)
        nf = np.zeros(n, np.int32)
        lg = np.zeros((n, max_faces), np.float32)
        fp = np.zeros(n, np.float64)
        self._check(self._lib.dfd_analyze_frames_host(
            self._p, frames.ctypes.data, n, int(batch), height, width, _ptr(forced) if forced is not None else None, forced_k,
            float(confidence_threshold), int(max_faces), int(bool(apply_clahe)), int(bool(with_forensics)),
            _ptr(xy), _ptr(nf), _ptr(lg), _ptr(fp)))
        boxes = [[tuple(int(v) for v in xy[f, i]) for i in range(nf[f])] for f in range(n)]
        return boxes, [lg[f, : nf[f]].copy() for f in range(n)], (fp if with_forensics else None)

    def pack_jpegs(self, datas):
        """the files back to back (64-byte aligned) in ONE pinned buffer -> (buffer, offsets, lengths); release the buffer
        with host_free.  What analyze_jpegs_host takes for full speed: DMA straight from the caller's memory."""
        offs, total = [], 0
        for d in datas:
            offs.append(total)
            total += (len(d) + 63) // 64 * 64
        buf = self.host_alloc((max(total, 64),))
        for o, d in zip(offs, datas):
            buf[o:o + len(d)] = np.frombuffer(d, np.uint8)
        return buf, offs, [len(d) for d in datas]

    def analyze_jpegs_host(self, datas, batch: int, forced_boxes=None, confidence_threshold: float = 0.5, max_faces: int = 4,
                           apply_clahe: bool = True, with_forensics: bool = False, packed=None):
        """JPEG files of one size (bytes objects, or packed = pack_jpegs(...) for pinned input) -> as analyze_batch_device:
        the files' bytes cross PCIe and are entropy-decoded on the device (dfd_analyze_jpegs_host)."""
        n = len(datas) if packed is None else len(packed[1])
        if packed is None:
            keep = [(C.c_char * len(d)).from_buffer_copy(d) for d in datas]
            ptrs = (C.c_void_p * n)(*[C.addressof(b) for b in keep])
            lens = (C.c_size_t * n)(*[len(d) for d in datas])
        else:
            buf, offs, ls = packed
            ptrs = (C.c_void_p * n)(*[buf.ctypes.data + o for o in offs])
            lens = (C.c_size_t * n)(*ls)
        forced, forced_k = None, 0
        if forced_boxes is not None:
            forced = np.ascontiguousarray(np.asarray(forced_boxes, np.int32).reshape(n, -1, 4))
            forced_k = forced.shape[1]
        xy = np.zeros((n, max_faces, 4), np.int32)
        nf = np.zeros(n, np.int32)
        lg = np.zeros((n, max_faces), np.float32)
        fp = np.zeros(n, np.float64)
        hh, ww = C.c_int(), C.c_int()
        self._check(self._lib.dfd_analyze_jpegs_host(
            self._p, ptrs, lens, n, int(batch), _ptr(forced) if forced is not None else None, forced_k, float(confidence_threshold),
            int(max_faces), int(bool(apply_clahe)), int(bool(with_forensics)), _ptr(xy), _ptr(nf), _ptr(lg), _ptr(fp),
            C.byref(hh), C.byref(ww)))
        boxes = [[tuple(int(v) for v in xy[f, i]) for i in range(nf[f])] for f in range(n)]
        return boxes, [lg[f, : nf[f]].copy() for f in range(n)], (fp if with_forensics else None), (hh.value, ww.value)

    def classifier_crop_count(self) -> int:
        """crops the classifier has run on since the handle was created (a crop the MTCNN stage rejects is not one)"""
        v = C.c_ulonglong(0)
        self._check(self._lib.dfd_classifier_crop_count(self._p, C.byref(v)))
        return int(v.value)

    def last_detection_count(self) -> int:
        """len(faces) of the last detect_faces / analyze_frame call, before its max_out / max_faces cut"""
        return int(self._lib.dfd_last_detection_count(self._p))

    def analyze_batch_device(self, frames_dev: int, n: int, height: int, width: int, forced_boxes=None,
                             confidence_threshold: float = 0.5, max_faces: int = 4, apply_clahe: bool = True,
                             with_forensics: bool = False):
        """n frames resident in HBM -> (boxes per frame, logits per frame, forensic probabilities or None)."""
        forced = None
        forced_k = 0
        if forced_boxes is not None:
            forced = np.ascontiguousarray(np.asarray(forced_boxes, np.int32).reshape(n, -1, 4))
            forced_k = forced.shape[1]
        xy = np.zeros((n, max_faces, 4), np.int32)
        nf = np.zeros(n, np.int32)
        lg = np.zeros((n, max_faces), np.float32)
        fp = np.zeros(n, np.float64)
        self._check(self._lib.dfd_analyze_batch_device(
            self._p, frames_dev, int(n), int(height), int(width), _ptr(forced) if forced is not None else None, forced_k,
            float(confidence_threshold), int(max_faces), int(bool(apply_clahe)), int(bool(with_forensics)),
            _ptr(xy), _ptr(nf), _ptr(lg), _ptr(fp)))
        boxes = [[tuple(int(v) for v in xy[f, i]) for i in range(nf[f])] for f in range(n)]
        logits = [lg[f, : nf[f]].copy() for f in range(n)]
        return boxes, logits, (fp if with_forensics else None)

    def forensic_signals_device(self, frames_dev: int, n: int, height: int, width: int, prev_index):
        """-> (scores [n][5] = frequency, noise, ela, edge, color; mean_diff [n], -1 where prev_index < 0).
        prev_index[f] = -2 marks a frame that is only a predecessor (tail of the batch): no signals, outputs -1."""
        pi = np.ascontiguousarray(np.asarray(prev_index, np.int32).reshape(-1))
        if pi.size != n:
            raise ValueError("prev_index must have one entry per frame")
        sc = np.empty((n, 5), np.float64)
        md = np.empty(n, np.float64)
        self._check(self._lib.dfd_forensic_signals_device(self._p, frames_dev, int(n), int(height), int(width), _ptr(pi),
                                                          _ptr(sc), _ptr(md)))
        return sc, md

    # -- vote exchange over RCCL (C ABI)
    COMM_ID_BYTES = 128

    @staticmethod
    def comm_unique_id() -> bytes:
        lib = load()
        buf = (C.c_char * Handle.COMM_ID_BYTES)()
        rc = lib.dfd_comm_unique_id(buf)
        if rc != 0:
            raise DfdError(rc, (lib.dfd_last_error(None) or b"dfd_comm_unique_id failed").decode())
        return bytes(buf)

    def comm_init(self, comm_id: bytes, rank: int, world: int):
        if len(comm_id) != self.COMM_ID_BYTES:
            raise ValueError("communicator id must be 128 bytes")
        buf = (C.c_char * self.COMM_ID_BYTES).from_buffer_copy(comm_id)
        self._check(self._lib.dfd_comm_init(self._p, buf, int(rank), int(world)))

    def comm_destroy(self):
        self._check(self._lib.dfd_comm_destroy(self._p))

    def comm_info(self):
        r, w = C.c_int(), C.c_int()
        self._check(self._lib.dfd_comm_info(self._p, C.byref(r), C.byref(w)))
        return r.value, w.value

    def vote_allgather(self, local: np.ndarray) -> np.ndarray:
        """One ncclAllGather of this rank's record block -> (world, *local.shape), rank-major."""
        a = np.ascontiguousarray(local)
        _, world = self.comm_info()
        if world <= 0:
            raise DfdError(-5, "vote_allgather: no communicator (comm_init)")
        out = np.empty((world,) + a.shape, a.dtype)
        self._check(self._lib.dfd_vote_allgather(self._p, _ptr(a), a.nbytes, _ptr(out)))
        return out

    def vote_allgather_waves(self, local: np.ndarray) -> np.ndarray:
        """(waves, *block) of this rank -> (waves, world, *block): one all-gather per wave, one upload / download / wait"""
        a = np.ascontiguousarray(local)
        _, world = self.comm_info()
        if world <= 0:
            raise DfdError(-5, "vote_allgather_waves: no communicator (comm_init)")
        out = np.empty((a.shape[0], world) + a.shape[1:], a.dtype)
        self._check(self._lib.dfd_vote_allgather_waves(self._p, _ptr(a), a.shape[0], a.nbytes // a.shape[0], _ptr(out)))
        return out

    @property
    def has_mtcnn(self) -> bool:
        return bool(self._lib.dfd_has_mtcnn(self._p))

    def mtcnn_align(self, face_bgr):
        """MTCNN.forward on an already-cropped face (reference deepfake_detection.py:376-377):
        ((3,160,160) float32 RGB 0..255, (x1,y1,x2,y2,prob)) or (None, None) when no face passes."""
        a = self._as_bgr(face_bgr)
        face = np.empty((3, 160, 160), np.float32)
        box = np.empty(5, np.float32)
        found = C.c_int()
        self._check(self._lib.dfd_mtcnn_align(self._p, _ptr(a), a.shape[0], a.shape[1], a.strides[0], _ptr(face),
                                              _ptr(box), C.byref(found)))
        return (face, box) if found.value else (None, None)

    def mtcnn_tap(self, face_bgr, name: str, capacity: int = 1 << 20) -> np.ndarray:
        a = self._as_bgr(face_bgr)
        out = np.empty(int(capacity), np.float32)
        cnt = C.c_size_t()
        dims = np.zeros(3, np.int32)
        self._check(self._lib.dfd_mtcnn_tap(self._p, _ptr(a), a.shape[0], a.shape[1], a.strides[0], name.encode(),
                                            _ptr(out), out.size, C.byref(cnt), _ptr(dims)))
        shape = tuple(int(d) for d in dims if d != 1) or (1,)
        if dims[1] == 5 and dims[2] == 1:
            shape = (int(dims[0]), 5)
        return out[: cnt.value].reshape(shape) if cnt.value else out[:0].reshape((0,) + shape[1:])

    @staticmethod
    def _mtcnn_tap_result(out, cnt, dims, name):
        d = tuple(int(v) for v in dims)
        if name == "pnet.cand":                              # raw 32-bit words, the launch's counter
            return out[:cnt].reshape(-1, 6), d[2]
        if d[2] == 1 and d[1] in (1, 4, 5):
            return out[:cnt].reshape(d[0]) if d[1] == 1 else out[:cnt].reshape(d[0], d[1])
        return out[:cnt].reshape(d)

    def mtcnn_tap_batch(self, images, crop: int, name: str, capacity: int = 1 << 24):
        """One named buffer (dfd_mtcnn_tap in include/dfd_hip.h lists them) of image `crop` of one batched cascade call
        over `images`, shaped as the header documents; "pnet.cand" -> (records (k, 6) float32 bit patterns, counter)."""
        imgs = [self._as_bgr(a) for a in images]
        n = len(imgs)
        ptrs = (C.c_void_p * n)(*[a.ctypes.data for a in imgs])
        hs = np.array([a.shape[0] for a in imgs], np.int32)
        ws = np.array([a.shape[1] for a in imgs], np.int32)
        st = np.array([a.strides[0] for a in imgs], np.int32)
        out = np.empty(int(capacity), np.float32)
        cnt = C.c_size_t()
        dims = np.zeros(3, np.int32)
        self._check(self._lib.dfd_mtcnn_tap_batch(self._p, n, ptrs, _ptr(hs), _ptr(ws), _ptr(st), int(crop), name.encode(),
                                                  _ptr(out), out.size, C.byref(cnt), _ptr(dims)))
        return self._mtcnn_tap_result(out, cnt.value, dims, name)

    def mtcnn_net_tap(self, net: str, windows, name: str, row0: int = 0, rows: Optional[int] = None, image=None):
        """Rows [row0, row0 + rows) of buffer `name` of the R-Net ("rnet") or O-Net ("onet") trunk run alone
        (dfd_mtcnn_net_tap): on the input windows (m, sz, sz, 3) float32 in place of the window resize, or - with
        `image` (H, W, 3) uint8 BGR - on its source windows (m, 4) int32 (x, y, w, h)."""
        sz = 48 if net == "onet" else 24
        if image is None:
            x = np.ascontiguousarray(windows, np.float32)
            assert x.ndim == 4 and x.shape[1:] == (sz, sz, 3), x.shape
            src = (_ptr(x), None, 0, 0, 0, None)
        else:
            a = self._as_bgr(image)
            x = np.ascontiguousarray(windows, np.int32)
            assert x.ndim == 2 and x.shape[1] == 4, x.shape
            src = (None, _ptr(a), a.shape[0], a.shape[1], a.strides[0], _ptr(x))
        rows = x.shape[0] - row0 if rows is None else rows
        out = np.empty(rows * sz * sz * 16, np.float32)        # (the widest buffer: conv2)
        cnt = C.c_size_t()
        dims = np.zeros(3, np.int32)
        self._check(self._lib.dfd_mtcnn_net_tap(self._p, int(net == "onet"), *src, x.shape[0], int(row0), int(rows), name.encode(),
                                                _ptr(out), out.size, C.byref(cnt), _ptr(dims)))
        return self._mtcnn_tap_result(out, cnt.value, dims, name)

    def _mtcnn_call(self, images, params: MtcnnParams, max_faces: int, landmarks: bool, faces: bool):
        imgs = [self._as_bgr(a) for a in images]
        n = len(imgs)
        ptrs = (C.c_void_p * n)(*[a.ctypes.data for a in imgs])
        hs = np.array([a.shape[0] for a in imgs], np.int32)
        ws = np.array([a.shape[1] for a in imgs], np.int32)
        st = np.array([a.strides[0] for a in imgs], np.int32)
        size = int(params.image_size)
        while True:
            boxes = np.zeros((n, max_faces, 5), np.float32)
            lm = np.zeros((n, max_faces, 5, 2), np.float32) if landmarks else None
            nf = np.zeros(n, np.int32)
            lmp = _ptr(lm) if landmarks else None
            if faces:
                out = np.empty((n, max_faces, 3, size, size), np.float32)
                rc = self._lib.dfd_mtcnn_extract(self._p, n, ptrs, _ptr(hs), _ptr(ws), _ptr(st), C.byref(params), max_faces,
                                                 _ptr(boxes), lmp, _ptr(nf), _ptr(out))
            else:
                out = None
                rc = self._lib.dfd_mtcnn_detect(self._p, n, ptrs, _ptr(hs), _ptr(ws), _ptr(st), C.byref(params), max_faces,
                                                _ptr(boxes), lmp, _ptr(nf))
            self._check(rc)
            most = int(nf.max()) if n else 0
            if most <= max_faces:
                break
            max_faces = most                      # an image holds more faces than there was room for: once more, with room
        res = []
        for i in range(n):
            k = int(nf[i])
            res.append((boxes[i, :k].copy(), lm[i, :k].copy() if landmarks else None, out[i, :k].copy() if faces else None))
        return res

    def mtcnn_detect(self, images, params: Optional[MtcnnParams] = None, landmarks: bool = True, max_faces: int = 16):
        """MTCNN.detect on a list of (H, W, 3) uint8 BGR images in one device pass (dfd_mtcnn_detect): per image
        (rows (k, 5) = x1, y1, x2, y2, probability, landmarks (k, 5, 2) or None, None), k = 0 when no face passes."""
        return self._mtcnn_call(images, params or mtcnn_params(), max_faces, landmarks, False)

    def mtcnn_extract(self, images, params: Optional[MtcnnParams] = None, landmarks: bool = False, max_faces: int = 16):
        """MTCNN.forward on a list of images (dfd_mtcnn_extract): as mtcnn_detect, plus the crops (k, 3, S, S) float32."""
        return self._mtcnn_call(images, params or mtcnn_params(), max_faces, landmarks, True)

    def ssd_tap(self, frame, name: str, capacity: int) -> np.ndarray:
        a = self._as_bgr(frame)
        out = np.empty(int(capacity), np.float32)
        cnt = C.c_size_t()
        self._check(self._lib.dfd_ssd_tap(self._p, _ptr(a), a.shape[0], a.shape[1], a.strides[0], name.encode(),
                                          _ptr(out), out.size, C.byref(cnt)))
        return out[: cnt.value]

    def ssd_detection_tap(self, heads=None, boxes=None, prob=None, n_priors: int = 8732, keep_top_k: int = 200):
        """The detector's tail on injected inputs (dfd_ssd_detection_tap), n images in one call.  `heads`: the six head
        outputs, source after source, each (n, cells, p * 6) flattened and concatenated -> decode + DetectionOutput,
        returns (boxes (n, P, 4), prob (n, P), rows, count).  `boxes` (n, P, 4) and `prob` (n, P): DetectionOutput
        alone, returns (rows, count).  rows (n, keep_top_k, 5) = score, x1, y1, x2, y2, zero past count[i]."""
        if heads is not None:
            x = np.ascontiguousarray(heads, np.float32).ravel()
            n, rem = divmod(x.size, n_priors * 6)
            assert rem == 0 and n >= 1, x.size
            bo, po = np.empty((n, n_priors, 4), np.float32), np.empty((n, n_priors), np.float32)
            args = (_ptr(x), None, None, _ptr(bo), _ptr(po))
        else:
            b, p = np.ascontiguousarray(boxes, np.float32), np.ascontiguousarray(prob, np.float32)
            assert b.ndim == 3 and b.shape[1:] == (n_priors, 4) and p.shape == b.shape[:2], (b.shape, p.shape)
            n = b.shape[0]
            args = (None, _ptr(b), _ptr(p), None, None)
        rows = np.empty((n, keep_top_k, 5), np.float32)
        count = np.zeros(n, np.int32)
        self._check(self._lib.dfd_ssd_detection_tap(self._p, n, *args, _ptr(rows), rows.size, _ptr(count)))
        return (bo, po, rows, count) if heads is not None else (rows, count)


class ClassifierLanes:
    """Several classifier forwards in flight on ONE device: `lanes` handles (each with its own stream and workspace,
    the same weights and the same measured GEMM tiles) take batches in turn, every call asynchronous.

    One batch-256 forward is ~54 dependent launches whose late layers (14 x 14 / 7 x 7 maps) leave CUs idle and whose
    launch gaps are 4-5 us each; a second forward's kernels fill both (2.97 -> 2.78 ms per
    batch).  The reference serves one frame at a time (deepfake_detection.py:357-406); a server that has two batches
    queued is the case this class is for, and the results are the same bits whichever lane computes a batch."""

    def __init__(self, blob: bytes, device: int = 0, max_batch: int = 8, lanes: int = 2, first: "Handle" = None):
        if lanes < 1:
            raise ValueError("lanes must be >= 1")
        self.handles = [first if first is not None else Handle(blob, device=device, max_batch=max_batch)]
        for _ in range(lanes - 1):
            self.handles.append(Handle(blob, device=device, max_batch=max_batch))
        self._owned = self.handles[1:] if first is not None else list(self.handles)
        self._next = 0
        # (if the lanes do not overlap in a process that has made many streams - two main streams mapped onto one hardware
        # queue run in line - give one lane another priority: handles[1].set_option("stream_priority", 1))

    def __len__(self):
        return len(self.handles)

    def warmup(self, n_crops: int):
        """lane 0 measures the tiles, the others take its table (a lane that tuned for itself could pick another of the
        bit-identical tiles; the table is shared so that every lane launches the same kernels)"""
        self.handles[0].warmup(n_crops, 0)
        table = self.handles[0].tiles_export()
        for h in self.handles[1:]:
            h.tiles_import(table)
            h.warmup(n_crops, 0)

    def set_option(self, name: str, value: int):
        for h in self.handles:
            h.set_option(name, value)

    def submit(self, x_dev: int, n: int, logits_dev: int) -> int:
        """queue one forward on the next lane (asynchronous); -> the lane index it went to"""
        k = self._next
        self.handles[k].classify_device(x_dev, n, logits_dev)
        self._next = (k + 1) % len(self.handles)
        return k

    def check_overlap(self, x_dev: int, n: int, outs, steps: int = 6, gain: float = 0.97):
        """Untimed check that the lanes really run side by side (the runtime may have mapped their main streams onto one
        hardware queue - then they run in line and two lanes are no faster than one).  Times `steps`
        forwards on lane 0 alone and on all lanes; if the lanes are not at least 3 % faster, lane 1's main stream is
        re-created in the high-priority pool and the measurement repeated, and whichever setting was faster stays.
        -> {"one_lane_ms", "lanes_ms", "lane1_priority", ...} (per forward)."""
        import time

        def run(handles):
            for h in handles:
                h.sync()
            t0 = time.perf_counter()
            for i in range(steps):
                handles[i % len(handles)].classify_device(x_dev, n, outs[i % len(handles)].ptr)
            for h in handles:
                h.sync()
            return (time.perf_counter() - t0) / steps * 1e3

        run(self.handles)                                           # clocks, first-use costs
        rep = {"one_lane_ms": round(run(self.handles[:1]), 4), "lanes_ms": round(run(self.handles), 4), "lane1_priority": 0}
        if len(self.handles) > 1 and rep["lanes_ms"] > gain * rep["one_lane_ms"]:
            self.handles[1].set_option("stream_priority", 1)
            rep["lanes_ms_high_priority"] = round(run(self.handles), 4)
            if rep["lanes_ms_high_priority"] < rep["lanes_ms"]:
                rep["lane1_priority"] = 1
            else:
                self.handles[1].set_option("stream_priority", 0)
        self._next = 0
        return rep

    def submit_alone(self, x_dev: int, n: int, logits_dev: int) -> int:
        """queue one forward that runs with NO other lane's kernels beside it, ordered on the device (dfd_wait_for: no
        host wait, the host stays ahead of the GPU): it starts when the other lanes have finished what they hold, and they
        continue when it has finished.  bench.py's instrumented step - per-launch events then time isolated kernels."""
        k = self._next
        me = self.handles[k]
        for o in self.handles:
            if o is not me:
                me.wait_for(o)
        me.classify_device(x_dev, n, logits_dev)
        for o in self.handles:
            if o is not me:
                o.wait_for(me)
        self._next = (k + 1) % len(self.handles)
        return k

    def sync(self):
        for h in self.handles:
            h.sync()

    def close(self):
        """closes the handles this object made; a `first` handle passed in stays open and remains the only lane"""
        for h in self._owned:
            h.close()
        self.handles = [h for h in self.handles if not any(h is o for o in self._owned)]
        self._owned = []
        self._next = 0
