"""ctypes binding of libtcamd_hip.so: HIP runtime glue and CDNA4 kernels.

Runtime: device memory, pinned host memory, IPC handles, copies, streams,
events, peer access.  Kernels (csrc/kernels/*.hip, gfx950):

* :func:`synth_fill`      K1 Philox synthetic data (random/zero/constant/normal)
* :func:`convert`         K4/K5 FP32 <-> BF16 (trunc|RNE) / FP16 / FP8 e4m3,e5m2
* :func:`layout_pack`     K6 fused gather + NCHW<->NHWC + convert + scale/bias
* :func:`resize_pack`     K20 bilinear / K21 antialiased resize + adapt + scale/bias + pack of uint8 images
* :func:`jpeg_decode`     K22 dequantise + IDCT + chroma upsample + YCbCr->RGB of entropy-decoded JPEG coefficients
* :func:`jpeg_huffman`    K23 Huffman decode of packed JPEG scans into the coefficients K22 reads
* :func:`jpeg_huffman_wide`  K24 the same across workgroups: scans up to 32 MiB, the compact buffer of any scale
* :func:`png_unfilter`    K25 PNG unfilter + palette / depth / alpha conversion of inflated scanlines
* :func:`compare_expected` K26 outputs against expectations on the device: mismatches, first index, largest difference
* :func:`batched_copy`    K7 one-launch gather/concat/scatter of byte ranges
* :func:`pack_bytes`      K2 BYTES serialisation (LDS block scan + scatter)
* :func:`index_bytes`     K3 BYTES index walk through an LDS window
* :func:`topk_rows`       K19 per-row top-K {score, index} pairs (classification)
* :func:`qa_spans`        K27 per-row n best answer spans of question-answering logits
* :func:`wordpiece_tokenize`  K28 UTF-8 text to BERT question-answering rows (WordPiece)
* :func:`wordpiece_windows`   K28w the same over doc-stride windows of a long context
* :func:`qa_spans_masked`     K27 with a start mask (the max-context rule of the windows)
* :func:`qa_merge`            K29 the n best spans of a document from those of its windows

Pointers are plain ints (device addresses).  ``stream`` is a hipStream_t as an
int (``torch.cuda.current_stream().cuda_stream`` works) or None for the
library's per-device copy stream / the null stream.
"""

import contextlib
import ctypes
import os
import sys

import numpy as np

from . import dtypes

# TCAMD_HIP_LIB: load another build of the library (A/B timing of two kernel
# builds in one tree, tools only)
_PATH = os.environ.get("TCAMD_HIP_LIB") or os.path.join(os.path.dirname(os.path.abspath(__file__)), "lib",
                                                        "libtcamd_hip.so")
IPC_HANDLE_SIZE = 64

MEMORY_UNREGISTERED = 0
MEMORY_HOST = 1
MEMORY_DEVICE = 2
MEMORY_MANAGED = 3


class HipError(RuntimeError):
    def __init__(self, code, what):
        self.code = code
        msg = _lib.tcamd_error_string(code).decode() if _lib is not None else str(code)
        super().__init__("%s failed: %s (hipError %d)" % (what, msg, code))


_lib = None

_SIGS = {
    "tcamd_error_string": ([ctypes.c_int], ctypes.c_char_p),
    "tcamd_ipc_handle_size": ([], ctypes.c_int),
    "tcamd_device_count": ([ctypes.POINTER(ctypes.c_int)], ctypes.c_int),
    "tcamd_set_device": ([ctypes.c_int], ctypes.c_int),
    "tcamd_get_device": ([ctypes.POINTER(ctypes.c_int)], ctypes.c_int),
    "tcamd_device_synchronize": ([ctypes.c_int], ctypes.c_int),
    "tcamd_device_uva": ([ctypes.c_int, ctypes.POINTER(ctypes.c_int)], ctypes.c_int),
    "tcamd_device_name": ([ctypes.c_int, ctypes.c_char_p, ctypes.c_int], ctypes.c_int),
    "tcamd_malloc": ([ctypes.c_int, ctypes.c_size_t, ctypes.POINTER(ctypes.c_void_p)], ctypes.c_int),
    "tcamd_free": ([ctypes.c_int, ctypes.c_void_p], ctypes.c_int),
    "tcamd_host_alloc": ([ctypes.c_size_t, ctypes.POINTER(ctypes.c_void_p)], ctypes.c_int),
    "tcamd_host_free": ([ctypes.c_void_p], ctypes.c_int),
    "tcamd_host_register": ([ctypes.c_void_p, ctypes.c_size_t], ctypes.c_int),
    "tcamd_host_unregister": ([ctypes.c_void_p], ctypes.c_int),
    "tcamd_ipc_get_handle": ([ctypes.c_void_p, ctypes.c_char_p], ctypes.c_int),
    "tcamd_ipc_open": ([ctypes.c_char_p, ctypes.c_int, ctypes.POINTER(ctypes.c_void_p)], ctypes.c_int),
    "tcamd_ipc_close": ([ctypes.c_void_p, ctypes.c_int], ctypes.c_int),
    "tcamd_pointer_info": (
        [ctypes.c_void_p, ctypes.POINTER(ctypes.c_int), ctypes.POINTER(ctypes.c_int)],
        ctypes.c_int,
    ),
    "tcamd_memcpy": ([ctypes.c_int, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_size_t], ctypes.c_int),
    "tcamd_memcpy_async": ([ctypes.c_void_p, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_void_p], ctypes.c_int),
    "tcamd_memset_async": ([ctypes.c_void_p, ctypes.c_int, ctypes.c_size_t, ctypes.c_void_p], ctypes.c_int),
    "tcamd_memcpy_peer_async": (
        [ctypes.c_void_p, ctypes.c_int, ctypes.c_void_p, ctypes.c_int, ctypes.c_size_t, ctypes.c_void_p],
        ctypes.c_int,
    ),
    "tcamd_enable_peer": ([ctypes.c_int, ctypes.c_int], ctypes.c_int),
    "tcamd_stream_create": ([ctypes.c_int, ctypes.POINTER(ctypes.c_void_p)], ctypes.c_int),
    "tcamd_stream_destroy": ([ctypes.c_void_p], ctypes.c_int),
    "tcamd_stream_synchronize": ([ctypes.c_void_p], ctypes.c_int),
    "tcamd_event_create": ([ctypes.POINTER(ctypes.c_void_p)], ctypes.c_int),
    "tcamd_event_destroy": ([ctypes.c_void_p], ctypes.c_int),
    "tcamd_event_record": ([ctypes.c_void_p, ctypes.c_void_p], ctypes.c_int),
    "tcamd_event_synchronize": ([ctypes.c_void_p], ctypes.c_int),
    "tcamd_event_elapsed_ms": ([ctypes.c_void_p, ctypes.c_void_p, ctypes.POINTER(ctypes.c_float)], ctypes.c_int),
    "tcamd_stream_wait_event": ([ctypes.c_void_p, ctypes.c_void_p], ctypes.c_int),
    "tcamd_last_error": ([], ctypes.c_int),
    # kernels
    "tcamd_synth_fill": (
        [
            ctypes.c_void_p, ctypes.c_size_t, ctypes.c_int, ctypes.c_int, ctypes.c_double,
            ctypes.c_double, ctypes.c_uint64, ctypes.c_uint64, ctypes.c_void_p,
        ],
        ctypes.c_int,
    ),
    "tcamd_convert": (
        [ctypes.c_void_p, ctypes.c_int, ctypes.c_void_p, ctypes.c_int, ctypes.c_size_t, ctypes.c_int, ctypes.c_void_p],
        ctypes.c_int,
    ),
    "tcamd_layout_pack": (
        [
            ctypes.POINTER(ctypes.c_void_p), ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_void_p,
            ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_int,
            ctypes.POINTER(ctypes.c_float), ctypes.POINTER(ctypes.c_float), ctypes.c_int, ctypes.c_void_p,
        ],
        ctypes.c_int,
    ),
    "tcamd_resize_pack": (
        [
            ctypes.POINTER(ctypes.c_void_p), ctypes.POINTER(ctypes.c_int32), ctypes.POINTER(ctypes.c_int32),
            ctypes.POINTER(ctypes.c_int32), ctypes.c_int, ctypes.POINTER(ctypes.c_void_p), ctypes.c_int, ctypes.c_int,
            ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.POINTER(ctypes.c_float), ctypes.POINTER(ctypes.c_float),
            ctypes.c_int, ctypes.c_void_p,
        ],
        ctypes.c_int,
    ),
    "tcamd_resize_pack_aa": (
        [
            ctypes.POINTER(ctypes.c_void_p), ctypes.POINTER(ctypes.c_int32), ctypes.POINTER(ctypes.c_int32),
            ctypes.POINTER(ctypes.c_int32), ctypes.c_int, ctypes.POINTER(ctypes.c_void_p), ctypes.c_int, ctypes.c_int,
            ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.POINTER(ctypes.c_float), ctypes.POINTER(ctypes.c_float),
            ctypes.c_int, ctypes.c_void_p,
        ],
        ctypes.c_int,
    ),
    "tcamd_jpeg_decode": (
        [
            ctypes.POINTER(ctypes.c_void_p), ctypes.POINTER(ctypes.c_int32), ctypes.POINTER(ctypes.c_int32),
            ctypes.POINTER(ctypes.c_int32), ctypes.POINTER(ctypes.c_int32), ctypes.POINTER(ctypes.c_int32),
            ctypes.c_int, ctypes.POINTER(ctypes.c_void_p), ctypes.c_void_p,
        ],
        ctypes.c_int,
    ),
    "tcamd_jpeg_decode_scaled": (
        [
            ctypes.POINTER(ctypes.c_void_p), ctypes.POINTER(ctypes.c_int32), ctypes.POINTER(ctypes.c_int32),
            ctypes.POINTER(ctypes.c_int32), ctypes.POINTER(ctypes.c_int32), ctypes.POINTER(ctypes.c_int32),
            ctypes.POINTER(ctypes.c_int32), ctypes.POINTER(ctypes.c_int32), ctypes.POINTER(ctypes.c_int32),
            ctypes.c_int, ctypes.POINTER(ctypes.c_void_p), ctypes.c_void_p,
        ],
        ctypes.c_int,
    ),
    "tcamd_jpeg_huffman": (
        [
            ctypes.POINTER(ctypes.c_void_p), ctypes.POINTER(ctypes.c_void_p), ctypes.c_void_p, ctypes.c_int,
            ctypes.c_void_p,
        ],
        ctypes.c_int,
    ),
    "tcamd_jpeg_huffman_wide_workspace": ([ctypes.c_uint64, ctypes.c_uint64], ctypes.c_uint64),
    "tcamd_jpeg_huffman_wide": (
        [
            ctypes.POINTER(ctypes.c_void_p), ctypes.POINTER(ctypes.c_void_p), ctypes.POINTER(ctypes.c_uint32),
            ctypes.c_void_p, ctypes.c_void_p, ctypes.c_uint64, ctypes.c_int, ctypes.c_uint32, ctypes.c_void_p,
        ],
        ctypes.c_int,
    ),
    "tcamd_png_unfilter_geometry": ([ctypes.POINTER(ctypes.c_int32)], None),
    "tcamd_png_unfilter": (
        [
            ctypes.POINTER(ctypes.c_void_p), ctypes.POINTER(ctypes.c_int32), ctypes.POINTER(ctypes.c_int32),
            ctypes.POINTER(ctypes.c_int32), ctypes.POINTER(ctypes.c_int32), ctypes.POINTER(ctypes.c_int32),
            ctypes.c_int, ctypes.POINTER(ctypes.c_void_p), ctypes.c_void_p,
        ],
        ctypes.c_int,
    ),
    "tcamd_compare_geometry": ([ctypes.POINTER(ctypes.c_uint64)], None),
    "tcamd_compare_expected": (
        [ctypes.POINTER(dtypes.ComparePair), ctypes.c_int, ctypes.c_double, ctypes.c_double, ctypes.c_void_p,
         ctypes.c_void_p],
        ctypes.c_int,
    ),
    "tcamd_batched_copy": (
        [
            ctypes.POINTER(ctypes.c_void_p), ctypes.POINTER(ctypes.c_void_p), ctypes.POINTER(ctypes.c_uint64),
            ctypes.c_int, ctypes.c_void_p,
        ],
        ctypes.c_int,
    ),
    "tcamd_topk_rows": (
        [
            ctypes.c_void_p, ctypes.c_uint64, ctypes.c_int32, ctypes.c_int32, ctypes.c_void_p, ctypes.c_int32,
            ctypes.c_void_p, ctypes.c_void_p,
        ],
        ctypes.c_int,
    ),
    "tcamd_qa_spans": (
        [
            ctypes.c_void_p, ctypes.c_void_p, ctypes.c_uint64, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_uint64,
            ctypes.c_int32, ctypes.c_int32, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int32, ctypes.c_void_p,
            ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p,
        ],
        ctypes.c_int,
    ),
    "tcamd_wordpiece_tokenize": (
        [
            ctypes.c_void_p, ctypes.c_uint64, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int32, ctypes.c_int32,
            ctypes.c_void_p, ctypes.c_uint64, ctypes.c_void_p, ctypes.c_uint64, ctypes.c_void_p, ctypes.c_void_p,
            ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p,
        ],
        ctypes.c_int,
    ),
    "tcamd_wordpiece_workspace": ([ctypes.c_int32, ctypes.c_uint64], ctypes.c_uint64),
    "tcamd_wordpiece_windows_workspace": ([ctypes.c_int32, ctypes.c_uint64], ctypes.c_uint64),
    "tcamd_wordpiece_windows": (
        [
            ctypes.c_void_p, ctypes.c_uint64, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p,
            ctypes.c_int32, ctypes.c_int32, ctypes.c_void_p, ctypes.c_uint64, ctypes.c_void_p, ctypes.c_uint64,
            ctypes.c_int32, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p,
            ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p,
        ],
        ctypes.c_int,
    ),
    "tcamd_qa_spans_masked": (
        [
            ctypes.c_void_p, ctypes.c_void_p, ctypes.c_uint64, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p,
            ctypes.c_uint64, ctypes.c_int32, ctypes.c_int32, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int32,
            ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p,
        ],
        ctypes.c_int,
    ),
    "tcamd_qa_merge": (
        [
            ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int32, ctypes.c_void_p, ctypes.c_void_p,
            ctypes.c_int32, ctypes.c_void_p, ctypes.c_int32, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p,
            ctypes.c_void_p, ctypes.c_void_p,
        ],
        ctypes.c_int,
    ),
    "tcamd_wordpiece_geometry": ([ctypes.POINTER(ctypes.c_int32)], None),
    # fused DenseNet kernels (csrc/kernels/densenet.hip)
    "tcamd_dn_conv1x1": (
        [
            ctypes.c_void_p, ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_void_p, ctypes.c_void_p,
            ctypes.c_void_p, ctypes.c_int, ctypes.c_void_p, ctypes.c_int, ctypes.c_void_p, ctypes.c_int,
            ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_void_p,
        ],
        ctypes.c_int,
    ),
    "tcamd_dn_conv1x1_ex": (
        [
            ctypes.c_void_p, ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_void_p, ctypes.c_void_p,
            ctypes.c_void_p, ctypes.c_int, ctypes.c_void_p, ctypes.c_int, ctypes.c_void_p, ctypes.c_int,
            ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_void_p, ctypes.c_size_t,
            ctypes.c_void_p,
        ],
        ctypes.c_int,
    ),
    "tcamd_dn_conv1x1_v": (
        [
            ctypes.c_void_p, ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_void_p, ctypes.c_void_p,
            ctypes.c_void_p, ctypes.c_int, ctypes.c_void_p, ctypes.c_int, ctypes.c_void_p, ctypes.c_int,
            ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_void_p,
        ],
        ctypes.c_int,
    ),
    "tcamd_dn_conv3x3_v": (
        [ctypes.c_void_p, ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int,
         ctypes.c_int, ctypes.c_void_p],
        ctypes.c_int,
    ),
    "tcamd_dn_conv3x3": (
        [ctypes.c_void_p, ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int,
         ctypes.c_void_p],
        ctypes.c_int,
    ),
    "tcamd_dn_stem_pool": (
        [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_int,
         ctypes.c_int, ctypes.c_void_p],
        ctypes.c_int,
    ),
    "tcamd_dn_stem_fused": (
        [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int,
         ctypes.c_int, ctypes.c_void_p],
        ctypes.c_int,
    ),
    "tcamd_dn_head_pool": (
        [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int, ctypes.c_int, ctypes.c_int,
         ctypes.c_void_p],
        ctypes.c_int,
    ),
    # fp32-parity (bf16x3 split-precision) DenseNet kernels (csrc/kernels/densenet_x3.hip)
    "tcamd_x3_conv1x1_ws_bytes": ([ctypes.c_int, ctypes.c_int, ctypes.c_int], ctypes.c_size_t),
    "tcamd_x3_conv1x1": (
        [
            ctypes.c_void_p, ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_void_p, ctypes.c_void_p,
            ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p,
            ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_void_p, ctypes.c_size_t,
            ctypes.c_void_p,
        ],
        ctypes.c_int,
    ),
    "tcamd_x3_conv3x3": (
        [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_void_p,
         ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int, ctypes.c_void_p],
        ctypes.c_int,
    ),
    "tcamd_x3_dense_layer": (
        [
            ctypes.c_void_p, ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_void_p,
            ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p,
            ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int, ctypes.c_void_p, ctypes.c_size_t,
            ctypes.c_void_p,
        ],
        ctypes.c_int,
    ),
    "tcamd_x3s_dense_layer": (
        [
            ctypes.c_void_p, ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_void_p,
            ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p,
            ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int, ctypes.c_void_p,
        ],
        ctypes.c_int,
    ),
    "tcamd_x3s_steps_per_block": ([ctypes.c_int, ctypes.c_int], ctypes.c_int),
    "tcamd_x3c_base": (
        [ctypes.c_void_p, ctypes.c_int, ctypes.c_void_p, ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_int,
         ctypes.c_void_p],
        ctypes.c_int,
    ),
    "tcamd_x3c_layer": (
        [ctypes.c_void_p, ctypes.c_int, ctypes.c_int, ctypes.c_void_p, ctypes.c_int, ctypes.c_int, ctypes.c_int,
         ctypes.c_int, ctypes.c_void_p],
        ctypes.c_int,
    ),
    "tcamd_x3_dense_fused": (
        [
            ctypes.c_void_p, ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_void_p,
            ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p,
            ctypes.c_void_p, ctypes.c_int, ctypes.c_void_p,
        ],
        ctypes.c_int,
    ),
    "tcamd_x3_dense_small": (
        [
            ctypes.c_void_p, ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_void_p,
            ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p,
            ctypes.c_void_p, ctypes.c_int, ctypes.c_int, ctypes.c_void_p,
        ],
        ctypes.c_int,
    ),
    "tcamd_x3_dense_small_pair": (
        [ctypes.c_void_p] + [ctypes.c_int] * 5 + [ctypes.c_void_p] * 15 + [ctypes.c_int, ctypes.c_int, ctypes.c_void_p],
        ctypes.c_int,
    ),
    "tcamd_x3_dense_small_pair_supported": ([ctypes.c_int, ctypes.c_int], ctypes.c_int),
    "tcamd_x3_small_tiles": ([ctypes.c_int, ctypes.c_int], ctypes.c_int),
    "tcamd_x3_small_tiles_shared": ([ctypes.c_int, ctypes.c_int, ctypes.c_int], ctypes.c_int),
    "tcamd_x3_dense_fused3": (
        [
            ctypes.c_void_p, ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_void_p,
            ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p,
            ctypes.c_void_p, ctypes.c_int, ctypes.c_void_p,
        ],
        ctypes.c_int,
    ),
    "tcamd_k3_set_check": ([ctypes.c_int], ctypes.c_int),
    "tcamd_knob_count": ([], ctypes.c_int),
    "tcamd_knob_info": (
        [ctypes.c_int, ctypes.POINTER(ctypes.c_char_p), ctypes.POINTER(ctypes.c_longlong),
         ctypes.POINTER(ctypes.c_longlong), ctypes.POINTER(ctypes.c_char_p)],
        ctypes.c_int,
    ),
    "tcamd_knob_set": ([ctypes.c_char_p, ctypes.c_longlong, ctypes.POINTER(ctypes.c_longlong)], ctypes.c_int),
    "tcamd_k17_gemm": (
        [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int, ctypes.c_int, ctypes.c_int,
         ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_void_p],
        ctypes.c_int,
    ),
    "tcamd_k17_last_tm": ([], ctypes.c_int),
    "tcamd_k18_gemm": (
        [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int, ctypes.c_int, ctypes.c_int,
         ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_int,
         ctypes.c_longlong, ctypes.c_void_p],
        ctypes.c_int,
    ),
    "tcamd_k18_cfg": (
        [ctypes.c_int, ctypes.POINTER(ctypes.c_int), ctypes.POINTER(ctypes.c_int), ctypes.POINTER(ctypes.c_int),
         ctypes.POINTER(ctypes.c_int)],
        ctypes.c_int,
    ),
    "tcamd_k18_calls": ([], ctypes.c_longlong),
    "tcamd_qa_head": (
        [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int,
         ctypes.c_int, ctypes.c_int, ctypes.c_void_p],
        ctypes.c_int,
    ),
    "tcamd_add_layernorm_parts": (
        [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int, ctypes.c_longlong, ctypes.c_void_p, ctypes.c_void_p,
         ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int, ctypes.c_int, ctypes.c_float, ctypes.c_int, ctypes.c_void_p],
        ctypes.c_int,
    ),
    "tcamd_add_layernorm_parts3": (
        [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int, ctypes.c_longlong, ctypes.c_void_p, ctypes.c_void_p,
         ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int, ctypes.c_int, ctypes.c_float, ctypes.c_int,
         ctypes.c_void_p],
        ctypes.c_int,
    ),
    "tcamd_k17_calls": ([], ctypes.c_longlong),
    "tcamd_x3_cat": ([ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int, ctypes.c_int, ctypes.c_void_p], ctypes.c_int),
    "tcamd_x3_stem": (
        [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int,
         ctypes.c_int, ctypes.c_void_p],
        ctypes.c_int,
    ),
    "tcamd_x3_head_pool": (
        [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int, ctypes.c_int, ctypes.c_int,
         ctypes.c_void_p],
        ctypes.c_int,
    ),
    "tcamd_x3_split": (
        [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_void_p],
        ctypes.c_int,
    ),
    "tcamd_add_layernorm": (
        [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int,
         ctypes.c_int, ctypes.c_float, ctypes.c_void_p],
        ctypes.c_int,
    ),
    "tcamd_embed_layernorm": (
        [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p,
         ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_int,
         ctypes.c_float, ctypes.c_void_p],
        ctypes.c_int,
    ),
    "tcamd_attention_bias": (
        [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int, ctypes.c_int, ctypes.c_int,
         ctypes.c_float, ctypes.c_void_p],
        ctypes.c_int,
    ),
    "tcamd_attention_f32": (
        [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_float,
         ctypes.c_int, ctypes.c_void_p],
        ctypes.c_int,
    ),
    "tcamd_attention": (
        [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_float,
         ctypes.c_void_p],
        ctypes.c_int,
    ),
    "tcamd_attention_plan": (
        [ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.POINTER(ctypes.c_int), ctypes.POINTER(ctypes.c_int)],
        ctypes.c_int,
    ),
    "tcamd_attention_f32_plan": (
        [ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.POINTER(ctypes.c_int)], ctypes.c_int,
    ),
    # padding-free bert_large: K30 pack plan / packed embed / unpack (csrc/kernels/bert_pack.hip), K12v
    "tcamd_bert_pad_logit": ([], ctypes.c_float),
    "tcamd_bert_pack_plan": (
        [ctypes.c_void_p, ctypes.c_longlong, ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_void_p,
         ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p],
        ctypes.c_int,
    ),
    "tcamd_embed_layernorm_packed": (
        [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p,
         ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_int,
         ctypes.c_int, ctypes.c_int, ctypes.c_float, ctypes.c_void_p],
        ctypes.c_int,
    ),
    "tcamd_unpack_logits": (
        [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int,
         ctypes.c_int, ctypes.c_void_p],
        ctypes.c_int,
    ),
    "tcamd_attention_packed": (
        [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int,
         ctypes.c_int, ctypes.c_int, ctypes.c_float, ctypes.c_void_p],
        ctypes.c_int,
    ),
    "tcamd_attention_packed_plan": (
        [ctypes.c_int, ctypes.c_int, ctypes.POINTER(ctypes.c_int), ctypes.POINTER(ctypes.c_int)], ctypes.c_int,
    ),
    # ... and its fp32-parity form: the fp32 packed embedding, K12xv
    "tcamd_embed_layernorm_packed_f32": (
        [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p,
         ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int, ctypes.c_int, ctypes.c_int,
         ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_float, ctypes.c_void_p],
        ctypes.c_int,
    ),
    "tcamd_attention_f32_packed": (
        [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int, ctypes.c_int, ctypes.c_int,
         ctypes.c_float, ctypes.c_int, ctypes.c_void_p],
        ctypes.c_int,
    ),
    "tcamd_attention_f32_packed_plan": (
        [ctypes.c_int, ctypes.c_int, ctypes.POINTER(ctypes.c_int)], ctypes.c_int,
    ),
    # native batch executor for pointer-table graph models (csrc/runtime/graph_exec.hip)
    "tcamd_pgx_create": (
        [ctypes.c_int32, ctypes.c_int32, ctypes.c_uint64, ctypes.c_uint64, ctypes.c_int32,
         ctypes.POINTER(ctypes.c_int32), ctypes.c_char_p, ctypes.c_int32],
        ctypes.c_void_p,
    ),
    "tcamd_pgx_set_instance": (
        [ctypes.c_void_p, ctypes.c_int32, ctypes.c_void_p, ctypes.POINTER(ctypes.c_uint64), ctypes.c_uint64,
         ctypes.c_uint64, ctypes.c_uint64, ctypes.POINTER(ctypes.c_uint64), ctypes.c_char_p, ctypes.c_int32],
        ctypes.c_int32,
    ),
    "tcamd_pgx_execute": (
        [ctypes.c_void_p, ctypes.c_int32, ctypes.c_void_p, ctypes.c_char_p, ctypes.c_int32], ctypes.c_int,
    ),
    "tcamd_pgx_stats": ([ctypes.c_void_p, ctypes.POINTER(ctypes.c_uint64)], ctypes.c_int32),
    "tcamd_pgx_destroy": ([ctypes.c_void_p], None),
    "tcamd_pack_bytes_workspace": ([ctypes.c_uint64], ctypes.c_uint64),
    "tcamd_pack_bytes": (
        [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_uint64, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p],
        ctypes.c_int,
    ),
    "tcamd_index_bytes_last_path": ([ctypes.POINTER(ctypes.c_uint64)], ctypes.c_int),
    "tcamd_pack_bytes_strided": (
        [ctypes.c_void_p, ctypes.c_uint64, ctypes.c_void_p, ctypes.c_uint64, ctypes.c_void_p, ctypes.c_void_p,
         ctypes.c_void_p],
        ctypes.c_int,
    ),
    "tcamd_index_bytes": (
        [
            ctypes.c_void_p, ctypes.c_uint64, ctypes.c_uint64, ctypes.c_void_p, ctypes.c_void_p,
            ctypes.c_void_p, ctypes.c_void_p,
        ],
        ctypes.c_int,
    ),
}


def _load():
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(_PATH):
        raise ImportError(
            "libtcamd_hip.so is not built (expected at %s); run `python __graft_entry__.py build`" % _PATH
        )
    # One HIP runtime per process: torch bundles libamdhip64.so.7 with the same
    # SONAME, so whichever copy is loaded first is shared by both.
    lib = ctypes.CDLL(_PATH, mode=ctypes.RTLD_GLOBAL)
    for name, (argtypes, restype) in _SIGS.items():
        if os.environ.get("TCAMD_HIP_LIB") and not hasattr(lib, name):
            continue  # an older A/B build: entry points it predates stay unbound
        fn = getattr(lib, name)
        fn.argtypes = argtypes
        fn.restype = restype
    _lib = lib
    return lib


def lib():
    return _load()


def _check(rc, what):
    if rc != 0:
        raise HipError(rc, what)


def _vp(x):
    return None if x is None or x == 0 else ctypes.c_void_p(int(x))


def loaded_path():
    return _PATH


# ---------------------------------------------------------------------------
# runtime
# ---------------------------------------------------------------------------
def device_count():
    n = ctypes.c_int(0)
    rc = _load().tcamd_device_count(ctypes.byref(n))
    return n.value if rc == 0 else 0


def set_device(dev):
    _check(_load().tcamd_set_device(dev), "hipSetDevice")


def get_device():
    d = ctypes.c_int(0)
    _check(_load().tcamd_get_device(ctypes.byref(d)), "hipGetDevice")
    return d.value


def synchronize(dev=0):
    _check(_load().tcamd_device_synchronize(dev), "hipDeviceSynchronize")


def device_uva(dev):
    v = ctypes.c_int(0)
    _check(_load().tcamd_device_uva(dev, ctypes.byref(v)), "hipGetDeviceProperties")
    return bool(v.value)


def device_arch(dev=0):
    buf = ctypes.create_string_buffer(128)
    _check(_load().tcamd_device_name(dev, buf, 128), "hipGetDeviceProperties")
    return buf.value.decode()


def malloc(dev, nbytes):
    p = ctypes.c_void_p()
    _check(_load().tcamd_malloc(dev, nbytes, ctypes.byref(p)), "hipMalloc(%d B)" % nbytes)
    return p.value


def free(dev, ptr):
    _check(_load().tcamd_free(dev, _vp(ptr)), "hipFree")


def host_alloc(nbytes):
    p = ctypes.c_void_p()
    _check(_load().tcamd_host_alloc(nbytes, ctypes.byref(p)), "hipHostMalloc")
    return p.value


def host_free(ptr):
    _check(_load().tcamd_host_free(_vp(ptr)), "hipHostFree")


def host_register(ptr, nbytes):
    _check(_load().tcamd_host_register(_vp(ptr), nbytes), "hipHostRegister")


def host_unregister(ptr):
    _check(_load().tcamd_host_unregister(_vp(ptr)), "hipHostUnregister")


def ipc_get_handle(ptr):
    buf = ctypes.create_string_buffer(IPC_HANDLE_SIZE)
    _check(_load().tcamd_ipc_get_handle(_vp(ptr), buf), "hipIpcGetMemHandle")
    return buf.raw


def ipc_open(handle, dev):
    if len(handle) != IPC_HANDLE_SIZE:
        raise ValueError("IPC handle must be %d bytes" % IPC_HANDLE_SIZE)
    p = ctypes.c_void_p()
    _check(_load().tcamd_ipc_open(bytes(handle), dev, ctypes.byref(p)), "hipIpcOpenMemHandle")
    return p.value


def ipc_close(ptr, dev):
    _check(_load().tcamd_ipc_close(_vp(ptr), dev), "hipIpcCloseMemHandle")


def pointer_info(ptr):
    mt = ctypes.c_int(0)
    dev = ctypes.c_int(-1)
    _check(_load().tcamd_pointer_info(_vp(ptr), ctypes.byref(mt), ctypes.byref(dev)), "hipPointerGetAttributes")
    return mt.value, dev.value


def _host_ptr(buf):
    if isinstance(buf, np.ndarray):
        if not buf.flags["C_CONTIGUOUS"]:
            raise ValueError("host buffer must be C-contiguous")
        return buf.ctypes.data
    if isinstance(buf, int):
        return buf
    return ctypes.addressof(ctypes.c_char.from_buffer(buf))


def memcpy(dst, src, nbytes, dev=0):
    """Synchronous copy (any direction, UVA) on the per-device copy stream."""
    if nbytes:
        _check(_load().tcamd_memcpy(dev, _vp(dst), _vp(src), nbytes), "hipMemcpy")


def memcpy_h2d(dst_ptr, host, nbytes, dev=0):
    memcpy(dst_ptr, _host_ptr(host), nbytes, dev)


def memcpy_d2h(host, src_ptr, nbytes, dev=0):
    memcpy(_host_ptr(host), src_ptr, nbytes, dev)


def memcpy_d2d(dst_ptr, src_ptr, nbytes, dev=0):
    memcpy(dst_ptr, src_ptr, nbytes, dev)


def memcpy_async(dst, src, nbytes, stream=None):
    if nbytes:
        _check(_load().tcamd_memcpy_async(_vp(dst), _vp(src), nbytes, _vp(stream)), "hipMemcpyAsync")


def memset_async(dst, value, nbytes, stream=None):
    _check(_load().tcamd_memset_async(_vp(dst), value, nbytes, _vp(stream)), "hipMemsetAsync")


def memcpy_peer_async(dst, dst_dev, src, src_dev, nbytes, stream=None):
    _check(
        _load().tcamd_memcpy_peer_async(_vp(dst), dst_dev, _vp(src), src_dev, nbytes, _vp(stream)),
        "hipMemcpyPeerAsync",
    )


def enable_peer(dev, peer):
    _check(_load().tcamd_enable_peer(dev, peer), "hipDeviceEnablePeerAccess(%d->%d)" % (dev, peer))


class Stream:
    """A non-blocking HIP stream owned by this library."""

    def __init__(self, dev=0):
        self.dev = dev
        s = ctypes.c_void_p()
        _check(_load().tcamd_stream_create(dev, ctypes.byref(s)), "hipStreamCreate")
        self.handle = s.value

    def synchronize(self):
        _check(_load().tcamd_stream_synchronize(_vp(self.handle)), "hipStreamSynchronize")

    def close(self):
        if self.handle:
            _load().tcamd_stream_destroy(_vp(self.handle))
            self.handle = None

    def __int__(self):
        return self.handle or 0


def stream_synchronize(stream):
    _check(_load().tcamd_stream_synchronize(_vp(stream)), "hipStreamSynchronize")


class Event:
    def __init__(self):
        e = ctypes.c_void_p()
        _check(_load().tcamd_event_create(ctypes.byref(e)), "hipEventCreate")
        self.handle = e.value

    def record(self, stream=None):
        _check(_load().tcamd_event_record(_vp(self.handle), _vp(stream)), "hipEventRecord")

    def synchronize(self):
        _check(_load().tcamd_event_synchronize(_vp(self.handle)), "hipEventSynchronize")

    def elapsed_ms(self, end):
        ms = ctypes.c_float(0)
        _check(_load().tcamd_event_elapsed_ms(_vp(self.handle), _vp(end.handle), ctypes.byref(ms)), "hipEventElapsedTime")
        return ms.value

    def close(self):
        if self.handle:
            _load().tcamd_event_destroy(_vp(self.handle))
            self.handle = None


# ---------------------------------------------------------------------------
# kernels
# ---------------------------------------------------------------------------
SYNTH_ZERO, SYNTH_CONST, SYNTH_UNIFORM, SYNTH_NORMAL = 0, 1, 2, 3


def synth_fill(ptr, n_elems, datatype, mode=SYNTH_UNIFORM, lo=0.0, hi=1.0, seed=0, stream_id=0, stream=None):
    """K1: fill ``n_elems`` of ``datatype`` at device ``ptr`` (16-B aligned).

    uniform: floats in [lo, hi), integers in [lo, hi]; normal: mean lo, std hi.
    Deterministic in (seed, stream_id, element offset).
    """
    _check(
        _load().tcamd_synth_fill(
            _vp(ptr), n_elems, dtypes.code(datatype), mode, float(lo), float(hi),
            seed & (2**64 - 1), stream_id & (2**64 - 1), _vp(stream),
        ),
        "synth_fill",
    )


def convert(src, src_dtype, dst, dst_dtype, n, rounding="trunc", stream=None):
    """K4/K5 elementwise conversion between FP32 and BF16/FP16/FP8."""
    r = 0 if rounding == "trunc" else 1
    _check(
        _load().tcamd_convert(_vp(src), dtypes.code(src_dtype), _vp(dst), dtypes.code(dst_dtype), n, r, _vp(stream)),
        "convert %s->%s" % (src_dtype, dst_dtype),
    )


LAYOUTS = {"NCHW": 0, "NHWC": 1}


def layout_pack(srcs, src_dtype, src_layout, dst, dst_dtype, dst_layout, C, H, W,
                scale=None, bias=None, rounding="rne", stream=None):
    """K6: gather len(srcs) images (each C*H*W) into ``dst`` with layout/dtype
    conversion and per-channel ``x*scale[c]+bias[c]``."""
    n = len(srcs)
    arr = (ctypes.c_void_p * max(n, 1))(*[int(p) for p in srcs])
    sc = (ctypes.c_float * C)(*scale) if scale is not None else None
    bi = (ctypes.c_float * C)(*bias) if bias is not None else None
    _check(
        _load().tcamd_layout_pack(
            arr, n, dtypes.code(src_dtype), LAYOUTS[src_layout], _vp(dst), dtypes.code(dst_dtype),
            LAYOUTS[dst_layout], C, H, W, sc, bi, 0 if rounding == "trunc" else 1, _vp(stream),
        ),
        "layout_pack",
    )


RESIZE_MAX_DIM = 16384  # csrc/kernels/resize.hip: the integer source coordinates fit 32 bits up to here


def resize_pack(srcs, sizes, dsts, dst_dtype, dst_layout, C, H, W, scale=None, bias=None, rounding="rne",
                stream=None, antialias=False):
    """K20: bilinear-resize (half-pixel centres, clamped, no antialiasing) the uint8
    HWC image at device pointer ``srcs[i]`` (any alignment) of ``sizes[i] = (h, w, c)``,
    c 1 or 3, to ``C x H x W`` outputs of ``dst_dtype`` (FP32 / FP16 / BF16) in
    ``dst_layout`` at its own device pointer ``dsts[i]``, with channel adapt
    (3->1 mean, 1->3 repeat) and per-channel ``x*scale[c]+bias[c]``:
    ``utils.image.preprocess`` on the device.  K20 reads 2x2 source pixels per
    output at any ratio; ``antialias=True`` runs K21 ``resize_pack_aa`` instead,
    the triangle filter widened by the downscale ratio
    (``utils.image.resize_area``; equal to the bilinear result on an upscaled
    axis), with the same arguments.  A dimension above
    :data:`RESIZE_MAX_DIM` or a channel count outside {1, 3} raises
    (hipErrorInvalidValue) without a launch."""
    n = len(srcs)
    if len(sizes) != n or len(dsts) != n:
        raise ValueError("resize_pack: srcs, sizes and dsts must have one entry per image")
    s = (ctypes.c_void_p * max(n, 1))(*[int(p) for p in srcs])
    d = (ctypes.c_void_p * max(n, 1))(*[int(p) for p in dsts])
    hs = (ctypes.c_int32 * max(n, 1))(*[int(z[0]) for z in sizes])
    ws = (ctypes.c_int32 * max(n, 1))(*[int(z[1]) for z in sizes])
    cs = (ctypes.c_int32 * max(n, 1))(*[int(z[2]) for z in sizes])
    sc = (ctypes.c_float * len(scale))(*scale) if scale is not None else None
    bi = (ctypes.c_float * len(bias))(*bias) if bias is not None else None
    if (sc is not None and len(scale) < C) or (bi is not None and len(bias) < C):
        raise ValueError("resize_pack: scale / bias need C entries")
    fn = _load().tcamd_resize_pack_aa if antialias else _load().tcamd_resize_pack
    _check(
        fn(
            s, hs, ws, cs, n, d, dtypes.code(dst_dtype), LAYOUTS[dst_layout], int(C), int(H), int(W), sc, bi,
            0 if rounding == "trunc" else 1, _vp(stream),
        ),
        "resize_pack",
    )


def jpeg_decode(srcs, infos, dsts, stream=None):
    """K22: the device half of a baseline JPEG decode.  ``srcs[i]`` is a device
    pointer, 16-byte aligned, to the coefficient buffer the host entropy decoder
    wrote for image i (``ops.host_codec.HostCodec.jpeg_entropy_decode``:
    quantisation tables, then int16 blocks); ``infos[i]`` is its parse, anything
    with ``h, w, ncomp, hs, vs`` (``host_codec.JpegInfo``); ``dsts[i]`` is a
    device pointer of any alignment that receives its ``h*w*ncomp`` uint8 HWC
    pixels, bitwise those of the host decode.  Images of mixed sizes and
    samplings share a launch, 64 at a time.  A dimension outside
    [1, :data:`RESIZE_MAX_DIM`], an unsupported component count or sampling or a
    misaligned source raises (hipErrorInvalidValue) without a launch.

    A parse with ``scale`` 2, 4 or 8 (``HostCodec.jpeg_parse(blob, scale)``:
    ``h x w`` the reduced size, ``ny`` / ``nx`` each component's transform size)
    asks for the reduced-size decode of the compact coefficient buffer of that
    scale.  One call takes images of mixed sizes, samplings and scales: the
    full-size images go through the full-size kernel in launches of their own,
    exactly as in a call without scaled images, and the images of scales 2, 4
    and 8 share launches of the scaled kernel, 64 at a time, which dispatches
    per image.  A scale outside {1, 2, 4, 8}, or an ``ny`` / ``nx`` that does
    not follow from the scale and the sampling, raises (hipErrorInvalidValue)
    without a launch."""
    n = len(srcs)
    if len(infos) != n or len(dsts) != n:
        raise ValueError("jpeg_decode: srcs, infos and dsts must have one entry per image")
    s = (ctypes.c_void_p * max(n, 1))(*[int(p) for p in srcs])
    d = (ctypes.c_void_p * max(n, 1))(*[int(p) for p in dsts])
    cols = [(ctypes.c_int32 * max(n, 1))(*[int(getattr(i, f)) for i in infos]) for f in ("h", "w", "ncomp", "hs", "vs")]
    scales = [int(getattr(i, "scale", 1)) for i in infos]
    if all(k == 1 for k in scales):
        _check(_load().tcamd_jpeg_decode(s, *cols, n, d, _vp(stream)), "jpeg_decode")
        return
    sc = (ctypes.c_int32 * n)(*scales)
    ny = (ctypes.c_int32 * (3 * n))(*[int(i.ny[c]) if k != 1 or hasattr(i, "ny") else 8 for i, k in zip(infos, scales)
                                      for c in range(3)])
    nx = (ctypes.c_int32 * (3 * n))(*[int(i.nx[c]) if k != 1 or hasattr(i, "nx") else 8 for i, k in zip(infos, scales)
                                      for c in range(3)])
    _check(_load().tcamd_jpeg_decode_scaled(s, *cols, sc, ny, nx, n, d, _vp(stream)), "jpeg_decode")


def jpeg_huffman(streams, coefs, status, stream=None):
    """K23: the Huffman stage of a baseline JPEG decode on the device.
    ``streams[i]`` is a device pointer, 16-byte aligned, to the stream buffer
    ``ops.host_codec.HostCodec.jpeg_stream_pack`` wrote for image i;
    ``coefs[i]`` is a device pointer, 16-byte aligned, to ``coef_bytes`` of its
    parse, which receive the buffer :func:`jpeg_decode` reads, byte for byte
    what ``jpeg_entropy_decode`` writes; ``status`` is a device pointer to one
    uint32 per image: 0, or the reason that image's coefficients are not to be
    used (invalid Huffman data; the host decoder then gives the error).  One
    workgroup per image, 64 images per launch.  A null or misaligned pointer
    raises (hipErrorInvalidValue) without a launch."""
    n = len(streams)
    if len(coefs) != n:
        raise ValueError("jpeg_huffman: streams and coefs must have one entry per image")
    s = (ctypes.c_void_p * max(n, 1))(*[int(p) for p in streams])
    c = (ctypes.c_void_p * max(n, 1))(*[int(p) for p in coefs])
    _check(_load().tcamd_jpeg_huffman(s, c, _vp(status), n, _vp(stream)), "jpeg_huffman")


JPEG_WIDE_CHUNK_SUBS = 1024  # the default chunk of jpeg_huffman_wide: one subsequence per thread


def jpeg_huffman_wide_workspace(nsubs, chunk_subs=0):
    """The bytes of device workspace a :func:`jpeg_huffman_wide` call over
    images of ``nsubs`` subsequences needs at ``chunk_subs``."""
    cs = int(chunk_subs) or JPEG_WIDE_CHUNK_SUBS
    return int(_load().tcamd_jpeg_huffman_wide_workspace(sum(int(n) for n in nsubs),
                                                         sum(-(-int(n) // cs) for n in nsubs)))


def jpeg_huffman_wide(streams, coefs, nsubs, status, workspace, workspace_bytes, chunk_subs=0, stream=None):
    """K24: the Huffman stage of a baseline JPEG decode across workgroups, for
    scans of up to 32 MiB and for any scale.  ``streams[i]`` is a device
    pointer, 16-byte aligned, to the stream buffer
    ``ops.host_codec.HostCodec.jpeg_stream_pack_wide`` wrote for image i at its
    scale, ``nsubs[i]`` the subsequence count the pack returned, ``coefs[i]`` a
    device pointer, 16-byte aligned, to ``coef_bytes`` of the parse at that
    scale, which receive the compact buffer :func:`jpeg_decode` reads, byte for
    byte what ``jpeg_entropy_decode(blob, out, scale)`` writes.  ``status`` is
    a device pointer to one uint32 per image: 0, or the reason that image's
    coefficients are not to be used.  ``workspace`` is a device pointer,
    16-byte aligned, to ``workspace_bytes`` of scratch memory, at least
    :func:`jpeg_huffman_wide_workspace` of the call.  ``chunk_subs`` (a power
    of two up to 1024; 0 = 1024) is the number of subsequences a workgroup
    handles.  A call is a sequence of launches on ``stream``, none of which
    waits for the host: ``5 + the largest chunk count of an image`` per 64
    images.  A null or misaligned pointer, a workspace too small, another
    ``chunk_subs`` or an ``nsubs[i]`` of 0 raises (hipErrorInvalidValue)
    without a launch."""
    n = len(streams)
    if len(coefs) != n or len(nsubs) != n:
        raise ValueError("jpeg_huffman_wide: streams, coefs and nsubs must have one entry per image")
    s = (ctypes.c_void_p * max(n, 1))(*[int(p) for p in streams])
    c = (ctypes.c_void_p * max(n, 1))(*[int(p) for p in coefs])
    k = (ctypes.c_uint32 * max(n, 1))(*[int(v) for v in nsubs])
    _check(_load().tcamd_jpeg_huffman_wide(s, c, k, _vp(status), _vp(workspace), int(workspace_bytes), n,
                                           int(chunk_subs), _vp(stream)), "jpeg_huffman_wide")


def png_unfilter_geometry():
    """The decomposition of K25 ``png_unfilter``, from the library:
    ``(rows per wave, rows per pass, units per column chunk)``, a unit being
    ``bpp`` bytes of a scanline."""
    g = (ctypes.c_int32 * 3)()
    _load().tcamd_png_unfilter_geometry(g)
    return int(g[0]), int(g[1]), int(g[2])


def png_unfilter(srcs, infos, dsts, stream=None):
    """K25: the device half of a PNG decode, unfilter and sample conversion.
    ``srcs[i]`` is a device pointer, 16-byte aligned, to ``stage_bytes`` of
    image i: the staged bytes ``ops.host_codec.HostCodec.png_inflate`` wrote
    (filtered scanlines, the palette of colour type 3) and, for an image of more
    rows than a pass, the scanline of scratch behind them, which the kernel
    writes; ``infos[i]`` is its parse, anything with ``h, w, ctype, depth,
    interlace`` (``host_codec.PngInfo``); ``dsts[i]`` is a device pointer of any
    alignment that receives its ``h * w * channels`` uint8 HWC pixels, bitwise
    those of ``HostCodec.png_unfilter``.  Images of mixed size, colour type and
    depth share a launch, one workgroup each, 64 per launch.  An interlaced
    parse, a side outside [1, :data:`RESIZE_MAX_DIM`], a colour type / depth
    pair PNG does not have, or a null or misaligned source raises
    (hipErrorInvalidValue) without a launch."""
    n = len(srcs)
    if len(infos) != n or len(dsts) != n:
        raise ValueError("png_unfilter: srcs, infos and dsts must have one entry per image")
    s = (ctypes.c_void_p * max(n, 1))(*[int(p) for p in srcs])
    d = (ctypes.c_void_p * max(n, 1))(*[int(p) for p in dsts])
    cols = [(ctypes.c_int32 * max(n, 1))(*[int(getattr(i, f)) for i in infos])
            for f in ("h", "w", "ctype", "depth", "interlace")]
    _check(_load().tcamd_png_unfilter(s, *cols, n, d, _vp(stream)), "png_unfilter")


COMPARE_MAX_PAIRS = dtypes.COMPARE_MAX_PAIRS
COMPARE_NO_INDEX = dtypes.COMPARE_NO_INDEX
COMPARE_RECORD_BYTES = ctypes.sizeof(dtypes.CompareRecord)


def compare_geometry():
    """The decomposition of K26 ``compare_expected``, from the library: ``(bytes
    of got a lane reads per step, bytes per workgroup, workgroups per pair at
    most)``."""
    g = (ctypes.c_uint64 * 3)()
    _load().tcamd_compare_geometry(g)
    return int(g[0]), int(g[1]), int(g[2])


def compare_expected(pairs, records, atol=0.0, rtol=0.0, stream=None):
    """K26: compare device-resident outputs with their expectations without
    copying either to the host.  ``pairs`` is up to :data:`COMPARE_MAX_PAIRS`
    tuples ``(got, expected, count, datatype)``: two device pointers at any
    element-aligned address (they need not be misaligned alike), the element
    count (0 is legal) and the datatype name; BYTES goes in as UINT8 over its
    serialized bytes.  ``records`` is a device pointer to ``len(pairs)`` records
    of :data:`COMPARE_RECORD_BYTES` (``dtypes.CompareRecord``), written in stream
    order: mismatches, lowest mismatching index (:data:`COMPARE_NO_INDEX` when
    none), largest ``|got - exp|`` over the finite pairs of a float type, and the
    bits of the two elements at that index.

    With ``atol == rtol == 0``, and always for the integer, BOOL and FP8 types,
    an element passes iff its bytes are identical.  Otherwise FP16 / BF16 / FP32
    (in fp32) and FP64 (in fp64) pass on equal bits, on two NaNs, or when both
    are finite and ``|got - exp| <= atol + rtol * |exp|``.  One launch when every
    pair fits a workgroup (``compare_geometry()[1]`` bytes), three otherwise.  A
    null or misaligned pointer, an unknown datatype or a negative or non-finite
    tolerance raises (hipErrorInvalidValue) without a launch."""
    tab = dtypes.compare_table(pairs)
    _check(_load().tcamd_compare_expected(tab, len(pairs), float(atol), float(rtol), _vp(records), _vp(stream)),
           "compare_expected")


def batched_copy(srcs, dsts, sizes, stream=None):
    """K7: copy sizes[i] bytes srcs[i] -> dsts[i] for all i in one launch."""
    n = len(srcs)
    if n == 0:
        return
    s = (ctypes.c_void_p * n)(*[int(p) for p in srcs])
    d = (ctypes.c_void_p * n)(*[int(p) for p in dsts])
    b = (ctypes.c_uint64 * n)(*[int(x) for x in sizes])
    _check(_load().tcamd_batched_copy(s, d, b, n, _vp(stream)), "batched_copy")


TOPK_KMAX = 64  # TCAMD_TOPK_KMAX (csrc/kernels/topk.hip)


def topk_rows(x_ptr, row_stride_bytes, rows, C, k_row_ptr, kmax, pairs_ptr, stream=None):
    """K19: the ``min(k_row[r], C)`` best entries of each fp32 row (``C`` values, rows
    ``row_stride_bytes`` apart) as ``{float32 score, int32 index}`` pairs at
    ``pairs[r][:kmax]``, ordered like ``np.argsort(-row, kind="stable")``.  ``k_row`` is a
    device int32 array, 0 skips the row; slots past a row's count are left untouched.
    ``kmax`` above :data:`TOPK_KMAX` raises (hipErrorInvalidValue) without a launch."""
    _check(_load().tcamd_topk_rows(_vp(x_ptr), int(row_stride_bytes), int(rows), int(C), _vp(k_row_ptr), int(kmax),
                                   _vp(pairs_ptr), _vp(stream)), "topk_rows")


QA_SPANS_KMAX = 64  # tcamd_qa::kKMax (csrc/kernels/qa_span_math.h)
QA_SPANS_MAX_SEQ = 1024  # tcamd_qa::kMaxSeq


def qa_spans(start_ptr, end_ptr, logit_stride_bytes, mask_ptr, token_type_ptr, ids_stride_bytes, rows, S, k_row_ptr,
             len_row_ptr, kmax, spans_ptr, scores_ptr, null_score_ptr, stream=None):
    """K27: the n best answer spans of each row of question-answering logits.
    ``start`` / ``end`` are device fp32 rows of ``S`` values ``logit_stride_bytes``
    apart, ``mask`` / ``token_type`` device int32 rows ``ids_stride_bytes`` apart;
    ``k_row`` and ``len_row`` are device int32 arrays, the answers wanted of each
    row and its longest answer in tokens.  A candidate is a pair ``s <= e`` with
    ``e - s < len_row[r]`` of tokens with ``mask >= 1`` and ``token_type == 1``;
    its score is ``start[s] + end[e]``; candidates order like K19 with the index
    ``s * S + e`` (csrc/kernels/qa_span_math.h).  Row ``r`` gets its first
    ``min(k_row[r], kmax)`` ranks as int32 ``spans[r][:kmax][2]`` and fp32
    ``scores[r][:kmax]``, ranks past its candidates as ``(-1, -1)`` and
    ``-FLT_MAX``, and ``null_score[r] = start[0] + end[0]``; ``k_row[r] < 1``
    skips the row and slots past a row's count are left untouched.  ``S`` outside
    1..:data:`QA_SPANS_MAX_SEQ`, ``kmax`` outside 1..:data:`QA_SPANS_KMAX`, a null
    or misaligned pointer, a stride that is no multiple of 4 or shorter than a
    row, or negative ``rows`` raises (hipErrorInvalidValue) without a launch."""
    _check(_load().tcamd_qa_spans(_vp(start_ptr), _vp(end_ptr), int(logit_stride_bytes), _vp(mask_ptr),
                                  _vp(token_type_ptr), int(ids_stride_bytes), int(rows), int(S), _vp(k_row_ptr),
                                  _vp(len_row_ptr), int(kmax), _vp(spans_ptr), _vp(scores_ptr), _vp(null_score_ptr),
                                  _vp(stream)), "qa_spans")


def qa_spans_masked(start_ptr, end_ptr, logit_stride_bytes, mask_ptr, token_type_ptr, start_ok_ptr, ids_stride_bytes,
                    rows, S, k_row_ptr, len_row_ptr, kmax, spans_ptr, scores_ptr, null_score_ptr, stream=None):
    """K27 with a start mask: :func:`qa_spans`, and a span may start only at a
    token with ``start_ok >= 1`` (device int32 rows ``ids_stride_bytes`` apart,
    the ``start_mask`` of :func:`wordpiece_windows`); its end needs eligibility
    only."""
    _check(_load().tcamd_qa_spans_masked(_vp(start_ptr), _vp(end_ptr), int(logit_stride_bytes), _vp(mask_ptr),
                                         _vp(token_type_ptr), _vp(start_ok_ptr), int(ids_stride_bytes), int(rows),
                                         int(S), _vp(k_row_ptr), _vp(len_row_ptr), int(kmax), _vp(spans_ptr),
                                         _vp(scores_ptr), _vp(null_score_ptr), _vp(stream)), "qa_spans_masked")


QA_MERGE_MAX_ROWS = 128  # tcamd_qa::kMergeMaxRows: the windows of one document


def qa_merge(spans_ptr, scores_ptr, null_score_ptr, rows, window_info_ptr, doc_info_ptr, docs, k_doc_ptr, kmax,
             out_spans_ptr, out_windows_ptr, out_scores_ptr, out_null_ptr, stream=None):
    """K29: the n best spans of each document from the n best of its windows
    (csrc/kernels/qa_span_math.h).  ``spans`` ``[rows, kmax, 2]``, ``scores``
    ``[rows, kmax]`` and ``null_score`` ``[rows]`` are what
    :func:`qa_spans_masked` left with ``k_row`` = the document's ``k``;
    ``window_info`` ``[rows, 4]`` and ``doc_info`` ``[docs, 4]`` what
    :func:`wordpiece_windows` left; ``k_doc`` device int32 ``[docs]``.  Document
    ``d`` gets int32 ``out_spans[d][:kmax][2]`` (tokens of the window's row),
    ``out_windows[d][:kmax]`` (the row), fp32 ``out_scores[d][:kmax]`` and
    ``out_null[d]`` (the lowest null score of its rows); ranks past the
    candidates hold ``(-1, -1)``, ``-1`` and ``-FLT_MAX``.  One launch."""
    _check(_load().tcamd_qa_merge(_vp(spans_ptr), _vp(scores_ptr), _vp(null_score_ptr), int(rows),
                                  _vp(window_info_ptr), _vp(doc_info_ptr), int(docs), _vp(k_doc_ptr), int(kmax),
                                  _vp(out_spans_ptr), _vp(out_windows_ptr), _vp(out_scores_ptr), _vp(out_null_ptr),
                                  _vp(stream)), "qa_merge")


WORDPIECE_GEOMETRY = ("chunk", "block", "max_text_bytes", "max_word_chars", "max_rows", "max_chunks")


def wordpiece_geometry():
    """The decomposition of K28 ``wordpiece_tokenize``, from the library, as a
    dict: ``chunk`` (the bytes, and then the folded positions, of a text one
    workgroup owns), ``block`` (threads of a workgroup; a thread takes ``chunk
    / block`` consecutive bytes), ``max_text_bytes``, ``max_word_chars``,
    ``max_rows`` per call and ``max_chunks`` per text."""
    g = (ctypes.c_int32 * 6)()
    _load().tcamd_wordpiece_geometry(g)
    return dict(zip(WORDPIECE_GEOMETRY, (int(x) for x in g)))


def wordpiece_workspace(rows, text_bytes):
    """Bytes of device workspace :func:`wordpiece_tokenize` needs for ``rows``
    rows whose texts have ``text_bytes`` bytes in all."""
    return int(_load().tcamd_wordpiece_workspace(int(rows), int(text_bytes)))


def wordpiece_tokenize(text_ptr, text_bytes, row_table_ptr, maxq_row_ptr, rows, S, vocab_ptr, vocab_words,
                       workspace_ptr, workspace_bytes, ids_ptr, mask_ptr, type_ids_ptr, offsets_ptr, overflow_ptr,
                       status_ptr, stream=None):
    """K28: UTF-8 questions and contexts to BERT question-answering rows, by the
    rule of csrc/kernels/wordpiece_core.h.  ``text`` is a device buffer of
    ``text_bytes`` bytes holding every text, ``row_table`` device uint32
    ``[rows, 4]`` = ``{question_off, question_len, context_off, context_len}``
    into it (``utils.wordpiece.pack_texts``), ``maxq_row`` device int32
    ``[rows]``, ``vocab`` the device copy of ``utils.wordpiece.Vocab.image``
    (``vocab_words`` 32-bit words), ``workspace`` at least
    :func:`wordpiece_workspace` bytes.  Row ``r`` gets int32 ``ids`` / ``mask``
    / ``type_ids`` ``[S]``, ``offsets`` ``[S, 2]`` (byte offsets into its
    context, on the context pieces), ``overflow`` and a uint32 ``status`` (0, or
    why the row is all zeros: ``utils.wordpiece.status_error``).  At most
    ``wordpiece_geometry()["max_rows"]`` rows, ``S`` in 4..1024; those, a null
    or misaligned pointer or a workspace below its fixed part raise
    (hipErrorInvalidValue) without a launch.  Ten launches on ``stream``,
    nothing on the host."""
    _check(_load().tcamd_wordpiece_tokenize(_vp(text_ptr), int(text_bytes), _vp(row_table_ptr), _vp(maxq_row_ptr),
                                            int(rows), int(S), _vp(vocab_ptr), int(vocab_words), _vp(workspace_ptr),
                                            int(workspace_bytes), _vp(ids_ptr), _vp(mask_ptr), _vp(type_ids_ptr),
                                            _vp(offsets_ptr), _vp(overflow_ptr), _vp(status_ptr), _vp(stream)),
           "wordpiece_tokenize")


WORDPIECE_MAX_WINDOWS = 128  # tcamd_wp::kMaxWindows: per document, and rows per windowed call


def wordpiece_windows_workspace(docs, text_bytes):
    """Bytes of device workspace :func:`wordpiece_windows` needs for ``docs``
    documents whose texts have ``text_bytes`` bytes in all (what
    :func:`wordpiece_workspace` says: the windows need none of their own)."""
    return int(_load().tcamd_wordpiece_windows_workspace(int(docs), int(text_bytes)))


def wordpiece_windows(text_ptr, text_bytes, row_table_ptr, maxq_row_ptr, stride_row_ptr, maxw_row_ptr, docs, S,
                      vocab_ptr, vocab_words, workspace_ptr, workspace_bytes, out_rows, ids_ptr, mask_ptr, type_ids_ptr,
                      start_mask_ptr, offsets_ptr, window_info_ptr, doc_info_ptr, n_rows_ptr, stream=None):
    """K28w: :func:`wordpiece_tokenize` over doc-stride windows (rule 8 of
    csrc/kernels/wordpiece_core.h).  A row of ``row_table`` is a document;
    ``stride_row`` / ``maxw_row`` are device int32 ``[docs]`` (``doc_stride`` in
    1..S-3, ``max_windows`` in 1..128), ``out_rows`` <= 128 the row capacity of
    the outputs: int32 ``ids`` / ``mask`` / ``type_ids`` / ``start_mask``
    ``[out_rows, S]``, ``offsets`` ``[out_rows, S, 2]``, ``window_info``
    ``[out_rows, 4]`` = ``{document, first context piece, context pieces, token
    of the first context piece}``, uint32 ``doc_info`` ``[docs, 4]`` = ``{first
    row, windows, context pieces, status}`` and int32 ``n_rows`` ``[1]``; rows
    from ``n_rows`` on are zero.  Eleven launches on ``stream`` (K28's ten, the
    clear among them, and one more), nothing on the host."""
    _check(_load().tcamd_wordpiece_windows(_vp(text_ptr), int(text_bytes), _vp(row_table_ptr), _vp(maxq_row_ptr),
                                           _vp(stride_row_ptr), _vp(maxw_row_ptr), int(docs), int(S), _vp(vocab_ptr),
                                           int(vocab_words), _vp(workspace_ptr), int(workspace_bytes), int(out_rows),
                                           _vp(ids_ptr), _vp(mask_ptr), _vp(type_ids_ptr), _vp(start_mask_ptr),
                                           _vp(offsets_ptr), _vp(window_info_ptr), _vp(doc_info_ptr), _vp(n_rows_ptr),
                                           _vp(stream)), "wordpiece_windows")


def dn_conv1x1(x, ldx, M, K, in_scale, in_bias, w, N, out_bias, relu_out, y, ldy, pool=0, H=0, W=0, stream=None,
               variant=0, splits=0, ws=None, ws_bytes=0):
    """K8: y[m, :N] = epi(relu(x[m, :K]*s + b) @ w[N, K]^T); pool=1 fuses a 2x2 avg-pool (transition).
    variant: 0 = heuristic, else 10*TM + BK/32 (tile-size override for benchmarking).
    splits: split-K factor (0 = heuristic when a fp32 workspace ``ws`` of ``ws_bytes`` is given)."""
    _check(_load().tcamd_dn_conv1x1_ex(x, ldx, M, K, in_scale, in_bias, w, N, out_bias, int(relu_out), y, ldy,
                                       int(pool), H, W, int(variant), int(splits), ws, int(ws_bytes), _vp(stream)),
           "dn_conv1x1")


def dn_conv3x3(z, imgs, H, W, w, y, ldy, stream=None, variant=0):
    """K9: 3x3/pad-1 conv 128->32 over NHWC rows z; 32 channels per pixel written at y + pixel*ldy.
    variant: 0 = heuristic, else 10*TM + taps-per-load-group."""
    _check(_load().tcamd_dn_conv3x3_v(z, imgs, H, W, w, y, ldy, int(variant), _vp(stream)), "dn_conv3x3")


def dn_stem_pool(x, bias, y, imgs, H, W, C, ldy, stream=None):
    """K10a: y = relu(maxpool3x3/2(x) + bias) into rows of ldy elements."""
    _check(_load().tcamd_dn_stem_pool(x, bias, y, imgs, H, W, C, ldy, _vp(stream)), "dn_stem_pool")


def dn_stem_fused(srcs, x, w, bias, y, imgs, ldy, stream=None):
    """K10s: y = relu(maxpool3x3/2(conv7x7/2(img)) + bias) for 224x224x3 images -> 56x56x64.
    ``srcs``: device array of per-image fp32 NCHW pointers (or None with ``x`` = bf16 NHWC batch);
    ``w``: [64][7][8][4] bf16 packed weights."""
    _check(_load().tcamd_dn_stem_fused(_vp(srcs), _vp(x), w, bias, y, imgs, ldy, _vp(stream)), "dn_stem_fused")


def add_layernorm(x, y, gamma, beta, out, rows, H, eps, stream=None):
    """K11: out = LayerNorm(x + y) * gamma + beta over ``rows`` rows of H bf16 (H in 512/1024/2048/4096)."""
    _check(_load().tcamd_add_layernorm(x, y, gamma, beta, out, rows, H, float(eps), _vp(stream)), "add_layernorm")


ATTENTION_MAX_SEQ = 384


def embed_layernorm(ids, types, word, pos, type_, gamma, beta, out, rows, S, H, vocab, ntypes, eps, stream=None):
    """BERT embeddings in one launch: out [rows][H] bf16 = LayerNorm(word[ids] +
    pos[row % S] + type[types]) * gamma + beta; ids / types int64 [rows]."""
    _check(_load().tcamd_embed_layernorm(_vp(ids), _vp(types), word, pos, type_, gamma, beta, out, int(rows), int(S),
                                         int(H), int(vocab), int(ntypes), float(eps), _vp(stream)), "embed_layernorm")


def attention(qkv, mask, out, seqs, S, heads, scale, stream=None, bias=None):
    """K12: multi-head attention (head dim 64, non-causal) over the fused QKV
    projection's output ``qkv`` [seqs*S][3*heads*64] bf16 into ``out``
    [seqs*S][heads*64] bf16; ``mask`` int32 [seqs][S] key-padding mask (0 =
    padded key) or None.  S % 64 == 0 and S <= ATTENTION_MAX_SEQ.  ``bias``
    (bf16 [3*heads*64] or None): the projection's bias, when ``qkv`` was
    computed without it (q + b_q feeds the scores, b_v is added to the output;
    b_k shifts every score of a query equally and cancels in the softmax)."""
    _check(_load().tcamd_attention_bias(qkv, _vp(bias), _vp(mask), out, int(seqs), int(S), int(heads), float(scale),
                                        _vp(stream)), "attention")


def attention_f32(qkv, mask, out, seqs, S, heads, scale, stream=None, x3=False):
    """K12x: fp32-parity attention (bf16x3 products, fp32 online softmax) over
    the fp32 QKV projection ``qkv`` [seqs*S][3*heads*64] (bias included) into
    ``out`` [seqs*S][heads*64] fp32 -- or, with ``x3``, into the out
    projection's bf16x3 operand, bf16 [seqs*S][3*heads*64] = [hi | hi | lo];
    ``mask`` int32 [seqs][S] (0 = padded key, additive -10000 as the
    reference) or None.  S % 64 == 0."""
    _check(_load().tcamd_attention_f32(qkv, _vp(mask), out, int(seqs), int(S), int(heads), float(scale),
                                       1 if x3 else 0, _vp(stream)), "attention_f32")


def attention_plan(seqs, S, heads):
    """(splits, waves) of K12's launch for this shape: blocks per (sequence,
    head) and waves of 32 queries per block.  Host only, no launch."""
    sp, w = ctypes.c_int(0), ctypes.c_int(0)
    _check(_load().tcamd_attention_plan(int(seqs), int(S), int(heads), ctypes.byref(sp), ctypes.byref(w)),
           "attention_plan")
    return sp.value, w.value


def attention_f32_plan(seqs, S, heads):
    """Waves per block (4 or 8, 16 queries each) of K12x's launch for this shape.  Host only, no launch."""
    w = ctypes.c_int(0)
    _check(_load().tcamd_attention_f32_plan(int(seqs), int(S), int(heads), ctypes.byref(w)), "attention_f32_plan")
    return w.value


# The logit a packed bert_large forward leaves where attention_mask < 1: the
# model's own additive mask constant (tcamd_bert_pad_logit, csrc/kernels/bert_pack.hip).
BERT_PAD_LOGIT = -10000.0
BERT_PACK_MAX_ROWS = 128


def bert_pack_plan(mask, mask_stride, rows, S, t_cap, row_len, cu, tok_src, tok_of, stream=None):
    """K30: the pack plan of a padding-free BERT forward.  ``mask`` int32
    [rows][S] at a row stride of ``mask_stride`` elements (any mask; valid =
    mask >= 1), rows <= 128, S <= 384 -> int32 device arrays ``row_len`` [rows],
    ``cu`` [rows + 1] (exclusive scan, cu[rows] = T), ``tok_src`` [t_cap]
    (r * S + p of packed token t, rows in order and positions ascending; -1 for
    T <= t < t_cap) and ``tok_of`` [rows * S] (the packed token of (r, p), or
    -1).  With T > t_cap nothing past t_cap is written and cu[rows] still holds
    the true T: the caller checks it."""
    _check(_load().tcamd_bert_pack_plan(mask, int(mask_stride), int(rows), int(S), int(t_cap), row_len, cu, tok_src,
                                        tok_of, _vp(stream)), "bert_pack_plan")


def embed_layernorm_packed(ids, types, tok_src, word, pos, type_, gamma, beta, out, t_cap, n_src, S, H, vocab, ntypes,
                           eps, stream=None, f32=False, out3=None):
    """BERT embeddings of the packed tokens: out [t_cap][H] bf16, token t from
    the int32 request tensors ``ids`` / ``types`` [n_src] at ``tok_src[t]``
    (ids wrap by remainder(vocab), types clamp to [0, ntypes - 1], position =
    src % S); a pad token (tok_src = -1) is id 0, position 0, type 0.  A real
    token has the bits ``embed_layernorm`` gives its (row, position).
    ``f32`` (the fp32-parity model): tables, gamma, beta and ``out`` are fp32,
    the fp32 sum goes through a two-pass fp32 LayerNorm; ``out3`` (or None) is
    then also written as the next bf16x3 GEMM's operand, bf16 [t_cap][3H] =
    [hi | hi | lo], bitwise ``x3_cat`` of ``out``."""
    if f32:
        _check(_load().tcamd_embed_layernorm_packed_f32(ids, types, tok_src, word, pos, type_, gamma, beta, out,
                                                        _vp(out3), int(t_cap), int(n_src), int(S), int(H), int(vocab),
                                                        int(ntypes), float(eps), _vp(stream)),
               "embed_layernorm_packed(f32)")
        return
    if out3 is not None:
        raise ValueError("embed_layernorm_packed: out3 needs f32=True")
    _check(_load().tcamd_embed_layernorm_packed(ids, types, tok_src, word, pos, type_, gamma, beta, out, int(t_cap),
                                                int(n_src), int(S), int(H), int(vocab), int(ntypes), float(eps),
                                                _vp(stream)), "embed_layernorm_packed")


def unpack_logits(packed_start, packed_end, tok_of, out_start, out_end, n, t_cap, stream=None):
    """out_start / out_end fp32 [n] (n = rows * S): the packed logits of the
    tokens ``tok_of`` names, BERT_PAD_LOGIT elsewhere, both planes in one launch."""
    _check(_load().tcamd_unpack_logits(packed_start, packed_end, tok_of, out_start, out_end, int(n), int(t_cap),
                                       _vp(stream)), "unpack_logits")


def attention_packed(qkv, row_len, cu, out, rows, t_cap, heads, scale, stream=None, bias=None):
    """K12v: K12 over packed rows.  ``qkv`` [t_cap][3*heads*64] bf16 holds row
    r's tokens at cu[r] .. cu[r] + row_len[r] - 1 (int32 device arrays from
    ``bert_pack_plan``; row_len <= ATTENTION_MAX_SEQ); ``out`` [t_cap][heads*64]
    bf16, of which only the rows' own tokens are written.  ``bias`` as K12's."""
    _check(_load().tcamd_attention_packed(qkv, _vp(bias), row_len, cu, out, int(rows), int(t_cap), int(heads),
                                          float(scale), _vp(stream)), "attention_packed")


def attention_packed_plan(rows, heads):
    """(splits, waves) of K12v's launch, fixed per (rows, heads): K12's plan at S = 384.  Host only."""
    sp, w = ctypes.c_int(0), ctypes.c_int(0)
    _check(_load().tcamd_attention_packed_plan(int(rows), int(heads), ctypes.byref(sp), ctypes.byref(w)),
           "attention_packed_plan")
    return sp.value, w.value


def attention_f32_packed(qkv, row_len, cu, out, rows, t_cap, heads, scale, stream=None, x3=False):
    """K12xv: K12x over packed rows.  ``qkv`` [t_cap][3*heads*64] fp32 (bias
    included) holds row r's tokens at cu[r] .. cu[r] + row_len[r] - 1 (int32
    device arrays from ``bert_pack_plan``; row_len <= ATTENTION_MAX_SEQ, rows
    <= BERT_PACK_MAX_ROWS); ``out`` [t_cap][heads*64] fp32 or, with ``x3``, the
    out projection's bf16x3 operand, bf16 [t_cap][3*heads*64].  Only the rows'
    own tokens are read and written; a valid token gets the bits K12x gives it
    in the row padded to 384 behind a prefix mask."""
    _check(_load().tcamd_attention_f32_packed(qkv, row_len, cu, out, int(rows), int(t_cap), int(heads), float(scale),
                                              1 if x3 else 0, _vp(stream)), "attention_f32_packed")


def attention_f32_packed_plan(rows, heads):
    """Waves per block (4 or 8) of K12xv's launch, fixed per (rows, heads): K12x's plan at S = 384.  Host only."""
    w = ctypes.c_int(0)
    _check(_load().tcamd_attention_f32_packed_plan(int(rows), int(heads), ctypes.byref(w)), "attention_f32_packed_plan")
    return w.value


def x3_conv1x1_ws_bytes(M, K, N=128):
    """Split-K workspace bytes K8x wants for an M x K -> N 1x1 conv (0: none)."""
    return int(_load().tcamd_x3_conv1x1_ws_bytes(int(M), int(K), int(N)))


def x3_conv1x1(x, ldx, M, K, in_scale, in_bias, w_hi, w_lo, out_bias=None, z_hi=None, z_lo=None, y=None, ldy=0,
               pool=0, H=0, W=0, ws=None, ws_bytes=0, stream=None, N=128):
    """K8x fp32-parity 1x1 conv (N out channels, a multiple of 128): z_hi/z_lo
    split bf16 planes with bias+ReLU (N = 128), or raw fp32 into ``y`` rows of ``ldy``."""
    _check(_load().tcamd_x3_conv1x1(x, ldx, M, K, int(N), in_scale, in_bias, w_hi, w_lo, _vp(out_bias), _vp(z_hi),
                                    _vp(z_lo), _vp(y), int(ldy), int(pool), int(H), int(W), _vp(ws),
                                    int(ws_bytes), _vp(stream)), "x3_conv1x1")


def x3_w3_fragments(w):
    """K9x weight layout: a [32][9*128] (out, tap-major K) tensor -> the MFMA
    fragment-major copy the kernel loads, [tap 9][kq 4][kc 2][h 2][col 32][8]
    (one wave's 16-B-per-lane fragment = 1 KB contiguous).  Apply it to the
    hi and lo planes alike."""
    return w.reshape(32, 9, 4, 2, 2, 8).permute(1, 2, 3, 4, 0, 5).contiguous().reshape(32, 9 * 128)


def x3_conv3x3(z_hi, z_lo, imgs, H, W, w_hi, w_lo, y, ldy, stream=None):
    """K9x fp32-parity 3x3 conv 128 -> 32 into fp32 rows of ``ldy``; ``w_hi`` /
    ``w_lo`` in the x3_w3_fragments layout."""
    _check(_load().tcamd_x3_conv3x3(z_hi, z_lo, imgs, H, W, w_hi, w_lo, y, ldy, _vp(stream)), "x3_conv3x3")


def x3_dense_layer(x, ldx, imgs, H, W, K, s1, t1, w1_hi, w1_lo, b1, z_hi, z_lo, w2_hi, w2_lo, y, ldy, ws=None,
                   ws_bytes=0, stream=None):
    """One fp32-parity dense layer: K8x BN1+ReLU+1x1 (K -> 128, BN2 folded, bias
    ``b1``) then K9x 3x3 (128 -> 32) into ``y`` rows of ``ldy`` (the layer's
    slice).  A split-K 1x1 hands its partials to the 3x3, which reduces them
    while staging its band (no reduce launch)."""
    _check(_load().tcamd_x3_dense_layer(x, int(ldx), int(imgs), int(H), int(W), int(K), s1, t1, w1_hi, w1_lo, b1,
                                        z_hi, z_lo, w2_hi, w2_lo, y, int(ldy), _vp(ws), int(ws_bytes), _vp(stream)),
           "x3_dense_layer")


def x3s_dense_layer(x, ldx, imgs, H, W, K, s1, t1, w1_hi, w1_lo, b1, zacc, zacc_next, w2_hi, w2_lo, y, ldy,
                    stream=None):
    """K13x small-M dense layer (csrc/kernels/densenet_x3s.hip): the 1x1 adds
    into ``zacc`` ([M][128] fp32, ZERO on entry) with float atomics over many
    workgroups, then the 3x3 reads it (bias ``b1`` + ReLU + split in registers)
    into ``y`` rows of ``ldy``, zeroing rows [0, M) of ``zacc_next`` (may be
    None) for the next layer.  ``w1_*`` in x3_w1_fragments, ``w2_*`` in
    x3_w3_fragments."""
    _check(_load().tcamd_x3s_dense_layer(x, int(ldx), int(imgs), int(H), int(W), int(K), s1, t1, w1_hi, w1_lo, b1,
                                         zacc, _vp(zacc_next), w2_hi, w2_lo, y, int(ldy), _vp(stream)),
           "x3s_dense_layer")


X3C_LAYER_WORDS = 9  # int64 words of one X3cLayer table entry


def x3c_layer_entry(w1_hi, w1_lo, s1, t1, b1, w2_hi, w2_lo, zacc, K):
    """One K13x chain table entry (9 int64: 8 device pointers + K); ``w1_*`` in
    x3_w1_fragments, ``w2_*`` in x3_w3_fragments, ``zacc`` [>= M][128] fp32."""
    return [int(w1_hi), int(w1_lo), int(s1), int(t1), int(b1), int(w2_hi), int(w2_lo), int(zacc), int(K)]


def x3c_base(layers, n, x, ldx, imgs, H, W, stream=None):
    """K13x chain, once per run of ``n`` small-M layers: every layer's 1x1 over
    the run's first K_f input channels (plain stores into its zacc) and every
    layer's y slice zeroed.  ``layers``: device table of chain entries."""
    _check(_load().tcamd_x3c_base(_vp(layers), int(n), _vp(x), int(ldx), int(imgs), int(H), int(W), _vp(stream)),
           "x3c_base")


def x3c_layer(layers, l, n, x, ldx, imgs, H, W, stream=None):
    """K13x chain, layer ``l`` of the run (one launch): its 3x3 (plus the
    previous layer's chunk of its 1x1, computed for the tile and halo) and the
    previous layer's chunk fanned out to every later layer's zacc."""
    _check(_load().tcamd_x3c_layer(_vp(layers), int(l), int(n), _vp(x), int(ldx), int(imgs), int(H), int(W),
                                   _vp(stream)), "x3c_layer")


def x3s_steps_per_block(M, K):
    """k16 steps per workgroup the K13x 1x1 plans for an M x K layer."""
    return int(_load().tcamd_x3s_steps_per_block(int(M), int(K)))


def x3_w1_fragments(w):
    """K11x 1x1 weight layout: [128][K] (out, in) -> the 32x32x16 MFMA
    fragment-major copy the fused layer reads from L2, [K/16][q 4][h 2][col 32][8]
    (lane (h, col) = w[32q + col][16ks + 8h .. +8]; one wave load = 1 KB)."""
    n, k = w.shape
    return w.reshape(4, 32, k // 16, 2, 8).permute(2, 0, 3, 1, 4).contiguous().reshape(n, k)


def x3_w3f_fragments(w):
    """K11x 3x3 weight layout: [32][9*128] (out, tap-major K) -> the 16x16x32
    MFMA fragment-major copy, [tap 9][kq 4][oh 2][h 4][col 16][8] (lane
    (h, col) = w[16oh + col][t][32kq + 8h .. +8])."""
    return w.reshape(2, 16, 9, 4, 4, 8).permute(2, 3, 0, 4, 1, 5).contiguous().reshape(32, 9 * 128)


def _x3_dense_fused(name, x, ldx, imgs, H, W, K, s1, t1, w1_hi, w1_lo, b1, w2_hi, w2_lo, y, ldy, stream):
    """The K11x entry point ``tcamd_<name>``: every version takes the same arguments."""
    _check(getattr(_load(), "tcamd_" + name)(x, int(ldx), int(imgs), int(H), int(W), int(K), s1, t1, w1_hi, w1_lo, b1,
                                             w2_hi, w2_lo, y, int(ldy), _vp(stream)), name)


def x3_dense_fused(x, ldx, imgs, H, W, K, s1, t1, w1_hi, w1_lo, b1, w2_hi, w2_lo, y, ldy, stream=None):
    """K11x: one fp32-parity dense layer in ONE kernel, the 128-channel
    bottleneck kept in LDS (never written to HBM).  ``w1_*`` in the
    x3_w1_fragments layout, ``w2_*`` in x3_w3f_fragments; 16 <= W <= 56, K a multiple
    of 32 in 64..224."""
    _x3_dense_fused("x3_dense_fused", x, ldx, imgs, H, W, K, s1, t1, w1_hi, w1_lo, b1, w2_hi, w2_lo, y, ldy, stream)


def x3_dense_small(x, ldx, imgs, H, W, K, s1, t1, w1f_hi, w1f_lo, b1, w2_hi, w2_lo, y, ldy, stream=None, tiles=0):
    """K14x: one fp32-parity dense layer of the 14x14 or 7x7 block in ONE
    kernel, ``tiles`` row tiles per image (each with the halo rows its 3x3
    needs, recomputed; 14x14: 2, 4 or 7, 7x7: 1, 2, 4 or 7; 0 = the fewest that give
    every CU a workgroup, :func:`x3_small_tiles`), z kept in a zero-padded LDS
    image of the tile.  ``w1f_*`` in x3_w1_fragments, ``w2_*`` in
    x3_w3f_fragments; K a multiple of 32 in 64..2048."""
    _check(_load().tcamd_x3_dense_small(x, int(ldx), int(imgs), int(H), int(W), int(K), s1, t1, w1f_hi, w1f_lo, b1,
                                        w2_hi, w2_lo, y, int(ldy), int(tiles), _vp(stream)), "x3_dense_small")


def x3_dense_small_pair(x, ldx, imgs, H, W, K, layer1, layer2, y, ldy, stream=None, tiles=0):
    """K14x pair: dense layers j and j+1 of a 14x14 block (``K`` and ``K + 32``
    input channels) in ONE kernel on one read of ``x[:, :K]``.  ``layer1`` /
    ``layer2``: each layer's ``(s1, t1, w1f_hi, w1f_lo, b1, w2_hi, w2_lo)``
    pointers as :func:`x3_dense_small` takes them.  ``y`` is layer j's 32-channel
    slice; layer j+1's follows it (``ldx >= K + 64``).  Only the (W, tiles)
    of :func:`x3_dense_small_pair_supported`; anything else is an error."""
    _check(_load().tcamd_x3_dense_small_pair(x, int(ldx), int(imgs), int(H), int(W), int(K), *layer1, *layer2, y,
                                             int(ldy), int(tiles), _vp(stream)), "x3_dense_small_pair")


def x3_dense_small_pair_supported(W, tiles):
    """Whether the K14x pair kernel is built for ``tiles`` row tiles of a ``W`` x ``W`` image."""
    return bool(_load().tcamd_x3_dense_small_pair_supported(int(W), int(tiles)))


def x3_small_tiles(imgs, W):
    """The tiles per image K14x picks for ``imgs`` images of side ``W``."""
    return int(_load().tcamd_x3_small_tiles(int(imgs), int(W)))


def x3_small_tiles_shared(imgs, W, streams):
    """:func:`x3_small_tiles` for one of ``streams`` concurrent streams: whole
    7x7 images (1 tile) once this stream's images alone fill its share of the
    CUs; on one stream, below that, and at 14x14 the same answer."""
    return int(_load().tcamd_x3_small_tiles_shared(int(imgs), int(W), int(streams)))


def x3_dense_fused3(x, ldx, imgs, H, W, K, s1, t1, w1_hi, w1_lo, b1, w2_hi, w2_lo, y, ldy, stream=None):
    """K11x v3: v1's roles and fragment layouts (``w2_*`` in x3_w3f_fragments),
    with the next chunk's 1x1 K steps interleaved into each tile's 3x3."""
    _x3_dense_fused("x3_dense_fused3", x, ldx, imgs, H, W, K, s1, t1, w1_hi, w1_lo, b1, w2_hi, w2_lo, y, ldy, stream)


def x3_cat(x, out, rows, K, stream=None):
    """fp32-parity bert operand: x fp32 [rows][K] -> out bf16 [rows][3K] =
    [hi | hi | lo] (csrc/kernels/bert.hip), for one bf16 GEMM against
    [W_hi | W_lo | W_hi] that accumulates the three split products."""
    _check(_load().tcamd_x3_cat(x, out, int(rows), int(K), _vp(stream)), "x3_cat")


def x3_stem_fragments(w):
    """K10x weight layout: [64][224] (out, (kh, kw[8], ch[4])) -> the MFMA
    fragment-major copy the stem loads, [half 2][k-step 14][h 2][col 32][8]."""
    return w.reshape(2, 32, 14, 2, 8).permute(0, 2, 3, 1, 4).contiguous().reshape(64, 224)


def x3_stem(srcs, w_hi, w_lo, bias, y, imgs, ldy, stream=None):
    """K10x fp32 stem from a device table of fp32 NCHW image pointers;
    ``w_hi`` / ``w_lo`` in the x3_stem_fragments layout."""
    _check(_load().tcamd_x3_stem(srcs, w_hi, w_lo, bias, y, imgs, ldy, _vp(stream)), "x3_stem")


def x3_head_pool(x, scale, bias, out, imgs, HW, C, stream=None):
    """K10x head: out[i, c] = mean_p relu(x[i, p, c]*scale[c] + bias[c]), fp32."""
    _check(_load().tcamd_x3_head_pool(x, scale, bias, out, imgs, HW, C, _vp(stream)), "x3_head_pool")


def x3_split(w, hi, lo, n, stream=None):
    """fp32 -> (bf16 hi, bf16 lo) planes on the device: w ~= hi + lo to 2^-17."""
    _check(_load().tcamd_x3_split(w, hi, lo, int(n), _vp(stream)), "x3_split")


def dn_head_pool(x, scale, bias, out, imgs, HW, C, stream=None):
    """K10b: out[i, c] = mean_p relu(x[i, p, c]*scale[c] + bias[c])."""
    _check(_load().tcamd_dn_head_pool(x, scale, bias, out, imgs, HW, C, _vp(stream)), "dn_head_pool")


def pack_bytes_workspace(n):
    return int(_load().tcamd_pack_bytes_workspace(n))


def pack_bytes(data_ptr, lens_ptr, n, out_ptr, workspace_ptr, stream=None):
    """K2: device BYTES serialisation (see csrc/kernels/bytes.hip)."""
    _check(
        _load().tcamd_pack_bytes(_vp(data_ptr), _vp(lens_ptr), n, _vp(out_ptr), _vp(workspace_ptr), _vp(stream)),
        "pack_bytes",
    )


def pack_bytes_strided(data_ptr, stride, lens_ptr, n, out_ptr, workspace_ptr, stream=None):
    """K2 over a fixed-width payload (numpy 'S' array): element i's bytes at data + i * stride."""
    _check(
        _load().tcamd_pack_bytes_strided(_vp(data_ptr), int(stride), _vp(lens_ptr), n, _vp(out_ptr),
                                         _vp(workspace_ptr), _vp(stream)),
        "pack_bytes_strided",
    )


def index_bytes_last_path():
    """(path, window) of this thread's last index_bytes: 0 serial walk, 1 v3
    speculative block walk (64-B candidate window), 3 v3 with the 256-B
    window (an element of 60..252 B crossed a block), 2 general
    pointer-doubling fallback."""
    w = ctypes.c_uint64(0)
    p = _load().tcamd_index_bytes_last_path(ctypes.byref(w))
    return p, w.value


def k3_set_check(on):
    """K3 overrun check mode (process-wide): each index_bytes call allocates its
    workspace at exactly the size it needs with a 4 KiB canary behind it and
    fails if the canary changed.  Returns the previous setting."""
    return bool(_load().tcamd_k3_set_check(1 if on else 0))


K17_EPI = {"none": 0, "bias": 1, "bias_gelu": 2, "bias_gelu_erf": 3, "bias_gelu_erf_x3": 4}


def k17_gemm(a, b, bias, c, M, N, K, lda, ldb, ldc, epilogue="none", out_f32=False, stream=None):
    """K17 (csrc/kernels/gemm.hip): C[M, N] = A[M, K] . B[N, K]^T (+ bias) (GELU)
    with bf16 A and B (K contiguous, row strides lda / ldb), fp32 bias [N], C
    bf16 or fp32 (``out_f32``) with row stride ldc; fp32 accumulate.  N a
    multiple of 256, K of 32."""
    _check(_load().tcamd_k17_gemm(a, b, _vp(bias), c, int(M), int(N), int(K), int(lda), int(ldb), int(ldc),
                                  K17_EPI[epilogue], 1 if out_f32 else 0, _vp(stream)), "k17_gemm")


def k18_gemm(a, b, bias, c, M, N, K, lda, ldb, ldc, epilogue="none", out_f32=False, cfg=0, splits=1,
             split_stride=0, stream=None):
    """K18 (csrc/kernels/gemm_tiles.hip): the small / mid-M tiled GEMM.  As
    k17_gemm, with the tile configuration ``cfg`` (k18_cfg) and, for
    ``splits`` > 1, K split over workgroups: C is then fp32, no epilogue, and
    split z writes its partial product at C + z * split_stride (elements)."""
    _check(_load().tcamd_k18_gemm(a, b, _vp(bias), c, int(M), int(N), int(K), int(lda), int(ldb), int(ldc),
                                  K17_EPI[epilogue], 1 if out_f32 else 0, int(cfg), int(splits), int(split_stride),
                                  _vp(stream)), "k18_gemm")


def k18_cfg(cfg):
    """(tile rows, tile columns, threads, ring stages) of K18 configuration ``cfg``, or None past the table."""
    v = [ctypes.c_int(0) for _ in range(4)]
    if _load().tcamd_k18_cfg(int(cfg), *[ctypes.byref(x) for x in v]) != 0:
        return None
    return tuple(x.value for x in v)


def k18_calls():
    """K18 launches so far in this process."""
    return int(_load().tcamd_k18_calls())


def qa_head(x, w, b, start, end, rows, H, f32=False, stream=None):
    """BERT's span head: start[r] = x[r] . w[0] + b[0], end[r] = x[r] . w[1] +
    b[1] in fp32; x [rows][H] and w [2][H] bf16 (or fp32 with ``f32``), b fp32 [2]."""
    _check(_load().tcamd_qa_head(x, w, b, start, end, int(rows), int(H), 1 if f32 else 0, _vp(stream)), "qa_head")


def add_layernorm_parts(x, parts, nparts, pstride, bias, gamma, beta, out, rows, H, eps, f32=False, stream=None,
                        out3=None):
    """K11p: out = LayerNorm(x + bias + sum of ``nparts`` fp32 partial slabs
    (``parts`` + z * ``pstride`` elements, [rows][H] each)) * gamma + beta.
    bias fp32 [H] or None; x / gamma / beta / out bf16, or fp32 with ``f32``.
    ``out3`` (f32 only, or None): the output also as a bf16x3 GEMM operand,
    bf16 [rows][3H] = [hi | hi | lo] (x3_cat's layout)."""
    _check(_load().tcamd_add_layernorm_parts3(x, _vp(parts), int(nparts), int(pstride), _vp(bias), gamma, beta, out,
                                              _vp(out3), int(rows), int(H), float(eps), 1 if f32 else 0, _vp(stream)),
           "add_layernorm_parts")


def k17_last_tm():
    """Tile height (128 / 256) the last k17_gemm picked (TCAMD_K17_TM forces one)."""
    return int(_load().tcamd_k17_last_tm())


def k17_calls():
    """K17 launches so far in this process."""
    return int(_load().tcamd_k17_calls())


def knobs():
    """The native knob registry (csrc/runtime/knobs.hip): {name: {"default",
    "value", "doc"}} -- every tuning / diagnostic switch the kernels' host
    entry points read, seeded from the environment variable of that name."""
    lib_ = _load()
    out = {}
    for i in range(lib_.tcamd_knob_count()):
        name, doc = ctypes.c_char_p(), ctypes.c_char_p()
        d, v = ctypes.c_longlong(), ctypes.c_longlong()
        if lib_.tcamd_knob_info(i, ctypes.byref(name), ctypes.byref(d), ctypes.byref(v), ctypes.byref(doc)) == 0:
            out[name.value.decode()] = {"default": d.value, "value": v.value, "doc": doc.value.decode()}
    return out


def knob_set(name, value):
    """Sets a native knob for this process (read at each launch; a captured HIP
    graph keeps what it captured); returns the previous value."""
    prev = ctypes.c_longlong()
    if _load().tcamd_knob_set(name.encode(), int(value), ctypes.byref(prev)) != 0:
        raise KeyError("unknown native knob %r (known: %s)" % (name, ", ".join(sorted(knobs()))))
    return prev.value


@contextlib.contextmanager
def knob(**settings):
    """``with hip.knob(TCAMD_X3_WS=0): ...`` -- native knobs set for the block, restored after."""
    prev = {}
    try:
        for k, v in settings.items():
            prev[k] = knob_set(k, v)
        yield
    finally:
        for k, v in prev.items():
            knob_set(k, v)


def index_bytes(buf_ptr, nbytes, n_expected, offs_ptr, lens_ptr, status_ptr, stream=None):
    """K3: device BYTES index (offsets/lengths of each element).  Synchronises
    ``stream`` (it reads its own status to size the scan window)."""
    _check(
        _load().tcamd_index_bytes(
            _vp(buf_ptr), nbytes, n_expected, _vp(offs_ptr), _vp(lens_ptr), _vp(status_ptr), _vp(stream)
        ),
        "index_bytes",
    )


class PtrGraphExecutor:
    """Native per-batch dispatch for a pointer-table graph model
    (csrc/runtime/graph_exec.hip): the server's C++ batcher calls
    ``fn_address`` with ``handle`` directly, so no Python runs per batch.

    ``bind(i, stream, graph_execs, tbl_dev, stage_dev, out_dev, pad_ptrs)``
    hands instance ``i`` its HIP stream, one graph exec per bucket, the
    engine's device row-pointer table, a device staging area for host rows,
    the graph's output buffer and per-row padding pointers."""

    STAT_KEYS = ("batches", "prep_ns", "enqueue_ns", "wait_ns", "post_ns", "total_ns", "rows")

    def __init__(self, device, instances, in_row_bytes, out_row_bytes, buckets):
        lib = _load()
        self.buckets = [int(b) for b in buckets]
        self.max_rows = max(self.buckets)
        err = ctypes.create_string_buffer(512)
        arr = (ctypes.c_int32 * len(self.buckets))(*self.buckets)
        h = lib.tcamd_pgx_create(int(device), int(instances), int(in_row_bytes), int(out_row_bytes),
                                 len(self.buckets), arr, err, 512)
        if not h:
            raise RuntimeError(err.value.decode(errors="replace"))
        self.handle = h

    def bind(self, i, stream, graph_execs, tbl_dev, stage_dev, out_dev, pad_ptrs):
        if len(graph_execs) != len(self.buckets) or len(pad_ptrs) < self.max_rows:
            raise ValueError("one graph exec per bucket and max_rows padding pointers are required")
        err = ctypes.create_string_buffer(512)
        ge = (ctypes.c_uint64 * len(graph_execs))(*[int(g) for g in graph_execs])
        pad = (ctypes.c_uint64 * self.max_rows)(*[int(p) for p in pad_ptrs[:self.max_rows]])
        rc = _load().tcamd_pgx_set_instance(self.handle, int(i), _vp(stream), ge, int(tbl_dev), int(stage_dev),
                                            int(out_dev), pad, err, 512)
        if rc != 0:
            raise RuntimeError(err.value.decode(errors="replace"))

    @property
    def fn_address(self):
        return ctypes.cast(_load().tcamd_pgx_execute, ctypes.c_void_p).value

    def execute(self, instance, batch_ptr):
        """Run one tcserve_batch (a ctypes pointer/address) on ``instance``."""
        err = ctypes.create_string_buffer(1024)
        rc = _load().tcamd_pgx_execute(self.handle, int(instance), batch_ptr, err, 1024)
        if rc != 0:
            raise RuntimeError(err.value.decode(errors="replace"))

    def stats(self):
        out = (ctypes.c_uint64 * len(self.STAT_KEYS))()
        _load().tcamd_pgx_stats(self.handle, out)
        return dict(zip(self.STAT_KEYS, [int(v) for v in out]))

    def close(self):
        if self.handle:
            _load().tcamd_pgx_destroy(self.handle)
            self.handle = None


def available():
    """True if the library loads and at least one GPU is visible."""
    try:
        _load()
    except Exception:
        return False
    return device_count() > 0


# eager load so a missing .so fails at import time (loudly) on GPU boxes
if os.environ.get("TCAMD_LAZY_HIP", "0") != "1":
    try:
        _load()
    except OSError as e:  # pragma: no cover
        print("warning: libtcamd_hip.so failed to load: %s" % e, file=sys.stderr)
        raise
