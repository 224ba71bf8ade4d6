"""ctypes binding of libspotter_hip.so (include/spotter_hip.h).

The product path has no fallback: if the library is missing or the device is
not gfx950, `lib()` raises. Every wrapper raises RuntimeError with
sp_last_error() on a non-zero status, so the unchanged AmenitiesDetector turns a
kernel failure into its per-image "Processing Error" (serve.py:152-157).
"""
from __future__ import annotations

import ctypes as C
import os
import threading

HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("SPOTTER_HIP_LIB", os.path.join(HERE, "libspotter_hip.so"))
ABI_VERSION = 20

vp = C.c_void_p
i32 = C.c_int32
i64 = C.c_int64
f32 = C.c_float


class SpImageU8(C.Structure):
    _fields_ = [("data", vp), ("height", i32), ("width", i32), ("row_stride", i32)]


class SpConvDesc(C.Structure):
    _fields_ = [
        ("A", vp), ("lda", i64), ("A2", vp), ("lda2", i64),
        ("N", i32), ("H", i32), ("W", i32), ("Cin", i32),
        ("KH", i32), ("KW", i32), ("stride", i32), ("pad", i32),
        ("Ho", i32), ("Wo", i32),
        ("Wt", vp), ("Cout", i32),
        ("scale", vp), ("shift", vp),
        ("row_scale", vp), ("row_period", i32),
        ("res1", vp), ("ldr1", i64),
        ("act", i32),
        ("res2", vp), ("ldr2", i64),
        ("C", vp), ("ldc", i64),
        ("out_rows_per_group", i32), ("out_group_stride", i64),
        ("workspace", vp), ("workspace_elems", i64),
        ("precision", i32), ("Wt_bf16", vp), ("wt_plane_stride", i64),
        ("ln_gamma", vp), ("ln_beta", vp), ("ln_eps", f32),
        ("A_bf16", vp),
        ("C_bf16", vp), ("res1_bf16", vp), ("res2_bf16", vp),
        ("splitk_counters", vp), ("splitk_counters_len", i64),
    ]


class SpConvPlanInfo(C.Structure):
    _fields_ = [(f, i32) for f in ("family", "tile", "planes", "generic", "a_bf16", "fast_1x1", "epilogue", "splits",
                                   "counters")]


class SpWinogradPlanInfo(C.Structure):
    _fields_ = [("gemm", SpConvPlanInfo), ("components", i32), ("in_vw", i32), ("out_vw", i32), ("tiles", i64)]


class SpWinogradExpandPlanInfo(C.Structure):
    _fields_ = [("expand", SpConvPlanInfo), ("fused", i32), ("reserved", i32), ("tiles", i64), ("units", i64)]


class SpMsdaDesc(C.Structure):
    _fields_ = [
        ("value", vp), ("ld_value", i64), ("value_col", i32),
        ("off_aw", vp), ("ld_off_aw", i64),
        ("ref", vp),
        ("out", vp), ("ld_out", i64),
        ("B", i32), ("S", i32), ("Q", i32), ("heads", i32), ("head_dim", i32),
        ("levels", i32), ("points", i32),
        ("level_h", i32 * 4), ("level_w", i32 * 4), ("level_start", i32 * 4),
        ("offset_scale", f32),
        ("value_bf16", vp),
    ]


class SpJpegLayout(C.Structure):
    _fields_ = [
        ("width", i32), ("height", i32), ("ncomp", i32), ("color", i32), ("progressive", i32),
        ("max_h", i32), ("max_v", i32), ("h", i32 * 3), ("v", i32 * 3), ("bw", i32 * 3), ("bh", i32 * 3),
        ("block_off", i64 * 3), ("total_blocks", i64), ("plane_off", i64 * 3), ("plane_bytes", i64),
        ("quant", (C.c_uint16 * 64) * 3),
    ]


SP_JPEG_BATCH_MAX, SP_JPEG_BATCH_IDCT_BLOCKS, SP_JPEG_BATCH_COLOR_PX = 64, 32, 1024


class SpJpegBatchItem(C.Structure):
    _fields_ = [("lay", SpJpegLayout), ("coef_off", i64), ("work_off", i64), ("rgb_off", i64), ("rgb_stride", i64),
                ("first_wg_idct", i32), ("first_wg_color", i32)]


class SpJpegBatchTotals(C.Structure):
    _fields_ = [("coef_elems", i64), ("work_bytes", i64), ("rgb_bytes", i64), ("wg_idct", i64), ("wg_color", i64)]


class SpJpegScan(C.Structure):
    _fields_ = [
        ("ncomp", i32), ("bpm", i32), ("mcux", i32), ("mcuy", i32), ("restart_interval", i32), ("sub_bits", i32),
        ("slot_comp", i32 * 10), ("slot_v", i32 * 10), ("slot_h", i32 * 10),
        ("nmcu", i64), ("nseg", i64), ("nsub", i64), ("tab_off", i64), ("seg_off", i64), ("stream_off", i64),
        ("stream_bits", i64), ("stream_bytes", i64), ("pkg_bytes", i64), ("work_bytes", i64),
    ]


class SpJpegEntropyItem(C.Structure):
    _fields_ = [("scan", SpJpegScan), ("h", i32 * 3), ("v", i32 * 3), ("bw", i32 * 3), ("bh", i32 * 3),
                ("block_off", i64 * 3), ("total_blocks", i64), ("geom", i64 * 28), ("pkg_off", i64), ("work_off", i64),
                ("coef_off", i64), ("dc_nchunk", i64), ("first_wg_sub", i32), ("first_wg_dc", i32)]


class SpJpegEntropyTotals(C.Structure):
    _fields_ = [("pkg_bytes", i64), ("work_bytes", i64), ("wg_sub", i64), ("wg_dc", i64)]


class SpJpegEncLayout(C.Structure):
    _fields_ = [
        ("width", i32), ("height", i32), ("quality", i32), ("h0", i32), ("v0", i32),
        ("mcux", i32), ("mcuy", i32), ("bpm", i32), ("wb0", i32), ("hb0", i32),
        ("total_blocks", i64), ("work_bytes", i64), ("bits_cap", i64),
        ("quant", (C.c_uint16 * 64) * 2), ("recip", (C.c_uint16 * 64) * 2), ("corr", (C.c_uint16 * 64) * 2),
        ("shift", (C.c_int16 * 64) * 2),
    ]


SP_JPEG_ENC_FDCT_MCUS, SP_JPEG_ENC_WG_MCUS = 4, 256


class SpJpegEncBatchItem(C.Structure):
    _fields_ = [("lay", SpJpegEncLayout), ("src", vp), ("row_stride", i64), ("work_off", i64), ("pixel_bytes", i32),
                ("first_wg_fdct", i32), ("first_wg_mcu", i32), ("reserved", i32)]


class SpJpegEncBatchTotals(C.Structure):
    _fields_ = [("work_bytes", i64), ("bits_cap", i64), ("wg_fdct", i64), ("wg_mcu", i64)]


class SpDrawOp(C.Structure):
    _fields_ = [
        ("kind", i32), ("x0", i32), ("y0", i32), ("x1", i32), ("y1", i32), ("ink", C.c_uint32),
        ("mask_off", i64), ("mask_stride", i32), ("sx", i32), ("sy", i32), ("reserved", i32),
    ]


class SpDrawTile(C.Structure):
    _fields_ = [("tx", i32), ("ty", i32), ("first", i32), ("count", i32)]


class SpDrawTable(C.Structure):
    _fields_ = [
        ("n_ops", i32), ("n_tiles", i32), ("n_refs", i32), ("height", i32), ("width", i32), ("reserved", i32),
        ("ops_off", i64), ("tiles_off", i64), ("refs_off", i64), ("masks_off", i64), ("mask_bytes", i64),
        ("total_bytes", i64),
    ]


SP_DRAW_BATCH_MAX = 64


class SpDrawBatchItem(C.Structure):
    _fields_ = [("rgb", vp), ("height", i32), ("width", i32), ("row_stride", i64), ("table_off", i64),
                ("table_bytes", i64), ("n_tiles", i32), ("first_wg", i32)]


SP_COPY_MAX_SEGMENTS, SP_COPY_BLOCK_ELEMS = 64, 4096


class SpCopySegment(C.Structure):
    _fields_ = [("src", vp), ("dst", vp), ("elems", i64)]


class SpCopySegmentsDesc(C.Structure):
    _fields_ = [("n", i32), ("reserved", i32), ("seg", SpCopySegment * SP_COPY_MAX_SEGMENTS)]


SP_DRAW_FILL, SP_DRAW_BLEND = 0, 1  # sp_draw_kind
SP_DRAW_TILE_W, SP_DRAW_TILE_H = 64, 8
SP_JPEG_UNSUPPORTED = -10
SP_JPEG_NOT_ELIGIBLE, SP_JPEG_PKG_SMALL = 1, 2  # sp_jpeg_entropy_pack's non-error returns
SP_BUILD_FUSED_LN = 1  # sp_build_flags bits (include/spotter_hip.h)
SP_BUILD_BOUNDS = 2

_SIGS = {
    "sp_abi_version": (i32, []),
    "sp_build_flags": (i32, []),
    "sp_bounds_report": (i64, [C.c_char_p, i64]),
    "sp_last_error": (C.c_char_p, []),
    "sp_device_init": (i32, [i32]),
    "sp_shutdown": (i32, []),
    "sp_preprocess_u8": (i32, [C.POINTER(SpImageU8), i32, i32, i32, vp, vp]),
    "sp_conv2d": (i32, [C.POINTER(SpConvDesc), vp]),
    "sp_set_conv_config": (i32, [i32]),
    "sp_set_splitk_config": (i32, [i32, i32, i32]),
    "sp_set_tuning": (i32, [i32, i32]),
    "sp_set_plan_batch": (i32, [i32, i32]),
    "sp_conv_plan": (i32, [C.POINTER(SpConvDesc), C.POINTER(SpConvPlanInfo)]),
    "sp_winograd_plan": (i32, [C.POINTER(SpConvDesc), i32, i64, i64, C.POINTER(SpWinogradPlanInfo)]),
    "sp_conv3x3_winograd": (i32, [C.POINTER(SpConvDesc), vp, i64, vp, i64, vp]),
    "sp_winograd_f23_input": (i32, [C.POINTER(SpConvDesc), vp, i64, vp]),
    "sp_winograd_f23_gemm": (i32, [C.POINTER(SpConvDesc), vp, i64, vp, i64, vp]),
    "sp_winograd_f23_output": (i32, [C.POINTER(SpConvDesc), vp, i64, vp]),
    "sp_winograd_f43_input": (i32, [C.POINTER(SpConvDesc), vp, i64, vp]),
    "sp_winograd_f43_gemm": (i32, [C.POINTER(SpConvDesc), vp, i64, vp, i64, vp]),
    "sp_winograd_f43_output": (i32, [C.POINTER(SpConvDesc), vp, i64, vp]),
    "sp_winograd_f43_expand": (i32, [C.POINTER(SpConvDesc), vp, i64, C.POINTER(SpConvDesc), vp, i64, i64, vp]),
    "sp_winograd_expand_plan": (i32, [C.POINTER(SpConvDesc), i64, C.POINTER(SpConvDesc), i32, i64,
                                      C.POINTER(SpWinogradExpandPlanInfo)]),
    "sp_nchw_to_nhwc": (i32, [vp, vp, i32, i32, i32, i32, vp]),
    "sp_stem_conv3x3s2_nchw": (i32, [vp, vp, vp, vp, vp, i32, i32, i32, i32, i32, vp]),
    "sp_maxpool3x3s2": (i32, [vp, vp, i64, i32, i32, i32, i32, vp]),
    "sp_avgpool2x2_ceil": (i32, [vp, vp, i64, i32, i32, i32, i32, vp]),
    "sp_maxpool3x3s2_bf16": (i32, [vp, vp, i64, i32, i32, i32, i32, vp]),
    "sp_avgpool2x2_ceil_bf16": (i32, [vp, vp, i64, i32, i32, i32, i32, vp]),
    "sp_stem_conv3x3s2_nchw_bf16": (i32, [vp, vp, vp, vp, vp, i32, i32, i32, i32, i32, vp]),
    "sp_conv3x3_c32_bf16": (i32, [vp, vp, vp, vp, vp, i32, i32, i32, i32, i32, vp]),
    "sp_conv3x3_c32": (i32, [vp, vp, vp, vp, vp, i32, i32, i32, i32, i32, vp]),
    "sp_conv3x3_c64_bf16": (i32, [vp, i64, vp, vp, vp, vp, i64, vp, i64, i32, i32, i32, i32, vp]),
    "sp_conv3x3_c64_x3": (i32, [vp, i64, vp, i64, vp, vp, vp, i64, i32, i32, i32, i32, vp]),
    "sp_conv3x3_c32_x3": (i32, [vp, vp, i64, vp, vp, vp, i32, i32, i32, i32, i32, vp]),
    "sp_upsample2x_nearest": (i32, [vp, i64, vp, i64, i32, i32, i32, i32, vp]),
    "sp_layernorm": (i32, [vp, i64, vp, vp, vp, i64, i32, i32, f32, vp]),
    "sp_layernorm_bf16": (i32, [vp, i64, vp, vp, vp, i64, i32, i32, f32, vp]),
    "sp_attention": (i32, [vp, i64, vp, i64, vp, i64, vp, i64, i32, i32, i32, i32, f32, vp]),
    "sp_attention_bf16": (i32, [vp, i64, vp, i64, vp, i64, vp, i64, i32, i32, i32, i32, f32, vp]),
    "sp_msda": (i32, [C.POINTER(SpMsdaDesc), vp]),
    "sp_topk_rows": (i32, [vp, i64, i32, i32, i32, i32, i32, vp, vp, vp]),
    "sp_rowmax": (i32, [vp, i64, i64, i32, vp, vp]),
    "sp_gather_rows": (i32, [vp, i64, i32, vp, i32, i32, i32, vp, i64, vp]),
    "sp_ref_init": (i32, [vp, i64, vp, vp, i32, i32, vp, vp]),
    "sp_box_refine": (i32, [vp, i64, vp, i32, vp]),
    "sp_add_rows": (i32, [vp, i64, vp, i64, vp, vp, i64, i32, i32, vp]),
    "sp_linear_rowmax_bf16": (i32, [vp, i64, vp, vp, i32, i32, i32, vp, vp]),
    "sp_postprocess": (i32, [vp, vp, vp, i32, i32, i32, i32, f32, vp, vp, vp, vp, vp, vp]),
    "sp_jpeg_decode_coefs": (i32, [vp, i64, C.POINTER(SpJpegLayout), vp, i64]),
    "sp_jpeg_to_rgb": (i32, [vp, C.POINTER(SpJpegLayout), vp, i64, vp, i64, vp, vp]),
    "sp_jpeg_batch_plan": (i32, [C.POINTER(SpJpegLayout), i32, C.POINTER(SpJpegBatchItem),
                                 C.POINTER(SpJpegBatchTotals)]),
    "sp_jpeg_batch_to_rgb": (i32, [vp, i64, vp, C.POINTER(SpJpegBatchItem), i32, C.POINTER(SpJpegBatchTotals), vp, i64,
                                   vp, i64, vp, vp]),
    "sp_jpeg_entropy_pack": (i32, [vp, i64, C.POINTER(SpJpegLayout), C.POINTER(SpJpegScan), vp, i64]),
    "sp_jpeg_entropy_decode": (i32, [vp, C.POINTER(SpJpegScan), C.POINTER(SpJpegLayout), vp, i64, vp, i64, vp, vp]),
    "sp_jpeg_entropy_emulate": (i32, [vp, C.POINTER(SpJpegScan), C.POINTER(SpJpegLayout), vp, i64, vp, vp]),
    "sp_jpeg_entropy_batch_plan": (i32, [C.POINTER(SpJpegScan), C.POINTER(SpJpegLayout), C.POINTER(SpJpegBatchItem), i32,
                                         C.POINTER(SpJpegEntropyItem), C.POINTER(SpJpegEntropyTotals)]),
    "sp_jpeg_entropy_batch_check": (i32, [C.POINTER(SpJpegEntropyItem), i32, C.POINTER(SpJpegEntropyTotals), i64, i64,
                                          i64]),
    "sp_jpeg_entropy_batch_decode": (i32, [vp, i64, vp, C.POINTER(SpJpegEntropyItem), i32,
                                           C.POINTER(SpJpegEntropyTotals), vp, i64, vp, i64, vp, vp]),
    "sp_jpeg_entropy_batch_emulate": (i32, [vp, i64, C.POINTER(SpJpegEntropyItem), i32,
                                            C.POINTER(SpJpegEntropyTotals), vp, i64, vp, i64, vp]),
    "sp_jpeg_enc_plan": (i32, [i32, i32, i32, i32, C.POINTER(SpJpegEncLayout)]),
    "sp_jpeg_enc_rgb": (i32, [vp, i64, i32, C.POINTER(SpJpegEncLayout), vp, i64, vp, i64, vp, vp]),
    "sp_jpeg_enc_max_bytes": (i64, [C.POINTER(SpJpegEncLayout), i64, i64]),
    "sp_jpeg_enc_finish": (i32, [C.POINTER(SpJpegEncLayout), vp, i64, vp, i64, vp, i64, C.POINTER(i64)]),
    "sp_jpeg_enc_batch_plan": (i32, [C.POINTER(SpJpegEncLayout), i32, C.POINTER(SpJpegEncBatchItem),
                                     C.POINTER(SpJpegEncBatchTotals)]),
    "sp_jpeg_enc_batch_rgb": (i32, [vp, C.POINTER(SpJpegEncBatchItem), i32, C.POINTER(SpJpegEncBatchTotals), vp, i64,
                                    vp, i64, vp, vp]),
    "sp_draw_pack": (i32, [vp, i32, vp, i64, i32, i32, vp, i64, C.POINTER(i64)]),
    "sp_draw_rgb": (i32, [vp, i32, i32, i64, vp, vp, i64, vp]),
    "sp_draw_batch_plan": (i64, [C.POINTER(SpDrawBatchItem), i32, vp, i64]),
    "sp_draw_batch_rgb": (i32, [vp, C.POINTER(SpDrawBatchItem), i32, vp, vp, i64, vp]),
    "sp_host_register": (i32, [vp, i64, C.POINTER(vp)]),
    "sp_host_unregister": (i32, [vp]),
    "sp_copy_segments": (i32, [C.POINTER(SpCopySegmentsDesc), vp]),
}

EXPORTS = tuple(_SIGS)

_lock = threading.Lock()
_lib = None


def load(path: str = LIB_PATH):
    """dlopen the library and bind every export (no device calls)."""
    if not os.path.exists(path):
        raise RuntimeError(
            f"libspotter_hip.so not found at {path}; build it with `python -m spotter_amd.build_ext` "
            "(there is no CPU fallback)")
    # torch first: its wheel bundles a HIP runtime (soname libamdhip64.so.7, found through libtorch_hip's
    # $ORIGIN rpath under the name libamdhip64.so). Loaded after torch, this library binds to that copy by
    # soname; loaded before it, this library brings in the system ROCm's copy and torch then loads its own
    # beside it: two HIP runtimes in one process, and the first hipMalloc / hipMemcpy here fails (build()
    # followed by smoke() in one process did: "coefficient upload failed").
    import torch  # noqa: F401

    L = C.CDLL(path)
    for name, (res, args) in _SIGS.items():
        fn = getattr(L, name)
        fn.restype = res
        fn.argtypes = args
    if L.sp_abi_version() != ABI_VERSION:
        raise RuntimeError(f"libspotter_hip ABI {L.sp_abi_version()} != {ABI_VERSION}")
    return L


def lib():
    global _lib
    with _lock:
        if _lib is None:
            _lib = load()
        return _lib


def check(rc: int, what: str = ""):
    if rc != 0:
        msg = lib().sp_last_error().decode(errors="replace")
        raise RuntimeError(f"spotter_hip {what} failed ({rc}): {msg}")


def call(name: str, *args):
    check(getattr(lib(), name)(*args), name)
