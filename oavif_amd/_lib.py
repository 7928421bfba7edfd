"""ctypes binding of liboavif_hip.so (C ABI: include/ssimu2_hip.h, include/oavif_tq.h).

The product path has no CPU fallback: if the library is missing or fails to load this
module raises, and every scorer call needs a gfx950 device.
"""
from __future__ import annotations

import ctypes
import os

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("OAVIF_AMD_LIB") or os.path.join(_HERE, "lib", "liboavif_hip.so")
# the same scorer sources plus the hooks of include/ssimu2_hip_internal.h: bench / scripts / a few tests
INSTR_LIB_PATH = os.environ.get("OAVIF_AMD_INSTR_LIB") or os.path.join(_HERE, "lib", "liboavif_hip_instr.so")
# the product library's sources plus the RGBA entry points of include/ssimu2_hip_ext.h (Ssimu2(..., extended=True))
EXT_LIB_PATH = os.environ.get("OAVIF_AMD_EXT_LIB") or os.path.join(_HERE, "lib", "liboavif_hip_ext.so")
# the extension library's sources plus the YUV entry points of include/ssimu2_hip_yuv.h (Ssimu2(..., yuv=True))
YUV_LIB_PATH = os.environ.get("OAVIF_AMD_YUV_LIB") or os.path.join(_HERE, "lib", "liboavif_hip_yuv.so")
# the YUV library's objects plus the error maps of 16-bit, RGBA and YUV frames of include/ssimu2_hip_map.h
# (Ssimu2(..., maps=True))
MAP_LIB_PATH = os.environ.get("OAVIF_AMD_MAP_LIB") or os.path.join(_HERE, "lib", "liboavif_hip_map.so")
# the map library's objects plus the 4:2:2 / 4:2:0 YUV calls of include/ssimu2_hip_chroma.h (Ssimu2(..., chroma=True))
CHROMA_LIB_PATH = os.environ.get("OAVIF_AMD_CHROMA_LIB") or os.path.join(_HERE, "lib", "liboavif_hip_chroma.so")
# the chroma library's objects plus the calls of include/ssimu2_hip_yuva.h that take YUV planes with an alpha plane
# (Ssimu2(..., yuva=True))
YUVA_LIB_PATH = os.environ.get("OAVIF_AMD_YUVA_LIB") or os.path.join(_HERE, "lib", "liboavif_hip_yuva.so")
# the YUVA library's objects plus the batch calls of include/ssimu2_hip_rbatch.h, which score in every blur mode
# (Ssimu2(..., rbatch=True))
RBATCH_LIB_PATH = os.environ.get("OAVIF_AMD_RBATCH_LIB") or os.path.join(_HERE, "lib", "liboavif_hip_rbatch.so")
# the rbatch library's objects plus the 16-bit and YUV batches of include/ssimu2_hip_hbatch.h (Ssimu2(..., hbatch=True))
HBATCH_LIB_PATH = os.environ.get("OAVIF_AMD_HBATCH_LIB") or os.path.join(_HERE, "lib", "liboavif_hip_hbatch.so")
# the hbatch library's objects plus the batches of RGBA and YUV-with-alpha frames of include/ssimu2_hip_abatch.h
# (Ssimu2(..., abatch=True))
ABATCH_LIB_PATH = os.environ.get("OAVIF_AMD_ABATCH_LIB") or os.path.join(_HERE, "lib", "liboavif_hip_abatch.so")

OK = 0
ERR_INVALID_ARG = -1
ERR_UNSUPPORTED = -2
ERR_OOM = -3
ERR_HIP = -4
ERR_NO_REFERENCE = -5
ERR_NO_DEVICE = -6

STAGE_PYRAMID, STAGE_MARCH, STAGE_FINALIZE = 0, 1, 2
NUM_SCALES = 6
STATS_PER_SCALE = 18
TQ_MAX_PASS = 12
ALPHA_CODES = 65026   # SSIMU2_ALPHA_CODES (include/ssimu2_hip_ext.h): composite codes 0 .. 255 * 255
MAX_BATCH = 4096   # SSIMU2_MAX_BATCH (include/ssimu2_hip.h): items of one ssimu2_score_batch_* call

YUV_444, YUV_400 = 1, 4   # SSIMU2_YUV_* (include/ssimu2_hip_yuv.h): libavif's avifPixelFormat values
YUV_422, YUV_420 = 2, 3   # SSIMU2_YUV_* (include/ssimu2_hip_chroma.h): subsampled chroma, the chroma library only
CHROMA_BILINEAR, CHROMA_NEAREST = 0, 1   # SSIMU2_CHROMA_* (include/ssimu2_hip_chroma.h)
BLUR_FIR, BLUR_RECURSIVE, BLUR_RECURSIVE_FMA = 0, 1, 2   # SSIMU2_BLUR_* (include/ssimu2_hip.h)


class TQOptions(ctypes.Structure):
    _fields_ = [("score_tgt", ctypes.c_double), ("tolerance", ctypes.c_double),
                ("max_pass", ctypes.c_uint32)]


class TQPass(ctypes.Structure):
    _fields_ = [("q", ctypes.c_uint32), ("score", ctypes.c_double)]


class TQResult(ctypes.Structure):
    _fields_ = [("q", ctypes.c_uint32), ("score", ctypes.c_double),
                ("num_pass", ctypes.c_uint32), ("buf_q", ctypes.c_int32),
                ("history_len", ctypes.c_uint32), ("history", TQPass * TQ_MAX_PASS)]


class PngInfo(ctypes.Structure):   # oavif_png_info (include/oavif_tq.h)
    _fields_ = [("width", ctypes.c_uint32), ("height", ctypes.c_uint32), ("channels", ctypes.c_uint32),
                ("hbd", ctypes.c_int), ("data_bytes", ctypes.c_size_t), ("icc_bytes", ctypes.c_size_t),
                ("bit_depth", ctypes.c_uint32), ("color_type", ctypes.c_uint32), ("interlaced", ctypes.c_uint32)]


class TQSpecOptions(ctypes.Structure):
    """oavif_tq_spec_options; struct_size = OAVIF_TQ_SPEC_OPTIONS_TAG | sizeof is the ABI guard
    (include/oavif_tq.h), filled in here."""
    TAG = 0x71530000
    _fields_ = [("struct_size", ctypes.c_uint32), ("max_fanout", ctypes.c_uint32), ("first_wave_fanout", ctypes.c_uint32)]

    def __init__(self, max_fanout: int = 1, first_wave_fanout: int = 0):
        super().__init__(self.TAG | ctypes.sizeof(TQSpecOptions), int(max_fanout), int(first_wave_fanout))


class DeviceInfo(ctypes.Structure):
    """ssimu2_device_info (include/ssimu2_hip.h): what the library read off a HIP device."""
    _fields_ = [("struct_size", ctypes.c_uint32), ("device", ctypes.c_int32), ("arch", ctypes.c_char * 64),
                ("name", ctypes.c_char * 128), ("pci_bus_id", ctypes.c_char * 32), ("compute_units", ctypes.c_uint32),
                ("lds_bytes_per_cu", ctypes.c_uint32), ("lds_bytes_per_workgroup", ctypes.c_uint32),
                ("wavefront_size", ctypes.c_uint32), ("hbm_bytes", ctypes.c_uint64), ("numa_node", ctypes.c_int32),
                ("usable", ctypes.c_int32)]

    def __init__(self):
        super().__init__()
        self.struct_size = ctypes.sizeof(DeviceInfo)

    def as_dict(self) -> dict:
        return {"device": int(self.device), "arch": self.arch.decode(), "name": self.name.decode(),
                "pci_bus_id": self.pci_bus_id.decode(), "compute_units": int(self.compute_units),
                "lds_bytes_per_cu": int(self.lds_bytes_per_cu), "lds_bytes_per_workgroup": int(self.lds_bytes_per_workgroup),
                "wavefront_size": int(self.wavefront_size), "hbm_bytes": int(self.hbm_bytes),
                "numa_node": int(self.numa_node), "usable": bool(self.usable)}


class YuvFrameC(ctypes.Structure):
    """ssimu2_yuv_frame (include/ssimu2_hip_yuv.h)."""
    _fields_ = [("planes", ctypes.c_void_p * 3), ("row_bytes", ctypes.c_uint32 * 3), ("depth", ctypes.c_uint32),
                ("format", ctypes.c_uint32), ("full_range", ctypes.c_uint32), ("matrix_coefficients", ctypes.c_uint32)]


class YuvaFrameC(ctypes.Structure):
    """ssimu2_yuva_frame (include/ssimu2_hip_yuva.h)."""
    _fields_ = [("yuv", YuvFrameC), ("alpha", ctypes.c_void_p), ("alpha_row_bytes", ctypes.c_uint32),
                ("alpha_premultiplied", ctypes.c_uint32)]


class TQSpecStats(ctypes.Structure):
    _fields_ = [("waves", ctypes.c_uint32), ("probes_issued", ctypes.c_uint32),
                ("cache_hits", ctypes.c_uint32)]


TQ_MAX_FANOUT = 16
BATCH_PROBE_FN = ctypes.CFUNCTYPE(ctypes.c_int, ctypes.c_void_p, ctypes.POINTER(ctypes.c_uint32),
                                  ctypes.c_uint32, ctypes.POINTER(ctypes.c_double))
PROBE_FN = ctypes.CFUNCTYPE(ctypes.c_int, ctypes.c_void_p, ctypes.c_uint32,
                            ctypes.POINTER(ctypes.c_double))
CODEC_FN = ctypes.CFUNCTYPE(ctypes.c_int, ctypes.c_void_p, ctypes.c_uint32,
                            ctypes.POINTER(ctypes.c_uint8), ctypes.POINTER(ctypes.c_size_t))

# ---- every C function, declared once: name -> (restype, argtypes) ------------------------------------
# In header order.  EXPORTED_SYMBOLS / INSTR_SYMBOLS are the names (tests/test_abi.py holds them to the
# libraries' exports and to the Zig shim), tests/test_binding_signatures.py holds every entry to its prototype.
_vp, _ci, _u32, _sz, _f64 = ctypes.c_void_p, ctypes.c_int, ctypes.c_uint32, ctypes.c_size_t, ctypes.c_double
_u8p, _u16p, _u32p = ctypes.POINTER(ctypes.c_uint8), ctypes.POINTER(ctypes.c_uint16), ctypes.POINTER(ctypes.c_uint32)
_f32p, _f64p, _cip, _szp = ctypes.POINTER(ctypes.c_float), ctypes.POINTER(_f64), ctypes.POINTER(_ci), ctypes.POINTER(_sz)
_vpp, _u8pp, _u16pp = ctypes.POINTER(_vp), ctypes.POINTER(_u8p), ctypes.POINTER(_u16p)
_P = ctypes.POINTER

PUBLIC_FUNCTIONS = {   # include/ssimu2_hip.h, then include/oavif_tq.h
    "ssimu2_ctx_create": (_ci, [_ci, _vp, _vpp]),
    "ssimu2_query_device": (_ci, [_ci, _P(DeviceInfo)]),
    "ssimu2_ctx_device_info": (_ci, [_vp, _P(DeviceInfo)]),
    "ssimu2_host_alloc": (_ci, [_vp, _sz, _vpp]),
    "ssimu2_host_free": (_ci, [_vp, _vp]),
    "ssimu2_prefetch": (_ci, [_ci]),
    "ssimu2_prefetch_join": (_ci, [_ci]),
    "ssimu2_ctx_destroy": (None, [_vp]),
    "ssimu2_ctx_set_blur": (_ci, [_vp, _ci]),
    "ssimu2_last_error": (ctypes.c_char_p, [_vp]),
    "ssimu2_score_rgb8": (_ci, [_vp, _u8p, _u8p, _u32, _u32, _u32, _f64p]),
    "ssimu2_set_reference": (_ci, [_vp, _u8p, _u32, _u32]),
    "ssimu2_score_against_reference": (_ci, [_vp, _u8p, _f64p]),
    "ssimu2_score_against_reference_strided": (_ci, [_vp, _u8p, _u32, _u32, _f64p]),
    "ssimu2_score_rgb8_device": (_ci, [_vp, _vp, _vp, _u32, _u32, _f64p]),
    "ssimu2_enqueue_rgb8_device": (_ci, [_vp, _vp, _vp, _u32, _u32]),
    "ssimu2_wait": (_ci, [_vp, _f64p]),
    "ssimu2_set_reference_device": (_ci, [_vp, _vp, _u32, _u32]),
    "ssimu2_enqueue_against_reference_device": (_ci, [_vp, _vp]),
    "ssimu2_last_averages": (_ci, [_vp, _f64p, _cip]),
    "ssimu2_error_map_rgb8": (_ci, [_vp, _u8p, _u8p, _u32, _u32, _u32, _f32p, _f64p]),
    "ssimu2_error_map_against_reference": (_ci, [_vp, _u8p, _f32p, _f64p]),
    "ssimu2_linear_table": (_ci, [_u32, _f32p]),
    "ssimu2_score_rgb16": (_ci, [_vp, _u16p, _u16p, _u32, _u32, _u32, _u32, _f64p]),
    "ssimu2_set_reference_rgb16": (_ci, [_vp, _u16p, _u32, _u32, _u32]),
    "ssimu2_score_against_reference_rgb16": (_ci, [_vp, _u16p, _u32, _f64p]),
    "ssimu2_score_against_reference_strided16": (_ci, [_vp, _u16p, _u32, _u32, _u32, _f64p]),
    "ssimu2_score_batch_rgb8": (_ci, [_vp, _u8pp, _u8pp, _u32, _u32, _u32, _f64p]),
    "ssimu2_score_batch_against_reference": (_ci, [_vp, _u8pp, _u32, _f64p]),
    "ssimu2_score_batch_rgb8_device": (_ci, [_vp, _vp, _vp, _sz, _u32, _u32, _u32, _f64p]),
    "ssimu2_score_batch_against_reference_device": (_ci, [_vp, _vp, _sz, _u32, _f64p]),
    "ssimu2_last_batch_averages": (_ci, [_vp, _u32, _f64p, _cip]),
    "ssimu2_version": (ctypes.c_char_p, []),
    "oavif_tq_default_options": (None, [_P(TQOptions)]),
    "oavif_tq_predict_q_from_score": (_u32, [_f64]),
    "oavif_tq_interpolate_quantizer": (_u32, [_u32, _u32, _P(TQPass), _u32, _f64]),
    "oavif_tq_find_target_quality": (_ci, [_P(TQOptions), PROBE_FN, _vp, _P(TQResult)]),
    "oavif_tq_search_hip": (_ci, [_P(TQOptions), _vp, _u8p, _u32, _u32, CODEC_FN, _vp, _P(TQResult), _szp]),
    "oavif_tq_find_target_quality_speculative": (_ci, [_P(TQOptions), _P(TQSpecOptions), BATCH_PROBE_FN, _vp,
                                                       _P(TQResult), _P(TQSpecStats)]),
    "oavif_prescale_8_to_10": (None, [_u8p, _sz, _u16p]),
    "oavif_prescale_16_to_10": (None, [_u16p, _sz, _u16p]),
    "oavif_prescale_16_to_8": (None, [_u16p, _sz, _u8p]),
    "oavif_png_info_from_memory": (_ci, [_u8p, _sz, _P(PngInfo)]),
    "oavif_png_decode": (_ci, [_u8p, _sz, _vp, _sz, _vp, _sz]),
}

HOOK_FUNCTIONS = {     # include/ssimu2_hip_internal.h: only liboavif_hip_instr.so has these
    "ssimu2_debug_download": (_ci, [_vp, _ci, _ci, _u32, _u32, _f32p, _u32p, _u32p]),
    "ssimu2_time_device": (_ci, [_vp, _vp, _vp, _u32, _u32, _ci, _f32p, _f64p]),
    "ssimu2_time_stage": (_ci, [_vp, _vp, _vp, _u32, _u32, _ci, _ci, _f32p]),
    "ssimu2_time_march_rotating": (_ci, [_vp, _vpp, _vpp, _ci, _u32, _u32, _ci, _f32p]),
    "ssimu2_measure_read_stream": (_ci, [_vp, _sz, _ci, _f64p]),
    "ssimu2_instr_set_segment_rows": (_ci, [_vp, _ci, _ci]),
    "ssimu2_instr_cache_reference_blur": (_ci, [_vp, _ci]),
    "ssimu2_instr_last_march": (_ci, [_vp, _cip]),
    "ssimu2_instr_set_batch_segment_rows": (_ci, [_vp, _ci]),
    "ssimu2_instr_batch_segment_rows": (_ci, [_vp, _u32, _u32, _ci, _cip]),
    "ssimu2_time_blur_stage_rotating": (_ci, [_vp, _vpp, _ci, _u32, _u32, _ci, _f32p, _f64p]),
    "ssimu2_time_kernels": (_ci, [_vp, _vp, _vpp, _vpp, _ci, _u32, _u32, _ci, _f32p, _cip, _f32p, _f32p]),
    "ssimu2_instr_placed_streams": (_ci, [_vp, _cip]),
    "ssimu2_instr_rg_stop_after_scale": (_ci, [_vp, _ci]),
}

EXT_FUNCTIONS = {      # include/ssimu2_hip_ext.h: only liboavif_hip_ext.so has these
    "ssimu2_alpha_table": (_ci, [_f32p]),
    "ssimu2_composite_rgba8": (_ci, [_vp, _u8p, _u32, _u32, _u32, _u32, _u16p]),
    "ssimu2_score_rgba8": (_ci, [_vp, _u8p, _u32, _u8p, _u32, _u32, _u32, _u32, _f64p]),
    "ssimu2_set_reference_rgba8": (_ci, [_vp, _u8p, _u32, _u32, _u32, _u32]),
    "ssimu2_score_against_reference_rgba8": (_ci, [_vp, _u8p, _u32, _f64p]),
}

YUV_FUNCTIONS = {      # include/ssimu2_hip_yuv.h: only liboavif_hip_yuv.so has these
    "ssimu2_convert_yuv": (_ci, [_vp, _P(YuvFrameC), _u32, _u32, _u32, _u16p]),
    "ssimu2_score_yuv": (_ci, [_vp, _P(YuvFrameC), _P(YuvFrameC), _u32, _u32, _u32, _f64p]),
    "ssimu2_set_reference_yuv": (_ci, [_vp, _P(YuvFrameC), _u32, _u32, _u32]),
    "ssimu2_score_against_reference_yuv": (_ci, [_vp, _P(YuvFrameC), _u32, _f64p]),
}

MAP_FUNCTIONS = {      # include/ssimu2_hip_map.h: only liboavif_hip_map.so has these
    "ssimu2_error_map_rgb16": (_ci, [_vp, _u16p, _u16p, _u32, _u32, _u32, _f32p, _f64p]),
    "ssimu2_error_map_against_reference_rgb16": (_ci, [_vp, _u16p, _u32, _f32p, _f64p]),
    "ssimu2_error_map_rgba8": (_ci, [_vp, _u8p, _u32, _u8p, _u32, _u32, _u32, _u32, _f32p, _f64p]),
    "ssimu2_error_map_against_reference_rgba8": (_ci, [_vp, _u8p, _u32, _f32p, _f64p]),
    "ssimu2_error_map_yuv": (_ci, [_vp, _P(YuvFrameC), _P(YuvFrameC), _u32, _u32, _u32, _f32p, _f64p]),
    "ssimu2_error_map_against_reference_yuv": (_ci, [_vp, _P(YuvFrameC), _u32, _f32p, _f64p]),
}

CHROMA_FUNCTIONS = {   # include/ssimu2_hip_chroma.h: only liboavif_hip_chroma.so has these
    "ssimu2_convert_yuv_chroma": (_ci, [_vp, _P(YuvFrameC), _u32, _u32, _u32, _u32, _u16p]),
    "ssimu2_score_yuv_chroma": (_ci, [_vp, _P(YuvFrameC), _P(YuvFrameC), _u32, _u32, _u32, _u32, _f64p]),
    "ssimu2_set_reference_yuv_chroma": (_ci, [_vp, _P(YuvFrameC), _u32, _u32, _u32, _u32]),
    "ssimu2_score_against_reference_yuv_chroma": (_ci, [_vp, _P(YuvFrameC), _u32, _u32, _f64p]),
    "ssimu2_error_map_yuv_chroma": (_ci, [_vp, _P(YuvFrameC), _P(YuvFrameC), _u32, _u32, _u32, _u32, _f32p, _f64p]),
    "ssimu2_error_map_against_reference_yuv_chroma": (_ci, [_vp, _P(YuvFrameC), _u32, _u32, _f32p, _f64p]),
}

YUVA_FUNCTIONS = {     # include/ssimu2_hip_yuva.h: only liboavif_hip_yuva.so has these
    "ssimu2_composite_yuva": (_ci, [_vp, _P(YuvaFrameC), _u32, _u32, _u32, _u32, _u32, _u16p]),
    "ssimu2_score_yuva": (_ci, [_vp, _P(YuvaFrameC), _P(YuvaFrameC), _u32, _u32, _u32, _u32, _u32, _f64p]),
    "ssimu2_set_reference_yuva": (_ci, [_vp, _P(YuvaFrameC), _u32, _u32, _u32, _u32, _u32]),
    "ssimu2_score_against_reference_yuva": (_ci, [_vp, _P(YuvaFrameC), _u32, _u32, _f64p]),
    "ssimu2_error_map_yuva": (_ci, [_vp, _P(YuvaFrameC), _P(YuvaFrameC), _u32, _u32, _u32, _u32, _u32, _f32p, _f64p]),
    "ssimu2_error_map_against_reference_yuva": (_ci, [_vp, _P(YuvaFrameC), _u32, _u32, _f32p, _f64p]),
}

RBATCH_FUNCTIONS = {   # include/ssimu2_hip_rbatch.h: only liboavif_hip_rbatch.so has these
    "ssimu2_rbatch_score_rgb8": (_ci, [_vp, _u8pp, _u8pp, _u32, _u32, _u32, _f64p]),
    "ssimu2_rbatch_score_against_reference": (_ci, [_vp, _u8pp, _u32, _f64p]),
    "ssimu2_rbatch_score_rgb8_device": (_ci, [_vp, _vp, _vp, _sz, _u32, _u32, _u32, _f64p]),
    "ssimu2_rbatch_score_against_reference_device": (_ci, [_vp, _vp, _sz, _u32, _f64p]),
}

HBATCH_FUNCTIONS = {   # include/ssimu2_hip_hbatch.h: only liboavif_hip_hbatch.so has these
    "ssimu2_hbatch_score_rgb16": (_ci, [_vp, _u16pp, _u16pp, _u32, _u32, _u32, _u32, _f64p]),
    "ssimu2_hbatch_score_against_reference_rgb16": (_ci, [_vp, _u16pp, _u32, _u32, _f64p]),
    "ssimu2_hbatch_score_rgb16_device": (_ci, [_vp, _vp, _vp, _sz, _u32, _u32, _u32, _u32, _f64p]),
    "ssimu2_hbatch_score_against_reference_rgb16_device": (_ci, [_vp, _vp, _sz, _u32, _u32, _f64p]),
    "ssimu2_hbatch_score_against_reference_yuv": (_ci, [_vp, _P(YuvFrameC), _u32, _u32, _u32, _f64p]),
    "ssimu2_hbatch_convert_yuv": (_ci, [_vp, _P(YuvFrameC), _u32, _u32, _u32, _u32, _u32, _u16p]),
}

ABATCH_FUNCTIONS = {   # include/ssimu2_hip_abatch.h: only liboavif_hip_abatch.so has these
    "ssimu2_abatch_score_against_reference_yuva": (_ci, [_vp, _P(YuvaFrameC), _u32, _u32, _u32, _f64p]),
    "ssimu2_abatch_composite_yuva": (_ci, [_vp, _P(YuvaFrameC), _u32, _u32, _u32, _u32, _u32, _u32, _u16p]),
    "ssimu2_abatch_score_against_reference_rgba8": (_ci, [_vp, _u8pp, _u32, _u32, _f64p]),
    "ssimu2_abatch_score_rgba8": (_ci, [_vp, _u8pp, _u32, _u8pp, _u32, _u32, _u32, _u32, _u32, _f64p]),
    "ssimu2_abatch_composite_rgba8": (_ci, [_vp, _u8pp, _u32, _u32, _u32, _u32, _u32, _u16p]),
}

EXPORTED_SYMBOLS = tuple(PUBLIC_FUNCTIONS)
INSTR_SYMBOLS = tuple(HOOK_FUNCTIONS)
EXT_SYMBOLS = tuple(EXT_FUNCTIONS)
YUV_SYMBOLS = tuple(YUV_FUNCTIONS)
MAP_SYMBOLS = tuple(MAP_FUNCTIONS)
CHROMA_SYMBOLS = tuple(CHROMA_FUNCTIONS)
YUVA_SYMBOLS = tuple(YUVA_FUNCTIONS)
RBATCH_SYMBOLS = tuple(RBATCH_FUNCTIONS)
HBATCH_SYMBOLS = tuple(HBATCH_FUNCTIONS)
ABATCH_SYMBOLS = tuple(ABATCH_FUNCTIONS)

_lib = None
_instr = None
_ext = None
_yuv = None
_map = None
_chroma = None
_yuva = None
_rbatch = None
_hbatch = None
_abatch = None


def lib() -> ctypes.CDLL:
    """The product library (what a caller of the C ABI links)."""
    global _lib
    if _lib is None:
        _lib = _load(LIB_PATH)
    return _lib


def instr_lib() -> ctypes.CDLL:
    """The instrumented build (include/ssimu2_hip_internal.h); never used by the product path."""
    global _instr
    if _instr is None:
        _instr = _load(INSTR_LIB_PATH)
    return _instr


def ext_lib() -> ctypes.CDLL:
    """The extension build (include/ssimu2_hip_ext.h): every public function plus the RGBA entry points."""
    global _ext
    if _ext is None:
        _ext = _load(EXT_LIB_PATH)
    return _ext


def yuv_lib() -> ctypes.CDLL:
    """The YUV build (include/ssimu2_hip_yuv.h): the extension library plus the YUV entry points."""
    global _yuv
    if _yuv is None:
        _yuv = _load(YUV_LIB_PATH)
    return _yuv


def map_lib() -> ctypes.CDLL:
    """The map build (include/ssimu2_hip_map.h): the YUV library plus the error maps of 16-bit, RGBA and YUV frames."""
    global _map
    if _map is None:
        _map = _load(MAP_LIB_PATH)
    return _map


def chroma_lib() -> ctypes.CDLL:
    """The chroma build (include/ssimu2_hip_chroma.h): the map library plus the calls that take 4:2:2 and 4:2:0 frames."""
    global _chroma
    if _chroma is None:
        _chroma = _load(CHROMA_LIB_PATH)
    return _chroma


def yuva_lib() -> ctypes.CDLL:
    """The alpha-plane build (include/ssimu2_hip_yuva.h): the chroma library plus the calls that take Y, U, V and A planes."""
    global _yuva
    if _yuva is None:
        _yuva = _load(YUVA_LIB_PATH)
    return _yuva


def rbatch_lib() -> ctypes.CDLL:
    """The batch build (include/ssimu2_hip_rbatch.h): the alpha-plane library plus the batch calls of every blur mode."""
    global _rbatch
    if _rbatch is None:
        _rbatch = _load(RBATCH_LIB_PATH)
    return _rbatch


def hbatch_lib() -> ctypes.CDLL:
    """The 16-bit batch build (include/ssimu2_hip_hbatch.h): the batch library plus the batches of 16-bit and YUV frames."""
    global _hbatch
    if _hbatch is None:
        _hbatch = _load(HBATCH_LIB_PATH)
    return _hbatch


def abatch_lib() -> ctypes.CDLL:
    """The alpha batch build (include/ssimu2_hip_abatch.h): the 16-bit batch library plus the batches of RGBA and
    YUV-with-alpha frames."""
    global _abatch
    if _abatch is None:
        _abatch = _load(ABATCH_LIB_PATH)
    return _abatch


def _load(path: str) -> ctypes.CDLL:
    if not os.path.exists(path):
        raise ImportError(
            f"{path} is missing: build it with `python -m oavif_amd.build` "
            "(hipcc --offload-arch=gfx950). There is no CPU fallback for the scorer.")
    # PyTorch-ROCm bundles its own libamdhip64/libhsa-runtime64 (same SONAME as /opt/rocm's).
    # Whichever HIP runtime is loaded first serves the whole process, and torch cannot
    # initialise on top of a foreign one ("No HIP GPUs are available").  Python callers
    # share device memory and streams with torch, so let torch's runtime load first.
    if os.environ.get("OAVIF_AMD_NO_TORCH") != "1":
        try:
            import torch  # noqa: F401
        except Exception:
            pass
    L = ctypes.CDLL(path)
    for table in (PUBLIC_FUNCTIONS, HOOK_FUNCTIONS, EXT_FUNCTIONS, YUV_FUNCTIONS, MAP_FUNCTIONS, CHROMA_FUNCTIONS,
                  YUVA_FUNCTIONS, RBATCH_FUNCTIONS, HBATCH_FUNCTIONS, ABATCH_FUNCTIONS):
        for name, (restype, argtypes) in table.items():
            fn = getattr(L, name, None)   # a build older than a symbol lacks it (scripts/gpu_ab.py loads such builds)
            if fn is not None:
                fn.restype, fn.argtypes = restype, argtypes
    return L
