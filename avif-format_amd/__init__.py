"""ctypes binding of libavifgpu.so (C-ABI in include/avifgpu.h) for tests, smoke and bench.

This package is plumbing: the product is the C-ABI shared library built from csrc/ (hand-written
gfx950 HIP kernels + the C++ host shim).  Python never computes pixels here and there is no CPU
fallback: `load()` raises if the library is missing, and `AvifGpu()` raises if no HIP device binds.

The directory name contains a hyphen (it mirrors the reference repository's name), so import it
through `importlib` -- see `__graft_entry__.load_package()`.
"""
from __future__ import annotations

import ctypes
import os
import sys
from ctypes import POINTER, c_char_p, c_float, c_int32, c_int64, c_void_p

from . import sharding  # noqa: E402,F401  (row-tile partition used by bench.py / host shim tests)
from . import host  # noqa: E402,F401      (ctypes mirror of include/avifgpu_host.h)
from . import distrib  # noqa: E402,F401   (barrier + MAX-over-ranks for bench.py)

_HERE = os.path.dirname(os.path.abspath(__file__))
# AVIFGPU_LIB: developer switch for A/B-ing kernel builds (tools/ab_variants.sh); the product name is libavifgpu.so
LIB_PATH = os.environ.get("AVIFGPU_LIB") or os.path.join(_HERE, "libavifgpu.so")

# ---- enums (include/avifgpu.h) ----------------------------------------------------------------
TRANSFER_PQ, TRANSFER_HLG, TRANSFER_SMPTE428, TRANSFER_CLIP = 0, 1, 2, 3
ALPHA_NONE, ALPHA_STRAIGHT, ALPHA_PREMULTIPLIED = 0, 1, 2
COLORSPACE_YCBCR, COLORSPACE_RGB, COLORSPACE_MONOCHROME = 0, 1, 2
CHROMA_MONOCHROME, CHROMA_420, CHROMA_422, CHROMA_444 = 0, 1, 2, 3
MATRIX_RGB_GBR, MATRIX_BT709, MATRIX_UNSPECIFIED, MATRIX_FCC, MATRIX_BT470BG, MATRIX_BT601 = 0, 1, 2, 4, 5, 6
MATRIX_SMPTE240M, MATRIX_YCGCO, MATRIX_BT2020_NCL, MATRIX_BT2020_CL, MATRIX_CHROMA_DERIVED_NCL = 7, 8, 9, 10, 12
PRIMARIES_BT709, PRIMARIES_BT470M, PRIMARIES_BT470BG, PRIMARIES_BT601, PRIMARIES_BT2020 = 1, 4, 5, 6, 9
PRIMARIES_SMPTE432 = 12
TC_SRGB, TC_PQ, TC_SMPTE428, TC_HLG = 13, 16, 17, 18
OUT_REFERENCE, OUT_YCBCR = 0, 1
DOWNSAMPLE_AVERAGE, DOWNSAMPLE_NEAREST = 0, 1
CHROMA_ZERO_LIBHEIF, CHROMA_ZERO_DECODER = 0, 1
PQ_AUTO, PQ_COMPACT, PQ_CLOSE = 0, 1, 2
MEM_HOST, MEM_DEVICE = 0, 1
UPSAMPLE_NEAREST, UPSAMPLE_BILINEAR_CENTER, UPSAMPLE_BILINEAR_LEFT = 0, 1, 2
# AVIFGPU_ICC_KIND_*: which prepared structure the icc argument of avifgpu_write_rows_grid points to
ICC_KIND_NONE, ICC_KIND_TRANSFORM, ICC_KIND_SAMPLED, ICC_KIND_SHAPER8, ICC_KIND_CLUT16, ICC_KIND_CLUT8_TABLE, ICC_KIND_PIPELINE32 = range(7)

noErr, userCanceledErr, readErr, writErr, memFullErr = 0, -128, -19, -20, -108
formatBadParameters, formatCannotRead = -30500, -30501


class WriteDesc(ctypes.Structure):
    _fields_ = [(n, c_int32) for n in (
        "width", "height", "depth", "planes", "bit_depth", "transfer", "peak_nits", "alpha_state",
        "output", "chroma", "matrix_coefficients", "color_primaries", "full_range", "chroma_downsampling",
        "chroma_zero_point", "pq_evaluation")]

    def __init__(self, **kw):
        super().__init__()
        self.peak_nits = 80          # pqDefaultBrightness, reference AvifFormat.h:59
        self.transfer = TRANSFER_CLIP
        self.full_range = 1
        self.chroma = CHROMA_444
        self.matrix_coefficients = MATRIX_BT601
        self.color_primaries = PRIMARIES_BT709
        for k, v in kw.items():
            if not hasattr(self, k):
                raise AttributeError(k)
            setattr(self, k, v)


class ReadDesc(ctypes.Structure):
    _fields_ = [(n, c_int32) for n in (
        "width", "height", "colorspace", "chroma", "bit_depth", "depth", "alpha_state", "has_nclx",
        "color_primaries", "transfer_characteristics", "matrix_coefficients", "full_range_flag",
        "pq_peak_nits", "hlg_apply_ootf")]
    _fields_ += [("hlg_display_gamma", c_float), ("hlg_peak_nits", c_int32), ("reserved", c_int32 * 2)]

    def __init__(self, **kw):
        super().__init__()
        self.has_nclx = 1
        self.color_primaries = PRIMARIES_BT709
        self.transfer_characteristics = TC_SRGB
        self.matrix_coefficients = MATRIX_BT601
        self.full_range_flag = 1
        self.pq_peak_nits = 80
        self.hlg_apply_ootf = 0
        self.hlg_display_gamma = 1.2   # reference AvifFormat.cpp:96-98 defaults
        self.hlg_peak_nits = 1000
        for k, v in kw.items():
            if not hasattr(self, k):
                raise AttributeError(k)
            setattr(self, k, v)


class IccTransform(ctypes.Structure):
    _fields_ = [("trc_type", c_int32 * 3), ("out_curve", c_int32), ("trc_params", (ctypes.c_double * 7) * 3),
                ("matrix", ctypes.c_double * 9), ("out_params", ctypes.c_double * 8)]


ICC_TARGET_REC2020_LINEAR = 0
ICC_TARGET_SRGB_FLOAT = 2
ICC_IS_REC2020, ICC_IS_SRGB = 1, 2


class IccSampled32(ctypes.Structure):
    _fields_ = [("base", IccTransform), ("curve", (c_float * 65536) * 3), ("table16", (ctypes.c_uint16 * 4096) * 3),
                ("entries", c_int32 * 3), ("parametric_mask", c_int32)]


class IccClut16(ctypes.Structure):
    _fields_ = [("grid_points", c_int32), ("reserved", c_int32 * 3), ("table", (ctypes.c_uint16 * 4) * (33 * 33 * 33))]


class IccShaper8(ctypes.Structure):
    _fields_ = [("shaper1", (c_int32 * 256) * 3), ("matrix", (c_int32 * 3) * 3), ("offset", c_int32 * 3), ("reserved", c_int32),
                ("shaper2", (ctypes.c_uint8 * 16388) * 3)]


ICC_PIPE_MAX_STAGES, ICC_PIPE_MAX_CURVE, ICC_PIPE_MAX_GRID = 16, 4096, 33
ICC_PIPE_MAX_WORDS = 33 * 33 * 33 * 3 + 4 * 3 * 4096
ICC_STAGE_CURVES, ICC_STAGE_MATRIX, ICC_STAGE_CLUT16, ICC_STAGE_LAB_TO_XYZ, ICC_STAGE_XYZ_TO_LAB = 1, 2, 3, 4, 5


class IccStage32(ctypes.Structure):
    _fields_ = [("kind", c_int32), ("curve_type", c_int32 * 3), ("entries", c_int32 * 3), ("offset", c_int32 * 3),
                ("has_bias", c_int32), ("reserved", c_int32), ("params", (ctypes.c_double * 10) * 3),
                ("matrix", ctypes.c_double * 9), ("bias", ctypes.c_double * 3)]


class IccPipeline32(ctypes.Structure):
    """lcms2's float stage program of a 32-bit document behind a LUT-based profile (include/avifgpu.h, avifgpu_icc_pipeline32)."""
    _fields_ = [("target", c_int32), ("stage_count", c_int32), ("word_count", c_int32), ("reserved", c_int32),
                ("proof", ctypes.c_uint64), ("stages", IccStage32 * ICC_PIPE_MAX_STAGES),
                ("words", ctypes.c_uint16 * ICC_PIPE_MAX_WORDS)]


LCMS_BRIDGE_PATH = os.path.join(_HERE, "libavifgpu_lcms_bridge.so")


def lcms_bridge():
    """integration/LcmsTableBridge.cpp, built next to the library where lcms2.h exists (None otherwise).  It resolves avifgpu_*
    against the already loaded library."""
    if not os.path.exists(LCMS_BRIDGE_PATH):
        return None
    load()
    B = ctypes.CDLL(LCMS_BRIDGE_PATH)
    B.avifgpu_lcms_document_to_pipeline32.restype = c_int32
    B.avifgpu_lcms_document_to_pipeline32.argtypes = [c_void_p, ctypes.c_uint32, c_int32, c_int32, POINTER(IccPipeline32)]
    return B


def icc_pipeline32_from_profile(profile_bytes: bytes, target=ICC_TARGET_REC2020_LINEAR, has_alpha=False):
    """(OSErr, IccPipeline32): the proven stage program the adapter builds for a document profile (bridge above; None if absent)."""
    B = lcms_bridge()
    if B is None:
        return None
    t = IccPipeline32()
    rc = B.avifgpu_lcms_document_to_pipeline32(profile_bytes, len(profile_bytes), target, 1 if has_alpha else 0, ctypes.byref(t))
    return rc, t


class CropRect(ctypes.Structure):
    """avifgpu_rect: a rectangle in STORED image coordinates."""
    _fields_ = [("x0", c_int32), ("y0", c_int32), ("width", c_int32), ("height", c_int32)]

    def astuple(self):
        return (self.x0, self.y0, self.width, self.height)


class Grid(ctypes.Structure):
    """avifgpu_grid: columns x rows tiles of tile_width x tile_height, row-major."""
    _fields_ = [("columns", c_int32), ("rows", c_int32), ("tile_width", c_int32), ("tile_height", c_int32)]


class GridTile(ctypes.Structure):
    """avifgpu_grid_tile: the planes of one decoded tile (64 bytes)."""
    _fields_ = [("plane", c_void_p * 4), ("stride", c_int64 * 4)]


class ContentLightLevel(ctypes.Structure):
    """avifgpu_content_light_level: the clli fields and what they were rounded from."""
    _fields_ = [("max_cll", ctypes.c_uint16), ("max_fall", ctypes.c_uint16), ("max_code", c_int32), ("pixels", ctypes.c_uint64),
                ("max_cll_nits", ctypes.c_double), ("max_fall_nits", ctypes.c_double)]


class SaveSummary(ctypes.Structure):
    """avifgpu_save_summary: what the summary counters of a save say (avifgpu_summary_read)."""
    _fields_ = [("channels", c_int32), ("min_code", c_int32 * 4), ("max_code", c_int32 * 4), ("spread", c_int32),
                ("alpha_opaque", c_int32), ("alpha_clear", c_int32), ("neutral", c_int32), ("advice", c_int32)]


SUMMARY_COUNTERS = 16
ADVICE_DROP_ALPHA = 1
ADVICE_MONOCHROME = 2


class DeviceInfo(ctypes.Structure):
    _fields_ = [("device", c_int32), ("numa_node", c_int32), ("workers", c_int32), ("workers_pinned", c_int32),
                ("pci_bus_id", ctypes.c_char * 32), ("cpulist", ctypes.c_char * 256)]


class DeviceTraffic(ctypes.Structure):
    _fields_ = [("device", c_int32), ("copy_helper_pools", c_int32), ("tiles", ctypes.c_uint64), ("bytes_h2d", ctypes.c_uint64),
                ("bytes_d2h", ctypes.c_uint64), ("bytes_bounced", ctypes.c_uint64)]


Transform16Fn = ctypes.CFUNCTYPE(None, c_void_p, POINTER(ctypes.c_uint16), POINTER(ctypes.c_uint16), ctypes.c_uint32)
TransformF32Fn = ctypes.CFUNCTYPE(None, c_void_p, POINTER(ctypes.c_float), POINTER(ctypes.c_float), ctypes.c_uint32)

_PLANES4 = c_void_p * 4
_STRIDES4 = c_int64 * 4

# every symbol include/avifgpu.h declares: (name, restype, argtypes)
ABI = [
    ("avifgpu_abi_version", c_int32, []),
    ("avifgpu_init", c_int32, [c_int32]),
    ("avifgpu_init_devices", c_int32, [POINTER(c_int32), c_int32]),
    ("avifgpu_device_count", c_int32, []),
    ("avifgpu_shutdown", None, []),
    ("avifgpu_device_topology", c_int32, [c_int32, POINTER(DeviceInfo)]),
    ("avifgpu_device_traffic_get", c_int32, [c_int32, POINTER(DeviceTraffic)]),
    ("avifgpu_device_traffic_reset", c_int32, []),
    ("avifgpu_topology_plan", c_int32, [c_char_p, POINTER(c_char_p), c_int32, POINTER(DeviceInfo)]),
    ("avifgpu_topology_probe", c_int32, [c_char_p, c_char_p, POINTER(c_int32), ctypes.c_char_p, c_int32]),
    ("avifgpu_last_error", c_char_p, []),
    ("avifgpu_write_rows", c_int32, [POINTER(WriteDesc), c_int32, c_int32, c_void_p, c_int64,
                                     POINTER(_PLANES4), POINTER(_STRIDES4), c_int32, c_void_p]),
    ("avifgpu_read_rows", c_int32, [POINTER(ReadDesc), c_int32, c_int32, POINTER(_PLANES4), POINTER(_STRIDES4),
                                    c_void_p, c_int64, c_int32, c_void_p]),
    ("avifgpu_icc_prepare", c_int32, [c_void_p, ctypes.c_uint32, c_int32, POINTER(IccTransform)]),
    ("avifgpu_write_rows_icc", c_int32, [POINTER(WriteDesc), POINTER(IccTransform), c_int32, c_int32, c_void_p, c_int64,
                                         POINTER(_PLANES4), POINTER(_STRIDES4), c_int32, c_void_p]),
    ("avifgpu_icc_prepare_sampled", c_int32, [c_void_p, ctypes.c_uint32, c_int32, POINTER(IccSampled32)]),
    ("avifgpu_write_rows_icc_sampled", c_int32, [POINTER(WriteDesc), POINTER(IccSampled32), c_int32, c_int32, c_void_p, c_int64,
                                                 POINTER(_PLANES4), POINTER(_STRIDES4), c_int32, c_void_p]),
    ("avifgpu_icc_detect", c_int32, [c_void_p, ctypes.c_uint32]),
    ("avifgpu_icc_prepare_clut16", c_int32, [c_void_p, ctypes.c_uint32, POINTER(IccClut16)]),
    ("avifgpu_icc_clut16_from_transforms", c_int32, [c_void_p, c_void_p, c_void_p, POINTER(IccClut16)]),
    ("avifgpu_write_rows_icc16", c_int32, [POINTER(WriteDesc), POINTER(IccClut16), c_int32, c_int32, c_void_p, c_int64,
                                           POINTER(_PLANES4), POINTER(_STRIDES4), c_int32, c_void_p]),
    ("avifgpu_icc_clut8_from_transforms", c_int32, [c_void_p, c_void_p, c_void_p, POINTER(IccClut16)]),
    ("avifgpu_write_rows_icc8_table", c_int32, [POINTER(WriteDesc), POINTER(IccClut16), c_int32, c_int32, c_void_p, c_int64,
                                                POINTER(_PLANES4), POINTER(_STRIDES4), c_int32, c_void_p]),
    ("avifgpu_icc_prepare_shaper8", c_int32, [c_void_p, ctypes.c_uint32, POINTER(IccShaper8)]),
    ("avifgpu_write_rows_icc8", c_int32, [POINTER(WriteDesc), POINTER(IccShaper8), c_int32, c_int32, c_void_p, c_int64,
                                          POINTER(_PLANES4), POINTER(_STRIDES4), c_int32, c_void_p]),
    ("avifgpu_icc_pipeline32_prove", c_int32, [POINTER(IccPipeline32), c_void_p, c_void_p]),
    ("avifgpu_icc_pipeline32_eval", c_int32, [POINTER(IccPipeline32), c_void_p, c_void_p, ctypes.c_uint32]),
    ("avifgpu_write_rows_icc_pipeline32", c_int32, [POINTER(WriteDesc), POINTER(IccPipeline32), c_int32, c_int32, c_void_p, c_int64,
                                                    POINTER(_PLANES4), POINTER(_STRIDES4), c_int32, c_void_p]),
    ("avifgpu_get_yuv_coefficients", c_int32, [c_int32, c_int32, c_int32, POINTER(c_float * 3)]),
    ("avifgpu_read_max_value", c_int32, [POINTER(ReadDesc)]),
    ("avifgpu_write_plane_count", c_int32, [POINTER(WriteDesc)]),
    ("avifgpu_write_plane_geometry", c_int32, [POINTER(WriteDesc), c_int32, POINTER(c_int32), POINTER(c_int32),
                                               POINTER(c_int32), POINTER(c_int32)]),
    ("avifgpu_write_algorithmic_bytes", c_int64, [POINTER(WriteDesc), c_int32]),
    ("avifgpu_read_algorithmic_bytes", c_int64, [POINTER(ReadDesc), c_int32]),
    ("avifgpu_last_kernel_name", c_char_p, []),
    ("avifgpu_set_hot_variant", None, [c_int32]),
    ("avifgpu_probe_pattern_read", c_int32, [POINTER(ReadDesc), c_int32, c_int32, POINTER(_PLANES4), POINTER(_STRIDES4), c_void_p, c_int64, c_void_p]),
    ("avifgpu_probe_set_shape", None, [c_int32, c_int32, c_int32]),
    ("avifgpu_probe_pattern_rgb32_444", c_int32, [c_void_p, c_int64, POINTER(c_void_p * 3), POINTER(c_int64 * 3), c_int32, c_int32, c_void_p]),
    ("avifgpu_histogram_attach", c_int32, [c_void_p, c_int32, c_int32]),
    ("avifgpu_light_level_from_histogram", c_int32, [c_void_p, c_int32, c_int32, ctypes.c_double, POINTER(ContentLightLevel)]),
    ("avifgpu_probe_histogram", c_int32, [POINTER(WriteDesc), c_int32, c_void_p, c_int64, c_void_p, c_void_p]),
    ("avifgpu_thumbnail_attach", c_int32, [c_void_p, c_int32, c_int32, c_int32]),
    ("avifgpu_thumbnail_fit", c_int32, [POINTER(WriteDesc), c_int32, POINTER(c_int32), POINTER(c_int32)]),
    ("avifgpu_thumbnail_from_sums", c_int32, [POINTER(WriteDesc), c_int32, c_int32, c_void_p, POINTER(_PLANES4), POINTER(_STRIDES4)]),
    ("avifgpu_probe_thumbnail", c_int32, [POINTER(WriteDesc), c_int32, c_int32, c_int32, POINTER(_PLANES4), POINTER(_STRIDES4), c_void_p, c_void_p]),
    ("avifgpu_summary_attach", c_int32, [c_void_p, c_int32]),
    ("avifgpu_summary_read", c_int32, [POINTER(WriteDesc), c_void_p, POINTER(SaveSummary)]),
    ("avifgpu_summary_merge", c_int32, [c_void_p, c_void_p]),
    ("avifgpu_probe_summary", c_int32, [POINTER(WriteDesc), c_int32, POINTER(_PLANES4), POINTER(_STRIDES4), c_void_p, c_void_p]),
    ("avifgpu_orientation_compose", c_int32, [c_int32, c_int32]),
    ("avifgpu_read_oriented_geometry", c_int32, [POINTER(ReadDesc), c_int32, POINTER(c_int32), POINTER(c_int32)]),
    ("avifgpu_read_oriented_next_tile", c_int32, [POINTER(ReadDesc), c_int32, c_int32, c_int32]),
    ("avifgpu_read_oriented_scratch_bytes", c_int64, [POINTER(ReadDesc), c_int32, c_int32]),
    ("avifgpu_read_rows_oriented", c_int32, [POINTER(ReadDesc), c_int32, c_int32, c_int32, POINTER(_PLANES4), POINTER(_STRIDES4),
                                             c_void_p, c_int64, c_void_p, c_int64, c_int32, c_void_p]),
    ("avifgpu_probe_orient", c_int32, [c_int32, c_int32, c_int32, c_int32, c_void_p, c_int64, c_void_p, c_int64, c_void_p]),
    ("avifgpu_read_upsampled_scratch_bytes", c_int64, [POINTER(ReadDesc), c_int32, c_int32, c_int32]),
    ("avifgpu_read_rows_upsampled", c_int32, [POINTER(ReadDesc), c_int32, c_int32, c_int32, c_int32, POINTER(_PLANES4), POINTER(_STRIDES4),
                                              c_void_p, c_int64, c_void_p, c_int64, c_int32, c_void_p]),
    ("avifgpu_probe_upsample", c_int32, [c_int32, c_int32, c_int32, c_int32, c_int32, c_int32, c_int32, c_int32, c_int32,
                                         POINTER(c_void_p * 2), POINTER(c_int64 * 2), POINTER(c_void_p * 2), c_int64, c_int32, c_void_p]),
    ("avifgpu_clap_to_rect", c_int32, [c_int32, c_int32, POINTER(c_int32 * 8), POINTER(CropRect)]),
    ("avifgpu_crop_compose", c_int32, [POINTER(CropRect), c_int32, POINTER(CropRect), POINTER(CropRect)]),
    ("avifgpu_read_cropped_geometry", c_int32, [POINTER(ReadDesc), POINTER(CropRect), c_int32, POINTER(c_int32), POINTER(c_int32)]),
    ("avifgpu_read_cropped_next_tile", c_int32, [POINTER(ReadDesc), POINTER(CropRect), c_int32, c_int32, c_int32, c_int32]),
    ("avifgpu_read_cropped_scratch_bytes", c_int64, [POINTER(ReadDesc), POINTER(CropRect), c_int32, c_int32, c_int32]),
    ("avifgpu_read_rows_cropped", c_int32, [POINTER(ReadDesc), POINTER(CropRect), c_int32, c_int32, c_int32, c_int32, POINTER(_PLANES4), POINTER(_STRIDES4),
                                            c_void_p, c_int64, c_void_p, c_int64, c_int32, c_void_p]),
    ("avifgpu_probe_crop", c_int32, [c_void_p, c_int64, c_void_p, c_int64, c_int64, c_int32, c_void_p]),
    ("avifgpu_grid_parse", c_int32, [c_void_p, c_int64, POINTER(c_int32), POINTER(c_int32), POINTER(c_int32), POINTER(c_int32)]),
    ("avifgpu_grid_check", c_int32, [POINTER(ReadDesc), POINTER(Grid)]),
    ("avifgpu_read_grid_scratch_bytes", c_int64, [POINTER(ReadDesc), POINTER(Grid), POINTER(CropRect), c_int32, c_int32, c_int32]),
    ("avifgpu_read_rows_grid", c_int32, [POINTER(ReadDesc), POINTER(Grid), c_void_p, POINTER(CropRect), c_int32, c_int32, c_int32, c_int32,
                                         c_void_p, c_int64, c_void_p, c_int64, c_int32, c_void_p]),
    ("avifgpu_probe_grid_gather", c_int32, [c_void_p, c_int32, c_int32, c_int32, c_int32, c_int32, c_int32, c_int32, c_int32, c_int32,
                                            c_void_p, c_int64, c_void_p]),
    ("avifgpu_write_grid_check", c_int32, [POINTER(WriteDesc), POINTER(Grid)]),
    ("avifgpu_write_grid_scratch_bytes", c_int64, [POINTER(WriteDesc), c_int32]),
    ("avifgpu_grid_fit", c_int32, [POINTER(WriteDesc), c_int32, c_int32, c_int32, POINTER(Grid)]),
    ("avifgpu_grid_payload", c_int32, [POINTER(Grid), c_int32, c_int32, c_void_p, c_int64]),
    ("avifgpu_write_rows_grid", c_int32, [POINTER(WriteDesc), c_int32, c_void_p, POINTER(Grid), c_void_p, c_int32, c_int32, c_void_p, c_int64,
                                          c_void_p, c_int64, c_int32, c_void_p]),
    ("avifgpu_probe_grid_scatter", c_int32, [c_void_p, c_int32, c_int32, c_int32, c_int32, c_int32, c_int32, c_int32, c_int32, c_int32,
                                             c_void_p, c_int64, c_void_p]),
]


# Entry points that a library of an OLDER round may lack (they arrived with ABI 4, rounds 3-4).  Only these may be missing, only when the
# developer asks for it (AVIFGPU_AB_OLD_LIB=1, the A/B of tools/gpu/ab_libs.sh against e.g. variants/libavifgpu_r03.so), and every skip is
# reported: a stale or wrong AVIFGPU_LIB must fail HERE, at bind time, not later with an AttributeError or a call without argtypes.
ABI4_NEW = frozenset(("avifgpu_probe_pattern_read", "avifgpu_probe_pattern_rgb32_444", "avifgpu_device_traffic_get", "avifgpu_device_traffic_reset",
                      "avifgpu_topology_plan", "avifgpu_icc_prepare_sampled", "avifgpu_write_rows_icc_sampled",
                      "avifgpu_icc_clut16_from_transforms",
                      "avifgpu_icc_clut8_from_transforms", "avifgpu_write_rows_icc8_table", "avifgpu_probe_set_shape",        # (ABI 5, round 6)
                      "avifgpu_histogram_attach", "avifgpu_light_level_from_histogram", "avifgpu_probe_histogram",
                      "avifgpu_host_save_wants_light_level",    # (the code histogram)
                      "avifgpu_thumbnail_attach", "avifgpu_thumbnail_fit", "avifgpu_thumbnail_from_sums", "avifgpu_probe_thumbnail",   # (the thumbnail)
                      "avifgpu_summary_attach", "avifgpu_summary_read", "avifgpu_summary_merge", "avifgpu_probe_summary",   # (the summary of a save)
                      "avifgpu_orientation_compose", "avifgpu_read_oriented_geometry", "avifgpu_read_oriented_next_tile",
                      "avifgpu_read_oriented_scratch_bytes", "avifgpu_read_rows_oriented", "avifgpu_probe_orient",
                      "avifgpu_host_read_heif_image_oriented",    # (the oriented open)
                      "avifgpu_read_upsampled_scratch_bytes", "avifgpu_read_rows_upsampled", "avifgpu_probe_upsample",
                      "avifgpu_host_read_heif_image_upsampled",   # (the upsampled open)
                      "avifgpu_clap_to_rect", "avifgpu_crop_compose", "avifgpu_read_cropped_geometry", "avifgpu_read_cropped_next_tile",
                      "avifgpu_read_cropped_scratch_bytes", "avifgpu_read_rows_cropped", "avifgpu_probe_crop",
                      "avifgpu_host_read_heif_image_cropped",   # (the cropped open)
                      "avifgpu_grid_parse", "avifgpu_grid_check", "avifgpu_read_grid_scratch_bytes", "avifgpu_read_rows_grid",
                      "avifgpu_probe_grid_gather", "avifgpu_host_read_heif_image_grid",   # (the grid open)
                      "avifgpu_write_grid_check", "avifgpu_write_grid_scratch_bytes", "avifgpu_grid_fit", "avifgpu_grid_payload",
                      "avifgpu_write_rows_grid", "avifgpu_probe_grid_scatter", "avifgpu_host_create_heif_image_grid"))   # (the grid save)


def bind(lib: ctypes.CDLL, table=ABI) -> ctypes.CDLL:
    skipped = []
    for name, res, args in table:
        try:
            fn = getattr(lib, name)    # AttributeError if the symbol is not exported
        except AttributeError:
            if os.environ.get("AVIFGPU_AB_OLD_LIB") == "1" and os.environ.get("AVIFGPU_LIB") and name in ABI4_NEW:
                skipped.append(name)
                continue
            raise
        fn.restype = res
        fn.argtypes = args
    if skipped:
        sys.stderr.write("avif-format_amd: AVIFGPU_AB_OLD_LIB=1: %s lacks %s\n" % (os.environ.get("AVIFGPU_LIB"), ", ".join(skipped)))
    return lib


_lib = None


def load() -> ctypes.CDLL:
    """Load libavifgpu.so (built in-tree by `make -C avif-format_amd`).  Fails loudly if absent."""
    global _lib
    if _lib is None:
        # PyTorch-ROCm wheels bundle their own libamdhip64 (same SONAME as /opt/rocm's).  Whichever copy is loaded
        # first serves the whole process, and torch cannot initialise on top of the system copy -- so when torch is
        # installed, let it load its runtime before libavifgpu.so pulls one in.  (torch is plumbing here: device
        # memory + streams for tests and bench; the library itself does not depend on it.)
        try:
            import torch  # noqa: F401
        except ImportError:
            pass
        if not os.path.exists(LIB_PATH):
            raise RuntimeError(
                f"{LIB_PATH} is missing: build it with `python -c 'import __graft_entry__ as g; g.build()'` "
                "or `make -C avif-format_amd`.  There is no CPU fallback.")
        _lib = bind(bind(ctypes.CDLL(LIB_PATH)), host.HOST_ABI)
    return _lib


class AvifGpuError(RuntimeError):
    def __init__(self, code: int, message: str):
        super().__init__(f"OSErr {code}: {message}")
        self.code = code
        self.message = message


def planes4(ptrs):
    arr = _PLANES4()
    for i in range(4):
        arr[i] = ptrs[i] if i < len(ptrs) and ptrs[i] else None
    return arr


def strides4(vals):
    arr = _STRIDES4()
    for i in range(4):
        arr[i] = int(vals[i]) if i < len(vals) and vals[i] else 0
    return arr


class AvifGpu:
    """One bound device.  Thin wrapper: raises AvifGpuError on any non-zero OSErr."""

    def __init__(self, device: int = 0, devices=None):
        """Bind `device`, or the list `devices` (one context per entry; an ordinal may repeat: N contexts on one GPU)."""
        self.lib = load()
        devs = [int(device)] if devices is None else [int(x) for x in devices]
        arr = (c_int32 * len(devs))(*devs)
        code = self.lib.avifgpu_init_devices(arr, len(devs))
        if code != 0:
            raise AvifGpuError(code, self.lib.avifgpu_last_error().decode())
        self.device = devs[0]
        self.devices = devs

    def _check(self, code):
        if code != 0:
            raise AvifGpuError(code, self.lib.avifgpu_last_error().decode())

    def write_rows(self, desc: WriteDesc, row0, nrows, src_ptr, src_row_bytes, dst_ptrs, dst_strides,
                   mem=MEM_DEVICE, stream=0, icc=None):
        if isinstance(icc, IccClut16) and desc.depth == 8:          # an 8-bit document behind a LUT-based profile: the same table, PrelinEval8's evaluation
            self._check(self.lib.avifgpu_write_rows_icc8_table(ctypes.byref(desc), ctypes.byref(icc), row0, nrows, src_ptr, src_row_bytes,
                                                               ctypes.byref(planes4(dst_ptrs)), ctypes.byref(strides4(dst_strides)),
                                                               mem, stream or None))
            return
        if isinstance(icc, IccClut16):
            self._check(self.lib.avifgpu_write_rows_icc16(ctypes.byref(desc), ctypes.byref(icc), row0, nrows, src_ptr, src_row_bytes,
                                                          ctypes.byref(planes4(dst_ptrs)), ctypes.byref(strides4(dst_strides)),
                                                          mem, stream or None))
            return
        if isinstance(icc, IccPipeline32):
            self._check(self.lib.avifgpu_write_rows_icc_pipeline32(ctypes.byref(desc), ctypes.byref(icc), row0, nrows, src_ptr, src_row_bytes,
                                                                   ctypes.byref(planes4(dst_ptrs)), ctypes.byref(strides4(dst_strides)),
                                                                   mem, stream or None))
            return
        if isinstance(icc, IccSampled32):
            self._check(self.lib.avifgpu_write_rows_icc_sampled(ctypes.byref(desc), ctypes.byref(icc), row0, nrows, src_ptr, src_row_bytes,
                                                                ctypes.byref(planes4(dst_ptrs)), ctypes.byref(strides4(dst_strides)),
                                                                mem, stream or None))
            return
        if isinstance(icc, IccShaper8):
            self._check(self.lib.avifgpu_write_rows_icc8(ctypes.byref(desc), ctypes.byref(icc), row0, nrows, src_ptr, src_row_bytes,
                                                         ctypes.byref(planes4(dst_ptrs)), ctypes.byref(strides4(dst_strides)),
                                                         mem, stream or None))
            return
        if icc is not None:
            self._check(self.lib.avifgpu_write_rows_icc(ctypes.byref(desc), ctypes.byref(icc), row0, nrows, src_ptr, src_row_bytes,
                                                        ctypes.byref(planes4(dst_ptrs)), ctypes.byref(strides4(dst_strides)),
                                                        mem, stream or None))
            return
        self._check(self.lib.avifgpu_write_rows(ctypes.byref(desc), row0, nrows, src_ptr, src_row_bytes,
                                                ctypes.byref(planes4(dst_ptrs)), ctypes.byref(strides4(dst_strides)),
                                                mem, stream or None))

    def icc_prepare_clut16(self, profile_bytes: bytes) -> "IccClut16":
        t = IccClut16()
        self._check(self.lib.avifgpu_icc_prepare_clut16(profile_bytes, len(profile_bytes), ctypes.byref(t)))
        return t

    def icc_prepare_shaper8(self, profile_bytes: bytes) -> "IccShaper8":
        t = IccShaper8()
        self._check(self.lib.avifgpu_icc_prepare_shaper8(profile_bytes, len(profile_bytes), ctypes.byref(t)))
        return t

    def icc_prepare_sampled(self, profile_bytes: bytes, target=ICC_TARGET_REC2020_LINEAR) -> "IccSampled32":
        t = IccSampled32()
        self._check(self.lib.avifgpu_icc_prepare_sampled(profile_bytes, len(profile_bytes), target, ctypes.byref(t)))
        return t

    def icc_prepare(self, profile_bytes: bytes, target=ICC_TARGET_REC2020_LINEAR) -> "IccTransform":
        t = IccTransform()
        self._check(self.lib.avifgpu_icc_prepare(profile_bytes, len(profile_bytes), target, ctypes.byref(t)))
        return t

    def read_rows(self, desc: ReadDesc, row0, nrows, src_ptrs, src_strides, dst_ptr, dst_row_bytes,
                  mem=MEM_DEVICE, stream=0):
        self._check(self.lib.avifgpu_read_rows(ctypes.byref(desc), row0, nrows,
                                               ctypes.byref(planes4(src_ptrs)), ctypes.byref(strides4(src_strides)),
                                               dst_ptr, dst_row_bytes, mem, stream or None))

    def read_rows_oriented(self, desc: ReadDesc, orientation, orow0, onrows, src_ptrs, src_strides, dst_ptr, dst_row_bytes,
                           scratch_ptr=None, scratch_bytes=0, mem=MEM_DEVICE, stream=0):
        """Output rows [orow0, orow0 + onrows) of the oriented open (avifgpu_read_rows_oriented): src_ptrs are the WHOLE image's planes."""
        self._check(self.lib.avifgpu_read_rows_oriented(ctypes.byref(desc), orientation, orow0, onrows,
                                                        ctypes.byref(planes4(src_ptrs)), ctypes.byref(strides4(src_strides)),
                                                        dst_ptr, dst_row_bytes, scratch_ptr or None, scratch_bytes, mem, stream or None))

    def read_rows_upsampled(self, desc: ReadDesc, upsampling, orientation, orow0, onrows, src_ptrs, src_strides, dst_ptr, dst_row_bytes,
                            scratch_ptr=None, scratch_bytes=0, mem=MEM_DEVICE, stream=0):
        """Output rows [orow0, orow0 + onrows) of the (oriented) open with interpolated chroma (avifgpu_read_rows_upsampled): src_ptrs are
        the WHOLE image's planes."""
        self._check(self.lib.avifgpu_read_rows_upsampled(ctypes.byref(desc), upsampling, orientation, orow0, onrows,
                                                         ctypes.byref(planes4(src_ptrs)), ctypes.byref(strides4(src_strides)),
                                                         dst_ptr, dst_row_bytes, scratch_ptr or None, scratch_bytes, mem, stream or None))

    def read_rows_cropped(self, desc: ReadDesc, rect, upsampling, orientation, orow0, onrows, src_ptrs, src_strides, dst_ptr, dst_row_bytes,
                          scratch_ptr=None, scratch_bytes=0, mem=MEM_DEVICE, stream=0):
        """Output rows [orow0, orow0 + onrows) of the cropped (upsampled, oriented) open (avifgpu_read_rows_cropped): rect is (x0, y0, w, h) in
        the stored image, src_ptrs are the WHOLE image's planes."""
        self._check(self.lib.avifgpu_read_rows_cropped(ctypes.byref(desc), ctypes.byref(crop_rect(rect)), upsampling, orientation, orow0, onrows,
                                                       ctypes.byref(planes4(src_ptrs)), ctypes.byref(strides4(src_strides)),
                                                       dst_ptr, dst_row_bytes, scratch_ptr or None, scratch_bytes, mem, stream or None))

    def read_rows_grid(self, desc: ReadDesc, grid, tiles, rect, upsampling, orientation, orow0, onrows, dst_ptr, dst_row_bytes,
                       scratch_ptr=None, scratch_bytes=0, mem=MEM_DEVICE, stream=0):
        """Output rows [orow0, orow0 + onrows) of the cropped (upsampled, oriented) open of a grid image (avifgpu_read_rows_grid): tiles is
        the address of columns * rows GridTile records where `mem` says (or a ctypes array of them for MEM_HOST); rect None: the whole canvas."""
        if isinstance(tiles, ctypes.Array):
            tiles = ctypes.addressof(tiles)
        self._check(self.lib.avifgpu_read_rows_grid(ctypes.byref(desc), ctypes.byref(grid_of(grid)), tiles or None,
                                                    ctypes.byref(crop_rect(rect)) if rect is not None else None, upsampling, orientation, orow0, onrows,
                                                    dst_ptr, dst_row_bytes, scratch_ptr or None, scratch_bytes, mem, stream or None))

    def probe_grid_gather(self, tiles_dev, columns, plane, tile_w, tile_h, bytes_per_sample, x0, y0, w, h, dst, dst_row_bytes, stream=None):
        """Launch the grid gather kernel alone on one plane (avifgpu_probe_grid_gather)."""
        self._check(self.lib.avifgpu_probe_grid_gather(tiles_dev, columns, plane, tile_w, tile_h, bytes_per_sample, x0, y0, w, h, dst, dst_row_bytes, stream))

    def write_rows_grid(self, desc: WriteDesc, grid, tiles, row0, nrows, src_ptr, src_row_bytes, scratch_ptr=None, scratch_bytes=0,
                        mem=MEM_DEVICE, stream=0, icc=None):
        """Save rows [row0, row0 + nrows) into the padded tiles of a grid (avifgpu_write_rows_grid): tiles is the address of columns * rows
        GridTile records where `mem` says (or a ctypes array of them for MEM_HOST); icc: a prepared ICC structure or None."""
        if isinstance(tiles, ctypes.Array):
            tiles = ctypes.addressof(tiles)
        self._check(self.lib.avifgpu_write_rows_grid(ctypes.byref(desc), icc_kind_of(icc, desc), ctypes.byref(icc) if icc is not None else None,
                                                     ctypes.byref(grid_of(grid)), tiles or None, row0, nrows, src_ptr, src_row_bytes,
                                                     scratch_ptr or None, scratch_bytes, mem, stream or None))

    def probe_grid_scatter(self, tiles_dev, columns, plane, tile_w, tile_h, bytes_per_pixel, plane_w, plane_h, y0, h, src, src_row_bytes, stream=None):
        """Launch the grid scatter kernel alone on one plane (avifgpu_probe_grid_scatter)."""
        self._check(self.lib.avifgpu_probe_grid_scatter(tiles_dev, columns, plane, tile_w, tile_h, bytes_per_pixel, plane_w, plane_h, y0, h, src, src_row_bytes, stream))

    def probe_crop(self, src, src_row_bytes, dst, dst_row_bytes, row_payload_bytes, rows, stream=None):
        """Launch the crop mover kernel alone on device buffers (avifgpu_probe_crop)."""
        self._check(self.lib.avifgpu_probe_crop(src, src_row_bytes, dst, dst_row_bytes, row_payload_bytes, rows, stream))

    def probe_upsample(self, bytes_per_sample, chroma, upsampling, width, height, x0, y0, w, h, src, src_strides, dst, dst_row_bytes, stream=None, twin=0):
        """Launch the chroma upsample kernel alone on device buffers (avifgpu_probe_upsample): src / dst are (Cb, Cr) pointer pairs; twin 1 / 2: its store-only / math-free twin."""
        self._check(self.lib.avifgpu_probe_upsample(bytes_per_sample, chroma, upsampling, width, height, x0, y0, w, h,
                                                    ctypes.byref((c_void_p * 2)(*src)), ctypes.byref((c_int64 * 2)(*src_strides)),
                                                    ctypes.byref((c_void_p * 2)(*dst)), dst_row_bytes, twin, stream))

    def probe_orient(self, orientation, bytes_per_pixel, width, height, src, src_row_bytes, dst, dst_row_bytes, stream=None):
        """Launch the orient kernel alone on device buffers (avifgpu_probe_orient)."""
        self._check(self.lib.avifgpu_probe_orient(orientation, bytes_per_pixel, width, height, src, src_row_bytes, dst, dst_row_bytes, stream))

    def topology(self):
        """[{device, pci_bus_id, numa_node, cpulist, workers, workers_pinned}] of the bound devices (avifgpu_device_topology)."""
        out = []
        for i in range(64):
            info = DeviceInfo()
            if self.lib.avifgpu_device_topology(i, ctypes.byref(info)) != 0:
                break
            out.append({"device": info.device, "pci_bus_id": info.pci_bus_id.decode(), "numa_node": info.numa_node,
                        "cpulist": info.cpulist.decode(), "workers": info.workers, "workers_pinned": bool(info.workers_pinned)})
        return out

    def probe_pattern_read(self, desc, row0, nrows, ptrs, strides, dst, dst_row_bytes, stream=None):
        """Launch the math-free twin of the read kernel of `desc` on device buffers (avifgpu_probe_pattern_read)."""
        self._check(self.lib.avifgpu_probe_pattern_read(ctypes.byref(desc), row0, nrows, ctypes.byref(planes4(ptrs)), ctypes.byref(strides4(strides)),
                                                        dst, dst_row_bytes, stream))

    def traffic(self, reset=False):
        """[{device, tiles, bytes_h2d, bytes_d2h, bytes_bounced, copy_helper_pools}] per bound device (avifgpu_device_traffic_get)."""
        out = []
        for i in range(64):
            t = DeviceTraffic()
            if self.lib.avifgpu_device_traffic_get(i, ctypes.byref(t)) != 0:
                break
            out.append({"device": t.device, "tiles": t.tiles, "bytes_h2d": t.bytes_h2d, "bytes_d2h": t.bytes_d2h,
                        "bytes_bounced": t.bytes_bounced, "copy_helper_pools": t.copy_helper_pools})
        if reset:
            self.lib.avifgpu_device_traffic_reset()
        return out

    def last_kernel(self) -> str:
        return self.lib.avifgpu_last_kernel_name().decode()

    def write_plane_geometry(self, desc: WriteDesc, plane: int):
        w, h, b, s = c_int32(), c_int32(), c_int32(), c_int32()
        self._check(self.lib.avifgpu_write_plane_geometry(ctypes.byref(desc), plane, ctypes.byref(w), ctypes.byref(h),
                                                          ctypes.byref(b), ctypes.byref(s)))
        return w.value, h.value, b.value, s.value

    def write_algorithmic_bytes(self, desc: WriteDesc, nrows: int) -> int:
        return self.lib.avifgpu_write_algorithmic_bytes(ctypes.byref(desc), nrows)

    def read_algorithmic_bytes(self, desc: ReadDesc, nrows: int) -> int:
        return self.lib.avifgpu_read_algorithmic_bytes(ctypes.byref(desc), nrows)


class code_histogram:
    """Arm the calling thread's code histogram for the `with` block, disarm it on the way out (avifgpu_histogram_attach).

    `bins` holds 1 << bit_depth 64-bit counters and is never zeroed by the library: a numpy uint64 array (mem = MEM_HOST), a
    contiguous torch int64 / uint64 tensor on the device the calls run on (mem = MEM_DEVICE), or a raw address."""

    def __init__(self, bins, bit_depth: int, mem=MEM_HOST):
        self.bins, self.bit_depth, self.mem = bins, int(bit_depth), mem

    def _address(self):
        b = self.bins
        if hasattr(b, "data_ptr"):
            n, ptr = b.numel(), b.data_ptr()
            if b.element_size() != 8 or not b.is_contiguous():
                raise ValueError("code_histogram: bins must be contiguous 64-bit counters")
        elif hasattr(b, "ctypes"):
            n, ptr = b.size, b.ctypes.data
            if b.dtype.itemsize != 8 or not b.flags["C_CONTIGUOUS"]:
                raise ValueError("code_histogram: bins must be contiguous 64-bit counters")
        else:
            return int(b)
        if n < (1 << self.bit_depth):
            raise ValueError("code_histogram: %d bins for %d-bit codes" % (n, self.bit_depth))
        return ptr

    def __enter__(self):
        lib = load()
        code = lib.avifgpu_histogram_attach(self._address(), self.bit_depth, self.mem)
        if code != 0:
            raise AvifGpuError(code, lib.avifgpu_last_error().decode())
        return self

    def __exit__(self, *exc):
        load().avifgpu_histogram_attach(None, 0, MEM_HOST)
        return False


def light_level_from_histogram(bins, bit_depth: int, transfer=TRANSFER_PQ, percentile: float = 1.0) -> ContentLightLevel:
    """MaxCLL / MaxFALL of a host histogram (numpy uint64 array of 1 << bit_depth bins): avifgpu_light_level_from_histogram."""
    lib = load()
    out = ContentLightLevel()
    if bins is not None and (bins.dtype.itemsize != 8 or not bins.flags["C_CONTIGUOUS"] or (bit_depth in (10, 12) and bins.size < (1 << bit_depth))):
        raise ValueError("light_level_from_histogram: bins must be 1 << bit_depth contiguous 64-bit counters")
    code = lib.avifgpu_light_level_from_histogram(bins.ctypes.data if bins is not None else None, bit_depth, transfer, percentile, ctypes.byref(out))
    if code != 0:
        raise AvifGpuError(code, lib.avifgpu_last_error().decode())
    return out


class thumbnail_sums:
    """Arm the calling thread's thumbnail sums for the `with` block, disarm them on the way out (avifgpu_thumbnail_attach).

    `sums` holds tw * th * planes 64-bit counters, [(ty * tw + tx) * planes + c], and is never zeroed by the library: a numpy uint64
    array (mem = MEM_HOST), a contiguous torch int64 / uint64 tensor on the device the calls run on (mem = MEM_DEVICE), or a raw address."""

    def __init__(self, sums, tw: int, th: int, mem=MEM_HOST):
        self.sums, self.tw, self.th, self.mem = sums, int(tw), int(th), mem

    def _address(self):
        b = self.sums
        if hasattr(b, "data_ptr"):
            n, ptr = b.numel(), b.data_ptr()
            if b.element_size() != 8 or not b.is_contiguous():
                raise ValueError("thumbnail_sums: sums must be contiguous 64-bit counters")
        elif hasattr(b, "ctypes"):
            n, ptr = b.size, b.ctypes.data
            if b.dtype.itemsize != 8 or not b.flags["C_CONTIGUOUS"]:
                raise ValueError("thumbnail_sums: sums must be contiguous 64-bit counters")
        else:
            return int(b)
        if n < self.tw * self.th:
            raise ValueError("thumbnail_sums: %d counters for a %dx%d thumbnail" % (n, self.tw, self.th))
        return ptr

    def __enter__(self):
        lib = load()
        code = lib.avifgpu_thumbnail_attach(self._address(), self.tw, self.th, self.mem)
        if code != 0:
            raise AvifGpuError(code, lib.avifgpu_last_error().decode())
        return self

    def __exit__(self, *exc):
        load().avifgpu_thumbnail_attach(None, 0, 0, MEM_HOST)
        return False


def thumbnail_fit(desc: WriteDesc, bbox: int):
    """(tw, th) of an aspect-preserving fit of the save into a bbox x bbox square: avifgpu_thumbnail_fit."""
    lib = load()
    tw, th = c_int32(0), c_int32(0)
    code = lib.avifgpu_thumbnail_fit(ctypes.byref(desc), bbox, ctypes.byref(tw), ctypes.byref(th))
    if code != 0:
        raise AvifGpuError(code, lib.avifgpu_last_error().decode())
    return tw.value, th.value


def thumbnail_from_sums(desc: WriteDesc, tw: int, th: int, sums, stride_pad: int = 0):
    """The thumbnail planes of host sums (numpy uint64, tw * th * planes): avifgpu_thumbnail_from_sums.  Returns {plane: array} in the
    form of the main output -- plane 0 (th, tw * planes) for a colour REFERENCE save, planes 0 (+ 3) for gray, 0, 1, 2 (+ 3) at
    tw x th for YCBCR output; uint8 at bit depth 8, uint16 otherwise.  stride_pad: extra samples per row (they keep their 0xA5 fill)."""
    import numpy as np
    lib = load()
    if sums.dtype.itemsize != 8 or not sums.flags["C_CONTIGUOUS"] or sums.size < tw * th * desc.planes:
        raise ValueError("thumbnail_from_sums: sums must be tw * th * planes contiguous 64-bit counters")
    dt = np.uint16 if desc.bit_depth > 8 else np.uint8
    color = desc.planes >= 3
    alpha = desc.planes in (2, 4)
    if desc.output == OUT_REFERENCE:
        shapes = {0: tw * desc.planes} if color else ({0: tw, 3: tw} if alpha else {0: tw})
    else:
        shapes = {0: tw, 1: tw, 2: tw}
        if alpha:
            shapes[3] = tw
    bufs = {pl: np.full((max(th, 1), w + stride_pad), 0xA5A5 if dt == np.uint16 else 0xA5, dtype=dt) for pl, w in shapes.items()}
    ptrs = _PLANES4(*[bufs[i].ctypes.data if i in bufs else None for i in range(4)])
    strides = _STRIDES4(*[bufs[i].strides[0] if i in bufs else 0 for i in range(4)])
    code = lib.avifgpu_thumbnail_from_sums(ctypes.byref(desc), tw, th, sums.ctypes.data, ctypes.byref(ptrs), ctypes.byref(strides))
    if code != 0:
        raise AvifGpuError(code, lib.avifgpu_last_error().decode())
    return bufs


def _summary_address(counters, what):
    b = counters
    if hasattr(b, "data_ptr"):
        n, ptr, ok = b.numel(), b.data_ptr(), b.element_size() == 4 and b.is_contiguous()
    elif hasattr(b, "ctypes"):
        n, ptr, ok = b.size, b.ctypes.data, b.dtype.itemsize == 4 and b.flags["C_CONTIGUOUS"]
    else:
        return int(b)
    if not ok or n < SUMMARY_COUNTERS:
        raise ValueError("%s: counters must be %d contiguous 32-bit words" % (what, SUMMARY_COUNTERS))
    return ptr


class plane_summary:
    """Arm the calling thread's summary counters for the `with` block, disarm them on the way out (avifgpu_summary_attach).

    `counters` holds SUMMARY_COUNTERS 32-bit running maxima -- hi[4], lo_inv[4], spread, reserved -- and is never cleared by the library:
    a numpy uint32 array (mem = MEM_HOST), a contiguous torch int32 tensor on the device the calls run on (mem = MEM_DEVICE), or a raw
    address.  All-zero is the empty summary."""

    def __init__(self, counters, mem=MEM_HOST):
        self.counters, self.mem = counters, mem

    def __enter__(self):
        lib = load()
        code = lib.avifgpu_summary_attach(_summary_address(self.counters, "plane_summary"), self.mem)
        if code != 0:
            raise AvifGpuError(code, lib.avifgpu_last_error().decode())
        return self

    def __exit__(self, *exc):
        load().avifgpu_summary_attach(None, MEM_HOST)
        return False


def summary_read(desc: WriteDesc, counters) -> SaveSummary:
    """What host counters (numpy uint32, SUMMARY_COUNTERS words) say about the save `desc` describes: avifgpu_summary_read."""
    lib = load()
    out = SaveSummary()
    code = lib.avifgpu_summary_read(ctypes.byref(desc), _summary_address(counters, "summary_read"), ctypes.byref(out))
    if code != 0:
        raise AvifGpuError(code, lib.avifgpu_last_error().decode())
    return out


def summary_merge(into, other):
    """into = max(into, other), element by element (host counters): avifgpu_summary_merge.  Returns `into`."""
    lib = load()
    code = lib.avifgpu_summary_merge(_summary_address(into, "summary_merge"), _summary_address(other, "summary_merge"))
    if code != 0:
        raise AvifGpuError(code, lib.avifgpu_last_error().decode())
    return into


def _oserr(code):
    lib = load()
    if code < 0:
        raise AvifGpuError(code, lib.avifgpu_last_error().decode())
    return code


def orientation_compose(first: int, then: int) -> int:
    """The EXIF code of "apply `first`, then `then`" (avifgpu_orientation_compose)."""
    return _oserr(load().avifgpu_orientation_compose(first, then))


def read_oriented_geometry(desc: ReadDesc, orientation: int):
    """(width, height) of the oriented open (avifgpu_read_oriented_geometry)."""
    w, h = c_int32(0), c_int32(0)
    _oserr(load().avifgpu_read_oriented_geometry(ctypes.byref(desc), orientation, ctypes.byref(w), ctypes.byref(h)))
    return w.value, h.value


def read_oriented_next_tile(desc: ReadDesc, orientation: int, orow0: int, max_rows: int) -> int:
    """Rows of the tile that starts at output row orow0 (avifgpu_read_oriented_next_tile)."""
    return _oserr(load().avifgpu_read_oriented_next_tile(ctypes.byref(desc), orientation, orow0, max_rows))


def read_upsampled_scratch_bytes(desc: ReadDesc, upsampling: int, orientation: int, onrows: int) -> int:
    """Device scratch a MEM_DEVICE call of onrows output rows of the upsampled open needs (avifgpu_read_upsampled_scratch_bytes)."""
    return _oserr(load().avifgpu_read_upsampled_scratch_bytes(ctypes.byref(desc), upsampling, orientation, onrows))


def crop_rect(rect) -> CropRect:
    """A CropRect from (x0, y0, width, height) or a CropRect."""
    return rect if isinstance(rect, CropRect) else CropRect(*rect)


def clap_to_rect(width: int, height: int, clap) -> tuple:
    """(x0, y0, w, h) of a clean aperture (widthN, D, heightN, D, horizOffN, D, vertOffN, D) in a width x height image (avifgpu_clap_to_rect)."""
    out = CropRect()
    _oserr(load().avifgpu_clap_to_rect(width, height, ctypes.byref((c_int32 * 8)(*clap)), ctypes.byref(out)))
    return out.astuple()


def crop_compose(current, code: int, crop_in_view) -> tuple:
    """The stored rectangle of a crop given in the view orient(code, F[current]) (avifgpu_crop_compose)."""
    out = CropRect()
    _oserr(load().avifgpu_crop_compose(ctypes.byref(crop_rect(current)), code, ctypes.byref(crop_rect(crop_in_view)), ctypes.byref(out)))
    return out.astuple()


def read_cropped_geometry(desc: ReadDesc, rect, orientation: int):
    """(width, height) of the cropped, oriented open (avifgpu_read_cropped_geometry)."""
    w, h = c_int32(), c_int32()
    _oserr(load().avifgpu_read_cropped_geometry(ctypes.byref(desc), ctypes.byref(crop_rect(rect)), orientation, ctypes.byref(w), ctypes.byref(h)))
    return w.value, h.value


def read_cropped_next_tile(desc: ReadDesc, rect, upsampling: int, orientation: int, orow0: int, max_rows: int) -> int:
    """Rows of the tile that starts at output row orow0 (avifgpu_read_cropped_next_tile)."""
    return _oserr(load().avifgpu_read_cropped_next_tile(ctypes.byref(desc), ctypes.byref(crop_rect(rect)), upsampling, orientation, orow0, max_rows))


def read_cropped_scratch_bytes(desc: ReadDesc, rect, upsampling: int, orientation: int, onrows: int) -> int:
    """Device scratch that is enough for any MEM_DEVICE call of onrows output rows of the cropped open (avifgpu_read_cropped_scratch_bytes)."""
    return _oserr(load().avifgpu_read_cropped_scratch_bytes(ctypes.byref(desc), ctypes.byref(crop_rect(rect)), upsampling, orientation, onrows))


def grid_of(grid) -> Grid:
    """A Grid from (columns, rows, tile_width, tile_height) or a Grid."""
    return grid if isinstance(grid, Grid) else Grid(*grid)


def grid_parse(payload: bytes) -> tuple:
    """(rows, columns, output_width, output_height) of an ImageGrid item payload (avifgpu_grid_parse)."""
    r, c, w, h = (c_int32() for _ in range(4))
    buf = ctypes.create_string_buffer(bytes(payload), max(len(payload), 1))
    _oserr(load().avifgpu_grid_parse(ctypes.addressof(buf), len(payload), ctypes.byref(r), ctypes.byref(c), ctypes.byref(w), ctypes.byref(h)))
    return r.value, c.value, w.value, h.value


def grid_check(desc: ReadDesc, grid) -> None:
    """Raise unless (desc, grid) is what the grid open takes (avifgpu_grid_check)."""
    _oserr(load().avifgpu_grid_check(ctypes.byref(desc), ctypes.byref(grid_of(grid))))


def read_grid_scratch_bytes(desc: ReadDesc, grid, rect, upsampling: int, orientation: int, onrows: int) -> int:
    """Device scratch of a MEM_DEVICE call of onrows output rows of the grid open (avifgpu_read_grid_scratch_bytes)."""
    return _oserr(load().avifgpu_read_grid_scratch_bytes(ctypes.byref(desc), ctypes.byref(grid_of(grid)),
                                                          ctypes.byref(crop_rect(rect)) if rect is not None else None, upsampling, orientation, onrows))


def write_grid_check(desc: WriteDesc, grid) -> None:
    """Raise unless (desc, grid) is what the grid save takes (avifgpu_write_grid_check)."""
    _oserr(load().avifgpu_write_grid_check(ctypes.byref(desc), ctypes.byref(grid_of(grid))))


def write_grid_scratch_bytes(desc: WriteDesc, nrows: int) -> int:
    """Device scratch of a MEM_DEVICE call of nrows rows of the grid save (avifgpu_write_grid_scratch_bytes)."""
    return _oserr(load().avifgpu_write_grid_scratch_bytes(ctypes.byref(desc), nrows))


def grid_fit(desc: WriteDesc, max_tile_width: int, max_tile_height: int, align: int = 1) -> tuple:
    """(columns, rows, tile_width, tile_height) of the grid with the fewest tiles within the caps (avifgpu_grid_fit)."""
    g = Grid()
    _oserr(load().avifgpu_grid_fit(ctypes.byref(desc), max_tile_width, max_tile_height, align, ctypes.byref(g)))
    return g.columns, g.rows, g.tile_width, g.tile_height


def grid_payload(grid, width: int, height: int, capacity: int = 12) -> bytes:
    """The ImageGrid item payload of (grid, width x height) (avifgpu_grid_payload)."""
    buf = ctypes.create_string_buffer(max(capacity, 1))
    n = _oserr(load().avifgpu_grid_payload(ctypes.byref(grid_of(grid)), width, height, ctypes.addressof(buf), capacity))
    return buf.raw[:n]


def icc_kind_of(icc, desc: WriteDesc) -> int:
    """The AVIFGPU_ICC_KIND_* value that names the prepared structure `icc` for avifgpu_write_rows_grid."""
    if icc is None:
        return ICC_KIND_NONE
    if isinstance(icc, IccClut16):
        return ICC_KIND_CLUT8_TABLE if desc.depth == 8 else ICC_KIND_CLUT16
    for cls, kind in ((IccPipeline32, ICC_KIND_PIPELINE32), (IccSampled32, ICC_KIND_SAMPLED), (IccShaper8, ICC_KIND_SHAPER8), (IccTransform, ICC_KIND_TRANSFORM)):
        if isinstance(icc, cls):
            return kind
    raise TypeError("not a prepared ICC structure: %r" % (icc,))


def read_oriented_scratch_bytes(desc: ReadDesc, orientation: int, onrows: int) -> int:
    """Device scratch a MEM_DEVICE call of onrows output rows needs (avifgpu_read_oriented_scratch_bytes)."""
    return _oserr(load().avifgpu_read_oriented_scratch_bytes(ctypes.byref(desc), orientation, onrows))


def yuv_coefficients(has_nclx: int, matrix: int, primaries: int):
    out = (c_float * 3)()
    load().avifgpu_get_yuv_coefficients(has_nclx, matrix, primaries, ctypes.byref(out))
    return tuple(out)
