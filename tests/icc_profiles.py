"""The document profiles of the ICC tests on determined sources (tests/test_truth64_icc.py, tests/test_gpu_icc_determined.py): the
PROFILES, SAMPLED and MIXED of tests/test_gpu_icc.py, built by the live lcms2 (oracle/liboracle_icc.so) where it exists and read
from tests/golden/icc_truth_profiles.npz (lcms2's output, tests/golden/make_icc_truth_profiles.py) where it does not; the
transforms the library prepares from them; and lcms2's in-place row conversion, as the reference's save loop runs it.

PER_CHANNEL is no profile but a transform put together from three prepared ones: Display P3's matrix behind a different parametric
curve per channel (gamma 1.8 as `para`, the sRGB curve, gamma 2.2).  None of the profiles above sends three different parametric
curves through the icc = 2 / icc = 4 kernels -- theirs are equal for R, G and B, and the mixed ones take icc = 6 -- so a kernel that
read one channel's parameters for another would pass every one of them.  The float64 truth needs the struct alone, and each of its
curves and its matrix are held against lcms2 through the profiles they come from."""
import ctypes
import functools
import os

import numpy as np

import harness
from test_gpu_icc import MIXED, PROFILES, SAMPLED

pkg = harness.pkg
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ICC_LIB = os.path.join(ROOT, "oracle", "liboracle_icc.so")
FIXTURE = os.path.join(ROOT, "tests", "golden", "icc_truth_profiles.npz")
NO_LCMS = "oracle/liboracle_icc.so not built (lcms2 absent)"

# name -> (kind, trc, g or table entries) of oracle_icc_make_profile
SPECS = {name: (kind, trc, float(g)) for name, kind, trc, g in PROFILES + SAMPLED}
SPECS.update({name: (kind, trc, float(n)) for name, kind, trc, n, _ in MIXED})
PARAMETRIC = [p[0] for p in PROFILES]
LINEAR = [p[0] for p in PROFILES if p[2] == 0 and p[3] == 1.0]
CURVED = [p[0] for p in PROFILES if not (p[2] == 0 and p[3] == 1.0)]
TABLES = [p[0] for p in SAMPLED] + [p[0] for p in MIXED]
MIXED_MASKS = {p[0]: p[4] for p in MIXED}
REC2020, SRGB = pkg.ICC_TARGET_REC2020_LINEAR, pkg.ICC_TARGET_SRGB_FLOAT
PER_CHANNEL = "p3-R-para-gamma1.8-G-srgb-parametric-B-gamma2.2"
PER_CHANNEL_FROM = ("p3-para-gamma1.8", "srgb-parametric", "adobergb-gamma2.2")
ALL = list(SPECS) + [PER_CHANNEL]


@functools.lru_cache(maxsize=None)
def lcms():
    """ctypes handle on the live lcms2 oracle, or None where it is not built."""
    if not os.path.exists(ICC_LIB):
        return None
    L = ctypes.CDLL(ICC_LIB)
    L.oracle_icc_make_profile.restype = ctypes.c_int32
    L.oracle_icc_make_profile.argtypes = [ctypes.c_int32, ctypes.c_int32, ctypes.c_double, ctypes.c_void_p, ctypes.c_uint32]
    for fn in (L.oracle_icc_convert_rows_to_rec2020, L.oracle_icc_convert_rows_to_srgb_float):
        fn.restype = ctypes.c_int32
        fn.argtypes = [ctypes.c_void_p, ctypes.c_uint32, ctypes.c_int32, ctypes.c_void_p, ctypes.c_uint32, ctypes.c_uint32, ctypes.c_uint32]
    return L


def make_profile(L, name):
    kind, trc, g = SPECS[name]
    buf = ctypes.create_string_buffer(1 << 16)
    n = L.oracle_icc_make_profile(kind, trc, g, buf, len(buf))
    assert n > 0, name
    return buf.raw[:n]


@functools.lru_cache(maxsize=None)
def profile_bytes(name):
    L = lcms()
    if L is not None:
        return make_profile(L, name)
    with np.load(FIXTURE) as z:
        return z[name].tobytes()


@functools.lru_cache(maxsize=None)
def prepared(name, target):
    """avifgpu_icc_transform / avifgpu_icc_sampled32 of a profile (host code of the library: no device needed).  One object per
    (profile, target), kept alive: the library recognises a table it has already uploaded by its address."""
    if name == PER_CHANNEL:
        xf = pkg.IccTransform.from_buffer_copy(prepared(PER_CHANNEL_FROM[0], target))
        for c in (1, 2):
            donor = prepared(PER_CHANNEL_FROM[c], target)
            xf.trc_type[c] = donor.trc_type[c]
            for k in range(7):
                xf.trc_params[c][k] = donor.trc_params[c][k]
        return xf
    icc = profile_bytes(name)
    lib = pkg.load()
    if name in TABLES:
        xf = pkg.IccSampled32()
        rc = lib.avifgpu_icc_prepare_sampled(icc, len(icc), target, ctypes.byref(xf))
    else:
        xf = pkg.IccTransform()
        rc = lib.avifgpu_icc_prepare(icc, len(icc), target, ctypes.byref(xf))
    assert rc == 0, (name, target, rc)
    return xf


def lcms_rows(name, target, src, width, planes):
    """What the reference hands its pixel loop: the rows converted in place by lcms2 (alpha copied)."""
    L, icc = lcms(), profile_bytes(name)
    conv = src.copy()
    fn = L.oracle_icc_convert_rows_to_srgb_float if target == SRGB else L.oracle_icc_convert_rows_to_rec2020
    assert fn(icc, len(icc), int(planes == 4), conv.ctypes.data, width, conv.shape[0], conv.strides[0]) == 0
    return conv
