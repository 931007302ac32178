// icc_pipeline32.h -- the stages of avifgpu_icc_pipeline32 (include/avifgpu.h) as lcms2 2.12 evaluates them on floats.
//
// One definition for both sides: icc_pipeline32.cpp evaluates it on the host (the proof's engine, avifgpu_icc_pipeline32_eval), the
// write kernel (write_px<..., icc = 8>, write_kernels.hip) per pixel.  Where the two sides differ it is in HOW a value is formed, never in
// which value: the 16-bit word of a float (the library's double expression on the host, quick_saturate_word_f32 on the device -- equal
// for every float that is a number, tools/satword_check.hip; a NaN's word from its payload bits on both sides) and w / 65535.0 as a float (equal for all 65536 words, tests/test_gpu_icc.py).  pow() is the
// platform's: the host calls the C library lcms2 calls, the device OCML's (within an ulp of double: tier 2 behind the transfer curve).
#pragma once
#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#endif
#include <stdint.h>
#include <math.h>
#include "../../include/avifgpu.h"
#ifdef __HIP_DEVICE_COMPILE__
#include "satword_f32.h"
#endif

#if defined(__HIPCC__)
#define ICC32_HD __host__ __device__ __forceinline__
#else
#define ICC32_HD inline
#endif

namespace avifgpu {
namespace icc32 {

constexpr double kMinusInf = (double)-1E22F;         // lcms2's MINUS_INF / PLUS_INF (float literals)
constexpr double kPlusInf = (double)1E22F;
constexpr double kDetTol = 0.0001;                   // MATRIX_DET_TOLERANCE
constexpr double kMaxXYZ = 1.0 + 32767.0 / 32768.0;  // MAX_ENCODEABLE_XYZ
constexpr double kD50X = 0.9642, kD50Y = 1.0, kD50Z = 0.8249;

// _cmsQuickSaturateWord(v * 65535.0)
ICC32_HD uint32_t sat_word(float v)
{
#ifdef __HIP_DEVICE_COMPILE__
    // A NaN takes neither saturation of the library's form below: its word is the floor of the low half of the double NaN, which holds
    // the three low payload bits of the float (32767 for the default NaN).  quick_saturate_word_f32 clamps a NaN to 0.
    if (v != v) return (uint32_t)(((int32_t)(__float_as_uint(v) << 29) >> 16) + 32767) & 0xffffu;
    return quick_saturate_word_f32(v);
#else
    double d = (double)v * 65535.0 + 0.5;
    if (d <= 0) return 0;
    if (d >= 65535.0) return 0xffff;
    union { double v; uint32_t h[2]; } t;
    t.v = (d - 32767.0) + 68719476736.0 * 1.5;       // _cmsQuickFloor
    return (uint32_t)(((int32_t)t.h[0] >> 16) + 32767) & 0xffffu;
#endif
}

// (float)(w / 65535.0) for a word w
ICC32_HD float word_to_float_d(uint32_t w)
{
#ifdef __HIP_DEVICE_COMPILE__
    constexpr float rh = (float)(1.0 / 65535.0), rl = (float)(1.0 / 65535.0 - (double)rh);
    const float f = (float)w;
    return __builtin_fmaf(f, rh, f * rl);
#else
    return (float)(w / 65535.0);
#endif
}

// _cmsToFixedDomain
ICC32_HD uint32_t to_fixed_domain(uint32_t a) { return a + ((a + 0x7fffu) / 0xffffu); }

// cmsEvalToneCurve16 on a sampled curve: LinLerp1D (n entries, n >= 2)
ICC32_HD uint32_t lerp1d(const uint16_t* T, uint32_t n, uint32_t w)
{
    const uint32_t val3 = to_fixed_domain((n - 1u) * w);
    const uint32_t cell0 = val3 >> 16, rest = val3 & 0xffffu;
    const uint32_t y0 = T[cell0], y1 = T[cell0 + 1u < n ? cell0 + 1u : n - 1u];   // w == 0xffff: rest == 0, y1 unused
    const uint32_t dif = (uint32_t)((int32_t)y1 - (int32_t)y0) * rest + 0x8000u;
    return ((dif >> 16) + y0) & 0xffffu;
}

// DefaultEvalParametricFn (cmsgamma.c) behind EvalSegmentedFn's one segment (-1e22, 1e22]
ICC32_HD double parametric(int type, const double* P, double R)
{
    if (!(R > kMinusInf && R <= kPlusInf)) return kMinusInf;
    double e, Val, disc;
    switch (type) {
    case 1:
        if (R < 0) Val = fabs(P[0] - 1.0) < kDetTol ? R : 0;
        else Val = pow(R, P[0]);
        break;
    case -1:
        if (R < 0) Val = fabs(P[0] - 1.0) < kDetTol ? R : 0;
        else Val = fabs(P[0]) < kDetTol ? kPlusInf : pow(R, 1 / P[0]);
        break;
    case 2:
        if (fabs(P[1]) < kDetTol) Val = 0;
        else {
            disc = -P[2] / P[1];
            if (R >= disc) { e = P[1] * R + P[2]; Val = e > 0 ? pow(e, P[0]) : 0; }
            else Val = 0;
        }
        break;
    case -2:
        if (fabs(P[0]) < kDetTol || fabs(P[1]) < kDetTol) Val = 0;
        else {
            Val = R < 0 ? 0 : (pow(R, 1.0 / P[0]) - P[2]) / P[1];
            if (Val < 0) Val = 0;
        }
        break;
    case 3:
        if (fabs(P[1]) < kDetTol) Val = 0;
        else {
            disc = -P[2] / P[1];
            if (disc < 0) disc = 0;
            if (R >= disc) { e = P[1] * R + P[2]; Val = e > 0 ? pow(e, P[0]) + P[3] : 0; }
            else Val = P[3];
        }
        break;
    case -3:
        if (fabs(P[1]) < kDetTol) Val = 0;
        else if (R >= P[3]) { e = R - P[3]; Val = e > 0 ? (pow(e, 1 / P[0]) - P[2]) / P[1] : 0; }
        else Val = -P[2] / P[1];
        break;
    case 4:
        if (R >= P[4]) { e = P[1] * R + P[2]; Val = e > 0 ? pow(e, P[0]) : 0; }
        else Val = R * P[3];
        break;
    case -4:
        e = P[1] * P[4] + P[2];
        disc = e < 0 ? 0 : pow(e, P[0]);
        if (R >= disc) Val = (fabs(P[0]) < kDetTol || fabs(P[1]) < kDetTol) ? 0 : (pow(R, 1.0 / P[0]) - P[2]) / P[1];
        else Val = fabs(P[3]) < kDetTol ? 0 : R / P[3];
        break;
    case 5:
        if (R >= P[4]) { e = P[1] * R + P[2]; Val = e > 0 ? pow(e, P[0]) + P[5] : P[5]; }
        else Val = R * P[3] + P[6];
        break;
    default:  // -5
        disc = P[3] * P[4] + P[6];
        if (R >= disc) {
            e = R - P[5];
            Val = e < 0 ? 0 : ((fabs(P[0]) < kDetTol || fabs(P[1]) < kDetTol) ? 0 : (pow(e, 1.0 / P[0]) - P[2]) / P[1]);
        } else {
            Val = fabs(P[3]) < kDetTol ? 0 : (R - P[6]) / P[3];
        }
        break;
    }
    if (isinf(Val)) return Val > 0 ? kPlusInf : kMinusInf;
    return Val;
}

// cmsEvalToneCurveFloat of one channel of a CURVES stage
ICC32_HD float curve(const avifgpu_icc_stage32& s, const uint16_t* words, int c, float v)
{
    const int type = s.curve_type[c];
    if (type == 0) return word_to_float_d(lerp1d(words + s.offset[c], (uint32_t)s.entries[c], sat_word(v)));
    // gamma 1 is the identity on every float of the segment's domain both ways (pow(R, 1) == R exactly; the negative branch returns R)
    if ((type == 1 || type == -1) && s.params[c][0] == 1.0 && v > -1E22F && v <= 1E22F) return v;
    return (float)parametric(type, s.params[c], (double)v);
}

// EvaluateMatrix
ICC32_HD void matrix(const avifgpu_icc_stage32& s, float (&v)[3])
{
    const float in[3] = { v[0], v[1], v[2] };
    for (int i = 0; i < 3; ++i) {
        double t = 0;
        t += (double)in[0] * s.matrix[3 * i + 0];
        t += (double)in[1] * s.matrix[3 * i + 1];
        t += (double)in[2] * s.matrix[3 * i + 2];
        if (s.has_bias) t += s.bias[i];
        v[i] = (float)t;
    }
}

// EvaluateCLUTfloatIn16: FromFloatTo16, TetrahedralInterp16 (3 -> 3, grid n[0] x n[1] x n[2], input 0 slowest), From16ToFloat.
// The library walks the cell from the base node along the axes in decreasing order of their fractions; ties pick one order of its
// if-tree, and any order gives the same sum modulo 2^32 (the tied terms collapse), which is all its int32 arithmetic keeps.  An input of
// 0xffff has its step zeroed (and its fraction is 0).
ICC32_HD void clut16(const avifgpu_icc_stage32& s, const uint16_t* words, float (&v)[3])
{
    const uint16_t* T = words + s.offset[0];
    const uint32_t opta[3] = { 3u * (uint32_t)s.entries[2] * (uint32_t)s.entries[1], 3u * (uint32_t)s.entries[2], 3u };
    uint32_t base = 0, r[3], step[3];
    for (int k = 0; k < 3; ++k) {
        const uint32_t w = sat_word(v[k]);
        const uint32_t f = to_fixed_domain(w * (uint32_t)(s.entries[k] - 1));
        r[k] = f & 0xffffu;
        base += opta[k] * (f >> 16);
        step[k] = w == 0xffffu ? 0u : opta[k];
    }
    // (fraction, step) pairs by decreasing fraction: three compare-exchanges on scalars (no dynamically indexed array on the device)
    uint32_t ra = r[0], sa = step[0], rb = r[1], sb = step[1], rc = r[2], sc = step[2], t;
    if (rb > ra) { t = ra; ra = rb; rb = t; t = sa; sa = sb; sb = t; }
    if (rc > rb) { t = rb; rb = rc; rc = t; t = sb; sb = sc; sc = t; }
    if (rb > ra) { t = ra; ra = rb; rb = t; t = sa; sa = sb; sb = t; }
    const uint32_t n1 = base + sa, n2 = n1 + sb, n3 = n2 + sc;
    for (int ch = 0; ch < 3; ++ch) {
        const int32_t c0 = T[base + ch], c1 = T[n1 + ch], c2 = T[n2 + ch], c3 = T[n3 + ch];
        const uint32_t rest = (uint32_t)(c1 - c0) * ra + (uint32_t)(c2 - c1) * rb + (uint32_t)(c3 - c2) * rc + 0x8001u;
        const int32_t t = (int32_t)rest;
        const uint32_t u = (uint32_t)t + (uint32_t)(t >> 16);
        const uint32_t o = ((uint32_t)c0 + (uint32_t)((int32_t)u >> 16)) & 0xffffu;
        v[ch] = (float)o / 65535.0f;
    }
}

// EvaluateLab2XYZ: v4 Lab encoding in, XYZ / MAX_ENCODEABLE_XYZ out (cmsLab2XYZ against D50)
ICC32_HD double lab_f1(double t)
{
    const double Limit = (24.0 / 116.0);
    if (t <= Limit) return (108.0 / 841.0) * (t - (16.0 / 116.0));
    return t * t * t;
}
ICC32_HD void lab_to_xyz(float (&v)[3])
{
    const double L = v[0] * 100.0, a = v[1] * 255.0 - 128.0, b = v[2] * 255.0 - 128.0;
    const double y = (L + 16.0) / 116.0, x = y + 0.002 * a, z = y - 0.005 * b;
    const double X = lab_f1(x) * kD50X, Y = lab_f1(y) * kD50Y, Z = lab_f1(z) * kD50Z;
    v[0] = (float)(X / kMaxXYZ); v[1] = (float)(Y / kMaxXYZ); v[2] = (float)(Z / kMaxXYZ);
}
// EvaluateXYZ2Lab (cmsXYZ2Lab against D50)
ICC32_HD double lab_f(double t)
{
    const double Limit = ((24.0 / 116.0) * (24.0 / 116.0) * (24.0 / 116.0));
    if (t <= Limit) return (841.0 / 108.0) * t + (16.0 / 116.0);
    return pow(t, 1.0 / 3.0);
}
ICC32_HD void xyz_to_lab(float (&v)[3])
{
    const double X = v[0] * kMaxXYZ, Y = v[1] * kMaxXYZ, Z = v[2] * kMaxXYZ;
    const double fx = lab_f(X / kD50X), fy = lab_f(Y / kD50Y), fz = lab_f(Z / kD50Z);
    const double L = 116.0 * fy - 16.0, a = 500.0 * (fx - fy), b = 200.0 * (fy - fz);
    v[0] = (float)(L / 100.0); v[1] = (float)((a + 128.0) / 255.0); v[2] = (float)((b + 128.0) / 255.0);
}

// One stage.  The kind is uniform across a launch: on the device every branch here is a scalar one.
ICC32_HD void stage(const avifgpu_icc_stage32& s, const uint16_t* words, float (&v)[3])
{
    switch (s.kind) {
    case AVIFGPU_ICC_STAGE_CURVES:
        for (int c = 0; c < 3; ++c) v[c] = curve(s, words, c, v[c]);
        break;
    case AVIFGPU_ICC_STAGE_MATRIX: matrix(s, v); break;
    case AVIFGPU_ICC_STAGE_CLUT16: clut16(s, words, v); break;
    case AVIFGPU_ICC_STAGE_LAB_TO_XYZ: lab_to_xyz(v); break;
    default: xyz_to_lab(v); break;
    }
}

}  // namespace icc32
}  // namespace avifgpu
