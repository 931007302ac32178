// avifgpu_api.hip -- the C-ABI of include/avifgpu.h: validation, nclx -> coefficients, kernel parameters, launches.
//
// There is no CPU fallback anywhere in this file: without a HIP device avifgpu_init fails and every
// *_rows call returns an error.  Host-pointer calls go through the bound device contexts of pipeline.hip
// (one worker thread + staging slots per context, row tiles dealt across contexts); device-pointer calls
// launch directly on the caller's stream and device.
#include <hip/hip_runtime.h>
#include <cstddef>
#include <cmath>
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <cstring>

#include "../../include/avifgpu.h"
#include "kernel_params.h"
#include "staging.h"

namespace avifgpu { void release_read_tables(); }

using namespace avifgpu;

namespace {
thread_local char g_err[512] = "";
thread_local char g_kernel[kLabelBytes] = "";
int g_hot_variant = kHotDefault;
}

namespace avifgpu {

int fail(int code, const char* fmt, ...)
{
    va_list ap; va_start(ap, fmt);
    vsnprintf(g_err, sizeof(g_err), fmt, ap);
    va_end(ap);
    return code;
}

int hip_fail(hipError_t e, const char* what, int code)
{
    return fail(code, "%s: %s", what, hipGetErrorString(e));
}

void set_error(const char* msg) { snprintf(g_err, sizeof(g_err), "%s", msg); }
const char* last_error() { return g_err; }
void set_last_kernel(const char* label) { snprintf(g_kernel, sizeof(g_kernel), "%s", label); }
int hot_variant() { return g_hot_variant; }

} // namespace avifgpu

namespace {

// ---- nclx -> (kr, kg, kb), the same derivation the plug-in performs (YUVCoefficiants.cpp:110-188) ----
struct PrimariesRow { int code; float rX, rY, gX, gY, bX, bY, wX, wY; };
const PrimariesRow kPrimariesRows[] = {              // ITU-T H.273 table 2 chromaticities (YUVCoefficiants.cpp:58-70)
    { AVIFGPU_PRIMARIES_BT709,        0.64f,  0.33f,  0.3f,   0.6f,   0.15f,  0.06f,  0.3127f, 0.329f  },
    { AVIFGPU_PRIMARIES_BT470M,       0.67f,  0.33f,  0.21f,  0.71f,  0.14f,  0.08f,  0.310f,  0.316f  },
    { AVIFGPU_PRIMARIES_BT470BG,      0.64f,  0.33f,  0.29f,  0.60f,  0.15f,  0.06f,  0.3127f, 0.3290f },
    { AVIFGPU_PRIMARIES_BT601,        0.630f, 0.340f, 0.310f, 0.595f, 0.155f, 0.070f, 0.3127f, 0.3290f },
    { AVIFGPU_PRIMARIES_SMPTE240M,    0.630f, 0.340f, 0.310f, 0.595f, 0.155f, 0.070f, 0.3127f, 0.3290f },
    { AVIFGPU_PRIMARIES_GENERIC_FILM, 0.681f, 0.319f, 0.243f, 0.692f, 0.145f, 0.049f, 0.310f,  0.316f  },
    { AVIFGPU_PRIMARIES_BT2020,       0.708f, 0.292f, 0.170f, 0.797f, 0.131f, 0.046f, 0.3127f, 0.3290f },
    { AVIFGPU_PRIMARIES_SMPTE428,     1.0f,   0.0f,   0.0f,   1.0f,   0.0f,   0.0f,   0.3333f, 0.3333f },
    { AVIFGPU_PRIMARIES_SMPTE431,     0.680f, 0.320f, 0.265f, 0.690f, 0.150f, 0.060f, 0.314f,  0.351f  },
    { AVIFGPU_PRIMARIES_SMPTE432,     0.680f, 0.320f, 0.265f, 0.690f, 0.150f, 0.060f, 0.3127f, 0.3290f },
    { AVIFGPU_PRIMARIES_EBU3213,      0.630f, 0.340f, 0.295f, 0.605f, 0.155f, 0.077f, 0.3127f, 0.3290f },
};

bool kr_kb_from_nclx(int matrix, int primaries, float& kr, float& kb)
{
    switch (matrix) {                                 // H.273 table 4 (YUVCoefficiants.cpp:94-106)
    case AVIFGPU_MATRIX_BT709:      kr = 0.2126f; kb = 0.0722f; return true;
    case AVIFGPU_MATRIX_FCC:        kr = 0.30f;   kb = 0.11f;   return true;
    case AVIFGPU_MATRIX_BT470BG:
    case AVIFGPU_MATRIX_BT601:      kr = 0.299f;  kb = 0.114f;  return true;
    case AVIFGPU_MATRIX_SMPTE240M:  kr = 0.212f;  kb = 0.087f;  return true;
    case AVIFGPU_MATRIX_BT2020_NCL: kr = 0.2627f; kb = 0.0593f; return true;
    case AVIFGPU_MATRIX_CHROMA_DERIVED_NCL: {
        const PrimariesRow* pr = &kPrimariesRows[0]; // unknown primaries fall back to BT.709 (:88-90)
        for (const PrimariesRow& row : kPrimariesRows) if (row.code == primaries) { pr = &row; break; }
        const float rX = pr->rX, rY = pr->rY, gX = pr->gX, gY = pr->gY, bX = pr->bX, bY = pr->bY, wX = pr->wX, wY = pr->wY;
        const float rZ = 1.0f - (rX + rY), gZ = 1.0f - (gX + gY), bZ = 1.0f - (bX + bY), wZ = 1.0f - (wX + wY);
        const float den = wY * (rX * (gY * bZ - bY * gZ) + gX * (bY * rZ - rY * bZ) + bX * (rY * gZ - gY * rZ));
        kr = (rY * (wX * (gY * bZ - bY * gZ) + wY * (bX * gZ - gX * bZ) + wZ * (gX * bY - bX * gY))) / den;   // H.273 eq. 32
        kb = (bY * (wX * (rY * gZ - gY * rZ) + wY * (gX * rZ - rX * gZ) + wZ * (rX * gY - gX * rY))) / den;   // H.273 eq. 33
        return true;
    }
    default: return false;
    }
}

void yuv_coefficients(int has_nclx, int matrix, int primaries, float out[3])
{
    float kr = 0.299f, kb = 0.114f;                   // MIAF default, matrix_coefficients 5/6 (:169-174)
    float kg = 1.0f - kr - kb;
    float a, b;
    if (has_nclx && kr_kb_from_nclx(matrix, primaries, a, b)) { kr = a; kb = b; kg = 1.0f - kr - kb; }
    out[0] = kr; out[1] = kg; out[2] = kb;
}

bool chroma_shift(int chroma, int& xs, int& ys)
{
    switch (chroma) {
    case AVIFGPU_CHROMA_444: xs = 0; ys = 0; return true;
    case AVIFGPU_CHROMA_422: xs = 1; ys = 0; return true;
    case AVIFGPU_CHROMA_420: xs = 1; ys = 1; return true;
    default: xs = 0; ys = 0; return false;
    }
}

} // namespace

namespace avifgpu {

// ---- write-side validation (same rules as the plug-in's option fix-ups and default branches) --------
int check_write(const avifgpu_write_desc* d, int row0, int nrows, WriteGeom& g)
{
    if (!d) return fail(AVIFGPU_formatBadParameters, "null descriptor");
    if (d->width <= 0 || d->height <= 0) return fail(AVIFGPU_formatBadParameters, "bad image size %dx%d", d->width, d->height);
    if (row0 < 0 || nrows < 0 || (int64_t)row0 + nrows > d->height) return fail(AVIFGPU_formatBadParameters, "rows [%d,%d) outside image", row0, row0 + nrows);
    if (d->depth != 8 && d->depth != 16 && d->depth != 32) return fail(AVIFGPU_formatBadParameters, "unsupported depth %d", d->depth);   // Write.cpp:318
    if (d->planes < 1 || d->planes > 4) return fail(AVIFGPU_formatBadParameters, "unsupported plane count %d", d->planes);
    if (d->bit_depth != 8 && d->bit_depth != 10 && d->bit_depth != 12) return fail(AVIFGPU_formatCannotRead, "unsupported image bit depth %d", d->bit_depth); // WriteHeifImage.cpp:57
    if (d->depth == 32 && d->bit_depth == 8) return fail(AVIFGPU_formatCannotRead, "32-bit documents save as 10 or 12 bit");
    g.color = d->planes >= 3;
    g.alpha = (d->planes == 2 || d->planes == 4);
    if (g.alpha != (d->alpha_state != AVIFGPU_ALPHA_NONE)) return fail(AVIFGPU_formatBadParameters, "alpha_state does not match planes");
    if (d->alpha_state < AVIFGPU_ALPHA_NONE || d->alpha_state > AVIFGPU_ALPHA_PREMULTIPLIED) return fail(AVIFGPU_formatBadParameters, "bad alpha_state");
    g.dst16 = d->bit_depth > 8;
    g.xs = g.ys = 0;
    // pq_evaluation took the place of a reserved field in ABI 3: it means something for PQ saves of 32-bit documents only and is
    // ignored (not range-checked) everywhere else, so a caller that never initialised the old field keeps working for those.
    if (d->depth == 32 && d->transfer == AVIFGPU_TRANSFER_PQ && (d->pq_evaluation < AVIFGPU_PQ_AUTO || d->pq_evaluation > AVIFGPU_PQ_CLOSE))
        return fail(AVIFGPU_formatBadParameters, "bad pq_evaluation %d", d->pq_evaluation);
    if (d->depth == 32) {
        if (d->transfer < AVIFGPU_TRANSFER_PQ || d->transfer > AVIFGPU_TRANSFER_CLIP) return fail(AVIFGPU_writErr, "Unsupported color transfer function.");
        if (!g.color && d->transfer != AVIFGPU_TRANSFER_PQ && d->transfer != AVIFGPU_TRANSFER_CLIP)
            return fail(AVIFGPU_writErr, "Unsupported color transfer function.");                                  // WriteHeifImage.cpp:581-582
        if (d->transfer == AVIFGPU_TRANSFER_PQ && (d->peak_nits < 1 || d->peak_nits > 10000))
            return fail(AVIFGPU_formatBadParameters, "nominalPeakBrightness %d outside [1,10000]", d->peak_nits); // AvifFormat.h:52-53
    }
    if (d->output == AVIFGPU_OUT_REFERENCE) {
        g.nplanes = g.color ? 1 : (g.alpha ? 2 : 1);
        return 0;
    }
    if (d->output != AVIFGPU_OUT_YCBCR) return fail(AVIFGPU_formatBadParameters, "bad output kind %d", d->output);
    if (!g.color) return fail(AVIFGPU_formatBadParameters, "YCbCr output needs an RGB source");
    if (!chroma_shift(d->chroma, g.xs, g.ys)) return fail(AVIFGPU_formatBadParameters, "bad chroma %d", d->chroma);
    if (!d->full_range) return fail(AVIFGPU_formatBadParameters, "limited-range output is not produced by the plug-in (full_range_flag is always set)");
    if (d->chroma_downsampling != AVIFGPU_DOWNSAMPLE_AVERAGE && d->chroma_downsampling != AVIFGPU_DOWNSAMPLE_NEAREST)
        return fail(AVIFGPU_formatBadParameters, "bad chroma_downsampling");
    if (d->chroma_zero_point != AVIFGPU_CHROMA_ZERO_LIBHEIF && d->chroma_zero_point != AVIFGPU_CHROMA_ZERO_DECODER)
        return fail(AVIFGPU_formatBadParameters, "bad chroma_zero_point");
    if (g.ys && (row0 & 1)) return fail(AVIFGPU_formatBadParameters, "4:2:0 tiles must start on an even row");
    if (g.ys && (nrows & 1) && row0 + nrows != d->height) return fail(AVIFGPU_formatBadParameters, "4:2:0 tiles must have even height unless they end the image");
    g.nplanes = g.alpha ? 4 : 3;
    return 0;
}

// avifgpu_shutdown: nothing is in flight any more.
void release_device_caches()
{
    release_read_tables();
    release_icc_tables();
}

int fill_write_params(const avifgpu_write_desc* d, int row0, int nrows, const WriteGeom&, const IccArgs& icc, WriteParams& p)
{
    memset(&p, 0, sizeof(p));
    if (const int rc = fill_icc_params(d, icc, p)) return rc;     // icc_tables.cpp: the ICC stage, its device tables included
    p.width = d->width; p.nrows = nrows; p.rows_to_end = d->height - row0;
    p.transfer = d->depth == 32 ? d->transfer : AVIFGPU_TRANSFER_CLIP;
    p.premultiply = d->alpha_state == AVIFGPU_ALPHA_PREMULTIPLIED;
    p.nearest = d->chroma_downsampling == AVIFGPU_DOWNSAMPLE_NEAREST;
    p.maxv = (1 << d->bit_depth) - 1;
    p.maxf = (float)p.maxv;
    p.rcp_maxf = 1.0f / p.maxf;
    p.pq_mult = (float)d->peak_nits / 10000.0f;          // ColorTransfer.cpp:86
    p.pq_log2_mult_m1 = (float)((2610.0 / 16384.0) * std::log2((double)p.pq_mult));
    p.log2_maxf = (float)std::log2((double)p.maxv);
    p.pq_close = d->pq_evaluation != AVIFGPU_PQ_COMPACT;   // AUTO = CLOSE at every depth since round 4 (the table form costs the kernels nothing measurable)
    p.half = d->chroma_zero_point == AVIFGPU_CHROMA_ZERO_DECODER ? p.maxf * 0.5f : (float)(1 << (d->bit_depth - 1));
    if (d->output == AVIFGPU_OUT_YCBCR) {
        if (d->matrix_coefficients == AVIFGPU_MATRIX_RGB_GBR) {       // lossless, WriteMetadata.cpp:143-146
            if (d->chroma != AVIFGPU_CHROMA_444) return fail(AVIFGPU_formatBadParameters, "identity (GBR) matrix requires 4:4:4");
            // Y <- G, Cb <- B, Cr <- R as a matrix: 0*R + 1*G + 0*B (+ 0.5, truncate) is the integer code G exactly, so the
            // kernels need no special case
            p.identity = 1;
            p.my[1] = 1.0f; p.mcb[2] = 1.0f; p.mcr[0] = 1.0f;
            p.half = 0.0f;
        } else {
            float kr, kb;
            if (!kr_kb_from_nclx(d->matrix_coefficients, d->color_primaries, kr, kb))
                return fail(AVIFGPU_formatBadParameters, "matrix_coefficients %d has no Kr/Kb form", d->matrix_coefficients);
            const float kg = 1.0f - kr - kb;
            p.my[0] = kr;                        p.my[1] = kg;                        p.my[2] = kb;
            p.mcb[0] = -kr / (1.0f - kb) / 2.0f; p.mcb[1] = -kg / (1.0f - kb) / 2.0f; p.mcb[2] = 0.5f;
            p.mcr[0] = 0.5f;                     p.mcr[1] = -kg / (1.0f - kr) / 2.0f; p.mcr[2] = -kb / (1.0f - kr) / 2.0f;
        }
        // The streaming kernels form luma without the upper clip (luma_code_nc / luma_pair_nc, write_kernels.hip): that is only the
        // reference's value while the luma row is a convex combination -- non-negative weights that sum to 1 within float rounding.  Every
        // matrix derived above is; a limited-range or scaled luma row added later must not get past this line silently.
        const float ysum = p.my[0] + p.my[1] + p.my[2];
        if (!(p.my[0] >= 0.0f && p.my[1] >= 0.0f && p.my[2] >= 0.0f && ysum <= 1.0f + 1e-6f))
            return fail(AVIFGPU_formatBadParameters, "luma coefficients %g %g %g are not a convex combination: the unclipped luma of the streaming kernels does not apply",
                        (double)p.my[0], (double)p.my[1], (double)p.my[2]);
    }
    return 0;
}

// plane -> (rows in this tile, bytes per row actually written)
void write_plane_extent(const avifgpu_write_desc* d, const WriteGeom& g, int plane, int nrows, int& rows, int64_t& row_bytes)
{
    const int ssz = g.dst16 ? 2 : 1;
    if (d->output == AVIFGPU_OUT_REFERENCE && g.color) { rows = nrows; row_bytes = (int64_t)d->width * d->planes * ssz; return; }
    if (d->output == AVIFGPU_OUT_YCBCR && (plane == 1 || plane == 2)) {
        rows = (nrows + g.ys) >> g.ys; row_bytes = (int64_t)((d->width + g.xs) >> g.xs) * ssz; return;
    }
    rows = nrows; row_bytes = (int64_t)d->width * ssz;
}

bool write_plane_used(const avifgpu_write_desc* d, const WriteGeom& g, int plane)
{
    if (d->output == AVIFGPU_OUT_REFERENCE) return g.color ? plane == 0 : (plane == 0 || (plane == 3 && g.alpha));
    return plane < 3 || g.alpha;
}

// ---- read-side validation (runtime_error / OSErr conditions of ReadHeifImage.cpp) --------------------
int transfer_from_tc(int tc)
{
    switch (tc) {                                       // ColorTransfer.cpp:47-67
    case AVIFGPU_TC_PQ: return AVIFGPU_TRANSFER_PQ;
    case AVIFGPU_TC_HLG: return AVIFGPU_TRANSFER_HLG;
    case AVIFGPU_TC_SMPTE428: return AVIFGPU_TRANSFER_SMPTE428;
    default: return -1;
    }
}

int check_read(const avifgpu_read_desc* d, int row0, int nrows, ReadGeom& g)
{
    if (!d) return fail(AVIFGPU_formatBadParameters, "null descriptor");
    if (d->width <= 0 || d->height <= 0) return fail(AVIFGPU_formatBadParameters, "bad image size");
    if (row0 < 0 || nrows < 0 || (int64_t)row0 + nrows > d->height) return fail(AVIFGPU_formatBadParameters, "rows outside image");
    if (d->depth != 8 && d->depth != 16 && d->depth != 32) return fail(AVIFGPU_formatBadParameters, "unsupported host depth %d", d->depth);
    if (d->bit_depth != 8 && d->bit_depth != 10 && d->bit_depth != 12 && d->bit_depth != 16)
        return fail(AVIFGPU_readErr, "The image has an unsupported bit depth, must be 8, 10, 12 or 16.");           // YuvLookupTables.cpp:118-124
    if ((d->depth == 8) != (d->bit_depth == 8)) return fail(AVIFGPU_readErr, "host depth %d cannot carry %d-bit planes", d->depth, d->bit_depth);
    if (d->colorspace != AVIFGPU_COLORSPACE_YCBCR && d->colorspace != AVIFGPU_COLORSPACE_RGB && d->colorspace != AVIFGPU_COLORSPACE_MONOCHROME)
        return fail(AVIFGPU_readErr, "Unsupported image color space, expected RGB.");                               // ReadHeifImage.cpp:575-578
    if (d->alpha_state < AVIFGPU_ALPHA_NONE || d->alpha_state > AVIFGPU_ALPHA_PREMULTIPLIED) return fail(AVIFGPU_formatBadParameters, "bad alpha_state");
    g.alpha = d->alpha_state != AVIFGPU_ALPHA_NONE;
    g.xs = g.ys = 0; g.transfer = AVIFGPU_TRANSFER_PQ;
    const bool mono = d->colorspace == AVIFGPU_COLORSPACE_MONOCHROME;
    g.nch = (mono ? 1 : 3) + (g.alpha ? 1 : 0);
    if (d->colorspace == AVIFGPU_COLORSPACE_YCBCR) {
        chroma_shift(d->chroma, g.xs, g.ys);            // GetChromaShift: anything else -> (0,0), ReadHeifImage.cpp:52-81
        if (g.ys && (row0 & 1)) return fail(AVIFGPU_formatBadParameters, "4:2:0 tiles must start on an even row");
    }
    if (d->depth == 32) {
        if (!d->has_nclx) return fail(AVIFGPU_readErr, "The nclxProfile is null.");                                 // ReadHeifImage.cpp:870-873, :956-959
        g.transfer = transfer_from_tc(d->transfer_characteristics);
        if (g.transfer < 0) return fail(AVIFGPU_readErr, "Unsupported NCLX transfer characteristic.");             // ColorTransfer.cpp:63
        if (mono && g.transfer != AVIFGPU_TRANSFER_PQ) return fail(AVIFGPU_readErr, "Unsupported color transfer function."); // YuvDecode.cpp:219-220
        if (g.transfer == AVIFGPU_TRANSFER_PQ && d->pq_peak_nits < 1) return fail(AVIFGPU_formatBadParameters, "bad pq_peak_nits");
    }
    return 0;
}

int fill_read_params(const avifgpu_read_desc* d, int nrows, const ReadGeom& g, ReadParams& p)
{
    memset(&p, 0, sizeof(p));
    p.width = d->width; p.nrows = nrows; p.bits = d->bit_depth; p.maxc = (1 << d->bit_depth) - 1;
    p.full_range = d->has_nclx ? (d->full_range_flag != 0) : 1;                                                    // YuvLookupTables.cpp:140
    const int matrix = d->has_nclx ? d->matrix_coefficients : AVIFGPU_MATRIX_BT601;                                // :141
    p.identity_lut = (d->colorspace == AVIFGPU_COLORSPACE_YCBCR) && matrix == AVIFGPU_MATRIX_RGB_GBR;              // :145
    p.premultiplied = d->alpha_state == AVIFGPU_ALPHA_PREMULTIPLIED;
    p.transfer = g.transfer;
    float k[3]; yuv_coefficients(d->has_nclx, d->matrix_coefficients, d->color_primaries, k);
    p.kr = k[0]; p.kg = k[1]; p.kb = k[2];
    // Every kg the reference's tables can produce (5 matrix rows + 10 chromaticity-derived rows).  For these divisors
    // tools/divcheck.hip proved on the GPU, for all 1.7e9 floats with 2^-100 <= |x| < 8, that
    //   q0 = x*r;  q = fma(fma(-q0, kg, x), r, q0)   with r = RN(1/kg)
    // is bit-identical to the IEEE quotient x / kg (profiles/r01/divcheck.txt).  Anything else keeps IEEE division.
    static const uint32_t kVerifiedKg[] = { 0x3f371759u, 0x3f170a3du, 0x3f1645a1u, 0x3f3374bcu, 0x3f2d9169u, 0x3f37154au, 0x3f161fb4u,
                                            0x3f34e753u, 0x3f3378a8u, 0x3f2da76au, 0x3f2d9147u, 0x3f800000u, 0x3f38ba77u, 0x3f3115c6u, 0x3f2c18a0u };
    uint32_t kg_bits; memcpy(&kg_bits, &p.kg, 4);
    p.fast_div = 0;
    for (uint32_t v : kVerifiedKg) if (v == kg_bits) p.fast_div = 1;
    if (g_hot_variant & 128) p.fast_div = 0;                     // bit 7 of the tuning word: tests exercise the fallback (an environment read until round 6)
    p.rcp_kg = 1.0f / p.kg;
    p.maxcf = (float)p.maxc;
    p.rcp_maxc = (float)(1.0 / (double)p.maxc);
    p.rcp_maxc_lo = (float)(1.0 / (double)p.maxc - (double)p.rcp_maxc);
    if (d->depth == 32) {
        p.pq_mult = 10000.0f / (float)(d->pq_peak_nits > 0 ? d->pq_peak_nits : 1);                                 // ColorTransfer.cpp:114
        p.pq_log2_mult = (float)std::log2((double)p.pq_mult);
        p.hlg_ootf = d->hlg_apply_ootf != 0;
        p.hlg_gamma_m1 = d->hlg_display_gamma - 1.0f;
        p.hlg_peak = (float)d->hlg_peak_nits;
        if (g.transfer == AVIFGPU_TRANSFER_HLG && p.hlg_ootf && d->colorspace != AVIFGPU_COLORSPACE_MONOCHROME) {
            switch (d->color_primaries) {               // GetHLGLumaCoefficients, ColorTransfer.cpp:31-45
            case AVIFGPU_PRIMARIES_BT709:  p.hlg_luma[0] = 0.2126f; p.hlg_luma[1] = 0.7152f; p.hlg_luma[2] = 0.0722f; break;
            case AVIFGPU_PRIMARIES_BT470BG:
            case AVIFGPU_PRIMARIES_BT601:  p.hlg_luma[0] = 0.299f;  p.hlg_luma[1] = 0.587f;  p.hlg_luma[2] = 0.114f;  break;
            case AVIFGPU_PRIMARIES_BT2020: p.hlg_luma[0] = 0.2627f; p.hlg_luma[1] = 0.6780f; p.hlg_luma[2] = 0.0593f; break;
            default: return fail(AVIFGPU_readErr, "Unsupported color primaries for the HLG Luma Coefficients ");
            }
        }
    }
    return 0;
}

bool read_plane_used(const avifgpu_read_desc* d, const ReadGeom& g, int plane)
{
    if (plane == 3) return g.alpha;
    if (d->colorspace == AVIFGPU_COLORSPACE_MONOCHROME) return plane == 0;
    return true;
}

void read_plane_extent(const avifgpu_read_desc* d, const ReadGeom& g, int plane, int nrows, int& rows, int64_t& row_bytes)
{
    const int ssz = d->bit_depth > 8 ? 2 : 1;
    if (d->colorspace == AVIFGPU_COLORSPACE_YCBCR && (plane == 1 || plane == 2)) {
        rows = (nrows + g.ys) >> g.ys; row_bytes = (int64_t)((d->width + g.xs) >> g.xs) * ssz; return;
    }
    rows = nrows; row_bytes = (int64_t)d->width * ssz;
}

// Buffer checks shared by the direct (device-pointer) entry and the staged (host-pointer) path.
int check_write_buffers(const avifgpu_write_desc* d, const WriteGeom& g, int nrows, const void* src, int64_t src_row_bytes,
                        void* const dst[4], const int64_t dst_stride[4])
{
    if (!src || !dst || !dst_stride) return fail(AVIFGPU_formatBadParameters, "null buffer");
    const int64_t min_src_row = (int64_t)d->width * d->planes * (d->depth / 8);
    if (src_row_bytes < min_src_row) return fail(AVIFGPU_formatBadParameters, "src_row_bytes %lld < %lld", (long long)src_row_bytes, (long long)min_src_row);
    for (int pl = 0; pl < 4; ++pl) {
        if (!write_plane_used(d, g, pl)) continue;
        int rows; int64_t rb; write_plane_extent(d, g, pl, nrows, rows, rb);
        if (!dst[pl]) return fail(AVIFGPU_formatBadParameters, "destination plane %d is null", pl);
        if (dst_stride[pl] < rb) return fail(AVIFGPU_formatBadParameters, "dst_stride[%d] %lld < %lld", pl, (long long)dst_stride[pl], (long long)rb);
    }
    return 0;
}

int check_read_buffers(const avifgpu_read_desc* d, const ReadGeom& g, int nrows, const void* const src[4], const int64_t src_stride[4],
                       const void* dst, int64_t dst_row_bytes)
{
    if (!src || !src_stride || !dst) return fail(AVIFGPU_formatBadParameters, "null buffer");
    const int64_t min_dst_row = (int64_t)d->width * g.nch * (d->depth / 8);
    if (min_dst_row > 0x7fffffffLL) return fail(AVIFGPU_memFullErr, "rowBytes exceeds int32");                      // SetupFormatRecord, ReadHeifImage.cpp:40-47
    if (dst_row_bytes < min_dst_row) return fail(AVIFGPU_formatBadParameters, "dst_row_bytes too small");
    for (int pl = 0; pl < 4; ++pl) {
        if (!read_plane_used(d, g, pl)) continue;
        int rows; int64_t rb; read_plane_extent(d, g, pl, nrows, rows, rb);
        if (!src[pl]) return fail(AVIFGPU_formatBadParameters, "source plane %d is null", pl);
        if (src_stride[pl] < rb) return fail(AVIFGPU_formatBadParameters, "src_stride[%d] too small", pl);
    }
    return 0;
}

} // namespace avifgpu

namespace {

const char* const kNoDevice = "avifgpu_init has not succeeded: no HIP device bound (no CPU fallback)";

int write_rows_any(const avifgpu_write_desc* d, const IccArgs& icc, int32_t row0, int32_t nrows, const void* src, int64_t src_row_bytes,
                   void* const dst[4], const int64_t dst_stride[4], int32_t mem_kind, void* stream)
{
    g_err[0] = 0;
    WriteGeom g;
    int err = check_write(d, row0, nrows, g);
    if (err) return err;
    if ((err = check_write_buffers(d, g, nrows, src, src_row_bytes, dst, dst_stride))) return err;
    if (context_count() == 0) return fail(AVIFGPU_formatBadParameters, "%s", kNoDevice);
    SaveStats stats;                               // the calling thread's armed statistics: a mismatch fails here, before anything is launched
    if ((err = save_stats_for_call(d, g, mem_kind, &stats))) return err;
    if (nrows == 0) return 0;
    if (icc.c16 || icc.s32 || icc.c8t) icc_epoch_for_call(row0, nrows);       // the device copies of these tables are re-verified once per device and epoch

    if (mem_kind == AVIFGPU_MEM_DEVICE) {
        // zero-copy: the kernel is enqueued on the caller's stream, on the caller's current device (where the pointers live)
        WriteParams p;
        if ((err = fill_write_params(d, row0, nrows, g, icc, p))) return err;
        hipStream_t st = (hipStream_t)stream;          // NULL = HIP's default stream, as in every HIP API
        p.src = (const uint8_t*)src; p.src_row_bytes = src_row_bytes;
        for (int pl = 0; pl < 4; ++pl) { p.dst[pl] = (uint8_t*)dst[pl]; p.dst_stride[pl] = dst_stride[pl]; }
        const hipError_t e = launch_write(p, d->depth, d->planes, g.dst16, d->output, g.xs, g.ys, g_hot_variant, st, g_kernel);
        if (e != hipSuccess) return hip_fail(e, "kernel launch", AVIFGPU_writErr);
        return launch_save_stats(d, g, row0, nrows, p, stats, st);   // behind it on the caller's stream, straight into the caller's device targets
    }
    if (mem_kind != AVIFGPU_MEM_HOST) return fail(AVIFGPU_formatBadParameters, "bad mem_kind %d", mem_kind);
    return write_rows_host(d, row0, nrows, src, src_row_bytes, dst, dst_stride, icc);
}

} // namespace

namespace avifgpu {
int write_rows_with_icc(const avifgpu_write_desc* d, const IccArgs& icc, int32_t row0, int32_t nrows, const void* src, int64_t src_row_bytes,
                        void* const dst[4], const int64_t dst_stride[4], int32_t mem_kind, void* stream)
{
    return write_rows_any(d, icc, row0, nrows, src, src_row_bytes, dst, dst_stride, mem_kind, stream);
}
} // namespace avifgpu

// ======================================================================================================
extern "C" {

int32_t avifgpu_abi_version(void) { return AVIFGPU_ABI_VERSION; }

const char* avifgpu_last_error(void) { return g_err; }
const char* avifgpu_last_kernel_name(void) { return g_kernel; }

void avifgpu_set_hot_variant(int32_t variant) { g_hot_variant = variant; }

int32_t avifgpu_init_devices(const int32_t* device_indices, int32_t count)
{
    g_err[0] = 0;
    if (const char* v = getenv("AVIFGPU_HOT_VARIANT")) g_hot_variant = (int)strtol(v, nullptr, 0);   // tuning only
    return contexts_init(device_indices, count);
}

int32_t avifgpu_init(int32_t device_index) { return avifgpu_init_devices(&device_index, 1); }

int32_t avifgpu_device_count(void) { return bound_device_count(); }

int32_t avifgpu_device_topology(int32_t index, avifgpu_device_info* out) { return device_topology(index, out); }
int32_t avifgpu_device_traffic_get(int32_t index, avifgpu_device_traffic* out)
{
    if (!out) return fail(AVIFGPU_formatBadParameters, "avifgpu_device_traffic_get: null result");
    return device_traffic(index, out, false);
}
int32_t avifgpu_topology_plan(const char* sysfs_root, const char* const* pci_bus_ids, int32_t count, avifgpu_device_info* out)
{
    const int rc = topology_plan(sysfs_root, pci_bus_ids, count, out);
    if (rc == AVIFGPU_formatBadParameters) return fail(rc, "avifgpu_topology_plan: bad arguments");
    if (rc < 0) return fail(rc, "avifgpu_topology_plan: a device is missing from the sysfs tree or its CPU list does not parse");
    return rc;
}
int32_t avifgpu_device_traffic_reset(void)
{
    for (int i = 0; device_traffic(i, nullptr, true) == 0; ++i) {}
    return 0;
}
int32_t avifgpu_topology_probe(const char* sysfs_root, const char* pci_bus_id, int32_t* numa_node, char* cpulist, int32_t cpulist_len)
{
    return topology_probe_c(sysfs_root, pci_bus_id, numa_node, cpulist, cpulist_len);
}

void avifgpu_shutdown(void)
{
    if (context_count() == 0) return;
    contexts_shutdown();                               // joins the workers: nothing staged is in flight any more
    int n = 0;
    if (hipGetDeviceCount(&n) == hipSuccess) {         // caller-stream (device-pointer) launches may still read the cached tables
        int cur = -1;
        (void)hipGetDevice(&cur);
        for (int dev = 0; dev < n; ++dev) { if (hipSetDevice(dev) == hipSuccess) (void)hipDeviceSynchronize(); }
        if (cur >= 0) (void)hipSetDevice(cur);
    }
    release_device_caches();
    release_open_staging();
}

int32_t avifgpu_get_yuv_coefficients(int32_t has_nclx, int32_t matrix_coefficients, int32_t color_primaries, float out[3])
{
    if (!out) return fail(AVIFGPU_formatBadParameters, "null output");
    yuv_coefficients(has_nclx, matrix_coefficients, color_primaries, out);
    return 0;
}

int32_t avifgpu_read_max_value(const avifgpu_read_desc* d)
{
    if (!d) return 0;
    if (d->colorspace == AVIFGPU_COLORSPACE_RGB) return (1 << d->bit_depth) - 1;        // ReadHeifImage.cpp:744-747
    return 32768;                                                                     // :206, :499
}

int32_t avifgpu_write_plane_count(const avifgpu_write_desc* d)
{
    WriteGeom g;
    if (check_write(d, 0, 0, g)) return 0;
    return g.nplanes;
}

int32_t avifgpu_write_plane_geometry(const avifgpu_write_desc* d, int32_t plane, int32_t* width, int32_t* height,
                                     int32_t* bytes_per_sample, int32_t* samples_per_pixel)
{
    WriteGeom g;
    const int err = check_write(d, 0, 0, g);
    if (err) return err;
    if (plane < 0 || plane > 3 || !write_plane_used(d, g, plane)) return fail(AVIFGPU_formatBadParameters, "plane %d not produced", plane);
    const bool chroma = d->output == AVIFGPU_OUT_YCBCR && (plane == 1 || plane == 2);
    if (width) *width = chroma ? (d->width + g.xs) >> g.xs : d->width;
    if (height) *height = chroma ? (d->height + g.ys) >> g.ys : d->height;
    if (bytes_per_sample) *bytes_per_sample = g.dst16 ? 2 : 1;
    if (samples_per_pixel) *samples_per_pixel = (d->output == AVIFGPU_OUT_REFERENCE && g.color) ? d->planes : 1;
    return 0;
}

int64_t avifgpu_write_algorithmic_bytes(const avifgpu_write_desc* d, int32_t nrows)
{
    WriteGeom g;
    if (check_write(d, 0, 0, g)) return 0;
    int64_t total = (int64_t)nrows * d->width * d->planes * (d->depth / 8);
    for (int pl = 0; pl < 4; ++pl) {
        if (!write_plane_used(d, g, pl)) continue;
        int rows; int64_t rb; write_plane_extent(d, g, pl, nrows, rows, rb);
        total += rows * rb;
    }
    return total;
}

int64_t avifgpu_read_algorithmic_bytes(const avifgpu_read_desc* d, int32_t nrows)
{
    ReadGeom g;
    if (check_read(d, 0, 0, g)) return 0;
    int64_t total = (int64_t)nrows * d->width * g.nch * (d->depth / 8);
    for (int pl = 0; pl < 4; ++pl) {
        if (!read_plane_used(d, g, pl)) continue;
        int rows; int64_t rb; read_plane_extent(d, g, pl, nrows, rows, rb);
        total += rows * rb;
    }
    return total;
}

// SMPTE ST 2084 EOTF, exact rational constants, double: code value in [0, 1] -> cd/m2
static double pq_eotf_nits(double e)
{
    const double m1 = 2610.0 / 16384.0, m2 = 2523.0 / 4096.0 * 128.0;
    const double c1 = 3424.0 / 4096.0, c2 = 2413.0 / 4096.0 * 32.0, c3 = 2392.0 / 4096.0 * 32.0;
    const double ep = pow(e, 1.0 / m2);
    const double num = ep - c1 > 0.0 ? ep - c1 : 0.0;
    return 10000.0 * pow(num / (c2 - c3 * ep), 1.0 / m1);
}

int32_t avifgpu_light_level_from_histogram(const uint64_t* bins, int32_t bit_depth, int32_t transfer, double percentile,
                                           avifgpu_content_light_level* out)
{
    g_err[0] = 0;
    if (!bins || !out) return fail(AVIFGPU_formatBadParameters, "avifgpu_light_level_from_histogram: null argument");
    if (bit_depth != 10 && bit_depth != 12) return fail(AVIFGPU_formatBadParameters, "avifgpu_light_level_from_histogram: bit depth %d is not 10 or 12", bit_depth);
    if (transfer != AVIFGPU_TRANSFER_PQ)
        return fail(AVIFGPU_formatBadParameters, "avifgpu_light_level_from_histogram: transfer %d: only PQ codes are absolute luminance", transfer);
    if (!(percentile > 0.0 && percentile <= 1.0)) return fail(AVIFGPU_formatBadParameters, "avifgpu_light_level_from_histogram: percentile outside (0, 1]");
    const int nbins = 1 << bit_depth;
    uint64_t n = 0;
    for (int c = 0; c < nbins; ++c) n += bins[c];
    if (n == 0) return fail(AVIFGPU_formatBadParameters, "avifgpu_light_level_from_histogram: the histogram is empty");
    const double need = ceil(percentile * (double)n);
    const double maxv = (double)(nbins - 1);
    uint64_t cum = 0;
    int cp = -1;
    double sum = 0.0;
    for (int c = 0; c < nbins; ++c) {                       // ascending code order
        if (!bins[c]) continue;
        cum += bins[c];
        if (cp < 0 && (double)cum >= need) cp = c;
        sum += (double)bins[c] * pq_eotf_nits((double)c / maxv);
    }
    if (cp < 0) { for (int c = nbins - 1; c >= 0; --c) if (bins[c]) { cp = c; break; } }     // ceil(p n) rounded past n in double: the highest non-empty bin
    out->max_code = cp;
    out->pixels = n;
    out->max_cll_nits = pq_eotf_nits((double)cp / maxv);
    out->max_fall_nits = sum / (double)n;
    const double a = floor(out->max_cll_nits + 0.5), b = floor(out->max_fall_nits + 0.5);
    out->max_cll = (uint16_t)(a > 65535.0 ? 65535.0 : a);
    out->max_fall = (uint16_t)(b > 65535.0 ? 65535.0 : b);
    return 0;
}

int32_t avifgpu_probe_histogram(const avifgpu_write_desc* d, int32_t twin, const void* src, int64_t src_row_bytes, uint64_t* bins, void* stream)
{
    g_err[0] = 0;
    WriteGeom g;
    int err = check_write(d, 0, d ? d->height : 0, g);
    if (err) return err;
    if (d->depth != 32 || !src || !bins || twin < 0 || twin > 2 || src_row_bytes < (int64_t)d->width * d->planes * 4)
        return fail(AVIFGPU_formatBadParameters, "avifgpu_probe_histogram: a depth-32 descriptor, device pointers and twin 0..2");
    if (context_count() == 0) return fail(AVIFGPU_formatBadParameters, "%s", kNoDevice);
    WriteParams p;
    if ((err = fill_write_params(d, 0, d->height, g, IccArgs(), p))) return err;
    p.src = (const uint8_t*)src; p.src_row_bytes = src_row_bytes;
    const hipError_t e = launch_write_hist(p, d->planes, reinterpret_cast<unsigned long long*>(bins), (hipStream_t)stream, twin);
    if (e != hipSuccess) return hip_fail(e, "avifgpu_probe_histogram (the twins take aligned RGB rows, PQ, no profile)", AVIFGPU_formatBadParameters);
    return 0;
}

int32_t avifgpu_write_rows(const avifgpu_write_desc* d, int32_t row0, int32_t nrows,
                           const void* src, int64_t src_row_bytes,
                           void* const dst[4], const int64_t dst_stride[4],
                           int32_t mem_kind, void* stream)
{
    return write_rows_any(d, IccArgs{}, row0, nrows, src, src_row_bytes, dst, dst_stride, mem_kind, stream);
}

int32_t avifgpu_write_rows_icc(const avifgpu_write_desc* d, const avifgpu_icc_transform* icc, int32_t row0, int32_t nrows,
                               const void* src, int64_t src_row_bytes, void* const dst[4], const int64_t dst_stride[4],
                               int32_t mem_kind, void* stream)
{
    IccArgs a; a.f32 = icc;
    return write_rows_any(d, a, row0, nrows, src, src_row_bytes, dst, dst_stride, mem_kind, stream);
}

int32_t avifgpu_write_rows_icc_sampled(const avifgpu_write_desc* d, const avifgpu_icc_sampled32* icc, int32_t row0, int32_t nrows,
                                       const void* src, int64_t src_row_bytes, void* const dst[4], const int64_t dst_stride[4],
                                       int32_t mem_kind, void* stream)
{
    IccArgs a; a.s32 = icc;
    return write_rows_any(d, a, row0, nrows, src, src_row_bytes, dst, dst_stride, mem_kind, stream);
}

int32_t avifgpu_write_rows_icc16(const avifgpu_write_desc* d, const avifgpu_icc_clut16* icc, int32_t row0, int32_t nrows,
                                 const void* src, int64_t src_row_bytes, void* const dst[4], const int64_t dst_stride[4],
                                 int32_t mem_kind, void* stream)
{
    IccArgs a; a.c16 = icc;
    return write_rows_any(d, a, row0, nrows, src, src_row_bytes, dst, dst_stride, mem_kind, stream);
}

int32_t avifgpu_write_rows_icc8(const avifgpu_write_desc* d, const avifgpu_icc_shaper8* icc, int32_t row0, int32_t nrows,
                                const void* src, int64_t src_row_bytes, void* const dst[4], const int64_t dst_stride[4],
                                int32_t mem_kind, void* stream)
{
    IccArgs a; a.s8 = icc;
    return write_rows_any(d, a, row0, nrows, src, src_row_bytes, dst, dst_stride, mem_kind, stream);
}

int32_t avifgpu_write_rows_icc8_table(const avifgpu_write_desc* d, const avifgpu_icc_clut16* icc, int32_t row0, int32_t nrows,
                                      const void* src, int64_t src_row_bytes, void* const dst[4], const int64_t dst_stride[4],
                                      int32_t mem_kind, void* stream)
{
    IccArgs a; a.c8t = icc;
    return write_rows_any(d, a, row0, nrows, src, src_row_bytes, dst, dst_stride, mem_kind, stream);
}

int32_t avifgpu_write_rows_icc_pipeline32(const avifgpu_write_desc* d, const avifgpu_icc_pipeline32* icc, int32_t row0, int32_t nrows,
                                          const void* src, int64_t src_row_bytes, void* const dst[4], const int64_t dst_stride[4],
                                          int32_t mem_kind, void* stream)
{
    g_err[0] = 0;
    if (icc && !icc_pipeline32_stamped(icc))
        return fail(AVIFGPU_formatBadParameters, "the ICC stage program is not proven: unstamped, or altered since avifgpu_icc_pipeline32_prove");
    IccArgs a; a.p32 = icc;
    return write_rows_any(d, a, row0, nrows, src, src_row_bytes, dst, dst_stride, mem_kind, stream);
}

int32_t avifgpu_read_rows(const avifgpu_read_desc* d, int32_t row0, int32_t nrows,
                          const void* const src[4], const int64_t src_stride[4],
                          void* dst, int64_t dst_row_bytes,
                          int32_t mem_kind, void* stream)
{
    g_err[0] = 0;
    ReadGeom g;
    int err = check_read(d, row0, nrows, g);
    if (err) return err;
    if ((err = check_read_buffers(d, g, nrows, src, src_stride, dst, dst_row_bytes))) return err;
    if (context_count() == 0) return fail(AVIFGPU_formatBadParameters, "%s", kNoDevice);
    if (nrows == 0) return 0;

    if (mem_kind == AVIFGPU_MEM_DEVICE) {
        ReadParams p;
        if ((err = fill_read_params(d, nrows, g, p))) return err;
        hipStream_t st = (hipStream_t)stream;          // NULL = HIP's default stream
        for (int pl = 0; pl < 4; ++pl) { p.src[pl] = (const uint8_t*)src[pl]; p.src_stride[pl] = src_stride[pl]; }
        p.dst = (uint8_t*)dst; p.dst_row_bytes = dst_row_bytes;
        const hipError_t e = launch_read(p, d->colorspace, d->depth, g.alpha, g.xs, g.ys, st, g_kernel);
        if (e != hipSuccess) return hip_fail(e, "kernel launch", AVIFGPU_readErr);
        return 0;
    }
    if (mem_kind != AVIFGPU_MEM_HOST) return fail(AVIFGPU_formatBadParameters, "bad mem_kind %d", mem_kind);
    return read_rows_host(d, row0, nrows, src, src_stride, dst, dst_row_bytes);
}

/* The math-free twin of the kernel avifgpu_read_rows(MEM_DEVICE) would launch for this descriptor (read_kernels.hip, TWIN): the
 * same loads, table copy, LDS transpose and stores, no decode; dst receives meaningless bytes.  Diagnostic hook for the measured
 * ceiling of a read pattern (tools/bench_configs.py); available for the 4:2:x colour opens to 8-bit and f32 (PQ) hosts on 16-byte
 * aligned buffers, AVIFGPU_formatBadParameters otherwise. */
int32_t avifgpu_probe_pattern_read(const avifgpu_read_desc* d, int32_t row0, int32_t nrows, const void* const src[4], const int64_t src_stride[4],
                                   void* dst, int64_t dst_row_bytes, void* stream)
{
    g_err[0] = 0;
    ReadGeom g;
    int err = check_read(d, row0, nrows, g);
    if (err) return err;
    if ((err = check_read_buffers(d, g, nrows, src, src_stride, dst, dst_row_bytes))) return err;
    if (context_count() == 0) return fail(AVIFGPU_formatBadParameters, "%s", kNoDevice);
    if (nrows == 0) return 0;
    ReadParams p;
    if ((err = fill_read_params(d, nrows, g, p))) return err;
    for (int pl = 0; pl < 4; ++pl) { p.src[pl] = (const uint8_t*)src[pl]; p.src_stride[pl] = src_stride[pl]; }
    p.dst = (uint8_t*)dst; p.dst_row_bytes = dst_row_bytes;
    p.twin = 1;
    const hipError_t e = launch_read(p, d->colorspace, d->depth, g.alpha, g.xs, g.ys, (hipStream_t)stream, g_kernel);
    if (e == hipErrorInvalidValue) return fail(AVIFGPU_formatBadParameters, "pattern probe: no twin for this configuration (4:2:x colour, no alpha, 8-bit or f32 PQ host, 16-byte aligned buffers)");
    if (e != hipSuccess) return hip_fail(e, "kernel launch", AVIFGPU_readErr);
    return 0;
}

} // extern "C"
