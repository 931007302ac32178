// write_dispatch.h -- which kernel a save takes: the decision between the descriptor and hipLaunchKernelGGL, with no HIP call.
//
// decide_write() below is what launch_write() (write_kernels.hip) asks: it reads WriteParams, the descriptor's geometry and the tuning
// word and returns a WriteLaunch -- the kernel family, the runtime values of its template arguments, the grid, the label.  The launch
// side is a switch from that to the instantiation.  tools/write_dispatch_check.cpp holds it, on the CPU, to the labels recorded from
// the library before the choice lived here (tests/golden/write_dispatch_labels.json.gz; tests/test_write_dispatch.py).
//
// The CANDIDATES are tried in the order of kWriteCandidatesInt / kWriteCandidatesF32 -- the order is the priority -- and each one's rule sits in one function:
// its predicate clause by clause, its work units, its label; take() turns the units into the grid.  A candidate whose units do not
// fit its kernel's 32-bit index hands the tile on to the next one; the generic kernel (write_px) takes whatever is left.
//
// The compile-time switches of the choice and the workgroup shapes it counts with have their defaults here (write_kernels.hip describes them).
#pragma once
#include <stdint.h>
#include <stdio.h>
#include <string.h>

#include "../../include/avifgpu.h"
#include "kernel_params.h"

// ---- switches of the choice: which streaming kernels are candidates at all ----------------------------------------------------------
#ifndef AG_WRITE_PART
#define AG_WRITE_PART 0         /* the code object being compiled (write_kernels.hip); 0 = all in one */
#endif
#ifndef AG_COPY8
#define AG_COPY8 1              /* 8-bit identity hand-off as a copy */
#endif
// AG_IREF8 (round 5): RGBA8 documents through the interleaved hand-off (what integration/ asks for by default; the integer premultiply where the
// alpha state asks for it) on the streaming hand-off kernel: 0.66 -> 0.73 of 8 TB/s on fresh data.  Round 2 had kept every 8-bit document on
// the generic kernel on one-set-loop figures (0.75-0.77 there).  The RGB8 hand-off -- a plain copy -- stays generic: 0.76 against 0.71 here.
#ifndef AG_IREF8
#define AG_IREF8 1
#endif
#ifndef AG_RGB8_HOT
#define AG_RGB8_HOT 1
#endif
#ifndef AG_RGBA16_TO8
#define AG_RGBA16_TO8 1
#endif
#ifndef AG_ICC1_HOT
#define AG_ICC1_HOT 1
#endif
#ifndef AG_ICC2_HOT
#define AG_ICC2_HOT 1
#endif
#ifndef AG_ICC_FASTPOW
#define AG_ICC_FASTPOW 1        /* icc_pow32, write_kernels.hip */
#endif
#ifndef AG_RGBA_HOT_ENABLE
#define AG_RGBA_HOT_ENABLE 1
#endif
#ifndef AG_FLAT
#define AG_FLAT 1
#endif
#ifndef AG_SUB_SPW2
#define AG_SUB_SPW2 1                  /* 4:2:2 tiles of whole 512-pixel spans: two spans per wave (write_rgb32_ycbcr_sub_hot's loop) */
#endif
#ifndef AG_SUB_SPW2_MIN_SPANS
#define AG_SUB_SPW2_MIN_SPANS 32768
#endif
#ifndef AG_RGB16_MIN_PX
#define AG_RGB16_MIN_PX 0
#endif
#ifndef AG_RGBA16_MIN_PX
#define AG_RGBA16_MIN_PX 0
#endif
// Build-time override of the per-launch choice of the PQ form (WriteParams::pq_close): 0 = the compact form everywhere, 2 = the close
// form everywhere, 1 = as the descriptor says (AUTO = the close form at every depth since round 4).
#ifndef AG_PQ_HI
#define AG_PQ_HI 1
#endif

// ---- workgroup shapes and grid caps the choice counts with (each described at its kernel) ------------------------------------------
#ifndef AG_COPY_BLOCK
#define AG_COPY_BLOCK 128
#endif
#ifndef AG_COPY_K
#define AG_COPY_K 2               /* 16-byte vectors per lane and wave trip */
#endif
#ifndef AG_STREAM_BLOCK
#define AG_STREAM_BLOCK 128
#endif
#ifndef AG_F32_REF_BLOCK
#define AG_F32_REF_BLOCK 64
#endif
#ifndef AG_GA_BLOCK
#define AG_GA_BLOCK 256
#endif
#ifndef AG_F32_STREAM_BLOCK
#define AG_F32_STREAM_BLOCK 256
#endif
#ifndef AG_HOT444_BLOCK
#define AG_HOT444_BLOCK AG_F32_STREAM_BLOCK
#endif
#ifndef AG_HOT444_BLOCK_LINES
#define AG_HOT444_BLOCK_LINES 128
#endif
#ifndef AG_RGBA_HOT_PXL
#define AG_RGBA_HOT_PXL 4
#endif
#ifndef AG_RGBA_STREAM_BLOCK
#define AG_RGBA_STREAM_BLOCK 256
#endif
#ifndef AG_RGB16_NS
#define AG_RGB16_NS 1      /* 2 and 4 measured 2-9 % slower on every geometry (profiles/r02/rgb16_streaming_geometry.txt) */
#endif
#ifndef AG_RGB8_16_WAVES
#define AG_RGB8_16_WAVES 2         /* waves per workgroup of write_rgb8_ycbcr16_hot */
#endif
#ifndef AG_W8_NC
#define AG_W8_NC 8
#endif
#ifndef AG_W16_NC
#define AG_W16_NC 4        /* chroma samples per lane of the generic kernel into u16 planes (no ICC) */
#endif
#ifndef AG_W8_NC_ALPHA
#define AG_W8_NC_ALPHA 4
#endif
#ifndef AG_ICC_TAB_NC2
#define AG_ICC_TAB_NC2 0        /* 1 = the table-driven ICC stages (5, 7) with sub-sampled chroma: 2 chroma samples per lane (A/B hook) */
#endif
#ifndef AG_RGBA_BLOCK_CAP
#define AG_RGBA_BLOCK_CAP (256LL * 512)       // C5 (1 M spans): 1.18 ms at 16k blocks, 1.01 at 64k, 0.99 at 128k, 1.01 at 256k
#endif
#ifndef AG_STREAM_BLOCK_CAP
#define AG_STREAM_BLOCK_CAP (256LL * 512)     // grid cap of the streaming kernels (grid-stride beyond it); see AG_WRITE_BLOCK_CAP
#endif
// 8192^2 frames are indifferent to 16k...128k blocks; 16384^2 frames are not (RGB16 -> 12-bit 4:4:4: 0.684 ms at 16k,
// 0.543 ms at 128k -- profiles/r01/ab_write_variants.txt): keep a wave's grid-stride loop short
#ifndef AG_WRITE_BLOCK_CAP
#define AG_WRITE_BLOCK_CAP (256LL * 512)
#endif
// The parametric ICC variants set up ~60 wave-uniform parameters (and their pow table) per workgroup: a capped grid lets a wave
// run several groups per set-up.
#ifndef AG_ICC_BLOCK_CAP
#define AG_ICC_BLOCK_CAP (256LL * 32)      /* 8192^2: 0.405 ms uncapped, 0.390 at 16k, 0.371 at 8k / 4k, 0.388 at 2k, 0.416 at 1k blocks (variant 2) */
#endif
// A workgroup of the generic kernel that evaluates PQ in its close form starts by copying the exponent table to LDS (2 KiB; 4 KiB when
// the figures below were taken): at one footprint group per workgroup that was 4 KiB of LDS fill per 6 KiB of pixels for a gray f32 document.  A capped grid lets a workgroup run several
// groups per copy: Gray32 -> 10-bit PQ at 8192^2 on fresh data 0.528 of 8 TB/s uncapped (65 536 blocks), 0.623 at 8192 or 16 384 blocks,
// 0.59 at 32 768 (round 5; the streaming kernels, whose waves own 6-12 KiB each, prefer one span per wave: profiles/r05/prefetch_pipeline_ab.txt).
#ifndef AG_PQ_TABLE_BLOCK_CAP
#define AG_PQ_TABLE_BLOCK_CAP (256LL * 32)
#endif

namespace avifgpu {

constexpr int kCopyWaves = AG_COPY_BLOCK / 64;
constexpr int kStreamWaves = AG_STREAM_BLOCK / 64;
constexpr int kGaWaves = AG_GA_BLOCK / 64;
constexpr int kF32RefWaves = AG_F32_REF_BLOCK / 64;
constexpr int kF32Waves = AG_F32_STREAM_BLOCK / 64;
constexpr int kRgbaWaves = AG_RGBA_STREAM_BLOCK / 64;

// kTransferPqHi: the PQ evaluation that reproduces more of the reference's bits, as a kernel-side transfer id of its own (write_kernels.hip)
constexpr int kTransferPqHi = 4;
inline bool pq_hi_launch(const WriteParams& p) { return AG_PQ_HI == 2 || (AG_PQ_HI == 1 && p.pq_close); }
// the kernel-side transfer id of a 32-bit document's launch
inline int transfer_id(const WriteParams& p)
{
    switch (p.transfer) {
    case AVIFGPU_TRANSFER_PQ:       return pq_hi_launch(p) ? kTransferPqHi : AVIFGPU_TRANSFER_PQ;
    case AVIFGPU_TRANSFER_HLG:      return AVIFGPU_TRANSFER_HLG;
    case AVIFGPU_TRANSFER_SMPTE428: return AVIFGPU_TRANSFER_SMPTE428;
    default:                        return AVIFGPU_TRANSFER_CLIP;
    }
}

// ---- the generic kernel's shape ------------------------------------------------------------------------------------------------------
enum { kOutRefColor = 0, kOutRefGray = 1, kOutYcbcr = 2 };
// chroma samples per lane: 4 for u16 planes, AG_W8_NC for u8 planes (every plane store >= 8 / 4 bytes per lane)
// The parametric ICC variants (2, 4) carry ~300 instructions and up to 86 parameter VGPRs per pixel stream: with sub-sampled chroma
// 2 chroma samples per lane keep a 4:2:0 footprint at 8 pixels (16: 197 VGPRs, 2 waves/SIMD, 6.9 k instructions; measured
// 0.412 -> 0.370 ms).  4:4:4 keeps 4 pixels per lane (2 measured slower: 0.487 -> 0.507 ms, narrower loads and stores).
// ICC == 5 (the 16-bit table transform) saved to u8 planes: 4 chroma samples per lane like the u16 layouts.  With 8, a 4:2:0 footprint
// is 32 pixels x two 16-byte gathers each, all hoisted: 315 VGPRs = ONE wave per SIMD (profiles/r02/isa/resources.tsv); with 4 it is
// 16 pixels and the kernel fits 3-4 waves.
constexpr int write_shape_nc(bool dst16, int planes, int xs, int icc)
{
    return ((icc == 2 || icc == 4 || icc == 8 || ((icc == 5 || icc == 7) && AG_ICC_TAB_NC2)) && xs == 1) ? 2 : ((dst16 && icc == 0) ? AG_W16_NC : ((dst16 || icc == 5 || icc == 7) ? 4 : ((planes == 2 || planes == 4) ? AG_W8_NC_ALPHA : AG_W8_NC)));
}
template <bool DST16, int PLANES, int XS, int ICC = 0> struct WriteShape {
    static constexpr int NC = write_shape_nc(DST16, PLANES, XS, ICC);
    static constexpr int PXT = NC << XS;
};
// Workgroup size of the generic write kernel (its waves share only the per-workgroup tables).
// Round 5, fresh data (profiles/r05/read_samples_per_lane_fresh_data.txt, block 5): 256 threads stand for every generic kernel (128: 0...-20 %,
// 512: -1...-9 %) except the sampled-curve profile kernel (icc = 6, a code object of its own: part 36), whose workgroups copy up to 48 KiB of
// curve tables to LDS -- 512 threads halve the copies per pixel: 0.437 -> 0.384 ms at 8192^2 (+14 %).
#ifdef AG_WPX_BLOCK
constexpr int wpx_block(int) { return AG_WPX_BLOCK; }
#else
constexpr int wpx_block(int icc) { return (icc == 6 && AG_WRITE_PART != 0) ? 512 : 256; }
#define AG_WPX_BLOCK wpx_block(AG_WRITE_PART == 36 ? 6 : 0)
#endif

// ---- the decision -----------------------------------------------------------------------------------------------------------------------
enum WriteKernel : int {
    kWkEmpty = 0,                // nothing to launch: a tile without work units
    kWkCopyRows, kWkIntRef, kWkGa16, kWkRgb8, kWkRgb8To16, kWkRgba8, kWkRgb16, kWkRgba16, kWkRgba16Sub, kWkRgb16Sub,      // part 2
    kWkGa32, kWkRgba32Sub, kWkRgba32, kWkRgb32Sub,                                                                         // part 3
    kWkRgb32IccRef, kWkF32Ref, kWkRgb32Icc, kWkRgb32,                                                                      // part 1
    kWkPx                        // the generic kernel, in the part of its depth (and of its ICC stage)
};
struct WriteLaunch {
    int kernel = kWkEmpty;
    bool invalid = false;        // the generic kernel cannot index the tile, or the descriptor is one fill_write_params rejects: hipErrorInvalidValue
    // the runtime values of the family's template arguments (the rest are depth, planes, dst16, xs, ys, p.nearest, p.premultiply)
    int tr = AVIFGPU_TRANSFER_CLIP, icc = 0, out = kOutRefColor;     // kernel-side transfer id, ICC stage, write_px's kOut*
    bool aligned = false;        // write_px: every pointer and stride a multiple of 16
    bool px8 = false, nt = false, lines = false;     // write_rgb32_ycbcr444_hot: pixels per lane, non-temporal, the two-wave workgroup
    bool one = false;            // write_copy_rows_stream: the contiguous tile as one row
    long long units = 0;         // the grid: spans, waves or footprint groups,
    int waves = 0;               // waves per workgroup (write_px: threads / 64),
    long long cap = 0, need = 0, blocks = 0;     // the compile-time cap, workgroups of a one-trip launch, workgroups launched
    size_t lds = 0;              // dynamic LDS bytes
    bool flat = false;           // launched as one long row (decide_write: with *q, not p)
    char label[kLabelBytes];
    WriteLaunch() { label[0] = 0; }
};

// What the save is asked with, and what several rules read of it.
struct WriteAsk {
    const WriteParams& p; int depth, planes; bool dst16; int output, xs, ys, word;
    bool stream() const { return (word & 1) != 0; }
    bool ycbcr() const { return output == AVIFGPU_OUT_YCBCR; }
    long long rows_ys() const { return (p.nrows + (1 << ys) - 1) >> ys; }           // luma row pairs at 4:2:0
    long long spans(int px) const { return (long long)((p.width + px - 1) / px); }  // per row
    const WriteParams* operator->() const { return &p; }                            // a-> reads the tile, a. the ask
};

// Every address and stride of the source under src_mask, and of the planes of a set (bit pl of `planes`) under that set's mask.
inline bool aligned_to(const WriteParams& p, uintptr_t src_mask, unsigned planes, uintptr_t mask, unsigned planes2 = 0, uintptr_t mask2 = 0)
{
    uintptr_t bad = (reinterpret_cast<uintptr_t>(p.src) | (uintptr_t)p.src_row_bytes) & src_mask;
    for (int pl = 0; pl < 4; ++pl) {
        const uintptr_t bits = reinterpret_cast<uintptr_t>(p.dst[pl]) | (uintptr_t)p.dst_stride[pl];
        if (planes >> pl & 1) bad |= bits & mask;
        if (planes2 >> pl & 1) bad |= bits & mask2;
    }
    return bad == 0;
}
constexpr unsigned kPlane0 = 1, kPlanesYA = 1 | 8, kPlanesCbCr = 2 | 4, kPlanes3 = 1 | 2 | 4, kPlanes4 = 15;

// Work units -> grid and label tail, behind the candidate's finished label.  False: the units do not fit the kernel's 32-bit index
// (the grid-stride loop adds up to 8 x 65536 x 4 to it) and the next candidate gets the tile.
inline bool take(WriteLaunch& L, int kernel, const WriteAsk& a, long long units, int waves, long long cap, int units_per_wave = 1)
{
    if (units == 0) { L.kernel = kWkEmpty; return true; }
    if (!(units + 8LL * 65536 * 4 < 0x7fffffffLL)) return false;
    L.kernel = kernel; L.units = units; L.waves = waves; L.cap = cap;
    L.need = (units + (long long)waves * units_per_wave - 1) / ((long long)waves * units_per_wave);
    L.blocks = capped_blocks(L.need, cap, a.word);
    label_cap(L.label, L.blocks, L.need, cap);
    return true;
}
#define AG_LABEL(...) snprintf(L.label, kLabelBytes, __VA_ARGS__)

// The ICC stage a streaming kernel of 32-bit RGB(A) documents can carry, derived ONCE: linear curves (1), linear curves and the sRGB
// output curve (4, Clip saves), one simple parametric curve for R, G and B (2).  At most one holds: icc_same_simple excludes linear
// curves, 1 and 4 differ in icc_out.  A sampled profile (icc_s_tab) has none of them -- a sampled channel's icc_trc_linear stays 0
// and at least one channel is sampled (icc_tables.cpp:152, :294), icc_same_simple is false with icc.s32 (icc_tables.cpp:319) -- so the
// `p.icc_s_tab == nullptr` the interleaved hand-off's copy of this derivation carried said nothing; neither does a stage program
// (icc_trc_type 8, nothing else set: icc_tables.cpp:218).  The 4:4:4 RGBA kernel takes 4 only with AG_ICC_FASTPOW: kept, in its rule.
struct StreamIcc {
    bool none, icc1, icc4, icc2;
    int stage() const { return icc1 ? 1 : icc4 ? 4 : icc2 ? 2 : 0; }
    const char* tail() const { return icc1 ? " icc=1" : icc4 ? " icc=4" : icc2 ? " icc=2" : ""; }
};
inline StreamIcc stream_icc(const WriteParams& p)
{
    const bool lin = AG_ICC1_HOT && p.icc_trc_type[0] != 0 && p.icc_trc_linear[0] && p.icc_trc_linear[1] && p.icc_trc_linear[2];
    StreamIcc k;
    k.none = p.icc_trc_type[0] == 0;
    k.icc1 = lin && p.icc_out == 0;
    k.icc4 = lin && p.icc_out == 4 && p.transfer == AVIFGPU_TRANSFER_CLIP;
    k.icc2 = AG_ICC2_HOT && p.icc_trc_type[0] != 0 && p.icc_same_simple && p.icc_out == 0;
    return k;
}

// ---- the candidates: 8- and 16-bit documents (part 2) ---------------------------------------------------------------------------------
// 8-bit document, 8-bit hand-off, nothing to premultiply: the reference copies the bytes (round 6).  A wave owns 4 KiB of a row; a tile
// whose rows are contiguous on both sides is ONE row.
inline bool cand_copy_rows(const WriteAsk& a, WriteLaunch& L)
{
    if (!(AG_COPY8 && a.stream() && a->icc8_s1 == nullptr && a.depth == 8 && !a.dst16 && a->maxv == 255 && a.output == AVIFGPU_OUT_REFERENCE)) return false;
    if (!(a.planes == 3 || a.planes == 1 || (a.planes == 4 && !a->premultiply))) return false;
    if (!((((long long)a->width * a.planes) & 3) == 0 && aligned_to(a.p, 3, kPlane0, 3))) return false;
    long long row_bytes = (long long)a->width * a.planes, nrows = a->nrows;
    L.one = !(a.word & 16) && nrows > 1 && a->src_row_bytes == row_bytes && a->dst_stride[0] == row_bytes;
    if (L.one) { row_bytes *= nrows; nrows = 1; }
    AG_LABEL("write_copy_rows_stream<planes=%d>", a.planes);
    if (!take(L, kWkCopyRows, a, ((row_bytes + 1024 * AG_COPY_K - 1) / (1024 * AG_COPY_K)) * nrows, kCopyWaves, AG_STREAM_BLOCK_CAP * 4 / kCopyWaves)) return false;
    if (L.one && L.kernel != kWkEmpty) snprintf(L.label + strlen(L.label), kLabelBytes - strlen(L.label), " flat");
    return true;
}
// The interleaved hand-off of 16-bit documents and of RGBA8 (AG_IREF8), and Gray16 -> Y plane (elementwise too, round 5): rows of whole
// 16-byte vectors
inline bool cand_int_ref(const WriteAsk& a, WriteLaunch& L)
{
    if (!(a.stream() && a->icc16_clut == nullptr && a->icc8_s1 == nullptr && (a.depth == 16 || (AG_IREF8 && a.depth == 8 && a.planes == 4)))) return false;
    if (!((a.planes >= 3 && a.output == AVIFGPU_OUT_REFERENCE) || (a.planes == 1 && a.depth == 16))) return false;
    const long long row_bytes = (long long)a->width * a.planes * (a.depth / 8);
    if (!(row_bytes % 16 == 0 && aligned_to(a.p, 15, kPlane0, 15))) return false;
    AG_LABEL("write_int_ref_stream<depth=%d,planes=%d,dst16=%d>", a.depth, a.planes, (int)a.dst16);
    return take(L, kWkIntRef, a, ((row_bytes / 16 + 255) / 256) * a->nrows, kStreamWaves, AG_STREAM_BLOCK_CAP * 4 / kStreamWaves);
}
// Gray16 + alpha -> Y and Alpha u16 planes (round 5): widths of whole 4-pixel vectors, dword-aligned rows and planes
inline bool cand_ga16(const WriteAsk& a, WriteLaunch& L)
{
    if (!(a.depth == 16 && (a->width % 4) == 0 && a.stream() && a.planes == 2 && a.dst16 && a->dst[3] != nullptr && aligned_to(a.p, 3, kPlanesYA, 3))) return false;
    AG_LABEL("write_ga_stream<depth=16>");
    return take(L, kWkGa16, a, (((long long)a->width / 4 + 255) / 256) * a->nrows, kGaWaves, AG_STREAM_BLOCK_CAP * 4 / kGaWaves);
}
// what the three RGB(A)8 -> planes kernels share: widths of whole 8-pixel groups, dword-aligned rows and planes
inline bool rgb8_planes(const WriteAsk& a, int planes, unsigned set)
{
    return AG_RGB8_HOT && a.stream() && a->icc8_s1 == nullptr && a.depth == 8 && a.planes == planes && a.ycbcr() && (a->width % 8) == 0 && aligned_to(a.p, 3, set, 3);
}
// RGB8 -> u8 Y, Cb, Cr (the plug-in's default save; BASELINE C2): spans of 1024 pixels, four waves a workgroup (two at 4:2:0)
inline bool cand_rgb8(const WriteAsk& a, WriteLaunch& L)
{
    if (!(rgb8_planes(a, 3, kPlanes3) && !a.dst16 && a->maxv == 255)) return false;
    const int wpb = a.ys ? 2 : 4;
    AG_LABEL("write_rgb8_ycbcr_hot<xs=%d,ys=%d,nearest=%d>", a.xs, a.ys, (a.xs || a.ys) ? a->nearest : 0);
    return take(L, kWkRgb8, a, a.spans(1024) * a.rows_ys(), wpb, AG_STREAM_BLOCK_CAP * 4 / wpb);
}
// RGB8 -> u16 Y, Cb, Cr (round 6): an 8-bit document saved at 10 / 12 bit
inline bool cand_rgb8_to16(const WriteAsk& a, WriteLaunch& L)
{
    if (!(rgb8_planes(a, 3, kPlanes3) && a.dst16 && (a->maxv == 1023 || a->maxv == 4095))) return false;
    AG_LABEL("write_rgb8_ycbcr16_hot<xs=%d,ys=%d,nearest=%d>", a.xs, a.ys, (a.xs || a.ys) ? a->nearest : 0);
    return take(L, kWkRgb8To16, a, a.spans(1024) * a.rows_ys(), AG_RGB8_16_WAVES, AG_STREAM_BLOCK_CAP * 4 / AG_RGB8_16_WAVES);
}
// RGBA8 -> u8 Y, Cb, Cr, A (a transparent 8-bit document's save): spans of 512 pixels
inline bool cand_rgba8(const WriteAsk& a, WriteLaunch& L)
{
    if (!(rgb8_planes(a, 4, kPlanes4) && !a.dst16 && a->maxv == 255 && a->dst[3] != nullptr)) return false;
    AG_LABEL("write_rgba8_ycbcra_hot<xs=%d,ys=%d,nearest=%d,premultiply=%d>", a.xs, a.ys, (a.xs || a.ys) ? a->nearest : 0, a->premultiply);
    return take(L, kWkRgba8, a, a.spans(512) * a.rows_ys(), 4, AG_STREAM_BLOCK_CAP);
}
// what the four RGB(A)16 -> planes kernels share: u16 planes or the `to8` form, widths of whole 8-pixel groups, 16-byte aligned source rows
inline bool rgb16_planes(const WriteAsk& a, int planes)
{
    const bool to8 = planes == 4 ? (AG_RGBA16_TO8 && a->maxv == 255) : a->maxv == 255;
    return a.stream() && a->icc16_clut == nullptr && a.depth == 16 && a.planes == planes && (a.dst16 || to8) && a.ycbcr() && (a->width % 8) == 0;
}
// RGB16 -> Y, Cb, Cr 4:4:4 (BASELINE C3).  At every size since round 5 (AG_RGB16_MIN_PX = 0; word bit 3 took it below the gate): round 2
// had gated it to launches of >= 40 Mpx on one-set-loop figures; on fresh data the streaming kernel wins wherever it was gated off
// (profiles/r05/rgb16_streaming_gates_fresh_data.txt).  Both produce the same bytes (tests/test_gpu_kernel_equivalence.py).
inline bool cand_rgb16(const WriteAsk& a, WriteLaunch& L)
{
    if (!(rgb16_planes(a, 3) && a.xs == 0 && a.ys == 0 && ((long long)a->width * a->nrows >= AG_RGB16_MIN_PX || (a.word & 8)) && aligned_to(a.p, 15, kPlanes3, 15))) return false;
    AG_LABEL("write_rgb16_ycbcr444_hot<ns=%d%s>", AG_RGB16_NS, a.dst16 ? "" : ",to8");
    return take(L, kWkRgb16, a, a.spans(512) * a->nrows, kStreamWaves, AG_STREAM_BLOCK_CAP * 4 / kStreamWaves, AG_RGB16_NS);
}
// RGBA16 -> Y, Cb, Cr, A 4:4:4
inline bool cand_rgba16(const WriteAsk& a, WriteLaunch& L)
{
    if (!(rgb16_planes(a, 4) && a.xs == 0 && a.ys == 0 && ((long long)a->width * a->nrows >= AG_RGBA16_MIN_PX || (a.word & 8)) && a->dst[3] != nullptr &&
          aligned_to(a.p, 15, kPlanes4, 15))) return false;
    AG_LABEL("write_rgba16_ycbcra444_hot%s", a.dst16 ? "" : "<to8>");
    return take(L, kWkRgba16, a, a.spans(512) * a->nrows, kStreamWaves, AG_STREAM_BLOCK_CAP * 4 / kStreamWaves);
}
// RGBA16 -> Y, Cb, Cr (4:2:2 / 4:2:0), A: the plug-in's default save of a transparent 16-bit document (round 5, last series); the
// chroma planes' rows are half as long: 8-byte aligned
inline bool cand_rgba16_sub(const WriteAsk& a, WriteLaunch& L)
{
    if (!(rgb16_planes(a, 4) && a.xs == 1 && a->dst[3] != nullptr && aligned_to(a.p, 15, kPlanesYA, 15, kPlanesCbCr, 7))) return false;
    AG_LABEL("write_rgba16_ycbcra_sub_hot<ys=%d,nearest=%d%s>", a.ys, a->nearest, a.dst16 ? "" : ",to8");
    return take(L, kWkRgba16Sub, a, a.spans(512) * a.rows_ys(), kStreamWaves, AG_STREAM_BLOCK_CAP * 4 / kStreamWaves);
}
// RGB16 -> Y, Cb, Cr 4:2:2 / 4:2:0.  Any width of whole 8-pixel groups since round 5: round 2 kept rows with a ragged last span
// (6000, 7952 wide) on the generic kernel, "4-6 % faster" there in a one-set loop; on fresh data the streaming kernel is 4-6 % ahead
// on exactly those rows (7952 x 5304 4:2:0 0.64 -> 0.67, 4:2:2 0.72 -> 0.765, 6000 x 4000 4:2:0 0.61 -> 0.65).  Same bytes either way.
inline bool cand_rgb16_sub(const WriteAsk& a, WriteLaunch& L)
{
    if (!(rgb16_planes(a, 3) && a.xs == 1 && aligned_to(a.p, 15, kPlanes3, 15))) return false;
    AG_LABEL("write_rgb16_ycbcr_sub_hot<ys=%d%s>", a.ys, a.dst16 ? "" : ",to8");
    return take(L, kWkRgb16Sub, a, a.spans(512) * a.rows_ys(), kStreamWaves, AG_STREAM_BLOCK_CAP * 4 / kStreamWaves);
}

// ---- the candidates: f32 documents saved 4:2:2 / 4:2:0 or with transparency (part 3) ---------------------------------------------
// Gray32 + alpha -> Y and Alpha u16 planes (round 5): even widths, dword-aligned rows and planes (gray saves: PQ or Clip, avifgpu_api.hip)
inline bool cand_ga32(const WriteAsk& a, WriteLaunch& L)
{
    if (!(a.depth == 32 && (a->width % 2) == 0 && a.stream() && a.planes == 2 && a.dst16 && a->dst[3] != nullptr && aligned_to(a.p, 3, kPlanesYA, 3))) return false;
    L.tr = a->transfer == AVIFGPU_TRANSFER_PQ ? transfer_id(a.p) : AVIFGPU_TRANSFER_CLIP;
    AG_LABEL("write_ga_stream<depth=32,transfer=%d>", a->transfer);
    return take(L, kWkGa32, a, (((long long)a->width / 2 + 255) / 256) * a->nrows, kGaWaves, AG_STREAM_BLOCK_CAP * 4 / kGaWaves);
}
// what the streaming kernels of RGB(A) f32 documents into Y, Cb, Cr planes share
inline bool rgb32_planes(const WriteAsk& a, int planes) { return a.stream() && a.depth == 32 && a.planes == planes && a.dst16 && a.ycbcr(); }
// RGBA f32 -> Y, Cb, Cr (4:2:2 / 4:2:0), A: the plug-in's default save of a transparent 32-bit document (no ICC variant: those stay
// generic); spans of 256 pixels
inline bool cand_rgba32_sub(const WriteAsk& a, WriteLaunch& L)
{
    if (!(rgb32_planes(a, 4) && a->icc_trc_type[0] == 0 && a->icc_s_tab == nullptr && a.xs == 1 && a->dst[3] != nullptr && aligned_to(a.p, 3, kPlanes4, 3))) return false;
    L.tr = transfer_id(a.p);
    AG_LABEL("write_rgba32_ycbcra_sub_hot<transfer=%d,xs=1,ys=%d,nearest=%d>", a->transfer, a.ys, a->nearest);
    return take(L, kWkRgba32Sub, a, a.spans(256) * a.rows_ys(), kRgbaWaves, AG_RGBA_BLOCK_CAP * 4 / kRgbaWaves);
}
// RGBA f32 -> Y, Cb, Cr, A 4:4:4, with or without a streaming ICC stage (4 only as icc_pow32's fast form)
inline bool cand_rgba32(const WriteAsk& a, WriteLaunch& L)
{
    StreamIcc k = stream_icc(a.p);
    k.icc4 = k.icc4 && AG_ICC_FASTPOW;
    if (!(AG_RGBA_HOT_ENABLE && rgb32_planes(a, 4) && (k.none || k.icc1 || k.icc4 || k.icc2) && a.xs == 0 && a.ys == 0 && a->dst[3] != nullptr &&
          aligned_to(a.p, 15, kPlanes4, 15))) return false;
    L.icc = k.stage(); L.tr = k.icc4 ? AVIFGPU_TRANSFER_CLIP : transfer_id(a.p);
    AG_LABEL("write_rgba32_ycbcra444_hot<transfer=%d>%s", a->transfer, k.tail());
    return take(L, kWkRgba32, a, a.spans(64 * AG_RGBA_HOT_PXL) * a->nrows, kRgbaWaves, AG_RGBA_BLOCK_CAP * 4 / kRgbaWaves);
}
// RGB f32 -> Y, Cb, Cr 4:2:2 / 4:2:0, with or without a streaming ICC stage.  Any width (round 4: buffer addressing clips the ragged
// lane in hardware); rows and planes dword-aligned.  4:2:2 tiles of many whole spans: two spans per wave (see the kernel's loop)
inline bool cand_rgb32_sub(const WriteAsk& a, WriteLaunch& L)
{
    const StreamIcc k = stream_icc(a.p);
    if (!(rgb32_planes(a, 3) && (k.none || k.icc1 || k.icc4 || k.icc2) && a.xs == 1 && aligned_to(a.p, 3, kPlanes3, 3))) return false;
    const long long spans = a.spans(512) * a.rows_ys();
    const int spw = (AG_SUB_SPW2 && a.ys == 0 && (a->width % 512) == 0 && spans >= AG_SUB_SPW2_MIN_SPANS) ? 2 : 1;
    L.icc = k.stage(); L.tr = k.icc4 ? AVIFGPU_TRANSFER_CLIP : transfer_id(a.p);
    AG_LABEL("write_rgb32_ycbcr_sub_hot<transfer=%d,xs=1,ys=%d>%s", a->transfer, a.ys, k.tail());
    return take(L, kWkRgb32Sub, a, spans, kF32Waves, AG_STREAM_BLOCK_CAP * 4 / kF32Waves, spw);
}

// ---- the candidates: RGB f32 4:4:4 and the f32 hand-off (part 1) -------------------------------------------------------------------
// Behind a linear (or one simple parametric) document profile: the streaming ICC kernel with the interleaved hand-off as its output
inline bool cand_rgb32_icc_ref(const WriteAsk& a, WriteLaunch& L)
{
    const StreamIcc k = stream_icc(a.p);
    if (!(a.stream() && (k.icc1 || k.icc4 || k.icc2) && a.depth == 32 && a.planes == 3 && a.dst16 && a.output == AVIFGPU_OUT_REFERENCE && aligned_to(a.p, 3, kPlane0, 15))) return false;
    L.icc = k.stage(); L.tr = k.icc4 ? AVIFGPU_TRANSFER_CLIP : transfer_id(a.p);
    AG_LABEL("write_rgb32_icc1_ycbcr444_hot<transfer=%d,out=ref> icc=%d", a->transfer, L.icc);
    return take(L, kWkRgb32IccRef, a, a.spans(512) * a->nrows, kF32Waves, AG_STREAM_BLOCK_CAP * 4 / kF32Waves);
}
// The interleaved f32 hand-off, and (round 5) Gray32 -> Y plane: a gray document without alpha IS its Y plane sample for sample
// (WriteHeifImage.cpp:181-252), the same elementwise kernel with one sample per pixel; rows of whole 4-sample vectors
inline bool cand_f32_ref(const WriteAsk& a, WriteLaunch& L)
{
    if (!(a.stream() && a->icc_trc_type[0] == 0 && a.depth == 32 && ((a.planes >= 3 && a.output == AVIFGPU_OUT_REFERENCE) || a.planes == 1) && a.dst16)) return false;
    if (!(((long long)a->width * a.planes) % 4 == 0 && aligned_to(a.p, 15, kPlane0, 7))) return false;
    L.tr = transfer_id(a.p);
    AG_LABEL("write_f32_ref_stream<transfer=%d,planes=%d>", a->transfer, a.planes);
    return take(L, kWkF32Ref, a, (((long long)a->width * a.planes / 4 + 255) / 256) * a->nrows, kF32RefWaves, AG_STREAM_BLOCK_CAP * 4 / kF32RefWaves);
}
// RGB f32 -> Y, Cb, Cr 4:4:4 with a streaming ICC stage in front
inline bool cand_rgb32_icc(const WriteAsk& a, WriteLaunch& L)
{
    const StreamIcc k = stream_icc(a.p);
    if (!(rgb32_planes(a, 3) && (k.icc1 || k.icc4 || k.icc2) && a.xs == 0 && a.ys == 0 && aligned_to(a.p, 3, kPlanes3, 3))) return false;
    L.icc = k.stage(); L.tr = k.icc4 ? AVIFGPU_TRANSFER_CLIP : transfer_id(a.p);
    AG_LABEL("write_rgb32_icc1_ycbcr444_hot<transfer=%d> icc=%d", a->transfer, L.icc);
    return take(L, kWkRgb32Icc, a, a.spans(512) * a->nrows, kF32Waves, AG_STREAM_BLOCK_CAP * 4 / kF32Waves);
}
// The headline: RGB f32 (no alpha, no profile) -> Y, Cb, Cr 4:4:4.  Any width (round 4): the last span of a row is clipped by the buffer
// resources.  Word bit 1: 8 pixels a lane (else 4), bit 2: non-temporal.  Spans on 128-byte lines (a flat tile is one row): the two-wave
// workgroup; rows that start inside a line: the four-wave one.  8192^2: one span per wave measured 5-6 % faster than two (the cap).
inline bool cand_rgb32(const WriteAsk& a, WriteLaunch& L)
{
    if (!(rgb32_planes(a, 3) && a->icc_trc_type[0] == 0 && a.xs == 0 && a.ys == 0 && aligned_to(a.p, 3, kPlanes3, 3))) return false;
    L.px8 = (a.word & 2) != 0; L.nt = (a.word & 4) != 0;
    const uintptr_t bases = reinterpret_cast<uintptr_t>(a->src) | reinterpret_cast<uintptr_t>(a->dst[0]) | reinterpret_cast<uintptr_t>(a->dst[1]) | reinterpret_cast<uintptr_t>(a->dst[2]);
    const uintptr_t strides = (uintptr_t)a->src_row_bytes | (uintptr_t)a->dst_stride[0] | (uintptr_t)a->dst_stride[1] | (uintptr_t)a->dst_stride[2];
    L.lines = (bases & 127) == 0 && (a->nrows == 1 || (strides & 127) == 0);
    const int wpb = (L.lines ? AG_HOT444_BLOCK_LINES : AG_HOT444_BLOCK) / 64;
    L.tr = transfer_id(a.p);
    AG_LABEL("write_rgb32_ycbcr444_hot<transfer=%d,pxl=%d,nt=%d>", a->transfer, L.px8 ? 8 : 4, (int)L.nt);
    return take(L, kWkRgb32, a, a.spans(L.px8 ? 512 : 256) * a->nrows, wpb, 256LL * 512 * 4 / wpb);
}

// ---- the generic kernel: every configuration the API accepts ------------------------------------------------------------------------
// One thread owns the footprint of NC chroma samples (WriteShape); the ICC stage picks the instantiation, the footprint and the cap:
//   3 the 8-bit matrix-shaper (tables copied per workgroup: 2048 workgroups at most), 7 / 5 the 33^3 table behind an 8- / 16-bit document,
//   8 lcms2's stage program, 6 sampled curves (both with their tables in LDS where they fit: " lds"), 4 / 2 / 1 the parametric curves
//   (4, 2: a smaller footprint, AG_ICC_BLOCK_CAP), none.  PQ in its close form copies its table per workgroup: AG_PQ_TABLE_BLOCK_CAP.
inline void decide_write_px(const WriteAsk& a, WriteLaunch& L)
{
    const WriteParams& p = a.p;
    const bool color = a.planes >= 3, ycbcr = color && a.output != AVIFGPU_OUT_REFERENCE;
    const int xs = ycbcr ? a.xs : 0, ys = ycbcr ? a.ys : 0;            // (launch_out: the hand-offs have no chroma planes)
    L.kernel = kWkPx;
    L.out = !color ? kOutRefGray : (ycbcr ? kOutYcbcr : kOutRefColor);
    L.tr = a.depth == 32 ? transfer_id(p) : AVIFGPU_TRANSFER_CLIP;
    if (a.depth == 32 && !a.dst16) { L.invalid = true; return; }      // a 32-bit document is never saved at 8 bit
    const long long rows = (p.nrows + (1 << ys) - 1) >> ys;
    auto groups_of = [&](int icc) { const int pxt = write_shape_nc(a.dst16, a.planes, xs, icc) << xs; return (long long)((p.width + pxt - 1) / pxt) * rows; };
    long long groups = groups_of(0);
    if (groups == 0) { L.kernel = kWkEmpty; return; }
    const bool linear = p.icc_trc_linear[0] != 0 && p.icc_trc_linear[1] != 0 && p.icc_trc_linear[2] != 0;
    const bool f32rgb = a.depth == 32 && color;
    if (f32rgb && p.icc_trc_type[0] != 0 && p.icc_s_tab == nullptr && (p.icc_out == 4 || !linear)) groups = groups_of(2);      // variants 2 and 4 use a smaller footprint
    if (groups >= 0x7fffffffLL - 256LL * 65536) { L.invalid = true; return; }     // 32-bit group index in the kernel
    L.aligned = aligned_to(p, 15, (p.dst[0] ? 1u : 0u) | (p.dst[1] ? 2u : 0u) | (p.dst[2] ? 4u : 0u) | (p.dst[3] ? 8u : 0u), 15);     // => the branch-free vector path
    const long long pq_cap = (L.tr == kTransferPqHi && AG_PQ_TABLE_BLOCK_CAP < AG_WRITE_BLOCK_CAP) ? AG_PQ_TABLE_BLOCK_CAP : AG_WRITE_BLOCK_CAP;
    const long long icc_cap = AG_ICC_BLOCK_CAP < AG_WRITE_BLOCK_CAP ? AG_ICC_BLOCK_CAP : AG_WRITE_BLOCK_CAP;
    long long cap = pq_cap;
    if (a.depth == 8 && color && p.icc8_s1 != nullptr) { L.icc = 3; cap = 2048 < AG_WRITE_BLOCK_CAP ? 2048 : AG_WRITE_BLOCK_CAP; }
    else if (a.depth == 8 && color && p.icc16_clut != nullptr) { L.icc = 7; groups = groups_of(7); cap = AG_WRITE_BLOCK_CAP; }
    else if (a.depth == 16 && color && p.icc16_clut != nullptr) { L.icc = 5; groups = groups_of(5); cap = AG_WRITE_BLOCK_CAP; }
    else if (f32rgb && p.icc_p8_stages != nullptr) {
        L.icc = 8; groups = groups_of(8); cap = AG_WRITE_BLOCK_CAP;
        L.lds = p.icc_p8_lds_words ? (size_t)((p.icc_p8_lds_words + 1) >> 1) * 4 : 0;                     // <= 48 KiB
    } else if (f32rgb && p.icc_s_tab != nullptr) {
        L.icc = 6; cap = AG_WRITE_BLOCK_CAP;
        L.lds = p.icc_s_lds ? (size_t)(p.icc_s_n[0] + p.icc_s_n[1] + p.icc_s_n[2]) * 4 : 0;               // <= 48 KiB
    } else if (f32rgb && p.icc_trc_type[0] != 0) {
        if (p.icc_out == 4) {                       // -> sRGB: the SDR (Clip) save of a 32-bit document
            if (L.tr != AVIFGPU_TRANSFER_CLIP) { L.invalid = true; return; }     // rejected earlier by fill_write_params
            L.icc = 4; cap = icc_cap;
        } else if (linear) L.icc = 1;
        else { L.icc = 2; cap = icc_cap; }
    }
    char icc[12] = "";
    if (L.icc) snprintf(icc, sizeof icc, ",icc=%d", L.icc);
    AG_LABEL("write_px<depth=%d,planes=%d,out=%d,dst16=%d,xs=%d,ys=%d,transfer=%d,aligned=%d%s>%s", a.depth, a.planes, L.out, (int)a.dst16, xs, ys,
             L.tr, (int)L.aligned, icc, L.lds ? " lds" : "");
    const int block = wpx_block(L.icc);
    L.units = groups; L.waves = block / 64; L.cap = cap;
    L.need = (groups + block - 1) / block;
    L.blocks = capped_blocks(L.need, cap, a.word);
    label_cap(L.label, L.blocks, L.need, cap);
}
#undef AG_LABEL

// The order is the priority: the first that takes the tile launches it.  8- and 16-bit documents (part 2), then 32-bit ones (parts 3, 1).
typedef bool (*WriteCandidate)(const WriteAsk&, WriteLaunch&);
constexpr WriteCandidate kWriteCandidatesInt[] = { cand_copy_rows, cand_int_ref, cand_ga16, cand_rgb8, cand_rgb8_to16, cand_rgba8, cand_rgb16, cand_rgba16,
                                                   cand_rgba16_sub, cand_rgb16_sub };
constexpr WriteCandidate kWriteCandidatesF32[] = { cand_ga32, cand_rgba32_sub, cand_rgba32, cand_rgb32_sub, cand_rgb32_icc_ref, cand_f32_ref, cand_rgb32_icc, cand_rgb32 };

inline void decide_write_rows(const WriteAsk& a, WriteLaunch& L)
{
    const bool f32 = a.depth == 32;
    // an 8-bit document behind a table profile: write_px<..., icc = 7> (the other table stages fail a clause of every rule)
    if (!(a.depth == 8 && a->icc16_clut != nullptr))
        for (const WriteCandidate* c = f32 ? kWriteCandidatesF32 : kWriteCandidatesInt, *end = c + (f32 ? 8 : 10); c != end; ++c) {
            if ((*c)(a, L)) return;
            if (L.label[0]) L = WriteLaunch();           // its units did not fit: nothing of it stays
        }
    decide_write_px(a, L);
}

// FLAT launches (round 3).  When nothing depends on where a row ends -- 4:4:4 or 4:2:2 planes or the interleaved hand-off, 16- /
// 32-bit documents -- and source and planes are contiguous (row stride == row bytes: the library's own staging buffers whenever a row is a
// multiple of 16 bytes, and any tightly packed caller buffer), the tile IS one long row of width x nrows pixels.  Launched as such,
// every wave's span starts on a span boundary of the buffer instead of a row boundary: no half-empty last span per row (7952-wide
// rows fill 15.53 spans of 512 pixels) and no rows that start in the middle of a 128-byte line (7952 x 12 B = 745.5 lines).  Same
// kernels, same per-pixel arithmetic, same bytes (tests/test_gpu_kernel_equivalence.py); word bit 4 (16) turns it off for A/B.
// 4:2:2 qualifies too (chroma is sub-sampled along the row only): even width, chroma planes of width / 2 samples per row.
// True: q is the tile as one row.
inline bool flat_tile(const WriteAsk& a, WriteParams& q)
{
    const WriteParams& p = a.p;
    const long long px = (long long)p.width * p.nrows;
    const bool h422 = a.xs == 1 && a.ys == 0 && (p.width & 1) == 0 && a.ycbcr();
    bool flat = AG_FLAT && a.stream() && !(a.word & 16) && p.nrows > 1 && a.planes >= 3 && (a.depth == 16 || a.depth == 32) && a.ys == 0 && (a.xs == 0 || h422) &&
                px < (1LL << 29) && p.src_row_bytes == (long long)p.width * a.planes * (a.depth / 8);
    if (!flat) return false;
    const int dsz = a.dst16 ? 2 : 1;
    auto plane_px = [&](int pl, long long w) { return (h422 && (pl == 1 || pl == 2)) ? w / 2 : w; };
    if (a.output == AVIFGPU_OUT_REFERENCE) flat = p.dst_stride[0] == (long long)p.width * a.planes * dsz;
    else for (int pl = 0; pl < (a.planes == 4 ? 4 : 3); ++pl) flat = flat && p.dst[pl] != nullptr && p.dst_stride[pl] == plane_px(pl, p.width) * dsz;
    if (!flat) return false;
    q = p;
    q.width = (int32_t)px; q.nrows = 1; q.rows_to_end = 1;
    q.src_row_bytes = px * a.planes * (a.depth / 8);
    for (int pl = 0; pl < 4; ++pl) if (q.dst[pl]) q.dst_stride[pl] = (a.output == AVIFGPU_OUT_REFERENCE ? px * a.planes : plane_px(pl, px)) * dsz;
    return true;
}

// The whole decision of launch_write().  L.flat: launch with q (which is written only then), else with p.
inline void decide_write(const WriteParams& p, int depth, int planes, bool dst16, int output, int xs, int ys, int word, WriteParams& q, WriteLaunch& L)
{
    const WriteAsk a = { p, depth, planes, dst16, output, xs, ys, word };
    if (!flat_tile(a, q)) { decide_write_rows(a, L); return; }
    const WriteAsk f = { q, depth, planes, dst16, output, xs, ys, word };
    decide_write_rows(f, L);
    L.flat = true;
    const size_t n = strlen(L.label);
    if (n + 6 < (size_t)kLabelBytes) snprintf(L.label + n, kLabelBytes - n, " flat");
}

} // namespace avifgpu
