// icc_tables.cpp -- the ICC stage of a write call on the host: the device copies of its tables (one cache, one record per HIP device and
// table kind) and the ICC fields of WriteParams (fill_icc_params).  Host code only: no kernel, no code object.
#include <hip/hip_runtime.h>
#include <array>
#include <atomic>
#include <cmath>
#include <cstddef>
#include <cstring>
#include <limits>
#include <map>
#include <mutex>
#include <vector>

#include "icc_tables.h"
#include "staging.h"

namespace avifgpu {
namespace {

// ---- the cache ----------------------------------------------------------------------------------------------------------------------------
// Device copies of the ICC tables, one set per HIP device (the row-tile scheduler converts one image on several GPUs).  Re-uploaded only
// when the contents change (one image = one upload per device); a change first drains that device so no in-flight kernel still reads the
// old table.  Callers run on the thread whose CURRENT device is the one they launch on.
enum IccKind { kPowBins, kClut33, kSampled, kShaper8, kProgram32, kIccKinds };   // kClut33: the 16-bit and the 8-bit-LUT saves share it
constexpr size_t kShaper8Bytes = sizeof(avifgpu_icc_shaper8::shaper1) + 16388;                 // [3][256] int32, then 16388 bytes of shaper2[0]
constexpr size_t kSampledBytes = sizeof(avifgpu_icc_sampled32::curve) + sizeof(avifgpu_icc_sampled32::table16);
constexpr size_t kProgramRecBytes = sizeof(avifgpu_icc_stage32) * AVIFGPU_ICC_PIPE_MAX_STAGES;  // the stage records; the words follow
void clut33_device_image(const uint8_t* image, uint8_t* device)
{
    icc16_device_image(reinterpret_cast<const uint16_t (*)[4]>(image), reinterpret_cast<uint16_t*>(device));
}
// cap: the device buffer, allocated on first use; device_image: the device form of an image, written into `cap` ZEROED bytes (none: the image itself)
struct IccKindInfo { size_t cap; IccVerify verify; void (*device_image)(const uint8_t* image, uint8_t* device); const char* alloc; const char* upload; int upload_code; };
const IccKindInfo kKinds[kIccKinds] = {
    { 128 * 4 * sizeof(float), IccVerify::EveryCall, nullptr, "upload of the pow table", "upload of the pow table", AVIFGPU_memFullErr },
    { kIcc16DeviceBytes, IccVerify::OncePerEpoch, clut33_device_image, "hipMalloc(icc16 table)", "upload of the ICC table", AVIFGPU_writErr },
    { kSampledBytes, IccVerify::OncePerEpoch, nullptr, "hipMalloc(sampled ICC curves)", "upload of the sampled ICC curves", AVIFGPU_writErr },
    { kShaper8Bytes, IccVerify::EveryCall, nullptr, "hipMalloc(icc8 tables)", "upload of ICC tables", AVIFGPU_writErr },
    { kProgramRecBytes + sizeof(avifgpu_icc_pipeline32::words) + 16, IccVerify::EveryCall, nullptr, "hipMalloc(ICC stage program)", "upload of the ICC stage program", AVIFGPU_writErr },
};
struct IccRecord {
    void* dev = nullptr;                             // the device copy, kKinds[kind].cap bytes
    std::vector<uint8_t> host;                       // the image of the last upload, as the caller's spans lay it out
    IccStamp stamp;                                  // the caller's address of that upload, its fingerprint, its epoch, the image's size
};
typedef std::array<IccRecord, kIccKinds> IccDeviceTables;
std::mutex g_icc_mu;
std::map<int, IccDeviceTables> g_icc_tables;         // keyed by HIP device ordinal
std::atomic<uint64_t> g_icc_epoch{1};

// The caller's bytes: `bytes` at `data` belong at offset `at` of the image; what no span covers is zero.  Spans are in image order.
struct IccSpan { const void* data; size_t bytes, at; };

bool image_equals(const std::vector<uint8_t>& image, const IccSpan* spans, int nspans)
{
    size_t at = 0;
    auto zero_up_to = [&](size_t end) {                    // every byte equals the one before it, and the first is 0
        const uint8_t* z = image.data() + at;
        const size_t n = end - at;
        at = end;
        return n == 0 || (z[0] == 0 && memcmp(z, z + 1, n - 1) == 0);
    };
    for (int i = 0; i < nspans; ++i) {
        if (!zero_up_to(spans[i].at) || memcmp(image.data() + at, spans[i].data, spans[i].bytes) != 0) return false;
        at += spans[i].bytes;
    }
    return zero_up_to(image.size());
}

// Brings the current device's record of `kind` up to date with an image of image_bytes made of `spans` and returns its device pointer:
// allocates on first use, decides staleness (icc_tables.h), and on a miss -- only then -- lays the image out, turns it into its device
// form, drains the device and copies.
int icc_table(IccKind kind, size_t image_bytes, const IccSpan* spans, int nspans, void*& out)
{
    const IccKindInfo& k = kKinds[kind];
    int dev = -1;
    hipError_t e = hipGetDevice(&dev);
    if (e != hipSuccess) return hip_fail(e, "hipGetDevice", AVIFGPU_writErr);
    std::lock_guard<std::mutex> lk(g_icc_mu);
    IccRecord& r = g_icc_tables[dev][kind];
    if (!r.dev) {
        e = hipMalloc(&r.dev, k.cap);
        if (e != hipSuccess) { r.dev = nullptr; return hip_fail(e, k.alloc, AVIFGPU_memFullErr); }
    }
    IccStamp call = { spans[0].data, 0, g_icc_epoch.load(std::memory_order_relaxed), image_bytes };
    if (k.verify == IccVerify::OncePerEpoch) for (int i = 0; i < nspans; ++i) call.fp = call.fp * 1099511628211ull ^ table_fingerprint(spans[i].data, spans[i].bytes);
    IccStale stale = icc_staleness(r.stamp, call, k.verify);
    if (stale == IccStale::CompareBytes) stale = image_equals(r.host, spans, nspans) ? IccStale::Trusted : IccStale::Upload;
    if (stale == IccStale::Upload) {
        r.stamp = IccStamp();                                   // nothing of this record is trusted until the copy below has succeeded
        r.host.clear();                                         // laid out in place: the buffer of the last upload serves again
        r.host.reserve(image_bytes);
        for (int i = 0; i < nspans; ++i) {                      // resize() zero-fills what no span covers; nothing is written twice
            const uint8_t* from = static_cast<const uint8_t*>(spans[i].data);
            r.host.resize(spans[i].at);
            r.host.insert(r.host.end(), from, from + spans[i].bytes);
        }
        r.host.resize(image_bytes);
        std::vector<uint8_t> built(k.device_image ? k.cap : 0, 0);
        if (k.device_image) k.device_image(r.host.data(), built.data());
        const std::vector<uint8_t>& up = k.device_image ? built : r.host;
        if (up.size() > k.cap) return fail(AVIFGPU_writErr, "%s: %zu bytes into a device buffer of %zu", k.upload, up.size(), k.cap);
        e = hipDeviceSynchronize();                             // a launch may still be reading the previous table
        if (e == hipSuccess) e = hipMemcpy(r.dev, up.data(), up.size(), hipMemcpyHostToDevice);
        if (e != hipSuccess) return hip_fail(e, k.upload, k.upload_code);
    }
    r.stamp = call;
    out = r.dev;
    return 0;
}

// ---- one function per table kind: validate, bring the record up to date, set the kernel's fields -----------------------------------------------
// The bins of icc_pow32 (write_kernels.hip): c = RN_float(1 / bin centre) and -log2(c) as a float pair.  Constants -- evaluated once on
// the host instead of once per workgroup on the device (a double log2 there costs ~200 instructions per thread, a quarter of what a
// streaming workgroup does in its whole life).
int icc_pow_bins(WriteParams& p)
{
    static const std::array<float, 128 * 4> bins = [] {
        std::array<float, 128 * 4> t;
        for (int i = 0; i < 128; ++i) {
            const double centre = 0.5 + ((double)i + 0.5) * (1.0 / 256.0);
            const float cf = (float)(1.0 / centre);
            const double L = -std::log2((double)cf);
            const float Lh = (float)L;
            t[4 * i] = cf; t[4 * i + 1] = Lh; t[4 * i + 2] = (float)(L - (double)Lh); t[4 * i + 3] = 0.0f;
        }
        return t;
    }();
    const IccSpan span = { bins.data(), sizeof(bins), 0 };
    void* dev = nullptr;
    const int rc = icc_table(kPowBins, sizeof(bins), &span, 1, dev);
    p.icc_pow_tab = static_cast<const float*>(dev);
    return rc;
}

int icc_clut33(const avifgpu_icc_clut16* t, WriteParams& p)
{
    if (t->grid_points != AVIFGPU_ICC_CLUT_GRID) return fail(AVIFGPU_formatBadParameters, "16-bit ICC table: grid_points must be 33");
    const IccSpan span = { t->table, sizeof(t->table), 0 };
    void* dev = nullptr;
    const int rc = icc_table(kClut33, sizeof(t->table), &span, 1, dev);
    p.icc16_clut = static_cast<const uint16_t*>(dev);
    return rc;
}

int icc_sampled(const avifgpu_icc_sampled32* t, WriteParams& p)
{
    for (int ch = 0; ch < 3; ++ch)
        if (t->entries[ch] < 0 || t->entries[ch] > AVIFGPU_ICC_SAMPLED_MAX || t->entries[ch] == 1)
            return fail(AVIFGPU_formatBadParameters, "sampled ICC curves: entries[] must be 0 or 2..%d", (int)AVIFGPU_ICC_SAMPLED_MAX);
    // a mixed profile: the channels of parametric_mask carry a parametric curve (base.trc_type / trc_params), the others a table
    if (t->parametric_mask < 0 || t->parametric_mask >= 7) return fail(AVIFGPU_formatBadParameters, "sampled ICC curves: parametric_mask must leave at least one sampled channel");
    bool lds = !(hot_variant() & 64);                           // bit 6: tests take the memory path
    for (int ch = 0; ch < 3; ++ch) {
        const bool par = (t->parametric_mask >> ch) & 1;
        if (par && t->entries[ch] != 0) return fail(AVIFGPU_formatBadParameters, "sampled ICC curves: a parametric channel has no table entries");
        if (par != (t->base.trc_type[ch] != 0)) return fail(AVIFGPU_formatBadParameters, "sampled ICC curves: parametric_mask and base.trc_type[] disagree");
        lds = lds && (par || t->entries[ch] > 0);
    }
    // curve[] (768 KiB) followed by table16[] (24 KiB), adjacent members: one span, one device buffer, one upload when the profile changes
    static_assert(offsetof(avifgpu_icc_sampled32, table16) == offsetof(avifgpu_icc_sampled32, curve) + sizeof(t->curve), "one span");
    const IccSpan span = { t->curve, kSampledBytes, 0 };
    void* dev = nullptr;
    if (const int rc = icc_table(kSampled, kSampledBytes, &span, 1, dev)) return rc;
    p.icc_s_tab = static_cast<const float*>(dev);
    p.icc_s_tab16 = reinterpret_cast<const uint16_t*>(static_cast<const uint8_t*>(dev) + sizeof(t->curve));
    for (int ch = 0; ch < 3; ++ch) p.icc_s_n[ch] = lds ? t->entries[ch] : 0;
    p.icc_s_lds = lds;
    p.icc_s_par = t->parametric_mask;
    return 0;
}

int icc_shaper8(const avifgpu_icc_shaper8* t, WriteParams& p)
{
    if (memcmp(t->shaper2[0], t->shaper2[1], 16385) != 0 || memcmp(t->shaper2[0], t->shaper2[2], 16385) != 0)
        return fail(AVIFGPU_formatBadParameters, "8-bit ICC shaper: the destination curve must be the same for R, G and B (sRGB)");
    // the kernel multiplies with v_mul_i32_i24: every factor must fit 24 signed bits (always true for real profiles: curve
    // values <= 1.0 -> 16384, matrix coefficients of a few units)
    for (int c = 0; c < 3; ++c) {
        for (int i = 0; i < 256; ++i)
            if (t->shaper1[c][i] < -(1 << 23) || t->shaper1[c][i] >= (1 << 23))
                return fail(AVIFGPU_formatCannotRead, "8-bit ICC shaper: curve value out of the 24-bit range, keep the lcms2 path");
        for (int j = 0; j < 3; ++j)
            if (t->matrix[c][j] < -(1 << 23) || t->matrix[c][j] >= (1 << 23))
                return fail(AVIFGPU_formatCannotRead, "8-bit ICC shaper: matrix coefficient out of the 24-bit range, keep the lcms2 path");
    }
    const size_t n1 = sizeof(t->shaper1);
    const IccSpan spans[2] = { { t->shaper1, n1, 0 }, { t->shaper2[0], kShaper8Bytes - n1, n1 } };
    void* dev = nullptr;
    if (const int rc = icc_table(kShaper8, kShaper8Bytes, spans, 2, dev)) return rc;
    p.icc8_s1 = static_cast<const int32_t*>(dev);
    p.icc8_s2 = static_cast<const uint8_t*>(dev) + n1;
    for (int i = 0; i < 3; ++i) { for (int j = 0; j < 3; ++j) p.icc8_m[3 * i + j] = t->matrix[i][j]; p.icc8_off[i] = t->offset[i]; }
    // the packed u8 kernel can take two of the three products of a matrix row in one v_dot2_i32_i16 when their operands fit 16
    // signed bits: the G and B columns (a coefficient of 2.0 or more -- 32768 in 1.14 -- sits on the diagonal of a wide-gamut red,
    // ProPhoto or ACES to sRGB, i.e. in column 0, which keeps its 24-bit multiply) and the G and B shaper tables (<= 16384 for curves into [0, 1])
    bool fits = true;
    for (int i = 0; i < 3; ++i) for (int j = 1; j < 3; ++j) fits = fits && t->matrix[i][j] >= -32768 && t->matrix[i][j] <= 32767;
    for (int c2 = 1; c2 < 3; ++c2) for (int v = 0; v < 256; ++v) fits = fits && t->shaper1[c2][v] >= 0 && t->shaper1[c2][v] <= 32767;
    p.icc8_dot2 = (fits && !(hot_variant() & 32)) ? 1 : 0;  // bit 5 of the tuning word: tests take the three-mad form on the same data
    for (int i = 0; i < 3; ++i) p.icc8_m12[i] = (int32_t)(((uint32_t)t->matrix[i][1] & 0xffffu) | ((uint32_t)t->matrix[i][2] << 16));
    return 0;
}

// The stage program of a 32-bit document (icc = 8): its stage records, then its words (padded: the kernel copies whole dwords to LDS).  Small
// -- a 17^3 program is ~36 KiB -- so every call compares the caller's program with the stored image outright and re-uploads on any
// difference: a program rewritten at the same address between two saves is never served stale.
int icc_program32(const avifgpu_icc_pipeline32* t, WriteParams& p)
{
    const size_t words = (size_t)t->word_count * 2;
    const IccSpan spans[2] = { { t->stages, sizeof(avifgpu_icc_stage32) * (size_t)t->stage_count, 0 }, { t->words, words, kProgramRecBytes } };
    void* dev = nullptr;
    if (const int rc = icc_table(kProgram32, kProgramRecBytes + ((words + 15) & ~(size_t)15), spans, 2, dev)) return rc;
    p.icc_p8_stages = dev;
    p.icc_p8_words = reinterpret_cast<const uint16_t*>(static_cast<const uint8_t*>(dev) + kProgramRecBytes);
    p.icc_p8_nstages = t->stage_count;
    p.icc_p8_lds_words = (words <= 48u * 1024u && !(hot_variant() & 64)) ? t->word_count : 0;    // bit 6: tests take the memory path
    for (int ch = 0; ch < 3; ++ch) p.icc_trc_type[ch] = 8;
    return 0;
}

// lcms2's parametric curve types 1..5 (DefaultEvalParametricFn; P = g, a, b, c, d, e, f as the library orders them) rewritten as
//     y = R >= thr ? (a*R + b > 0 ? pow(a*R + b, g) + add : nonpos) : c*R + f
// so that the kernel evaluates one branch-free expression.  Q = g, a, b, thr, c, f, add, nonpos.
void normalise_trc(int type, const double* P, double* Q)
{
    const double inf = std::numeric_limits<double>::infinity();
    double g = P[0], a = 1, b = 0, thr = 0, c = 0, f = 0, add = 0, nonpos = 0;
    switch (type) {
    case 1:                                   // R < 0: R when |g - 1| < 1e-4, else 0;  R >= 0: pow(R, g)   (pow(0, g) = 0 = nonpos)
        c = std::fabs(g - 1.0) < 0.0001 ? 1.0 : 0.0;
        break;
    case 2:                                   // |a| < 1e-4: 0;  R >= -b/a: (a*R + b > 0 ? pow : 0), else 0
        if (std::fabs(P[1]) < 0.0001) { thr = inf; break; }
        a = P[1]; b = P[2]; thr = -P[2] / P[1];
        break;
    case 3:                                   // as 2 with + c above and c below the (non-negative) break
        if (std::fabs(P[1]) < 0.0001) { thr = inf; break; }
        a = P[1]; b = P[2]; thr = std::max(-P[2] / P[1], 0.0); add = P[3]; f = P[3];
        break;
    case 4:                                   // R >= d: (a*R + b > 0 ? pow : 0), else c*R
        a = P[1]; b = P[2]; thr = P[4]; c = P[3];
        break;
    default:                                  // 5: R >= d: (a*R + b > 0 ? pow + e : e), else c*R + f
        a = P[1]; b = P[2]; thr = P[4]; c = P[3]; f = P[6]; add = P[5]; nonpos = P[5];
        break;
    }
    Q[0] = g; Q[1] = a; Q[2] = b; Q[3] = thr; Q[4] = c; Q[5] = f; Q[6] = add; Q[7] = nonpos;
}

} // namespace

// Called once per C-ABI write call (or shim tile) that carries an ICC table, on the caller's thread, before any tile is dealt.  Only a call
// that CONTINUES the calling thread's previous one -- row0 == the row after its last -- stays in its epoch: the tiles of one save, handed over
// top to bottom.  Anything else (row 0, a restart, a gap, tiles out of order, another geometry) starts a new epoch and costs each device
// one byte-for-byte comparison of the table.
void icc_epoch_for_call(int row0, int nrows)
{
    thread_local long long next_row = -1;
    if (row0 == 0 || (long long)row0 != next_row) g_icc_epoch.fetch_add(1, std::memory_order_relaxed);
    next_row = (long long)row0 + nrows;
}

// avifgpu_shutdown: nothing is in flight any more.
void release_icc_tables()
{
    std::lock_guard<std::mutex> lk(g_icc_mu);
    int cur = -1;
    (void)hipGetDevice(&cur);
    for (auto& kv : g_icc_tables) {
        (void)hipSetDevice(kv.first);
        for (IccRecord& r : kv.second) if (r.dev) (void)hipFree(r.dev);
    }
    g_icc_tables.clear();
    if (cur >= 0) (void)hipSetDevice(cur);
}

int fill_icc_params(const avifgpu_write_desc* d, const IccArgs& icc, WriteParams& p)
{
    const avifgpu_icc_transform* g_icc = icc.s32 ? &icc.s32->base : icc.f32;
    if (icc.p32) {
        if (d->depth != 32 || d->planes < 3) return fail(AVIFGPU_formatBadParameters, "the ICC stage program applies to 32-bit RGB(A) documents");
        if (g_icc) return fail(AVIFGPU_formatBadParameters, "one ICC transform per call");
        // the reference converts to sRGB only for the SDR save of a 32-bit document (ColorProfileConversion.cpp:118-123)
        if (icc.p32->target == AVIFGPU_ICC_TARGET_SRGB_FLOAT && d->transfer != AVIFGPU_TRANSFER_CLIP)
            return fail(AVIFGPU_formatBadParameters, "the sRGB ICC target goes with transfer Clip");
        if (const int rc = icc_program32(icc.p32, p)) return rc;
    }
    if (g_icc) {
        if (d->depth != 32 || d->planes < 3) return fail(AVIFGPU_formatBadParameters, "the ICC row transform applies to 32-bit RGB(A) documents");
        // sampled curves: the curve stage is the device table; the matrix / output curve below are shared with the parametric form
        if (const int rc = icc.s32 ? icc_sampled(icc.s32, p) : 0) return rc;
        for (int c = 0; c < 3; ++c) {
            if (icc.s32 && !((p.icc_s_par >> c) & 1)) { p.icc_trc_type[c] = 6; continue; }     // 6 marks "sampled" for the launchers
            if (g_icc->trc_type[c] < 1 || g_icc->trc_type[c] > 5) return fail(AVIFGPU_formatBadParameters, "bad ICC curve type");
            p.icc_trc_type[c] = g_icc->trc_type[c];
            p.icc_trc_linear[c] = g_icc->trc_type[c] == 1 && g_icc->trc_params[c][0] == 1.0;
            normalise_trc(g_icc->trc_type[c], g_icc->trc_params[c], p.icc_trc[c]);
            const float gh = (float)p.icc_trc[c][0];
            p.icc_trc_f[c][0] = gh; p.icc_trc_f[c][1] = (float)(p.icc_trc[c][0] - (double)gh);
            for (int k = 1; k < 8; ++k) p.icc_trc_f[c][k + 1] = (float)p.icc_trc[c][k];
        }
        // One curve for R, G and B (what every matrix/TRC display profile with a parametric or gamma curve has) whose general form
        //     y = R >= thr ? (a R + b > 0 ? pow(a R + b, g) + add : nonpos) : c R + f
        // never takes the "a R + b <= 0" side with a value other than what pow(0, g) + add gives: a > 0, a thr + b >= 0 and
        // nonpos == add, g > 0.  Then exp2(g log2(a R + b)) + add is the whole upper branch (log2 0 = -inf -> 0), and the streaming
        // kernels evaluate the curve on the samples exactly as loaded (icc = 2 on write_rgb32_icc1_ycbcr444_hot and its siblings).
        {
            bool same = true;
            for (int c = 1; c < 3; ++c)
                for (int k = 0; k < 8; ++k) same = same && p.icc_trc[c][k] == p.icc_trc[0][k];
            const double* Q = p.icc_trc[0];                    // g, a, b, thr, c, f, add, nonpos
            const bool linear = p.icc_trc_linear[0] && p.icc_trc_linear[1] && p.icc_trc_linear[2];
            // The kernels evaluate fmaf(a, R, b) with the FLOAT-rounded a, b and thr (icc_trc_f) and no "a R + b > 0" guard, so the
            // qualification is made on those: fmaf is monotone in R for a > 0, hence fmaf(a, thr, b) >= 0 covers every R >= thr and the
            // v_log_f32 never sees a negative number (a type-2/3 curve with b != 0 has thr = -b / a, where the rounded operands can land
            // an ulp below zero: such a curve takes the generic kernel, which has the guard).
            const float af = p.icc_trc_f[0][2], bf = p.icc_trc_f[0][3], thrf = p.icc_trc_f[0][4];
            p.icc_same_simple = !icc.s32 && same && !linear && Q[0] > 0.0 && af > 0.0f && std::isfinite(Q[3]) && std::isfinite(thrf) &&
                                Q[1] * Q[3] + Q[2] >= 0.0 && std::fmaf(af, thrf, bf) >= 0.0f && Q[7] == Q[6];
        }
        for (int k = 0; k < 9; ++k) { p.icc_m[k] = g_icc->matrix[k]; p.icc_m_f[k] = (float)g_icc->matrix[k]; }
        if (const int rc = icc_pow_bins(p)) return rc;
        if (g_icc->out_curve != 0) {
            if (g_icc->out_curve != 4) return fail(AVIFGPU_formatBadParameters, "bad ICC output curve");
            // the reference converts to sRGB only for the SDR save of a 32-bit document (ColorProfileConversion.cpp:118-123)
            if (d->transfer != AVIFGPU_TRANSFER_CLIP) return fail(AVIFGPU_formatBadParameters, "the sRGB ICC target goes with transfer Clip");
            p.icc_out = 4;
            for (int k = 0; k < 8; ++k) p.icc_out_p[k] = g_icc->out_params[k];
            p.icc_out_rcp[0] = std::fabs(g_icc->out_params[1]) < 0.0001 ? 0.0 : 1.0 / g_icc->out_params[1];
            p.icc_out_rcp[1] = std::fabs(g_icc->out_params[3]) < 0.0001 ? 0.0 : 1.0 / g_icc->out_params[3];
            const double ig = p.icc_out_p[6];                  // 1/g
            const float ih = (float)ig;
            p.icc_out_f[0] = ih; p.icc_out_f[1] = (float)(ig - (double)ih);
            p.icc_out_f[2] = (float)p.icc_out_p[2];
            p.icc_out_f[3] = (float)p.icc_out_rcp[0];
            p.icc_out_f[4] = (float)p.icc_out_rcp[1];
            p.icc_out_f[5] = (float)p.icc_out_p[5];
            p.icc_out_f[6] = (std::fabs(p.icc_out_p[0]) < 0.0001 || std::fabs(p.icc_out_p[1]) < 0.0001) ? 0.0f : 1.0f;
            p.icc_out_f[7] = std::fabs(p.icc_out_p[3]) < 0.0001 ? 0.0f : 1.0f;
        }
    }
    if (icc.c16) {
        if (d->depth != 16 || d->planes < 3) return fail(AVIFGPU_formatBadParameters, "the 16-bit ICC table applies to 16-bit RGB(A) documents");
        if (const int rc = icc_clut33(icc.c16, p)) return rc;
    }
    if (icc.c8t) {
        if (d->depth != 8 || d->planes < 3) return fail(AVIFGPU_formatBadParameters, "the 8-bit ICC table applies to 8-bit RGB(A) documents");
        if (icc.s8) return fail(AVIFGPU_formatBadParameters, "one ICC transform per call");
        if (const int rc = icc_clut33(icc.c8t, p)) return rc;   // the same 33^3 table, the same device layout; the kernel differs (icc = 7)
    }
    if (icc.s8) {
        if (d->depth != 8 || d->planes < 3) return fail(AVIFGPU_formatBadParameters, "the 8-bit ICC shaper applies to 8-bit RGB(A) documents");
        if (const int rc = icc_shaper8(icc.s8, p)) return rc;
    }
    return 0;
}

} // namespace avifgpu
