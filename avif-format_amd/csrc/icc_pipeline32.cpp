// icc_pipeline32.cpp -- host side of avifgpu_icc_pipeline32 (include/avifgpu.h): the program's shape checks, its checksum stamp, the host
// restatement (avifgpu_icc_pipeline32_eval) and the proof against the caller's own lcms2 float transform.  The stage arithmetic itself is
// icc_pipeline32.h, shared with the write kernel.
#include "icc_pipeline32.h"
#include "staging.h"

#include <cmath>
#include <cstdio>
#include <cstring>
#include <vector>

namespace avifgpu {

// 0 = a program the evaluators can run; else the reason (every index below stays inside words[] / the stage's table).
const char* icc_pipeline32_shape_error(const avifgpu_icc_pipeline32* p)
{
    if (p->target != AVIFGPU_ICC_TARGET_REC2020_LINEAR && p->target != AVIFGPU_ICC_TARGET_SRGB_FLOAT) return "unknown target";
    if (p->stage_count < 1 || p->stage_count > AVIFGPU_ICC_PIPE_MAX_STAGES) return "stage_count outside 1..16";
    if (p->word_count < 0 || p->word_count > AVIFGPU_ICC_PIPE_MAX_WORDS) return "word_count outside the words[] array";
    int cluts = 0;
    for (int i = 0; i < p->stage_count; ++i) {
        const avifgpu_icc_stage32& s = p->stages[i];
        switch (s.kind) {
        case AVIFGPU_ICC_STAGE_CURVES:
            for (int c = 0; c < 3; ++c) {
                const int t = s.curve_type[c];
                if (t == 0) {
                    if (s.entries[c] < 2 || s.entries[c] > AVIFGPU_ICC_PIPE_MAX_CURVE) return "a curve table has fewer than 2 or more than 4096 entries";
                    if (s.offset[c] < 0 || (int64_t)s.offset[c] + s.entries[c] > p->word_count) return "a curve table lies outside words[]";
                } else if (t < -5 || t > 5) {
                    return "a curve is neither a 16-bit table nor an lcms2 parametric type +-1..+-5";
                }
            }
            break;
        case AVIFGPU_ICC_STAGE_MATRIX:
            if (s.has_bias != 0 && s.has_bias != 1) return "has_bias must be 0 or 1";
            break;
        case AVIFGPU_ICC_STAGE_CLUT16:
            if (++cluts > 1) return "more than one CLUT stage";
            for (int k = 0; k < 3; ++k)
                if (s.entries[k] < 2 || s.entries[k] > AVIFGPU_ICC_PIPE_MAX_GRID) return "a CLUT grid has fewer than 2 or more than 33 points";
            if (s.offset[0] < 0 || (int64_t)s.offset[0] + 3LL * s.entries[0] * s.entries[1] * s.entries[2] > p->word_count) return "the CLUT grid lies outside words[]";
            break;
        case AVIFGPU_ICC_STAGE_LAB_TO_XYZ:
        case AVIFGPU_ICC_STAGE_XYZ_TO_LAB:
            break;
        default:
            return "unknown stage kind";
        }
    }
    return nullptr;
}

// The stamp: a 64-bit checksum of everything but the stamp itself -- the header, all stage records, the words in use -- under a key of
// this library's own, so that a zeroed or copied-then-edited struct does not carry a valid one by accident.
uint64_t icc_pipeline32_checksum(const avifgpu_icc_pipeline32* p)
{
    uint64_t h = 0x6a09e667f3bcc909ull;
    auto mix = [&](const void* data, size_t bytes) {
        const uint8_t* b = static_cast<const uint8_t*>(data);
        size_t i = 0;
        for (; i + 8 <= bytes; i += 8) { uint64_t w; memcpy(&w, b + i, 8); h = (h ^ w) * 0x100000001b3ull; h ^= h >> 29; }
        for (; i < bytes; ++i) { h = (h ^ b[i]) * 0x100000001b3ull; }
    };
    mix(p, offsetof(avifgpu_icc_pipeline32, proof));
    mix(p->stages, sizeof(p->stages));
    const int32_t wc = p->word_count < 0 ? 0 : (p->word_count > AVIFGPU_ICC_PIPE_MAX_WORDS ? AVIFGPU_ICC_PIPE_MAX_WORDS : p->word_count);
    mix(p->words, (size_t)wc * 2);
    return h | 1ull;                                                   // never 0 (= not proven)
}

// Does the program end in its target's destination curves?  The proof compares values with the caller's transform, which says nothing of the
// tag; this says the tag and the values belong together.  Linear Rec.2020 (ColorProfileGeneration.cpp:141-178: gamma 1.0) ends in lcms2's
// reverse of that curve, parametric type -1 with gamma 1; sRGB (cmsCreate_sRGBProfile) in the reverse of its type-4 curve.
static bool target_tail_matches(const avifgpu_icc_pipeline32* p)
{
    const avifgpu_icc_stage32& s = p->stages[p->stage_count - 1];
    if (s.kind != AVIFGPU_ICC_STAGE_CURVES) return false;
    static const double srgb[5] = { 2.4, 1.0 / 1.055, 0.055 / 1.055, 1.0 / 12.92, 0.04045 };
    for (int c = 0; c < 3; ++c) {
        if (p->target == AVIFGPU_ICC_TARGET_REC2020_LINEAR) {
            if (!(s.curve_type[c] == -1 && s.params[c][0] == 1.0)) return false;
        } else {
            if (s.curve_type[c] != -4) return false;
            for (int k = 0; k < 5; ++k) if (std::fabs(s.params[c][k] - srgb[k]) > 1e-6) return false;
        }
    }
    return true;
}

bool icc_pipeline32_stamped(const avifgpu_icc_pipeline32* p)
{
    return p->proof != 0 && !icc_pipeline32_shape_error(p) && p->proof == icc_pipeline32_checksum(p);
}

static void eval_host(const avifgpu_icc_pipeline32* p, const float* in, float* out, uint32_t n)
{
    for (uint32_t i = 0; i < n; ++i) {
        float v[3] = { in[3 * i], in[3 * i + 1], in[3 * i + 2] };
        for (int s = 0; s < p->stage_count; ++s) icc32::stage(p->stages[s], p->words, v);
        out[3 * i] = v[0]; out[3 * i + 1] = v[1]; out[3 * i + 2] = v[2];
    }
}

}  // namespace avifgpu

using namespace avifgpu;

extern "C" int32_t avifgpu_icc_pipeline32_eval(const avifgpu_icc_pipeline32* pipe, const float* rgb_in, float* rgb_out, uint32_t n)
{
    if (!pipe || (n && (!rgb_in || !rgb_out))) return fail(AVIFGPU_formatBadParameters, "null program / buffer");
    if (const char* why = icc_pipeline32_shape_error(pipe)) return fail(AVIFGPU_formatBadParameters, "ICC stage program: %s", why);
    eval_host(pipe, rgb_in, rgb_out, n);
    return 0;
}

extern "C" int32_t avifgpu_icc_pipeline32_prove(avifgpu_icc_pipeline32* pipe, avifgpu_transform_f32_fn float_fn, void* user)
{
    if (!pipe || !float_fn) return fail(AVIFGPU_formatBadParameters, "null program / transform callback");
    pipe->proof = 0;
    if (const char* why = icc_pipeline32_shape_error(pipe)) return fail(AVIFGPU_formatCannotRead, "ICC stage program: %s: keep the CPU path", why);
    if (!target_tail_matches(pipe))
        return fail(AVIFGPU_formatCannotRead, "ICC stage program: it does not end in the destination curves of its target %d: keep the CPU path", pipe->target);

    // the probe set: neutrals, the CLUT's nodes and their word neighbours (in the program's INPUT space, which is the CLUT's own when the
    // curves in front of it are the identity, and a dense sample of it otherwise), random triples in [-0.25, 4], NaN-free extremes
    std::vector<float> pin;
    auto put = [&](float r, float g, float b) { pin.push_back(r); pin.push_back(g); pin.push_back(b); };
    for (int i = 0; i <= 4096; ++i) { const float v = (float)i / 1024.0f; put(v, v, v); }
    for (int i = 1; i <= 256; ++i) { const float v = -(float)i / 1024.0f; put(v, v, v); }
    uint64_t st = 0x3c6ef372fe94f82bull;
    auto rnd = [&]() { st = st * 6364136223846793005ull + 1442695040888963407ull; return (uint32_t)(st >> 33); };
    auto unit = [&]() { return (float)((rnd() & 0xffffff) / 16777216.0); };
    int grid = 0;
    for (int s = 0; s < pipe->stage_count; ++s)
        if (pipe->stages[s].kind == AVIFGPU_ICC_STAGE_CLUT16) grid = pipe->stages[s].entries[0];
    if (grid >= 2) {
        for (int i = 0; i < 8192; ++i) {
            float c[3];
            for (int k = 0; k < 3; ++k) {
                const uint32_t node = rnd() % (uint32_t)grid;
                const int w = (int)((node * 65535u + (uint32_t)(grid - 1) / 2) / (uint32_t)(grid - 1)) + (int)(rnd() % 3) - 1;
                c[k] = (float)(w < 0 ? 0 : (w > 65535 ? 65535 : w)) / 65535.0f;
            }
            put(c[0], c[1], c[2]);
        }
    }
    for (int i = 0; i < 65536; ++i) put(unit() * 4.25f - 0.25f, unit() * 4.25f - 0.25f, unit() * 4.25f - 0.25f);
    for (int i = 0; i < 8192; ++i) put(unit(), unit(), unit());
    const float ext[] = { 0.0f, -0.0f, 1.0f, -1.0f, 1e-30f, -1e-30f, 1.4e-45f, 65535.0f / 65536.0f, 1.0f + 1.0f / 65536.0f, 16.0f, 100.0f,
                          1e4f, -1e4f, 1e20f, -1e20f, 3.0e38f, -3.0e38f };
    for (float a : ext) for (float b : ext) put(a, b, a);

    const uint32_t n = (uint32_t)(pin.size() / 3);
    std::vector<float> want(pin.size()), got(pin.size());
    for (uint32_t i = 0; i < n; i += 4096) float_fn(user, &pin[3 * (size_t)i], &want[3 * (size_t)i], n - i < 4096 ? n - i : 4096);
    eval_host(pipe, pin.data(), got.data(), n);
    uint32_t bad = 0, first = n;
    for (uint32_t i = 0; i < 3 * n; ++i) {
        if (memcmp(&want[i], &got[i], 4) != 0) { if (!bad) first = i / 3; ++bad; }
    }
    if (bad) {
        return fail(AVIFGPU_formatCannotRead,
                    "the ICC stage program is not the caller's float transform (%u of %u probe values differ; first at (%.9g, %.9g, %.9g): %.9g %.9g %.9g, want %.9g %.9g %.9g): keep the CPU path",
                    bad, 3 * n, (double)pin[3 * first], (double)pin[3 * first + 1], (double)pin[3 * first + 2],
                    (double)got[3 * first], (double)got[3 * first + 1], (double)got[3 * first + 2],
                    (double)want[3 * first], (double)want[3 * first + 1], (double)want[3 * first + 2]);
    }
    pipe->proof = icc_pipeline32_checksum(pipe);
    return 0;
}
