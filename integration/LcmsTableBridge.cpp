// integration/LcmsTableBridge.cpp -- see LcmsTableBridge.h.  Little CMS public API only.
#include "LcmsTableBridge.h"

#include <lcms2.h>
#include <lcms2_plugin.h>       // avifgpu_lcms_document_to_pipeline32 only: the optimization plug-in and the stages' data

#include <cstring>
#include <memory>
#include <vector>

namespace
{
    struct ContextDeleter { using pointer = cmsContext; void operator()(cmsContext c) const noexcept { if (c) cmsDeleteContext(c); } };
    struct ProfileDeleter { void operator()(cmsHPROFILE p) const noexcept { if (p) cmsCloseProfile(p); } };
    struct TransformDeleter { void operator()(cmsHTRANSFORM t) const noexcept { if (t) cmsDeleteTransform(t); } };
    using ScopedContext = std::unique_ptr<_cmsContext_struct, ContextDeleter>;        // the reference keeps the same three RAII handles
    using ScopedProfile = std::unique_ptr<void, ProfileDeleter>;          // (ScopedLcms.h)
    using ScopedTransform = std::unique_ptr<void, TransformDeleter>;

    struct TwoTransforms { cmsHTRANSFORM words, floats; };

    void RunWords(void* user, const uint16_t* in, uint16_t* out, uint32_t pixels)
    {
        cmsDoTransform(static_cast<TwoTransforms*>(user)->words, in, out, pixels);
    }

    void RunBytes(void* user, const uint8_t* in, uint8_t* out, uint32_t pixels)
    {
        cmsDoTransform(static_cast<TwoTransforms*>(user)->words, in, out, pixels);
    }

    void RunFloats(void* user, const float* in, float* out, uint32_t pixels)
    {
        cmsDoTransform(static_cast<TwoTransforms*>(user)->floats, in, out, pixels);
    }
}

extern "C" int32_t avifgpu_lcms_document_to_srgb_clut16(const void* iccProfile, uint32_t size, avifgpu_icc_clut16* out)
{
    if (!iccProfile || size == 0 || !out) return AVIFGPU_formatBadParameters;

    ScopedContext context(cmsCreateContext(nullptr, nullptr));
    if (!context) return AVIFGPU_formatCannotRead;
    ScopedProfile document(cmsOpenProfileFromMemTHR(context.get(), iccProfile, size));
    ScopedProfile srgb(cmsCreate_sRGBProfileTHR(context.get()));
    if (!document || !srgb || cmsGetColorSpace(document.get()) != cmsSigRgbData) return AVIFGPU_formatCannotRead;

    const cmsUInt32Number flags = cmsFLAGS_BLACKPOINTCOMPENSATION;        // ColorProfileConversion.cpp:278
    ScopedTransform words(cmsCreateTransformTHR(context.get(), document.get(), TYPE_RGB_16, srgb.get(), TYPE_RGB_16, INTENT_PERCEPTUAL, flags));
    ScopedTransform floats(cmsCreateTransformTHR(context.get(), document.get(), TYPE_RGB_FLT, srgb.get(), TYPE_RGB_FLT, INTENT_PERCEPTUAL, flags));
    if (!words || !floats) return AVIFGPU_formatCannotRead;

    TwoTransforms both{ words.get(), floats.get() };
    return avifgpu_icc_clut16_from_transforms(RunFloats, RunWords, &both, out);
}

// Round 6: the same for an 8-bit document -- the TYPE_RGB_8 transform InitializeForSRGBConversion creates for hostBitsPerChannel == 8
// (ColorProfileConversion.cpp:280-289) in the proof's slot.  A matrix/TRC profile is refused by the proof (lcms2 runs its matrix-shaper
// there): the library's own avifgpu_icc_prepare_shaper8 has taken it before an adapter gets here.
extern "C" int32_t avifgpu_lcms_document_to_srgb_clut8(const void* iccProfile, uint32_t size, avifgpu_icc_clut16* out)
{
    if (!iccProfile || size == 0 || !out) return AVIFGPU_formatBadParameters;

    ScopedContext context(cmsCreateContext(nullptr, nullptr));
    if (!context) return AVIFGPU_formatCannotRead;
    ScopedProfile document(cmsOpenProfileFromMemTHR(context.get(), iccProfile, size));
    ScopedProfile srgb(cmsCreate_sRGBProfileTHR(context.get()));
    if (!document || !srgb || cmsGetColorSpace(document.get()) != cmsSigRgbData) return AVIFGPU_formatCannotRead;

    const cmsUInt32Number flags = cmsFLAGS_BLACKPOINTCOMPENSATION;        // ColorProfileConversion.cpp:278
    ScopedTransform bytes(cmsCreateTransformTHR(context.get(), document.get(), TYPE_RGB_8, srgb.get(), TYPE_RGB_8, INTENT_PERCEPTUAL, flags));
    ScopedTransform floats(cmsCreateTransformTHR(context.get(), document.get(), TYPE_RGB_FLT, srgb.get(), TYPE_RGB_FLT, INTENT_PERCEPTUAL, flags));
    if (!bytes || !floats) return AVIFGPU_formatCannotRead;

    TwoTransforms both{ bytes.get(), floats.get() };
    return avifgpu_icc_clut8_from_transforms(RunFloats, RunBytes, &both, out);
}

// ---- 32-bit documents: lcms2's float stage program (avifgpu_icc_pipeline32) -----------------------------------------------------------
namespace
{
    struct PipelineDeleter { void operator()(cmsPipeline* p) const noexcept { if (p) cmsPipelineFree(p); } };
    using ScopedPipeline = std::unique_ptr<cmsPipeline, PipelineDeleter>;

    // The optimization plug-in: lcms2 calls it with the linked, pre-optimised pipeline of every transform created in its context -- for
    // float formatters the very pipeline cmsDoTransform evaluates (the built-in optimizations all decline float formats).  It keeps a copy
    // and declines, so lcms2 carries on exactly as without it.  The capture slot is the context's user data: no globals.
    struct Capture { cmsPipeline* lut = nullptr; };
    cmsBool CapturePipeline(cmsPipeline** lut, cmsUInt32Number, cmsUInt32Number*, cmsUInt32Number*, cmsUInt32Number*)
    {
        Capture* cap = static_cast<Capture*>(cmsGetContextUserData(cmsGetPipelineContextID(*lut)));
        if (cap && !cap->lut) cap->lut = cmsPipelineDup(*lut);
        return FALSE;
    }
    cmsPluginOptimization g_capture_plugin = { { cmsPluginMagicNumber, 2060, cmsPluginOptimizationSig, nullptr }, CapturePipeline };

    cmsHPROFILE Rec2020Linear(cmsContext ctx)          // CreateRec2020LinearRGBProfile (ColorProfileGeneration.cpp:141-178)
    {
        const cmsCIExyY whitepoint = { 0.3127, 0.3290, 1.0f };
        const cmsCIExyYTRIPLE primaries = { { 0.708, 0.292, 1.0 }, { 0.170, 0.797, 1.0 }, { 0.131, 0.046, 1.0 } };
        cmsToneCurve* c = cmsBuildGamma(ctx, 1.0);
        if (!c) return nullptr;
        cmsToneCurve* three[3] = { c, c, c };
        cmsHPROFILE h = cmsCreateRGBProfileTHR(ctx, &whitepoint, &primaries, three);
        cmsFreeToneCurve(c);
        return h;
    }

    struct FloatTransform { cmsHTRANSFORM t; bool alpha; std::vector<float> buf; };
    void RunFloatsRGB(void* user, const float* in, float* out, uint32_t pixels)
    {
        FloatTransform* f = static_cast<FloatTransform*>(user);
        if (!f->alpha) { cmsDoTransform(f->t, in, out, pixels); return; }
        f->buf.assign((size_t)pixels * 4, 1.0f);                      // the RGBA transform the plug-in runs, alpha copied
        for (uint32_t i = 0; i < pixels; ++i) memcpy(&f->buf[4 * (size_t)i], in + 3 * (size_t)i, 12);
        cmsDoTransform(f->t, f->buf.data(), f->buf.data(), pixels);
        for (uint32_t i = 0; i < pixels; ++i) memcpy(out + 3 * (size_t)i, &f->buf[4 * (size_t)i], 12);
    }

    // Translate one lcms2 stage into *s (tables appended to out->words).  false: no form for it.
    bool TranslateStage(cmsStage* st, avifgpu_icc_pipeline32* out, avifgpu_icc_stage32* s, bool lab_xyz_swapped)
    {
        std::memset(s, 0, sizeof(*s));
        if (cmsStageInputChannels(st) != 3 || cmsStageOutputChannels(st) != 3) return false;
        const cmsStageSignature tag = cmsStageType(st);
        const void* data = cmsStageData(st);
        // _cmsStageAllocLabV2ToV4 is a matrix stage and _cmsStageAllocLabV2ToV4curves a curve set under the same tag; a curve set's data
        // starts with nCurves (3), a matrix's with a heap pointer (never 3)
        const bool v2v4 = tag == cmsSigLabV2toV4 || tag == cmsSigLabV4toV2;
        const bool curves = tag == cmsSigCurveSetElemType || (v2v4 && data && *static_cast<const cmsUInt32Number*>(data) == 3);
        if (curves) {
            const _cmsStageToneCurvesData* d = static_cast<const _cmsStageToneCurvesData*>(data);
            if (!d || d->nCurves != 3 || !d->TheCurves) return false;
            s->kind = AVIFGPU_ICC_STAGE_CURVES;
            for (int c = 0; c < 3; ++c) {
                const cmsToneCurve* t = d->TheCurves[c];
                if (!t || cmsIsToneCurveMultisegment(t)) return false;
                const cmsInt32Number type = cmsGetToneCurveParametricType(t);
                if (type != 0) {
                    if (type < -5 || type > 5) return false;
                    s->curve_type[c] = type;
                    const cmsFloat64Number* P = cmsGetToneCurveParams(t);
                    if (!P) return false;
                    for (int k = 0; k < 10; ++k) s->params[c][k] = P[k];
                } else {
                    const cmsUInt32Number n = cmsGetToneCurveEstimatedTableEntries(t);
                    const cmsUInt16Number* T = cmsGetToneCurveEstimatedTable(t);
                    if (!T || n < 2 || n > AVIFGPU_ICC_PIPE_MAX_CURVE || out->word_count + (int64_t)n > AVIFGPU_ICC_PIPE_MAX_WORDS) return false;
                    s->entries[c] = (int32_t)n;
                    s->offset[c] = out->word_count;
                    std::memcpy(out->words + out->word_count, T, n * 2);
                    out->word_count += (int32_t)n;
                }
            }
            return true;
        }
        if (tag == cmsSigMatrixElemType || v2v4) {
            const _cmsStageMatrixData* d = static_cast<const _cmsStageMatrixData*>(data);
            if (!d || !d->Double) return false;
            s->kind = AVIFGPU_ICC_STAGE_MATRIX;
            for (int k = 0; k < 9; ++k) s->matrix[k] = d->Double[k];
            if (d->Offset) { s->has_bias = 1; for (int k = 0; k < 3; ++k) s->bias[k] = d->Offset[k]; }
            return true;
        }
        if (tag == cmsSigCLutElemType) {
            const _cmsStageCLutData* d = static_cast<const _cmsStageCLutData*>(data);
            if (!d || d->HasFloatValues || !d->Tab.T || !d->Params) return false;
            const cmsInterpParams* ip = d->Params;
            if (ip->nInputs != 3 || ip->nOutputs != 3 || (ip->dwFlags & CMS_LERP_FLAGS_TRILINEAR)) return false;
            int64_t nodes = 1;
            for (int k = 0; k < 3; ++k) {
                if (ip->nSamples[k] < 2 || ip->nSamples[k] > AVIFGPU_ICC_PIPE_MAX_GRID) return false;
                s->entries[k] = (int32_t)ip->nSamples[k];
                nodes *= ip->nSamples[k];
            }
            if ((int64_t)d->nEntries != 3 * nodes || out->word_count + 3 * nodes > AVIFGPU_ICC_PIPE_MAX_WORDS) return false;
            s->kind = AVIFGPU_ICC_STAGE_CLUT16;
            s->offset[0] = out->word_count;
            std::memcpy(out->words + out->word_count, d->Tab.T, (size_t)(3 * nodes) * 2);
            out->word_count += (int32_t)(3 * nodes);
            return true;
        }
        // lcms2.h's comments on these two tags are swapped; which conversion a stage performs is settled by the check below
        // (lab_xyz_swapped = the second attempt)
        if (tag == cmsSigLab2XYZElemType || tag == cmsSigXYZ2LabElemType) {
            const bool lab2xyz = (tag == cmsSigLab2XYZElemType) != lab_xyz_swapped;
            s->kind = lab2xyz ? AVIFGPU_ICC_STAGE_LAB_TO_XYZ : AVIFGPU_ICC_STAGE_XYZ_TO_LAB;
            return true;
        }
        return false;
    }

    // The translation of one stage against lcms2's own evaluation of it (a one-stage pipeline): bit-identical floats on a probe set that
    // covers words, grid nodes and values outside [0, 1].
    bool StageAgrees(cmsContext ctx, cmsStage* st, const avifgpu_icc_pipeline32& prog, const avifgpu_icc_stage32& s, avifgpu_icc_pipeline32* scratch)
    {
        ScopedPipeline one(cmsPipelineAlloc(ctx, 3, 3));
        cmsStage* dup = cmsStageDup(st);
        if (!one || !dup) { if (dup) cmsStageFree(dup); return false; }
        if (!cmsPipelineInsertStage(one.get(), cmsAT_END, dup)) return false;
        scratch->target = prog.target;
        scratch->stage_count = 1;
        scratch->word_count = prog.word_count;
        scratch->stages[0] = s;
        std::memcpy(scratch->words, prog.words, (size_t)prog.word_count * 2);
        std::vector<float> in;
        uint64_t state = 0xbb67ae8584caa73bull;
        auto rnd = [&]() { state = state * 6364136223846793005ull + 1442695040888963407ull; return (uint32_t)(state >> 33); };
        for (int i = 0; i < 4096; ++i) for (int c = 0; c < 3; ++c) in.push_back((float)((rnd() & 0xffffff) / 16777216.0) * 4.25f - 0.25f);
        for (int i = 0; i < 4096; ++i) for (int c = 0; c < 3; ++c) in.push_back((float)(rnd() & 0xffff) / 65535.0f + (float)((int)(rnd() % 3) - 1) * 7.6e-6f);
        const int grid = s.kind == AVIFGPU_ICC_STAGE_CLUT16 ? s.entries[0] : 17;
        for (int i = 0; i < 2048; ++i)
            for (int c = 0; c < 3; ++c) in.push_back((float)((rnd() % (uint32_t)grid) * 65535u / (uint32_t)(grid - 1) + rnd() % 3) / 65535.0f);
        for (int i = 0; i <= 256; ++i) for (int c = 0; c < 3; ++c) in.push_back((float)i / 256.0f);
        const uint32_t n = (uint32_t)(in.size() / 3);
        std::vector<float> want(in.size()), got(in.size());
        for (uint32_t i = 0; i < n; ++i) cmsPipelineEvalFloat(&in[3 * (size_t)i], &want[3 * (size_t)i], one.get());
        if (avifgpu_icc_pipeline32_eval(scratch, in.data(), got.data(), n) != AVIFGPU_noErr) return false;
        return std::memcmp(want.data(), got.data(), want.size() * sizeof(float)) == 0;
    }
}

extern "C" int32_t avifgpu_lcms_document_to_pipeline32(const void* iccProfile, uint32_t size, int32_t target, int32_t has_alpha,
                                                       avifgpu_icc_pipeline32* out)
{
    if (!iccProfile || size == 0 || !out) return AVIFGPU_formatBadParameters;
    if (target != AVIFGPU_ICC_TARGET_REC2020_LINEAR && target != AVIFGPU_ICC_TARGET_SRGB_FLOAT) return AVIFGPU_formatBadParameters;

    Capture cap;
    ScopedContext context(cmsCreateContext(&g_capture_plugin, &cap));
    if (!context) return AVIFGPU_formatCannotRead;
    ScopedPipeline captured;
    ScopedTransform floats;
    {
        ScopedProfile document(cmsOpenProfileFromMemTHR(context.get(), iccProfile, size));
        ScopedProfile dest(target == AVIFGPU_ICC_TARGET_SRGB_FLOAT ? cmsCreate_sRGBProfileTHR(context.get()) : Rec2020Linear(context.get()));
        if (!document || !dest || cmsGetColorSpace(document.get()) != cmsSigRgbData) return AVIFGPU_formatCannotRead;
        cmsUInt32Number format = TYPE_RGB_FLT, flags = cmsFLAGS_BLACKPOINTCOMPENSATION;      // ColorProfileConversion.cpp:244-251, :278-289
        if (has_alpha) { format = TYPE_RGBA_FLT; flags |= cmsFLAGS_COPY_ALPHA; }
        floats.reset(cmsCreateTransformTHR(context.get(), document.get(), format, dest.get(), format, INTENT_PERCEPTUAL, flags));
        captured.reset(cap.lut);
        cap.lut = nullptr;
        if (!floats || !captured) return AVIFGPU_formatCannotRead;
    }

    std::memset(out, 0, offsetof(avifgpu_icc_pipeline32, words));
    out->target = target;
    std::unique_ptr<avifgpu_icc_pipeline32> scratch(new avifgpu_icc_pipeline32);
    for (cmsStage* st = cmsPipelineGetPtrToFirstStage(captured.get()); st; st = cmsStageNext(st)) {
        if (out->stage_count == AVIFGPU_ICC_PIPE_MAX_STAGES) return AVIFGPU_formatCannotRead;
        avifgpu_icc_stage32 s;
        bool ok = false;
        for (int attempt = 0; attempt < 2 && !ok; ++attempt) {
            const int32_t words_before = out->word_count;
            ok = TranslateStage(st, out, &s, attempt == 1) && StageAgrees(context.get(), st, *out, s, scratch.get());
            if (!ok) out->word_count = words_before;
            if (s.kind != AVIFGPU_ICC_STAGE_LAB_TO_XYZ && s.kind != AVIFGPU_ICC_STAGE_XYZ_TO_LAB) break;     // only those have a second reading
        }
        if (!ok) return AVIFGPU_formatCannotRead;
        out->stages[out->stage_count++] = s;
    }
    if (out->stage_count == 0) return AVIFGPU_formatCannotRead;

    FloatTransform f{ floats.get(), has_alpha != 0, {} };
    return avifgpu_icc_pipeline32_prove(out, RunFloatsRGB, &f);
}
