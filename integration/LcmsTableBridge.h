/*
 * integration/LcmsTableBridge.h -- the adapter-side glue for 16-bit (and, since round 6, 8-bit) documents whose profile the library's own ICC parser does
 * not take (LUT-based / A2B profiles, v4 multi-process-element tags ...).  Depends on lcms2.h and include/avifgpu.h only, so
 * unlike the two *_gpu.cpp adapters it compiles and is tested in this image (tests/test_icc16.py, against Little CMS 2.12).
 *
 * The plug-in links lcms2 and would otherwise run ColorProfileConversion::ConvertRow (ColorProfileConversion.cpp:159-187) on
 * every row on the CPU.  For 16-bit data that transform IS a 33^3 table (avifgpu.h, avifgpu_icc_clut16_from_transforms): this
 * helper creates the two transforms exactly as InitializeForSRGBConversion does (:268-331: sRGB destination,
 * INTENT_PERCEPTUAL, cmsFLAGS_BLACKPOINTCOMPENSATION; COPY_ALPHA changes the formatter, not the colour table), hands
 * cmsDoTransform to the library as the two callbacks, and returns the proven table -- or the library's refusal.  For 32-bit documents
 * lcms2 evaluates the pipeline itself, stage by stage: avifgpu_lcms_document_to_pipeline32 captures and translates it.
 */
#ifndef AVIFGPU_LCMS_TABLE_BRIDGE_H
#define AVIFGPU_LCMS_TABLE_BRIDGE_H

#include "../include/avifgpu.h"

#ifdef __cplusplus
extern "C" {
#endif

/* 0 and *out filled; AVIFGPU_formatCannotRead: keep ConvertRow on the CPU (the profile does not open, no transform, or the
 * proof failed -- avifgpu_last_error() says which); AVIFGPU_formatBadParameters: null arguments. */
int32_t avifgpu_lcms_document_to_srgb_clut16(const void* iccProfile, uint32_t size, avifgpu_icc_clut16* out);
/* The same for an 8-BIT document (round 6): the table proven against the TYPE_RGB_8 transform (avifgpu_icc_clut8_from_transforms). */
int32_t avifgpu_lcms_document_to_srgb_clut8(const void* iccProfile, uint32_t size, avifgpu_icc_clut16* out);
/* A 32-BIT document: the stage program of the float transform ColorProfileConversion creates for `target` -- InitializeForRec2020Conversion
 * (AVIFGPU_ICC_TARGET_REC2020_LINEAR) or InitializeForSRGBConversion(..., 32) (AVIFGPU_ICC_TARGET_SRGB_FLOAT): TYPE_RGB[A]_FLT, perceptual,
 * cmsFLAGS_BLACKPOINTCOMPENSATION (+ COPY_ALPHA).  lcms2 hands its linked pipeline to an optimization plug-in registered in a context of
 * this call's own; each stage is translated, checked alone against lcms2's evaluation of it, and the whole program is proven against the
 * transform (avifgpu_icc_pipeline32_prove).  0 and *out stamped; AVIFGPU_formatCannotRead: keep ConvertRow on the CPU (a stage without a
 * form in avifgpu_icc_pipeline32, or the proof failed -- avifgpu_last_error() says which). */
int32_t avifgpu_lcms_document_to_pipeline32(const void* iccProfile, uint32_t size, int32_t target, int32_t has_alpha,
                                            avifgpu_icc_pipeline32* out);

#ifdef __cplusplus
}
#endif
#endif
