// save_stats.cpp -- the three statistics a save can carry, on the host: the code histogram behind the content light
// level (6.6), the thumbnail sums (6.7), the summary of the written planes (6.11).  The calling thread's arms, the check of a write call
// against them and the launch sequence behind a tile's conversion, each once, for the device-pointer path (avifgpu_api.hip) and the
// workers (pipeline.hip) alike.  Host code only: no kernel, no code object.
#include "staging.h"
#include "written_planes.h"

namespace avifgpu {

namespace {

// the calling thread's arms (the three *_attach entries below): host-only bookkeeping, survives a re-binding of the devices
struct Arms {
    SaveStats to;                                    // the targets as attached, whatever a call's descriptor is
    int hist_bits = 0;
    int hist_kind = AVIFGPU_MEM_HOST, thumb_kind = AVIFGPU_MEM_HOST, summary_kind = AVIFGPU_MEM_HOST;
};
thread_local Arms g_arms;

const char* kind_name(int kind) { return kind == AVIFGPU_MEM_DEVICE ? "device" : "host"; }
bool bad_kind(int kind) { return kind != AVIFGPU_MEM_HOST && kind != AVIFGPU_MEM_DEVICE; }

} // namespace

int save_stats_for_call(const avifgpu_write_desc* d, const WriteGeom& g, int mem_kind, SaveStats* s)
{
    const Arms& a = g_arms;
    *s = SaveStats();
    if (a.to.hist && d->depth == 32) {
        if (d->bit_depth != a.hist_bits)
            return fail(AVIFGPU_formatBadParameters, "the armed code histogram has %d-bit bins, this call writes %d-bit codes", a.hist_bits, d->bit_depth);
        if (mem_kind != a.hist_kind)
            return fail(AVIFGPU_formatBadParameters, "the armed code histogram lives in %s memory, this call's pointers do not", kind_name(a.hist_kind));
        s->hist = a.to.hist;
    }
    if (a.to.thumb) {
        if (mem_kind != a.thumb_kind)
            return fail(AVIFGPU_formatBadParameters, "the armed thumbnail sums live in %s memory, this call's pointers do not", kind_name(a.thumb_kind));
        int pw, ph;
        smallest_plane(d, g, pw, ph);
        if (a.to.tw > pw || a.to.th > ph)
            return fail(AVIFGPU_formatBadParameters, "the armed thumbnail is %dx%d, the smallest plane of this save %dx%d", a.to.tw, a.to.th, pw, ph);
        s->thumb = a.to.thumb; s->tw = a.to.tw; s->th = a.to.th;
    }
    if (a.to.summary) {
        if (mem_kind != a.summary_kind)
            return fail(AVIFGPU_formatBadParameters, "the armed summary counters live in %s memory, this call's pointers do not", kind_name(a.summary_kind));
        s->summary = a.to.summary;
    }
    return 0;
}

SaveStats save_stats_host(int* nbins)
{
    const Arms& a = g_arms;
    SaveStats s = a.to;
    *nbins = a.to.hist ? 1 << a.hist_bits : 0;
    if (a.hist_kind != AVIFGPU_MEM_HOST) s.hist = nullptr;
    if (a.thumb_kind != AVIFGPU_MEM_HOST) s.thumb = nullptr;
    if (a.summary_kind != AVIFGPU_MEM_HOST) s.summary = nullptr;
    return s;
}

int launch_save_stats(const avifgpu_write_desc* d, const WriteGeom& g, int row0, int nrows, const WriteParams& p, const SaveStats& s, hipStream_t st)
{
    hipError_t e;
    if (s.hist && (e = launch_write_hist(p, d->planes, reinterpret_cast<unsigned long long*>(s.hist), st)) != hipSuccess)
        return hip_fail(e, "histogram kernel launch", AVIFGPU_writErr);
    if (s.thumb && (e = launch_thumbnail(d, g, row0, nrows, p.dst, p.dst_stride, s.tw, s.th, reinterpret_cast<unsigned long long*>(s.thumb), st)) != hipSuccess)
        return hip_fail(e, "thumbnail kernel launch", AVIFGPU_writErr);
    if (s.summary && (e = launch_summary(d, g, row0, nrows, p.dst, p.dst_stride, s.summary, st)) != hipSuccess)
        return hip_fail(e, "summary kernel launch", AVIFGPU_writErr);
    return 0;
}

} // namespace avifgpu

using namespace avifgpu;

extern "C" {

int32_t avifgpu_histogram_attach(uint64_t* bins, int32_t bit_depth, int32_t mem_kind)
{
    set_error("");
    if (!bins) { g_arms.to.hist = nullptr; g_arms.hist_bits = 0; g_arms.hist_kind = AVIFGPU_MEM_HOST; return 0; }
    if (bit_depth != 10 && bit_depth != 12)
        return fail(AVIFGPU_formatBadParameters, "avifgpu_histogram_attach: bit depth %d (a 32-bit document is saved at 10 or 12 bit)", bit_depth);
    if (bad_kind(mem_kind)) return fail(AVIFGPU_formatBadParameters, "avifgpu_histogram_attach: bad mem_kind %d", mem_kind);
    g_arms.to.hist = bins; g_arms.hist_bits = bit_depth; g_arms.hist_kind = mem_kind;
    return 0;
}

int32_t avifgpu_thumbnail_attach(uint64_t* sums, int32_t tw, int32_t th, int32_t mem_kind)
{
    set_error("");
    if (!sums) { g_arms.to.thumb = nullptr; g_arms.to.tw = g_arms.to.th = 0; g_arms.thumb_kind = AVIFGPU_MEM_HOST; return 0; }
    if (tw < 1 || tw > kThumbMaxSide || th < 1 || th > kThumbMaxSide)
        return fail(AVIFGPU_formatBadParameters, "avifgpu_thumbnail_attach: size %dx%d outside 1..%d", tw, th, kThumbMaxSide);
    if (bad_kind(mem_kind)) return fail(AVIFGPU_formatBadParameters, "avifgpu_thumbnail_attach: bad mem_kind %d", mem_kind);
    g_arms.to.thumb = sums; g_arms.to.tw = tw; g_arms.to.th = th; g_arms.thumb_kind = mem_kind;
    return 0;
}

int32_t avifgpu_summary_attach(uint32_t* counters, int32_t mem_kind)
{
    set_error("");
    if (!counters) { g_arms.to.summary = nullptr; g_arms.summary_kind = AVIFGPU_MEM_HOST; return 0; }
    if (bad_kind(mem_kind)) return fail(AVIFGPU_formatBadParameters, "avifgpu_summary_attach: bad mem_kind %d", mem_kind);
    g_arms.to.summary = counters; g_arms.summary_kind = mem_kind;
    return 0;
}

} // extern "C"
