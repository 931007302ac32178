// staged_open.cpp -- what the oriented, upsampled and cropped opens (orient_kernels.hip, upsample_kernels.hip, crop_kernels.hip) share on
// the host: the argument checks of their avifgpu_read_rows_* entries, and the staged path of their host-pointer calls.
// Host code only: no kernel, no code object.
//
// The staged path cuts the caller's rows into tiles and alternates two slots of the library's own on the first bound context: a tile's
// planes go up, the feature's device path is enqueued, the rows come down -- all on the slot's stream, so tile k + 1 goes up while tile k
// is computed.  What goes up and what is enqueued is the feature's (StagedPlan, StagedEnqueue); everything else is here, once.
#include <algorithm>

#include "staging.h"

namespace avifgpu {

namespace {

// ONE pool for the three features.  That is safe: their host loops never nest (the upsampled and the cropped one call only
// device-pointer entries from inside), HostCallGuard admits one of them at a time, and every call drains both streams before it
// returns, so nothing is in flight between calls and a buffer grown by one feature is free for the next.
struct OpenSlot {
    hipStream_t stream = nullptr;
    void* buf[6] = { nullptr, nullptr, nullptr, nullptr, nullptr, nullptr };      // the four planes, scratch, out
    size_t cap[6] = { 0, 0, 0, 0, 0, 0 };
};
OpenSlot g_open_slots[2];
int g_open_device = -1;

void free_open_slots()
{
    for (OpenSlot& s : g_open_slots) {
        for (int i = 0; i < 6; ++i) if (s.buf[i]) (void)hipFree(s.buf[i]);
        if (s.stream) (void)hipStreamDestroy(s.stream);
        s = OpenSlot();
    }
    g_open_device = -1;
}

hipError_t grow(OpenSlot& s, int i, int64_t bytes)
{
    const size_t need = (size_t)std::max<int64_t>(bytes, 256);   // a 1 x 1 crop of an image without scratch still gets a buffer
    if (s.cap[i] >= need) return hipSuccess;
    if (s.buf[i]) { (void)hipFree(s.buf[i]); s.buf[i] = nullptr; s.cap[i] = 0; }
    const size_t want = need + need / 4;
    const hipError_t e = hipMalloc(&s.buf[i], want);
    if (e == hipSuccess) s.cap[i] = want;
    return e;
}

// one tile on slot s; the caller has synchronised the slot's stream
int stage_tile(OpenSlot& s, const StagedTile& t, const StagedEnqueue& enqueue, uint8_t* dst, int64_t dst_row_bytes, int64_t row_bytes)
{
    hipError_t e;
    StagedBuffers b = { { nullptr, nullptr, nullptr, nullptr }, { 0, 0, 0, 0 }, nullptr, nullptr, s.stream };
    for (int pl = 0; pl < 4; ++pl) {
        const StagedUpload& u = t.up[pl];
        if (!u.host) continue;
        if ((e = grow(s, pl, u.pitch * u.rows)) != hipSuccess) return hip_fail(e, "hipMalloc", AVIFGPU_memFullErr);
        if ((e = hipMemcpy2DAsync(s.buf[pl], (size_t)u.pitch, u.host, (size_t)u.host_stride, (size_t)u.row_bytes, (size_t)u.rows, hipMemcpyHostToDevice, s.stream)) != hipSuccess)
            return hip_fail(e, "hipMemcpy2DAsync (planes)", AVIFGPU_readErr);
        b.plane[pl] = s.buf[pl]; b.pitch[pl] = u.pitch;
    }
    if ((e = grow(s, 5, t.out_pitch * t.n)) != hipSuccess || (e = grow(s, 4, t.scratch_bytes)) != hipSuccess) return hip_fail(e, "hipMalloc", AVIFGPU_memFullErr);
    b.scratch = s.buf[4]; b.out = s.buf[5];
    const int err = enqueue(b);
    if (err) return err;
    if ((e = hipMemcpy2DAsync(dst, (size_t)dst_row_bytes, b.out, (size_t)t.out_pitch, (size_t)row_bytes, (size_t)t.n, hipMemcpyDeviceToHost, s.stream)) != hipSuccess)
        return hip_fail(e, "hipMemcpy2DAsync (rows)", AVIFGPU_readErr);
    return 0;
}

} // namespace

int staged_open(const char* name, size_t tile_bytes, int64_t row_bytes, int orow0, int onrows, uint8_t* dst, int64_t dst_row_bytes,
                const StagedPlan& plan, const StagedEnqueue& enqueue)
{
    HostCallGuard serial;
    char what[64];
    snprintf(what, sizeof(what), "%s: staged tile", name);
    const int device = context_device(0);
    int prev = -1;
    if (hipGetDevice(&prev) != hipSuccess) { (void)hipGetLastError(); prev = -1; }
    hipError_t e = hipSetDevice(device);
    if (e != hipSuccess) return hip_fail(e, "hipSetDevice", AVIFGPU_readErr);
    if (g_open_device != device) {                             // device 0 of the bound contexts changed: the pool moves
        if (g_open_device >= 0) { (void)hipSetDevice(g_open_device); free_open_slots(); (void)hipSetDevice(device); }
        g_open_device = device;
    }
    int err = 0;
    const int max_rows = (int)std::max<int64_t>(2, std::min<int64_t>((int64_t)(tile_bytes / (size_t)std::max<int64_t>(row_bytes, 1)), 1 << 30));
    int k = 0;
    for (int o0 = orow0; o0 < orow0 + onrows && !err; ++k) {
        StagedTile t = {};
        if ((err = plan(o0, orow0 + onrows - o0, max_rows, t))) break;
        if (t.n < 1) { err = fail(AVIFGPU_readErr, "%s: empty tile", name); break; }
        OpenSlot& s = g_open_slots[k & 1];
        if (!s.stream && (e = hipStreamCreateWithFlags(&s.stream, hipStreamNonBlocking)) != hipSuccess) { err = hip_fail(e, "hipStreamCreate", AVIFGPU_readErr); break; }
        if ((e = hipStreamSynchronize(s.stream)) != hipSuccess) { err = hip_fail(e, what, AVIFGPU_readErr); break; }
        err = stage_tile(s, t, enqueue, dst + (int64_t)(o0 - orow0) * dst_row_bytes, dst_row_bytes, row_bytes);
        o0 += t.n;
    }
    for (OpenSlot& s : g_open_slots) {                         // drained also after a failure: nothing of this call stays in flight
        if (!s.stream) continue;
        e = hipStreamSynchronize(s.stream);
        if (e != hipSuccess && !err) err = hip_fail(e, what, AVIFGPU_readErr);
    }
    if (prev >= 0 && prev != device) (void)hipSetDevice(prev);
    return err;
}

void release_open_staging()
{
    HostCallGuard serial;
    if (g_open_device < 0) return;
    int prev = -1;
    if (hipGetDevice(&prev) != hipSuccess) { (void)hipGetLastError(); prev = -1; }
    if (hipSetDevice(g_open_device) == hipSuccess) free_open_slots();
    else { (void)hipGetLastError(); g_open_device = -1; for (OpenSlot& s : g_open_slots) s = OpenSlot(); }
    if (prev >= 0) (void)hipSetDevice(prev);
}

int check_open_entry(const OpenEntry& a, int64_t need, const std::function<int(int)>& own)
{
    int err;
    const int64_t row_bytes = a.out_w * a.bpp;
    if (a.mem_kind != AVIFGPU_MEM_HOST && a.mem_kind != AVIFGPU_MEM_DEVICE) return fail(AVIFGPU_formatBadParameters, "bad mem_kind %d", a.mem_kind);
    if (!a.src || !a.src_stride || !a.dst) return fail(AVIFGPU_formatBadParameters, "null buffer");
    if (row_bytes > 0x7fffffffLL) return fail(AVIFGPU_memFullErr, "rowBytes exceeds int32");
    if (a.dst_row_bytes < row_bytes) return fail(AVIFGPU_formatBadParameters, "dst_row_bytes %lld < %lld", (long long)a.dst_row_bytes, (long long)row_bytes);
    // the whole image's planes, as avifgpu_read_rows checks a tile's
    if ((err = check_read_buffers(a.desc, *a.g, a.desc->height, a.src, a.src_stride, a.dst, (int64_t)a.desc->width * a.bpp))) return err;
    if ((err = own(0))) return err;
    if (a.mem_kind == AVIFGPU_MEM_DEVICE && need > 0 && (!a.scratch || a.scratch_bytes < need))
        return fail(AVIFGPU_formatBadParameters, "%s: %lld bytes of scratch, %lld needed (%s)", a.who, (long long)(a.scratch ? a.scratch_bytes : 0), (long long)need, a.scratch_helper);
    if ((err = own(1))) return err;
    if (context_count() == 0) return fail(AVIFGPU_formatBadParameters, "avifgpu_init has not succeeded: no HIP device bound (no CPU fallback)");
    return a.onrows == 0 ? kOpenEntryOver : 0;
}

} // namespace avifgpu
