// upsample_window.h -- which chroma samples a rectangle of the upsampled planes needs, and how the host path stages them.
// Plain integer arithmetic shared by the kernel (what it clamps its loads to), the host path (what it uploads) and a stand-alone
// host program (tools/upsample_window_check.cpp) that runs it under the sanitizers: no HIP type, no device call.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define AG_UPW_HD __host__ __device__
#else
#define AG_UPW_HD
#endif

namespace avifgpu {

// Chroma columns [lo, hi] and rows [rlo, rhi] that the taps of rectangle [x0, x0 + w) x [y0, y0 + h) touch once their indices are clamped
// to the WHOLE plane (cw x ch): one sample of halo on each side that exists; 4:2:2 (ys == 0) needs its own rows only.  `left` widens the
// halo on the left to that many samples (the host path asks for 8 bytes of them, see stage_window).
struct UpNeed { int lo, hi, rlo, rhi; };
AG_UPW_HD inline UpNeed up_need(int cw, int ch, int ys, int x0, int y0, int w, int h, int left = 1)
{
    UpNeed n;
    n.lo = (x0 >> 1) - left; if (n.lo < 0) n.lo = 0;
    n.hi = ((x0 + w - 1) >> 1) + 1; if (n.hi > cw - 1) n.hi = cw - 1;
    if (ys) {
        n.rlo = (y0 >> 1) - 1; if (n.rlo < 0) n.rlo = 0;
        n.rhi = ((y0 + h - 1) >> 1) + 1; if (n.rhi > ch - 1) n.rhi = ch - 1;
    } else { n.rlo = y0; n.rhi = y0 + h - 1; }
    return n;
}

// The resident window the host path uploads for that rectangle: `rows` rows of `row_bytes` bytes from host byte offset
// rlo * stride + lo * ssz of a chroma plane, to the first byte of a device buffer of `pitch`-byte rows; the window's origin in chroma
// coordinates is (lo, rlo).  The left halo is 8 bytes of samples where the plane has them: the copy then starts on the buffer's first
// byte (an unaligned destination makes a strided upload slow) AND the sample under x0 sits on an 8-byte boundary, which keeps the
// kernel's 8-byte loads aligned.
struct UpStage { UpNeed need; int64_t row_bytes, rows, pitch; };
inline UpStage stage_window(int cw, int ch, int ys, int ssz, int x0, int y0, int w, int h)
{
    UpStage s;
    s.need = up_need(cw, ch, ys, x0, y0, w, h, 8 / ssz);
    s.row_bytes = (int64_t)(s.need.hi - s.need.lo + 1) * ssz;
    s.rows = (int64_t)s.need.rhi - s.need.rlo + 1;
    s.pitch = (s.row_bytes + 255) / 256 * 256;
    return s;
}
inline int64_t stage_host_offset(const UpStage& s, int64_t stride, int ssz) { return (int64_t)s.need.rlo * stride + (int64_t)s.need.lo * ssz; }

} // namespace avifgpu
