/*
 * avifgpu.h -- C-ABI of the MI355X-native pixel-conversion layer for the
 * avif-format Photoshop plug-in (reference: 0xC0000054/avif-format @ 1.0.7.0).
 *
 * This is the drop-in boundary.  It replaces the per-pixel work of
 *   - the six CreateHeifImage{Gray,RGB}{Eight,Sixteen,ThirtyTwo}Bit functions
 *     (reference src/common/WriteHeifImage.h:29-63, bodies WriteHeifImage.cpp:169-1139),
 *   - optionally libheif's RGB -> YCbCr + chroma-subsample stage that runs inside
 *     heif_context_encode_image (reference call site src/common/Write.cpp:44, selected by
 *     src/common/WriteMetadata.cpp:107-149 and src/common/Write.cpp:96-127),
 *   - the six ReadHeifImage{Gray,RGB}{Eight,Sixteen,ThirtyTwo}Bit functions
 *     (reference src/common/ReadHeifImage.h:27-63) together with the twelve Decode*Row* kernels
 *     (reference src/common/YUVDecode.h:29-145, bodies YuvDecode.cpp:55-696).
 *
 * Everything crossing this boundary is plain C: PODs, raw pointers, sizes.  No C++ types, no
 * torch types.  Pointers are either all host pointers (AVIFGPU_MEM_HOST: the library cuts the rows into
 * one tile per bound device, streams each through its own device buffers and returns when the planes
 * are back in host memory; page-locked buffers are used for DMA directly, pageable ones are bounced
 * through pinned staging by the library's worker threads; `stream` is ignored) or all device pointers
 * (AVIFGPU_MEM_DEVICE: zero-copy, the kernel is enqueued on `stream` -- a hipStream_t, NULL = HIP's
 * default stream -- on the caller's current device and the call returns without synchronising).
 *
 * Return values are Photoshop OSErr codes (reference error convention: src/common/Write.cpp:345-364,
 * src/common/Read.cpp:531-550): 0 = noErr.
 *
 * Threading: AVIFGPU_MEM_DEVICE calls may come from any thread (they only enqueue a kernel).  AVIFGPU_MEM_HOST calls and the
 * FormatRecord shim of avifgpu_host.h share the bound contexts' staging slots: the library serialises them (one conversion at a time
 * per process, later callers wait) -- the plug-in itself is called serially on Photoshop's main thread (AvifFormat.cpp:104-199).
 */
#ifndef AVIFGPU_H
#define AVIFGPU_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define AVIFGPU_ABI_VERSION 5

/* ---- OSErr codes used by the hot path (Photoshop SDK values) ------------------------------- */
#define AVIFGPU_noErr                0
#define AVIFGPU_userCanceledErr   (-128)  /* abortProc() returned true: WriteHeifImage.cpp:1019-1022 */
#define AVIFGPU_readErr            (-19)
#define AVIFGPU_writErr            (-20)
#define AVIFGPU_memFullErr        (-108)  /* std::bad_alloc mapping: Write.cpp:345-348 */
#define AVIFGPU_formatBadParameters (-30500) /* Write.cpp:318,334 default branch */
#define AVIFGPU_formatCannotRead    (-30501) /* WriteHeifImage.cpp:57,81 default branch */

/* ---- enums (numeric values follow the reference / libheif / ITU-T H.273) -------------------- */

/* ColorTransferFunction, reference src/common/ColorTransfer.h:28-34 (same order).  HLG on the WRITE side is an extension:
 * the reference defines LinearToHLG (ColorTransfer.cpp:141-164) but its save loops throw for it; avifgpu_write_rows accepts it
 * for colour images, the FormatRecord-protocol shim (avifgpu_host.h) rejects it with writErr like the plug-in. */
enum {
    AVIFGPU_TRANSFER_PQ       = 0,
    AVIFGPU_TRANSFER_HLG      = 1,
    AVIFGPU_TRANSFER_SMPTE428 = 2,
    AVIFGPU_TRANSFER_CLIP     = 3
};

/* AlphaState, reference src/common/AlphaState.h:24-29 (same order). */
enum {
    AVIFGPU_ALPHA_NONE          = 0,
    AVIFGPU_ALPHA_STRAIGHT      = 1,
    AVIFGPU_ALPHA_PREMULTIPLIED = 2
};

/* heif_colorspace / heif_chroma subset (libheif public header values). */
enum {
    AVIFGPU_COLORSPACE_YCBCR      = 0,
    AVIFGPU_COLORSPACE_RGB        = 1,
    AVIFGPU_COLORSPACE_MONOCHROME = 2
};
enum {
    AVIFGPU_CHROMA_MONOCHROME = 0,
    AVIFGPU_CHROMA_420        = 1,
    AVIFGPU_CHROMA_422        = 2,
    AVIFGPU_CHROMA_444        = 3
};

/* nclx matrix_coefficients (H.273 table 4 == heif_matrix_coefficients). */
enum {
    AVIFGPU_MATRIX_RGB_GBR        = 0,
    AVIFGPU_MATRIX_BT709          = 1,
    AVIFGPU_MATRIX_UNSPECIFIED    = 2,
    AVIFGPU_MATRIX_FCC            = 4,
    AVIFGPU_MATRIX_BT470BG        = 5,
    AVIFGPU_MATRIX_BT601          = 6,
    AVIFGPU_MATRIX_SMPTE240M      = 7,
    AVIFGPU_MATRIX_YCGCO          = 8,
    AVIFGPU_MATRIX_BT2020_NCL     = 9,
    AVIFGPU_MATRIX_BT2020_CL      = 10,
    AVIFGPU_MATRIX_SMPTE2085      = 11,
    AVIFGPU_MATRIX_CHROMA_DERIVED_NCL = 12,
    AVIFGPU_MATRIX_CHROMA_DERIVED_CL  = 13,
    AVIFGPU_MATRIX_ICTCP          = 14
};

/* nclx colour_primaries (H.273 table 2 == heif_color_primaries). */
enum {
    AVIFGPU_PRIMARIES_BT709      = 1,
    AVIFGPU_PRIMARIES_UNSPECIFIED = 2,
    AVIFGPU_PRIMARIES_BT470M     = 4,
    AVIFGPU_PRIMARIES_BT470BG    = 5,
    AVIFGPU_PRIMARIES_BT601      = 6,
    AVIFGPU_PRIMARIES_SMPTE240M  = 7,
    AVIFGPU_PRIMARIES_GENERIC_FILM = 8,
    AVIFGPU_PRIMARIES_BT2020     = 9,
    AVIFGPU_PRIMARIES_SMPTE428   = 10,
    AVIFGPU_PRIMARIES_SMPTE431   = 11,
    AVIFGPU_PRIMARIES_SMPTE432   = 12,
    AVIFGPU_PRIMARIES_EBU3213    = 22
};

/* nclx transfer_characteristics (only the three HDR curves the read path accepts,
 * reference src/common/ColorTransfer.cpp:47-67). */
enum {
    AVIFGPU_TC_SRGB     = 13,
    AVIFGPU_TC_PQ       = 16,
    AVIFGPU_TC_SMPTE428 = 17,
    AVIFGPU_TC_HLG      = 18
};

/* What the write path emits. */
enum {
    /* Exactly what CreateHeifImage* hands to libheif: interleaved RGB(A) at bit_depth for colour
     * (heif_channel_interleaved, WriteHeifImage.cpp:643-646), planar Y(+Alpha) for gray
     * (WriteHeifImage.cpp:181-194).  dst[0] = interleaved / Y, dst[3] = Alpha (gray only). */
    AVIFGPU_OUT_REFERENCE = 0,
    /* Fused: stage A above followed by libheif's RGB->YCbCr + chroma subsample (Write.cpp:44).
     * dst[0..2] = Y, Cb, Cr planes, dst[3] = Alpha plane.  Colour sources only. */
    AVIFGPU_OUT_YCBCR = 1
};

/* Chroma down-sampling filter of the fused path (libheif's stage; libheif is not vendored by the reference).
 * NEAREST is what libheif 1.14.0 -- the version the reference pins (3rd-party/README.md:44) -- does when it converts the plug-in's
 * interleaved RGB(A) / RRGGBB(AA)_LE hand-off itself (heif_colorconversion.cc: Op_RGB24_32_to_YCbCr, Op_RRGGBBxx_HDR_to_YCbCr420,
 * Op_RGB_to_YCbCr<>: the chroma loops step by the sub-sampling factors and read the block's top-left pixel); the FormatRecord shim
 * (avifgpu_host.h) uses it by default.  AVERAGE is the box filter later libheif versions (>= 1.16, heif_chroma_downsampling_average)
 * default to; it is kept as an option and for comparison. */
enum {
    AVIFGPU_DOWNSAMPLE_AVERAGE = 0,  /* box average of the 2x1 / 2x2 footprint, edge-replicated */
    AVIFGPU_DOWNSAMPLE_NEAREST = 1   /* top-left (co-sited) sample: libheif 1.14.0's own behaviour */
};

/* Zero point of the full-range chroma codes written by the fused path.
 *   LIBHEIF : Cb' = round(Cb + 2^(bits-1))      -- what libheif's encoder-side conversion emits (drop-in default)
 *   DECODER : Cb' = round(Cb + (2^bits-1)/2)    -- exact inverse of the plug-in's own decoder tables
 *                                                  (T_UV[i] = i/max - 0.5, YuvLookupTables.cpp:182); round trip <= 1 code */
enum {
    AVIFGPU_CHROMA_ZERO_LIBHEIF = 0,
    AVIFGPU_CHROMA_ZERO_DECODER = 1
};

/* How LinearToPQ (ColorTransfer.cpp:69-92) is evaluated -- tier 2 either way (|delta code| <= 1 against the reference's powf): what
 * differs is the share of codes that are EXACTLY the reference's, and the cost (900 k-sample sweep at 80 nits):
 *   COMPACT  5 transcendentals + 6 packed operations per sample:                         99.94 % exact at 10 bit, 99.77 % at 12 bit
 *   CLOSE    + 3 plain, + 1 packed issue slots: the exponent's share of t^m1 from LDS
 *            tables indexed by the exponent field (exact m1 * E, round-to-nearest split): 99.99 % exact at 10 bit, 99.96 % at 12 bit
 * AUTO = CLOSE at every depth and in every kernel since ABI 4 (round 3's AUTO took its much costlier CLOSE for 12-bit output only).
 * Meaningful for PQ saves of 32-bit documents; ignored (not even range-checked) everywhere else.  Sampled-curve ICC documents take it
 * too.  COMPACT is there for callers who want the earlier arithmetic (byte-exact goldens of an older build). */
enum {
    AVIFGPU_PQ_AUTO    = 0,
    AVIFGPU_PQ_COMPACT = 1,
    AVIFGPU_PQ_CLOSE   = 2
};

enum {
    AVIFGPU_MEM_HOST   = 0,
    AVIFGPU_MEM_DEVICE = 1
};

/* ---- descriptors ---------------------------------------------------------------------------- */

/*
 * Write direction: FormatRecord rows -> heif_image planes.
 * Mirrors the arguments of CreateHeifImage*(formatRecord, alphaState, imageSize, saveOptions)
 * (reference WriteHeifImage.h:29-63) reduced to the fields the pixel loops read.
 */
typedef struct avifgpu_write_desc {
    int32_t width;               /* imageSize.h */
    int32_t height;              /* imageSize.v */
    int32_t depth;               /* formatRecord->depth: 8, 16 (0..32768), 32 (float).  Samples outside that are DEFINED (the reference's
                                  * behaviour is not): a 16-bit sample above 32768 -- alpha included -- counts as 32768, in front of
                                  * the ICC stage as well; a 32-bit NaN saves as code 0, +-Inf as code 0 or the maximum code. */
    int32_t planes;              /* formatRecord->planes: 1|2 gray(+A), 3|4 RGB(+A); alpha last */
    int32_t bit_depth;           /* saveOptions.imageBitDepth as 8 | 10 | 12 */
    int32_t transfer;            /* saveOptions.hdrTransferFunction (depth 32 only), AVIFGPU_TRANSFER_* */
    int32_t peak_nits;           /* saveOptions.pq.nominalPeakBrightness (1..10000) */
    int32_t alpha_state;         /* AVIFGPU_ALPHA_* ; must agree with planes */
    int32_t output;              /* AVIFGPU_OUT_* */
    /* ---- stage B (AVIFGPU_OUT_YCBCR only) ---- */
    int32_t chroma;              /* AVIFGPU_CHROMA_420|422|444 ("chroma" encoder parameter, Write.cpp:100-120) */
    int32_t matrix_coefficients; /* nclx matrix the plug-in selects, WriteMetadata.cpp:113-146 */
    int32_t color_primaries;     /* only consulted for AVIFGPU_MATRIX_CHROMA_DERIVED_NCL */
    int32_t full_range;          /* reference always writes 1 (WriteMetadata.cpp:46); 0 is rejected */
    int32_t chroma_downsampling; /* AVIFGPU_DOWNSAMPLE_* */
    int32_t chroma_zero_point;   /* AVIFGPU_CHROMA_ZERO_* */
    int32_t pq_evaluation;       /* AVIFGPU_PQ_* (transfer PQ only); 0 = the default */
} avifgpu_write_desc;

/*
 * Read direction: heif_image planes -> FormatRecord rows.
 * Mirrors ReadHeifImage*(image, alphaState, nclxProfile, [loadOptions,] formatRecord)
 * (reference ReadHeifImage.h:27-63).
 */
typedef struct avifgpu_read_desc {
    int32_t width;
    int32_t height;
    int32_t colorspace;          /* heif_image_get_colorspace: AVIFGPU_COLORSPACE_* */
    int32_t chroma;              /* heif_image_get_chroma_format: AVIFGPU_CHROMA_* (YCbCr only) */
    int32_t bit_depth;           /* heif_image_get_bits_per_pixel_range(Y or R): 8 | 10 | 12 | 16.  A 10- / 12-bit sample above
                                  * 2^bit_depth - 1 in its 16-bit container is DEFINED: planar RGB (and its alpha) opened at depth 16
                                  * keeps the low bit_depth bits (mask), opened at depth 32 counts as 2^bit_depth - 1 (clamp); YCbCr
                                  * and monochrome planes and their alpha clamp at every depth. */
    int32_t depth;               /* host depth the driver chose (Read.cpp:359-515): 8 | 16 | 32 */
    int32_t alpha_state;         /* AVIFGPU_ALPHA_* (Read.cpp:155-172) */
    int32_t has_nclx;            /* 0 => nclxProfile == nullptr (BT.601, full range defaults) */
    int32_t color_primaries;
    int32_t transfer_characteristics;
    int32_t matrix_coefficients;
    int32_t full_range_flag;
    /* LoadUIOptions (reference AvifFormat.h:61-85) */
    int32_t pq_peak_nits;        /* loadOptions.pq.nominalPeakBrightness */
    int32_t hlg_apply_ootf;      /* loadOptions.hlg.applyOOTF */
    float   hlg_display_gamma;   /* loadOptions.hlg.displayGamma */
    int32_t hlg_peak_nits;       /* loadOptions.hlg.nominalPeakBrightness */
    int32_t reserved[2];
} avifgpu_read_desc;

/* ---- entry points --------------------------------------------------------------------------- */

/* ABI version of the loaded library (== AVIFGPU_ABI_VERSION of the header it was built from). */
int32_t avifgpu_abi_version(void);

/* Bind the calling process to one HIP device: avifgpu_init_devices(&device_index, 1).
 * Fails with AVIFGPU_formatBadParameters if no HIP device is present: there is NO CPU fallback. */
int32_t avifgpu_init(int32_t device_index);

/* Bind `count` device contexts (the GPUs of the node: {0,1,...,7}).  Host-pointer conversions -- avifgpu_write_rows /
 * avifgpu_read_rows with AVIFGPU_MEM_HOST and the FormatRecord shim of avifgpu_host.h -- are then cut into contiguous even-row
 * tiles, one per context (tile k = rows [k*H/N, (k+1)*H/N) rounded to even: no 2x2 chroma block straddles a tile, no tile
 * depends on another, no device-to-device traffic), each streamed through its GPU in sub-tiles with copies and kernels
 * overlapped; the planes are gathered in place at plane + row * stride.  The result is byte-identical for every N.
 * Everything is driven from the calling thread (the plug-in is called serially on Photoshop's main thread,
 * AvifFormat.cpp:104-199); each context owns one internal worker thread that feeds its device.  An ordinal may appear more
 * than once (N contexts on one GPU: how the scheduler is tested on a single-GPU machine).  Re-binding a different list
 * releases the previous contexts first.  Replaces the single-threaded row loops WriteHeifImage.cpp:1017-1029 /
 * ReadHeifImage.cpp:141-160 as the unit of parallelism. */
int32_t avifgpu_init_devices(const int32_t* device_indices, int32_t count);
int32_t avifgpu_device_count(void);            /* contexts currently bound (0 before avifgpu_init*) */
void    avifgpu_shutdown(void);

/* Where bound device `index` (0 .. distinct devices of the binding - 1) sits in the host: SURVEY.md 8(e), "report which GPUs hang
 * off which root complex".  avifgpu_init_devices reads each device's PCI bus id (hipDeviceGetPCIBusId) and, from sysfs,
 * /sys/bus/pci/devices/<bdf>/numa_node and that node's CPU list; the device's worker threads pin themselves to those CPUs
 * (AVIFGPU_PIN_WORKERS=0 turns that off), and they -- not the calling thread -- allocate the context's pinned staging and tile
 * buffers, so the pages are first touched and page-locked on the socket the GPU's x16 link is attached to.  On an 8-GPU MI355X
 * node (4 GPUs per socket) that keeps every H2D / D2H stream off the inter-socket fabric.  numa_node is -1 and cpulist empty when
 * the host does not say (single-node machines, containers without sysfs): nothing is pinned then.
 * AVIFGPU_formatBadParameters for an index outside the binding. */
typedef struct avifgpu_device_info {
    int32_t device;              /* HIP ordinal */
    int32_t numa_node;           /* -1 = unknown */
    int32_t workers;             /* worker threads (lanes) feeding this device */
    int32_t workers_pinned;      /* 1 = their CPU affinity is `cpulist` */
    char    pci_bus_id[32];      /* "0000:c1:00.0" */
    char    cpulist[256];        /* "0-63,128-191" */
} avifgpu_device_info;
int32_t avifgpu_device_topology(int32_t index, avifgpu_device_info* out);

/* What bound device `index` (same numbering as avifgpu_device_topology) has carried over its own link since the binding or the last
 * reset: tiles issued, payload bytes host -> device and device -> host, and how many of those bytes went through a pinned bounce
 * buffer because the caller's memory was pageable.  With the wall time of a job this is the per-device H2D / D2H rate -- on an
 * 8-GPU node the first thing to look at is whether the eight x16 links add up (bench.py pcie_inclusive.per_device).
 * copy_helper_pools = helper-thread pools alive for pageable copies: one per NUMA node that has needed one. */
typedef struct avifgpu_device_traffic {
    int32_t  device;             /* HIP ordinal */
    int32_t  copy_helper_pools;
    uint64_t tiles;
    uint64_t bytes_h2d;
    uint64_t bytes_d2h;
    uint64_t bytes_bounced;
} avifgpu_device_traffic;
int32_t avifgpu_device_traffic_get(int32_t index, avifgpu_device_traffic* out);
int32_t avifgpu_device_traffic_reset(void);    /* all bound devices */

/* The sysfs part of the above on its own (no device needed): NUMA node and CPU list of PCI device `pci_bus_id` under
 * `sysfs_root` (NULL = "/sys").  Returns the number of CPUs in the list (0 = none known), AVIFGPU_readErr when the tree has no
 * such device or the list does not parse, AVIFGPU_formatBadParameters for a null bus id. */
int32_t avifgpu_topology_probe(const char* sysfs_root, const char* pci_bus_id, int32_t* numa_node, char* cpulist, int32_t cpulist_len);

/* The placement avifgpu_init_devices would give these PCI devices, computed from sysfs alone (no device needed): out[i] = NUMA node,
 * CPU list, workers (AVIFGPU_LANES) and whether they would be pinned, for pci_bus_ids[i].  Returns the number of NUMA domains the
 * binding spans -- each gets its own pool of helper threads for pageable copies and first-touches its own pinned staging -- or a
 * negative AVIFGPU_* code.  On an 8-GPU MI355X node: 2 domains, four devices (= four worker sets) each. */
int32_t avifgpu_topology_plan(const char* sysfs_root, const char* const* pci_bus_ids, int32_t count, avifgpu_device_info* out);

/* Message for the last non-zero return on this thread (what LibHeifException / runtime_error carry
 * in the reference, UIWin.cpp:1827-1843). */
const char* avifgpu_last_error(void);

/*
 * Convert rows [row0, row0 + nrows) of the image described by `desc`.
 *
 *   src            first byte of source row `row0` (interleaved, planes * depth/8 bytes per pixel,
 *                  exactly the layout advanceState() leaves in formatRecord->data, Write.cpp:279-299)
 *   src_row_bytes  distance between source rows (formatRecord->rowBytes)
 *   dst[i]         first byte of destination plane i at row `row0` (chroma planes: row row0 >> yShift)
 *   dst_stride[i]  libheif's stride for that plane (heif_image_get_plane, WriteHeifImage.cpp:646)
 *
 * row0 must be even for 4:2:0; nrows may be odd only for the tile that ends at `height`.
 * Replaces the row loops WriteHeifImage.cpp:208-263,...,1017-1135.
 */
int32_t avifgpu_write_rows(const avifgpu_write_desc* desc,
                           int32_t row0, int32_t nrows,
                           const void* src, int64_t src_row_bytes,
                           void* const dst[4], const int64_t dst_stride[4],
                           int32_t mem_kind, void* stream);

/* ---- content light level of an HDR save (clli: MaxCLL / MaxFALL, CTA-861.3 Annex P) ----------------------------------------------
 * An extension: the reference does not compute it.  The statistic is a histogram of the brightest stage-A code of each pixel --
 * m = max(R, G, B) (gray: Y) of the integer codes the 32-bit write loops hand to libheif (after the ICC row transform, the alpha
 * clamp and the optional premultiply, before any YCbCr step; alpha codes are not counted), count[m] += 1 -- taken by a kernel of
 * its own behind the conversion of the same rows.  Integer counts add in any order: the result is the same for every tiling, every
 * number of bound devices and every launch shape.
 *
 * Arm (bins != NULL) or disarm (NULL) the calling thread's code histogram.  While armed, every avifgpu_write_rows* call of this
 * thread on a depth-32 descriptor adds its rows' pixels to bins[0 .. (1 << bit_depth) - 1] (bit_depth 10 or 12, anything else is
 * formatBadParameters here); calls at depth 8 / 16 and every read are unaffected and do not touch it.  The FormatRecord shim's
 * saves (avifgpu_host.h) run on the caller's thread and honour it with mem_kind HOST, all tiles of a save summed.  The library
 * never zeroes the bins.  mem_kind says where bins live and must equal the mem_kind of the calls: HOST -- the counts are complete
 * when each call returns (a call that fails adds nothing); DEVICE -- the adds are enqueued on the call's stream behind its kernel.
 * A call whose desc->bit_depth differs from the armed one, or whose mem_kind differs, fails with formatBadParameters before
 * anything is launched.  Host-only bookkeeping: needs no device. */
int32_t avifgpu_histogram_attach(uint64_t* bins, int32_t bit_depth, int32_t mem_kind);

typedef struct avifgpu_content_light_level {
    uint16_t max_cll, max_fall;       /* the clli fields: min(65535, floor(nits + 0.5)) */
    int32_t  max_code;                /* c_p: the smallest code with sum_{k <= c_p} count[k] >= ceil(percentile * pixels) */
    uint64_t pixels;                  /* n = sum of the bins */
    double   max_cll_nits, max_fall_nits;
} avifgpu_content_light_level;

/* Host only, float64.  For PQ at bit depth b code c stands for L(c) = 10000 * EOTF_PQ(c / (2^b - 1)) cd/m2 (SMPTE ST 2084 with its
 * exact rational constants; the codes in the file are absolute, peak_nits plays no part).  max_cll_nits = L(c_p); max_fall_nits =
 * (sum_c count[c] L(c)) / n, summed in ascending code order.  percentile in (0, 1]; 1 gives the highest non-empty bin.  Any other
 * transfer, an empty histogram, a bit depth other than 10 or 12 or a percentile outside (0, 1] is formatBadParameters. */
int32_t avifgpu_light_level_from_histogram(const uint64_t* bins, int32_t bit_depth, int32_t transfer, double percentile,
                                           avifgpu_content_light_level* out);

/* Measuring aid (tools/bench_light_level.py): launch the histogram kernel of `desc` (depth 32) ALONE on the whole frame at device pointer
 * `src`, into device bins, on `stream`.  twin 0 = the kernel itself (the same counts an armed avifgpu_write_rows adds); 1 / 2 = its
 * atomics-free / math-free twin for attribution (RGB, PQ, no profile, 16-byte aligned rows; the counts they leave are meaningless). */
int32_t avifgpu_probe_histogram(const avifgpu_write_desc* desc, int32_t twin, const void* src, int64_t src_row_bytes, uint64_t* bins, void* stream);

/* ---- thumbnail of a save: box average of the output codes ----------------------------------------------------------------------
 * An extension: the reference declares fmtCannotCreateThumbnail and writes no thumbnail.  The statistic is taken from the OUTPUT of a
 * save -- the planes the conversion kernel has just written -- by a kernel of its own behind the conversion of the same rows, so it
 * is the same for every document depth, transfer, profile and output form, and the thumbnail is in exactly the colour representation
 * of the main image.  Every CHANNEL of the output is reduced on its own: a channel is one plane of pw x ph samples, or one of the
 * `planes` interleaved channels of plane 0 of a colour save in AVIFGPU_OUT_REFERENCE form; 4:2:x chroma planes are reduced from their
 * own (W + xs) >> xs by (H + ys) >> ys.  Sample (x, y) of a channel belongs to cell (floor(x tw / pw), floor(y th / ph)), and
 *     sums[(ty * tw + tx) * C + c] += code,      C = desc->planes, c in output order R,G,B[,A] | Y[,A] | Y,Cb,Cr[,A].
 * Integer sums add in any order: they are the same for every tiling, every number of bound devices, every launch shape, pinned or
 * pageable memory, HOST or DEVICE pointers.  Alpha is averaged like any channel and colour is the plain mean of the codes: right for
 * premultiplied saves, and for straight alpha what every plain scaler does.  ALPHA-WEIGHTED COLOUR MEANS ARE NOT COMPUTED.
 *
 * Arm (sums != NULL) or disarm (NULL: always succeeds) the calling thread.  1 <= tw, th <= 1024, else formatBadParameters.  sums holds
 * tw * th * planes counters (4 * tw * th is always enough) and is never zeroed by the library.  While armed, every avifgpu_write_rows*
 * call of this thread, at any depth, adds its rows' output codes; reads are unaffected.  The FormatRecord shim's saves run on the
 * caller's thread and honour it with mem_kind HOST, all tiles of a save summed.  mem_kind says where sums live and must equal the
 * mem_kind of the calls: HOST -- the sums are complete when each call returns (a call that fails adds nothing); DEVICE -- the adds are
 * enqueued on the call's stream behind its kernel, they read the caller's dst planes.  A call whose mem_kind differs, or whose
 * smallest used plane is narrower than tw or lower than th, fails with formatBadParameters before anything is launched or queued.  A
 * code histogram may be armed at the same time.  Host-only bookkeeping: needs no device. */
int32_t avifgpu_thumbnail_attach(uint64_t* sums, int32_t tw, int32_t th, int32_t mem_kind);

/* Host only.  The size an aspect-preserving fit of the image into a bbox x bbox square gives: the image's own size when
 * max(W, H) <= bbox; otherwise the longer side becomes bbox and the other max(1, (2 other bbox + longer) / (2 longer)).  Both are then
 * clamped to the smallest used plane's width and height (so that avifgpu_thumbnail_attach + the save accept them) and to 1024.
 * bbox < 1, a null argument or an invalid desc is formatBadParameters. */
int32_t avifgpu_thumbnail_fit(const avifgpu_write_desc* desc, int32_t bbox, int32_t* tw, int32_t* th);

/* Host only, integer arithmetic.  The thumbnail code of a cell is floor((2 sum + n) / (2 n)), n = the cell's sample count in that plane,
 * taken from the geometry: n = (ceil((tx + 1) pw / tw) - ceil(tx pw / tw)) * (the same in y).  Written in the form of the main output at
 * tw x th: plane 0 interleaved for a colour REFERENCE save; Y (+ plane 3 = A) for gray; Y, Cb, Cr (+ A) planes, always 4:4:4, for YCBCR
 * output.  Samples are u8 at bit depth 8, little-endian u16 otherwise; dst_stride in bytes.  formatBadParameters when a sum exceeds
 * n * (2^bit_depth - 1) -- the caller did not feed a whole frame exactly once -- and then nothing is written. */
int32_t avifgpu_thumbnail_from_sums(const avifgpu_write_desc* desc, int32_t tw, int32_t th, const uint64_t* sums,
                                    void* const dst[4], const int64_t dst_stride[4]);

/* Measuring aid (tools/bench_thumbnail.py): launch the thumbnail kernel ALONE on the whole frame's output planes at device pointers
 * `planes` (as avifgpu_write_rows wrote them: the same plane use, strides in bytes), into device sums, on `stream`.  twin 0 = the kernel
 * itself (the same sums an armed avifgpu_write_rows adds); 1 = its atomics-free twin for attribution (the loads and the register adds
 * only: sums is left alone). */
int32_t avifgpu_probe_thumbnail(const avifgpu_write_desc* desc, int32_t twin, int32_t tw, int32_t th, const void* const planes[4],
                                const int64_t stride[4], uint64_t* sums, void* stream);

/* ---- summary of a save: the range of every written channel, and whether R, G and B ever differ ---------------------------------
 * An extension: what an adapter wants to know before it hands the planes to the encoder -- does the alpha plane say anything, does the
 * chroma?  Taken from the OUTPUT of a save like the thumbnail, by a kernel of its own behind the conversion of the same rows.  Channels
 * are in the thumbnail's order, R,G,B[,A] | Y[,A] | Y,Cb,Cr[,A], C = desc->planes.  The counters, 32-bit unsigned:
 *     counters[0 + c] = hi[c]     = max(code)             of channel c
 *     counters[4 + c] = lo_inv[c] = max(65535 - code)     so that the smallest code is 65535 - lo_inv[c]
 *     counters[8]     = spread    = max over pixels of max(R,G,B) - min(R,G,B)
 *     counters[9..15]             reserved, zero
 * The spread is defined for colour saves in AVIFGPU_OUT_REFERENCE form (from the interleaved pixel) and for AVIFGPU_OUT_YCBCR with
 * AVIFGPU_MATRIX_RGB_GBR (the three planes are copies of G, B, R at 4:4:4); it stays 0 everywhere else.
 * Every counter is a RUNNING MAXIMUM.  So an all-zero block (calloc, hipMemset 0) is the empty summary; two summaries merge by an
 * element-wise max; the result is the same for every tiling, every number of bound devices, every launch shape, pinned or pageable
 * memory, HOST or DEVICE pointers; feeding a row twice changes nothing -- and therefore A PARTIAL FEED CANNOT BE DETECTED: the facts
 * hold for the rows that were fed.  A channel that was fed has lo_inv > 0 (codes are at most 4095).
 *
 * Arm (counters != NULL) or disarm (NULL: always succeeds) the calling thread.  counters holds AVIFGPU_SUMMARY_COUNTERS words and is
 * never cleared by the library.  While armed, every avifgpu_write_rows* call of this thread, at any depth, folds its rows' output codes
 * in; reads are unaffected.  The FormatRecord shim's saves run on the caller's thread and honour it with mem_kind HOST.  mem_kind says
 * where the counters live and must equal the mem_kind of the calls: HOST -- the counters are complete when each call returns (a call that
 * fails adds nothing); DEVICE -- the kernel is enqueued on the call's stream behind the conversion, it reads the caller's dst planes
 * and raises the caller's device counters.  A call whose mem_kind differs fails with formatBadParameters before anything is launched or
 * queued.  A code histogram and a thumbnail may be armed at the same time.  Host-only bookkeeping: needs no device. */
enum { AVIFGPU_SUMMARY_COUNTERS = 16 };
int32_t avifgpu_summary_attach(uint32_t* counters, int32_t mem_kind);

enum {
    AVIFGPU_ADVICE_DROP_ALPHA = 1,   /* every alpha code is the maximum: the alpha item says nothing */
    AVIFGPU_ADVICE_MONOCHROME = 2    /* a colour save whose content is neutral: it can be encoded without chroma */
};
typedef struct avifgpu_save_summary {
    int32_t channels;         /* desc->planes */
    int32_t min_code[4];
    int32_t max_code[4];
    int32_t spread;           /* -1: not applicable */
    int32_t alpha_opaque;     /* 1: the smallest alpha code is 2^bit_depth - 1; -1: no alpha */
    int32_t alpha_clear;      /* 1: every alpha code is 0; -1: no alpha */
    int32_t neutral;          /* 0 | 1 */
    int32_t advice;           /* AVIFGPU_ADVICE_* bits */
} avifgpu_save_summary;

/* Host only, integer arithmetic.  neutral: gray saves 1; REFERENCE colour and G,B,R planes spread == 0; YCBCR with
 * AVIFGPU_CHROMA_ZERO_LIBHEIF min == max == 1 << (bit_depth - 1) on both chroma planes (R = G = B gives exactly that code); YCBCR with
 * AVIFGPU_CHROMA_ZERO_DECODER both chroma planes within [2^(bit_depth-1) - 1, 2^(bit_depth-1)] -- that zero point is the half-integer
 * (2^bit_depth - 1) / 2, R = G = B lands on either neighbour, so this rule says NEUTRAL TO WITHIN THE QUANTISER, not exactly grey.
 * advice: DROP_ALPHA when alpha_opaque, MONOCHROME when a colour save is neutral.  formatBadParameters when a channel of the descriptor
 * was never fed (lo_inv 0), or when a maximum exceeds 2^bit_depth - 1 (the counters are not of this descriptor); out is then untouched. */
int32_t avifgpu_summary_read(const avifgpu_write_desc* desc, const uint32_t* counters, avifgpu_save_summary* out);

/* Host only.  into[k] = max(into[k], from[k]) over the AVIFGPU_SUMMARY_COUNTERS words: for ranks and threads that saved row tiles of
 * one image. */
int32_t avifgpu_summary_merge(uint32_t* into, const uint32_t* from);

/* Measuring aid (tools/bench_summary.py): launch the summary kernel ALONE on the whole frame's output planes at device pointers
 * `planes` (as avifgpu_write_rows wrote them: the same plane use, strides in bytes), into device counters, on `stream`.  twin 0 = the
 * kernel itself (the same counters an armed avifgpu_write_rows leaves); 1 = its atomics-free twin for attribution (the loads and the
 * register work only: counters is left alone). */
int32_t avifgpu_probe_summary(const avifgpu_write_desc* desc, int32_t twin, const void* const planes[4], const int64_t stride[4],
                              uint32_t* counters, void* stream);

/*
 * Inverse direction.  src[i] / src_stride[i] are what heif_image_get_plane_readonly returns
 * (ReadHeifImage.cpp:104-111) advanced to row `row0` (chroma: row0 >> yShift); plane order is
 * Y,Cb,Cr,Alpha / R,G,B,Alpha / Y,-,-,Alpha.  dst receives interleaved host rows
 * (formatRecord->data layout, ReadHeifImage.cpp:31-50).  Replaces ReadHeifImage.cpp:141-181 etc.
 */
int32_t avifgpu_read_rows(const avifgpu_read_desc* desc,
                          int32_t row0, int32_t nrows,
                          const void* const src[4], const int64_t src_stride[4],
                          void* dst, int64_t dst_row_bytes,
                          int32_t mem_kind, void* stream);

/* ---- ICC row transform of the HDR save path ---------------------------------------------------
 * The reference converts every 32-bit row to linear Rec.2020 with lcms2 before the pixel loop when the document
 * carries a non-Rec.2020 profile (ColorProfileConversion::ConvertRow, src/common/ColorProfileConversion.cpp:159-187,
 * transform built at :235-266 against CreateRec2020LinearRGBProfile, ColorProfileGeneration.cpp:141-178).  For
 * matrix/TRC RGB profiles that lcms2 pipeline is [per-channel TRC] -> [one 3x3 matrix in double] -> float, which the
 * write kernels can apply in place of the CPU call.  (Tier 2, like every float path: the kernels evaluate the curves and --
 * on the streaming kernels -- the matrix in single precision; the bar is on the integer codes behind the transfer curve,
 * |delta code| <= 1 and >= 99 % exact against the real lcms2, measured 99.7-100 %: tests/test_gpu_icc.py.)  Sampled `curv` tables
 * are not parametric: avifgpu_icc_prepare returns AVIFGPU_formatCannotRead for them and avifgpu_icc_prepare_sampled (below) takes
 * them; LUT-based profiles (A2B tags) are covered by neither: the adapter captures lcms2's own stage program for them
 * (avifgpu_icc_pipeline32 below) or keeps its lcms2 path. */
typedef struct avifgpu_icc_transform {
    int32_t trc_type[3];         /* lcms2 parametric curve type 1..5 per channel (1 = plain gamma; gamma 1 = linear) */
    int32_t out_curve;           /* 0 = none (linear destination); 4 = inverse of lcms2 parametric type 4 (sRGB) after the matrix */
    double  trc_params[3][7];    /* g, a, b, c, d, e, f as lcms2 orders them */
    double  matrix[9];           /* row-major: out_i = (float) sum_j matrix[3i+j] * (double) trc_j(in_j) */
    double  out_params[8];       /* out_curve == 4: g, a, b, c, d of the forward curve, then the break point
                                    pow(a*d + b, g) and 1/g, 0 */
} avifgpu_icc_transform;

/* REC2020_LINEAR: HDR saves (transfer PQ / SMPTE 428), ColorProfileConversion.cpp:235-266.
 * SRGB_FLOAT: 32-bit documents saved as SDR (transfer Clip) are converted to sRGB whenever keepColorProfile is off -- even
 * from an sRGB profile, "because the 32-bit mode uses linear gamma" (ColorProfileConversion.cpp:105,:118-123, :268-331 with
 * TYPE_RGB[A]_FLT; with keepColorProfile on, NO transform is installed): lcms2's float pipeline is then
 * [TRC] -> [3x3 in double] -> [inverse sRGB parametric curve in double] -> float. */
enum { AVIFGPU_ICC_TARGET_REC2020_LINEAR = 0, AVIFGPU_ICC_TARGET_SRGB_FLOAT = 2 };

/* Parse the document's ICC profile bytes (formatRecord->iCCprofileData) and build the transform to `target`. */
int32_t avifgpu_icc_prepare(const void* icc_profile, uint32_t size, int32_t target, avifgpu_icc_transform* out);

/* avifgpu_write_rows with the ICC transform applied to every pixel's R,G,B first (alpha is copied, as
 * cmsFLAGS_COPY_ALPHA does).  depth must be 32 and planes 3 or 4.  icc == NULL behaves like avifgpu_write_rows. */
int32_t avifgpu_write_rows_icc(const avifgpu_write_desc* desc, const avifgpu_icc_transform* icc,
                               int32_t row0, int32_t nrows,
                               const void* src, int64_t src_row_bytes,
                               void* const dst[4], const int64_t dst_stride[4],
                               int32_t mem_kind, void* stream);

/* ---- ... for 32-bit documents whose profile carries SAMPLED curves (`curv` tables) ------------------------------------------------
 * lcms2's float pipeline does not interpolate such a curve in floating point: cmsEvalToneCurveFloat saturates the sample to a 16-bit
 * word (_cmsQuickSaturateWord(v * 65535.0)), interpolates the table in 16-bit fixed point (cmsEvalToneCurve16 = LinLerp1D) and
 * divides back by 65535 -- so per channel the curve stage is a function of a 16-bit index.  avifgpu_icc_prepare_sampled tabulates
 * it (65536 floats per channel, the library's arithmetic restated on the host: csrc/icc_profile.cpp), the kernel computes the same
 * index and looks the float up (or interpolates the profile's own table in LDS: the same value); matrix and, for the sRGB target, the inverse curve follow as in avifgpu_icc_transform.
 * At least one channel must be sampled; a profile that MIXES sampled and parametric channels is taken too (parametric_mask: those
 * channels are evaluated on the unquantised sample like avifgpu_icc_transform's, as lcms2 does channel by channel in its curves
 * stage).  All-parametric profiles take avifgpu_icc_prepare; LUT-based / A2B profiles still return AVIFGPU_formatCannotRead (the
 * caller keeps lcms2).  792 KiB: allocate it once per save. */
enum { AVIFGPU_ICC_SAMPLED_MAX = 4096 };
typedef struct avifgpu_icc_sampled32 {
    avifgpu_icc_transform base;  /* matrix, out_curve, out_params as above; trc_type[c] = 0 for a sampled channel */
    float curve[3][65536];       /* curve[c][_cmsQuickSaturateWord(v * 65535.0)] = what lcms2's curve stage hands to the matrix for sample v */
    /* The profile's own tables, when none has more than AVIFGPU_ICC_SAMPLED_MAX entries (entries[] = 0 otherwise): the kernel then keeps
     * them in LDS and performs LinLerp1D itself -- the same words, the same floats as curve[], without a scattered memory load per sample. */
    uint16_t table16[3][AVIFGPU_ICC_SAMPLED_MAX];
    int32_t  entries[3];
    int32_t  parametric_mask;    /* bit c: channel c of a MIXED profile is parametric (base.trc_type[c] / trc_params[c] hold it, curve[c] is unused,
                                  * entries[c] = 0); 0 for a profile whose three curves are all sampled.  Never 7. */
} avifgpu_icc_sampled32;
int32_t avifgpu_icc_prepare_sampled(const void* icc_profile, uint32_t size, int32_t target, avifgpu_icc_sampled32* out);
int32_t avifgpu_write_rows_icc_sampled(const avifgpu_write_desc* desc, const avifgpu_icc_sampled32* icc,
                                       int32_t row0, int32_t nrows,
                                       const void* src, int64_t src_row_bytes,
                                       void* const dst[4], const int64_t dst_stride[4],
                                       int32_t mem_kind, void* stream);

/* Which working space the document profile already is: the checks that decide whether the reference installs a transform
 * at all -- IsRec2020ColorProfile / IsSRGBColorProfile (src/common/ColorProfileDetection.cpp:331-374): the cicp tag when
 * present, else a description prefix ("Rec2020-elle-V", "Colorist BT. 2020", "ITU-R BT. 2020 Reference Display" / "sRGB"),
 * else colorants + media white point within 0.01 in xy after un-adapting from D50 (V2 display profiles count as D50, as
 * the reference does).  Returns a bit mask of AVIFGPU_ICC_IS_*, or a negative OSErr for a buffer that is not a profile. */
enum { AVIFGPU_ICC_IS_REC2020 = 1, AVIFGPU_ICC_IS_SRGB = 2 };
int32_t avifgpu_icc_detect(const void* icc_profile, uint32_t size);

/* ---- ICC row transform of the 8-bit SDR save path --------------------------------------------------------------------
 * With keepColorProfile == false (the default, AvifFormat.cpp:96) every 8-bit row of a non-sRGB document goes through
 * lcms2 to sRGB first (ColorProfileConversion.cpp:134-157, :268-331, TYPE_RGB[A]_8).  For a matrix/TRC profile lcms2
 * runs its 8-bit "matrix-shaper" fast path: 256-entry curve tables in 1.14 fixed point, a 1.14 fixed-point 3x3, a
 * 16385-entry output table -- pure integer arithmetic once the tables exist, reproduced here bit for bit
 * (tests/test_icc8.py: all 2^24 RGB inputs against the real library). */
typedef struct avifgpu_icc_shaper8 {
    int32_t  shaper1[3][256];    /* per channel: round(TRC(i/255) * 16384) */
    int32_t  matrix[3][3];       /* round(M * 16384) */
    int32_t  offset[3];
    int32_t  reserved;
    uint8_t  shaper2[3][16388];  /* per channel, index 0..16384: 8-bit output of the inverse destination curve */
} avifgpu_icc_shaper8;

enum { AVIFGPU_ICC_TARGET_SRGB8 = 1 };

/* Build the tables for document profile -> sRGB (the profile cmsCreate_sRGBProfile makes).  Matrix/TRC RGB profiles with
 * `para` curves, `curv` gammas or sampled `curv` tables (interpolated in 16-bit fixed point like cmsEvalToneCurve16);
 * AVIFGPU_formatCannotRead for anything else. */
int32_t avifgpu_icc_prepare_shaper8(const void* icc_profile, uint32_t size, avifgpu_icc_shaper8* out);

/* avifgpu_write_rows for 8-bit RGB(A) documents with that transform applied to R,G,B first (alpha copied). */
int32_t avifgpu_write_rows_icc8(const avifgpu_write_desc* desc, const avifgpu_icc_shaper8* icc,
                                int32_t row0, int32_t nrows,
                                const void* src, int64_t src_row_bytes,
                                void* const dst[4], const int64_t dst_stride[4],
                                int32_t mem_kind, void* stream);

/* (kr, kg, kb) exactly as GetYUVCoefficiants derives them (reference YUVCoefficiants.cpp:154-188).
 * has_nclx == 0 => BT.601 default. */
int32_t avifgpu_get_yuv_coefficients(int32_t has_nclx, int32_t matrix_coefficients,
                                     int32_t color_primaries, float out_kr_kg_kb[3]);

/* Value formatRecord->maxValue must be set to for a 16-bit read (ReadHeifImage.cpp:206,499,747):
 * 32768 for YCbCr / gray, 2^bits-1 for planar RGB (host rescales). */
int32_t avifgpu_read_max_value(const avifgpu_read_desc* desc);

/* Geometry helpers shared by host shim, tests and bench. */
int32_t avifgpu_write_plane_count(const avifgpu_write_desc* desc);              /* planes written   */
int32_t avifgpu_write_plane_geometry(const avifgpu_write_desc* desc, int32_t plane,
                                     int32_t* width, int32_t* height,
                                     int32_t* bytes_per_sample, int32_t* samples_per_pixel);
int64_t avifgpu_write_algorithmic_bytes(const avifgpu_write_desc* desc, int32_t nrows); /* in + out */
int64_t avifgpu_read_algorithmic_bytes(const avifgpu_read_desc* desc, int32_t nrows);

/* Tuning hook for benchmarks and tests (not part of the reference mapping): the low byte selects the implementation variant of the
 * dominant kernel and a few A/B switches; bits 8.. , when not zero, are a number of workgroups no capped launch of the library exceeds
 * (write, read and histogram kernels alike) -- it can only lower a grid, so that every wave walks several trips of its grid-stride loop
 * on a small tile, and avifgpu_last_kernel_name() then carries " cap=N/M" (N workgroups launched, M for one trip per wave).  See
 * avif-format_amd/csrc/kernel_params.h.  Results are byte-identical for every value (with an ICC transform of
 * a 32-bit document: identical within tier 2 -- the streaming kernels run the 3x3 in single precision). */
void avifgpu_set_hot_variant(int32_t variant);

/* Measurement hook (not part of the reference mapping): launches the MATH-FREE twin of the dominant kernel -- the memory accesses
 * of RGB f32 -> Y, Cb, Cr u16 4:4:4 (six coalesced non-temporal 16-byte loads and three non-temporal 16-byte plane stores per lane,
 * one 512-pixel span per wave) with no conversion -- on device pointers, on `stream`.  bench.py times it next to the real kernel:
 * what this box's memory system gives this access pattern is the measured ceiling `roofline.peak_measured`.  width % 512 == 0,
 * 16-byte aligned pointers and strides; the planes receive a checksum, not pixels. */
int32_t avifgpu_probe_pattern_rgb32_444(const void* src, int64_t src_row_bytes, void* const dst[3], const int64_t dst_stride[3],
                                        int32_t width, int32_t nrows, void* stream);
/* Launch shape of that probe (round 6; process-wide): workgroups of 4 / 2 / 1 waves, buffer (0) or 64-bit global (1) addressing, pacing 0. */
void avifgpu_probe_set_shape(int32_t waves, int32_t global_addressing, int32_t pace);
/* ... and of the READ kernels: the math-free twin of what avifgpu_read_rows(AVIFGPU_MEM_DEVICE) would launch for `desc` (same loads,
 * table copy, LDS transpose and stores; dst receives meaningless bytes).  4:2:x colour opens to 8-bit and f32 (PQ) hosts on 16-byte
 * aligned device buffers; AVIFGPU_formatBadParameters for anything else. */
int32_t avifgpu_probe_pattern_read(const avifgpu_read_desc* desc, int32_t row0, int32_t nrows, const void* const src[4], const int64_t src_stride[4],
                                   void* dst, int64_t dst_row_bytes, void* stream);

/* Name + last launch geometry of the kernel the previous *_rows call dispatched (for bench/profiles). */
const char* avifgpu_last_kernel_name(void);

/* ---- ICC row transform of the 16-bit SDR save path ------------------------------------------------------------------
 * 16-bit rows of a non-sRGB document go through lcms2 as TYPE_RGB[A]_16 between two range maps ([0, 32768] <-> [0, 65535],
 * ColorProfileConversion.cpp:37-95,:159-187,:268-331).  For 16-bit data lcms2 does not run the matrix/curve pipeline per
 * pixel: at transform creation it resamples it into a 33 x 33 x 33 table of 16-bit RGB nodes (float pipeline evaluated at
 * the nodes) and then interpolates that table tetrahedrally in 16.16 fixed point.  Both halves are reproduced: the table is
 * built on the host from the profile bytes, the interpolation (integer arithmetic) runs in the write kernel; the result is
 * bit-identical to lcms2 2.12 (tests/test_icc16.py). */
enum { AVIFGPU_ICC_CLUT_GRID = 33 };
typedef struct avifgpu_icc_clut16 {
    int32_t  grid_points;                                   /* 33 */
    int32_t  reserved[3];
    uint16_t table[AVIFGPU_ICC_CLUT_GRID * AVIFGPU_ICC_CLUT_GRID * AVIFGPU_ICC_CLUT_GRID][4];   /* [r][g][b] -> R, G, B, 0 */
} avifgpu_icc_clut16;

/* Build the table for document profile -> sRGB.  Matrix/TRC RGB profiles with `para` curves, `curv` gammas or sampled
 * `curv` tables (AVIFGPU_formatCannotRead otherwise: the caller keeps lcms2). */
int32_t avifgpu_icc_prepare_clut16(const void* icc_profile, uint32_t size, avifgpu_icc_clut16* out);

/* The same table for ANY profile -- LUT-based (A2B) ones included -- computed from transforms the CALLER owns.  For 16-bit formatters
 * lcms2 resamples every profile pair into a 33^3 table + tetrahedral interpolation when the transform is created (the reference's
 * flags, ColorProfileConversion.cpp:268-331), filling it from the linked float pipeline -- which is what a TYPE_RGB_FLT transform of
 * the same profiles, intent and flags evaluates.  The plug-in, which links lcms2, passes
 *   float_fn: cmsDoTransform on that float transform (interleaved RGB floats, 1.0 = white), used to compute the 35937 nodes the way
 *             lcms2 computes them, and
 *   word_fn:  cmsDoTransform on the TYPE_RGB_16 transform it would have used per row (interleaved RGB words in [0, 65535]), used to
 *             PROVE the table: 4096 probe colours must come out of the library's interpolation exactly as out of word_fn.
 * AVIFGPU_formatCannotRead (keep the CPU path) if they do not -- another CMM, cmsFLAGS_NOOPTIMIZE, another grid.  Host-only: no device
 * needed; both callbacks are called on the calling thread, before the function returns. */
typedef void (*avifgpu_transform_f32_fn)(void* user, const float* rgb_in, float* rgb_out, uint32_t pixel_count);
typedef void (*avifgpu_transform16_fn)(void* user, const uint16_t* rgb_in, uint16_t* rgb_out, uint32_t pixel_count);
int32_t avifgpu_icc_clut16_from_transforms(avifgpu_transform_f32_fn float_fn, avifgpu_transform16_fn word_fn, void* user,
                                           avifgpu_icc_clut16* out);

/* avifgpu_write_rows for 16-bit RGB(A) documents with that transform applied first; alpha takes the reference's
 * [0,32768] -> [0,65535] -> [0,32768] round trip (cmsFLAGS_COPY_ALPHA in between).
 * Lifetime of a prepared table (this one, avifgpu_icc_sampled32, the 8-bit table form): the library keeps a copy per device.  Within one
 * save -- calls that continue one another row for row on one thread: row0 of a call = the row after the previous call's last -- the table
 * must not change (a strided fingerprint is all that is compared).  Between saves it may be rewritten, freed or reallocated at the same
 * address: every call that does not continue the previous one (row 0, a gap, another order, another thread) re-verifies each device's
 * copy byte for byte before it is used. */
int32_t avifgpu_write_rows_icc16(const avifgpu_write_desc* desc, const avifgpu_icc_clut16* icc,
                                 int32_t row0, int32_t nrows,
                                 const void* src, int64_t src_row_bytes,
                                 void* const dst[4], const int64_t dst_stride[4],
                                 int32_t mem_kind, void* stream);

/* ---- ... and of the 8-bit SDR save path behind a LUT-based (A2B) document profile (round 6) --------------------------------
 * avifgpu_icc_prepare_shaper8 covers matrix/TRC profiles (lcms2's 8-bit matrix-shaper).  For every other profile pair lcms2 resamples the
 * pipeline into the SAME 33^3 table as for 16-bit formatters (OptimizeByResampling does not look at the formatters' depth) and evaluates it
 * for 8-bit rows with PrelinEval8: the byte b enters as the word 257 b, the tetrahedral sum and its rounding are TetrahedralInterp16's,
 * the output formatter packs the word with FROM_16_TO_8 -- integer arithmetic once the table exists, reproduced bit for bit
 * (tests/test_icc8.py: all 2^24 RGB triples against the real library).  As for 16-bit documents the table comes from transforms the
 * CALLER owns and is PROVEN before use:
 *   float_fn: cmsDoTransform on a TYPE_RGB_FLT transform of the same profiles, intent and flags (computes the 35937 nodes), and
 *   byte_fn:  cmsDoTransform on the TYPE_RGB_8 transform the plug-in would have run per row (ColorProfileConversion.cpp:268-331):
 *             16384 probe colours -- every neutral, words around the nodes, random triples -- must come out of the library's evaluation
 *             of the table exactly as out of byte_fn.
 * AVIFGPU_formatCannotRead (keep lcms2) if they do not: a matrix/TRC profile (lcms2 runs its matrix-shaper there -- use
 * avifgpu_icc_prepare_shaper8), another CMM, cmsFLAGS_NOOPTIMIZE.  Host-only; both callbacks run on the calling thread.
 * 32-bit documents behind such a profile do not resample: see avifgpu_icc_pipeline32 below. */
typedef void (*avifgpu_transform8_fn)(void* user, const uint8_t* rgb_in, uint8_t* rgb_out, uint32_t pixel_count);
int32_t avifgpu_icc_clut8_from_transforms(avifgpu_transform_f32_fn float_fn, avifgpu_transform8_fn byte_fn, void* user,
                                          avifgpu_icc_clut16* out);

/* avifgpu_write_rows for 8-bit RGB(A) documents with that table transform applied to R, G, B first (alpha copied: cmsFLAGS_COPY_ALPHA). */
int32_t avifgpu_write_rows_icc8_table(const avifgpu_write_desc* desc, const avifgpu_icc_clut16* icc,
                                      int32_t row0, int32_t nrows,
                                      const void* src, int64_t src_row_bytes,
                                      void* const dst[4], const int64_t dst_stride[4],
                                      int32_t mem_kind, void* stream);

/* ---- ... and of the HDR / 32-bit save path behind a LUT-based (A2B) document profile ----------------------------------------
 * For float formatters lcms2 does not resample (OptimizeByResampling refuses float formats): cmsDoTransform evaluates the linked,
 * pre-optimised pipeline stage by stage in floating point, a float between stages.  avifgpu_icc_pipeline32 is that stage program,
 * flat and pointer-free; the adapter captures it from lcms2 (integration/LcmsTableBridge.h) and each stage kind is evaluated exactly as
 * lcms2 2.12 evaluates it on floats:
 *   CURVES     per channel a parametric curve (lcms2 type +-1..+-5 and its parameters: EvalSegmentedFn + DefaultEvalParametricFn in
 *              double, cast to float) or a 16-bit table of 2..4096 entries (cmsEvalToneCurveFloat with nSegments == 0: the word
 *              _cmsQuickSaturateWord(v * 65535.0), LinLerp1D, (float)(w / 65535.0))
 *   MATRIX     3x3 in double, the optional bias added last, cast to float (EvaluateMatrix)
 *   CLUT16     3 in / 3 out, 2..33 grid points per input, non-uniform grids allowed; FromFloatTo16, TetrahedralInterp16 on the words,
 *              (float)w / 65535.0f (EvaluateCLUTfloatIn16).  At most one per program.
 *   LAB_TO_XYZ / XYZ_TO_LAB   lcms2's float PCS encodings (EvaluateLab2XYZ / EvaluateXYZ2Lab, D50)
 * Anything else -- multi-segment curves, float CLUTs, larger grids, other stages -- has no form here: the adapter gets
 * AVIFGPU_formatCannotRead and keeps lcms2.  A program is PROVEN before use: avifgpu_icc_pipeline32_prove evaluates the library's host
 * restatement on a fixed probe set and requires bit-identical floats from the caller's own cmsDoTransform; only then is it stamped, and
 * avifgpu_write_rows_icc_pipeline32 refuses an unstamped or altered program.  (The write kernel evaluates the same program -- curves and
 * matrices in double, the words with the library's arithmetic.  Held exactly: for a program without pow() -- table curves, the CLUT,
 * matrices, Lab -> XYZ, gamma-1 curves -- the kernel's float after the last stage is the float avifgpu_icc_pipeline32_eval gives, for every
 * input, NaN (whose 16-bit word lcms2 takes from its payload bits), +-Inf and values far outside [0, 1] included: the codes of the save equal
 * those of a save without ICC of the host's floats.  Behind pow() or the cube root of XYZ -> Lab the float may be a float32 neighbour of the
 * host's -- the device's pow() is not the C library's --, which is tier 2 like every float path: the bar is on the integer codes behind
 * the transfer curve.  tests/test_zzzz_gpu_icc32_programs.py.) */
enum { AVIFGPU_ICC_PIPE_MAX_STAGES = 16, AVIFGPU_ICC_PIPE_MAX_CURVE = 4096, AVIFGPU_ICC_PIPE_MAX_GRID = 33,
       AVIFGPU_ICC_PIPE_MAX_WORDS = 33 * 33 * 33 * 3 + 4 * 3 * 4096 };
enum { AVIFGPU_ICC_STAGE_CURVES = 1, AVIFGPU_ICC_STAGE_MATRIX = 2, AVIFGPU_ICC_STAGE_CLUT16 = 3,
       AVIFGPU_ICC_STAGE_LAB_TO_XYZ = 4, AVIFGPU_ICC_STAGE_XYZ_TO_LAB = 5 };
typedef struct avifgpu_icc_stage32 {
    int32_t kind;                /* AVIFGPU_ICC_STAGE_* */
    int32_t curve_type[3];       /* CURVES: lcms2 parametric type +-1..+-5 per channel, 0 = 16-bit table */
    int32_t entries[3];          /* CURVES: entries of a table channel (2..4096); CLUT16: grid points of input 0, 1, 2 (input 0 varies slowest) */
    int32_t offset[3];           /* CURVES: first word of a table channel in words[]; CLUT16: offset[0] = first word of the grid (3 words per node) */
    int32_t has_bias;            /* MATRIX: 1 = lcms2's stage carries an offset (added after the products) */
    int32_t reserved;
    double  params[3][10];       /* CURVES: parameters of a parametric channel, as lcms2 orders them */
    double  matrix[9];           /* MATRIX: row-major, out_i = (float)(((0 + in_0 m[3i]) + in_1 m[3i+1]) + in_2 m[3i+2] [+ bias_i]) */
    double  bias[3];
} avifgpu_icc_stage32;
typedef struct avifgpu_icc_pipeline32 {
    int32_t  target;             /* AVIFGPU_ICC_TARGET_REC2020_LINEAR | AVIFGPU_ICC_TARGET_SRGB_FLOAT: the destination it was built for */
    int32_t  stage_count;        /* 1..AVIFGPU_ICC_PIPE_MAX_STAGES */
    int32_t  word_count;         /* words[] in use */
    int32_t  reserved;
    uint64_t proof;              /* stamped by avifgpu_icc_pipeline32_prove (a checksum of everything else); 0 = not proven */
    avifgpu_icc_stage32 stages[AVIFGPU_ICC_PIPE_MAX_STAGES];
    uint16_t words[AVIFGPU_ICC_PIPE_MAX_WORDS];      /* curve tables and the CLUT grid */
} avifgpu_icc_pipeline32;

/* Prove `pipe` against float_fn -- cmsDoTransform on the caller's TYPE_RGB_FLT transform of the same profiles, intent and flags: neutrals,
 * the CLUT's nodes and their word neighbours, random triples in [-0.25, 4] and NaN-free extremes must come out of the library's
 * restatement bit for bit as out of float_fn.  0 and pipe->proof stamped; AVIFGPU_formatCannotRead (keep lcms2) with the reason in
 * avifgpu_last_error() otherwise -- a misread stage costs speed, never pixels.  Host-only; float_fn runs on the calling thread. */
int32_t avifgpu_icc_pipeline32_prove(avifgpu_icc_pipeline32* pipe, avifgpu_transform_f32_fn float_fn, void* user);

/* The library's host restatement of the program on n interleaved RGB triples (proven or not).  A DIAGNOSTIC -- the proof's engine and a
 * test hook: no write call ever evaluates pixels on the CPU.  AVIFGPU_formatBadParameters for a malformed program. */
int32_t avifgpu_icc_pipeline32_eval(const avifgpu_icc_pipeline32* pipe, const float* rgb_in, float* rgb_out, uint32_t n);

/* avifgpu_write_rows for 32-bit RGB(A) documents with the program applied to R, G, B first (alpha copied: cmsFLAGS_COPY_ALPHA); every
 * output the other 32-bit ICC entries take.  The target must agree with the transfer (SRGB_FLOAT: Clip).  AVIFGPU_formatBadParameters for an
 * unstamped or altered program.  The lifetime of the program follows the contract written above avifgpu_write_rows_icc16; every call
 * compares the device copy with the caller's program, so a program rewritten at the same address between saves is re-uploaded. */
int32_t avifgpu_write_rows_icc_pipeline32(const avifgpu_write_desc* desc, const avifgpu_icc_pipeline32* pipe,
                                          int32_t row0, int32_t nrows,
                                          const void* src, int64_t src_row_bytes,
                                          void* const dst[4], const int64_t dst_stride[4],
                                          int32_t mem_kind, void* stream);

/* ---- oriented open: the file's irot / imir properties applied on the GPU ------------------------------------------------------------
 * The reference decodes with heif_decode_image(handle, &img, colorSpace, chroma, nullptr) (Read.cpp:99): with no decoding options libheif
 * applies the item's `irot` and `imir` to the decoded planes before the plug-in sees them, and the plug-in resets the EXIF orientation to
 * top-left because of it (ReadMetadata.cpp:105-107).  An adapter that sets ignore_transformations gets the STORED planes and asks for
 * the orientation here instead.  An orientation is one of the eight EXIF codes.  With I the H x W x C array of host
 * samples avifgpu_read_rows produces for `desc` and its planes, the oriented open yields EXACTLY (numpy on I; no tolerance, floats too):
 *     1  I                          W x H        5  I.transpose(1, 0, 2)                  H x W
 *     2  I[:, ::-1]                 W x H        6  np.rot90(I, -1)  (clockwise)           H x W
 *     3  I[::-1, ::-1]              W x H        7  I[::-1, ::-1].transpose(1, 0, 2)       H x W
 *     4  I[::-1, :]                 W x H        8  np.rot90(I, 1)   (anticlockwise)       H x W
 * irot with angle a (anticlockwise quarter turns) is np.rot90(I, a): codes 1, 8, 3, 6; imir is code 2 or code 4.  The definition is in
 * the PIXEL domain: chroma is upsampled as the reference does it (nearest: x >> xs, y >> ys), then pixels are moved.  Where a subsampled
 * dimension is even that equals moving the planes first; where it is odd the two differ by one chroma sample's phase, and a quarter turn
 * of 4:2:2 has no plane-domain form at all (what libheif 1.14.0 does there is not verified).  The clean aperture (clap)
 * is applied by the cropped open below (avifgpu_read_rows_cropped), not by this entry.
 *
 * Output rows [orow0, orow0 + onrows) correspond to a source REGION -- a row range for codes 1-4, a column band for codes 5-8 -- that the
 * existing read kernels decode as a sub-image into scratch; a kernel of a code object of its own then moves whole pixels from scratch to
 * dst.  Where the cut direction is subsampled the region must start on an even source index (a region of ONE row / column may start
 * anywhere: it is its own chroma sample); with a flipped direction of odd size that makes the first tile odd, so callers cut with
 * avifgpu_read_oriented_next_tile. */

/* "apply `first`, then `then`" as one code.  Host only; closed over 1..8; formatBadParameters (negative) outside. */
int32_t avifgpu_orientation_compose(int32_t first, int32_t then);

/* Size of the oriented image: (W, H) for codes 1-4, (H, W) for codes 5-8. */
int32_t avifgpu_read_oriented_geometry(const avifgpu_read_desc* desc, int32_t orientation, int32_t* out_w, int32_t* out_h);

/* The largest onrows <= max_rows (max_rows >= 1) that output row orow0 may be followed by: all of max_rows, or the rest of the image,
 * where the cut direction is not subsampled; otherwise such that this tile's source region and the next one's both start on an even
 * index (or are single).  Always > 0 inside the image, so tiles cut with it partition the image for every max_rows; a negative OSErr
 * for bad arguments.  Host only. */
int32_t avifgpu_read_oriented_next_tile(const avifgpu_read_desc* desc, int32_t orientation, int32_t orow0, int32_t max_rows);

/* Device scratch a MEM_DEVICE call for `onrows` output rows needs: the decoded sub-image (rows padded to 256 bytes); 0 for code 1. */
int64_t avifgpu_read_oriented_scratch_bytes(const avifgpu_read_desc* desc, int32_t orientation, int32_t onrows);

/* Open output rows [orow0, orow0 + onrows) of the oriented image.  src[i] / src_stride[i] are the planes of the WHOLE stored image (row 0,
 * the plane order of avifgpu_read_rows); dst is the first byte of output row orow0; bytes of a dst row beyond out_w * bytes per pixel are
 * not touched.  AVIFGPU_MEM_DEVICE: `scratch` is the caller's device memory (avifgpu_read_oriented_scratch_bytes), the decode and the
 * orient kernel are enqueued on `stream` and the call does not synchronise.  AVIFGPU_MEM_HOST: scratch is NULL (ignored); the library
 * stages tiles of the range through two slots of its own on the FIRST bound context (planes up, decode, orient, rows down -- column bands
 * go up and down as strided copies); the bytes are the same for every number of bound contexts, pinned or pageable memory.  Code 1 is
 * avifgpu_read_rows on the range.  formatBadParameters before anything is launched for a code outside 1..8, an illegal cut, too little
 * scratch, too small dst_row_bytes. */
int32_t avifgpu_read_rows_oriented(const avifgpu_read_desc* desc, int32_t orientation, int32_t orow0, int32_t onrows,
                                   const void* const src[4], const int64_t src_stride[4],
                                   void* dst, int64_t dst_row_bytes,
                                   void* scratch, int64_t scratch_bytes,
                                   int32_t mem_kind, void* stream);

/* Measuring aid (tools/bench_orient.py): the orient kernel ALONE on device pointers -- a width x height image of bytes_per_pixel-byte
 * pixels (1, 2, 3, 4, 6, 8, 12, 16) at src, moved by code 2..8 to dst (height x width for codes 5-8), on `stream`. */
int32_t avifgpu_probe_orient(int32_t orientation, int32_t bytes_per_pixel, int32_t width, int32_t height,
                             const void* src, int64_t src_row_bytes, void* dst, int64_t dst_row_bytes, void* stream);

/* ---- upsampled open: 4:2:0 / 4:2:2 chroma interpolated instead of replicated ------------------------------------------------------------
 * Every other open replicates chroma (x >> xs, y >> ys), as the reference does (YuvDecode.cpp:302, ReadHeifImage.cpp:143); that stays the
 * default.  This is the read-side counterpart of AVIFGPU_DOWNSAMPLE_AVERAGE: an extension for adapters that want what later decoders are
 * believed to show (libheif >= 1.16 and libavif through libyuv are said to interpolate by default; the agreement of these taps with
 * either is NOT verified).  The definition is integer and exact.  For a YCbCr image of W x H with xs = 1 (4:2:0: ys = 1, 4:2:2: ys = 0)
 * each chroma plane C of cw = (W + 1) >> 1 by ch = (H + ys) >> ys samples is replaced by a plane U of W x H samples in the same
 * container type.  Taps are (index, weight in quarters), indices clamped to [0, cw - 1] / [0, ch - 1] (edge replication):
 *     horizontal, i = x >> 1   CENTER   even x: (i - 1, 1), (i, 3)     odd x: (i, 3), (i + 1, 1)
 *                              LEFT     even x: (i, 4)                 odd x: (i, 2), (i + 1, 2)
 *     vertical, j = y >> 1     4:2:0, both modes: the CENTER rule on y;    4:2:2: (y, 4)
 *     U[y, x] = (sum_a sum_b wy_a wx_b C[jy_a, ix_b] + 8) >> 4            -- ONE rounding of the joint 16-weight sum
 * on the raw container values as unsigned integers (a 10- / 12-bit sample above 2^bits - 1 is filtered as it is; the decode behind it
 * applies its own rule).  CENTER is the midpoint siting (AV1 chroma sample position "unknown", JPEG style); LEFT is AV1's "vertical":
 * co-sited with even luma columns, midway between rows.  "Colocated" is not offered.
 *
 * The upsampled open IS avifgpu_read_rows on the same descriptor with chroma = 4:4:4 and the planes (Y, U(Cb), U(Cr), A): every matrix,
 * range, transfer, alpha state, host depth and out-of-range rule is that of the 4:4:4 open.  With an orientation it is orient(code, .) of
 * that image, as avifgpu_read_rows_oriented defines it.  AVIFGPU_UPSAMPLE_NEAREST, a 4:4:4, a monochrome and a planar-RGB image yield the
 * bytes of avifgpu_read_rows_oriented (code 1: avifgpu_read_rows), whatever the mode. */
enum {
    AVIFGPU_UPSAMPLE_NEAREST         = 0,
    AVIFGPU_UPSAMPLE_BILINEAR_CENTER = 1,
    AVIFGPU_UPSAMPLE_BILINEAR_LEFT   = 2
};

/* Device scratch a MEM_DEVICE call for `onrows` output rows needs.  With the source region of those rows sw x sh (W x onrows for codes
 * 1-4, onrows x H for codes 5-8), s bytes per plane sample and b bytes per host pixel:
 *     2 * align256(sw * s) * sh   (the two upsampled chroma rectangles)   +   codes 2-8: align256(sw * b) * sh   (the oriented open's)
 * 0 where the call degenerates to an existing entry point (such a call hands `scratch` on to avifgpu_read_rows_oriented: size it with
 * avifgpu_read_oriented_scratch_bytes).  A negative OSErr for an unknown enum or a bad descriptor.  Host only: needs no device. */
int64_t avifgpu_read_upsampled_scratch_bytes(const avifgpu_read_desc* desc, int32_t upsampling, int32_t orientation, int32_t onrows);

/* Open output rows [orow0, orow0 + onrows) of the (oriented) upsampled image.  Arguments as for avifgpu_read_rows_oriented: src[i] are the
 * planes of the WHOLE stored image -- which is why this is an entry of its own: avifgpu_read_rows gets planes advanced to its first row and
 * cannot see the chroma row above a tile -- and tiles are cut with avifgpu_read_oriented_next_tile (even source indices).  The bytes of a
 * tile do not depend on the tiling.  AVIFGPU_MEM_DEVICE: the upsample kernel (a code object of its own), the existing 4:4:4 open on
 * (Y, scratch Cb, scratch Cr, A) and for codes 2-8 the existing orient kernels are enqueued on `stream`; the call does not synchronise.
 * AVIFGPU_MEM_HOST: scratch is ignored; tiles are staged through two slots of the library's own on the FIRST bound context; of the chroma
 * planes only the region's samples plus a halo (one sample; 8 bytes of them on the left, for alignment) on each side that exists go up.  The bytes are the same for every number of bound
 * contexts, pinned or pageable memory.  formatBadParameters before anything is launched for an unknown upsampling or orientation, an
 * illegal cut, too little scratch, too small dst_row_bytes. */
int32_t avifgpu_read_rows_upsampled(const avifgpu_read_desc* desc, int32_t upsampling, int32_t orientation, int32_t orow0, int32_t onrows,
                                    const void* const src[4], const int64_t src_stride[4],
                                    void* dst, int64_t dst_row_bytes,
                                    void* scratch, int64_t scratch_bytes,
                                    int32_t mem_kind, void* stream);

/* Measuring aid (tools/bench_upsample.py): the upsample kernel ALONE on device pointers.  src[0..1] are the whole Cb / Cr planes of a
 * width x height image of `chroma` (AVIFGPU_CHROMA_420 | 422) with bytes_per_sample 1 | 2; rectangle [x0, x0 + w) x [y0, y0 + h) of U(Cb)
 * and U(Cr) goes to dst[0..1] (first byte = sample (y0, x0)), on `stream`.  upsampling: one of the two bilinear modes.  twin 0 = the kernel
 * itself; 1 = its store-only twin (no source load, no cross-lane move), 2 = its math-free twin (the same loads and stores, no neighbour
 * samples, no sums) -- CENTER only, for attribution: what they leave in dst is meaningless. */
int32_t avifgpu_probe_upsample(int32_t bytes_per_sample, int32_t chroma, int32_t upsampling, int32_t width, int32_t height,
                               int32_t x0, int32_t y0, int32_t w, int32_t h,
                               const void* const src[2], const int64_t src_stride[2],
                               void* const dst[2], int64_t dst_row_bytes, int32_t twin, void* stream);

/* ---- cropped open: the file's clean aperture (clap) applied on the GPU ------------------------------------------------------------------
 * libheif applies three transformative properties inside heif_decode_image: clap, irot and imir.  An adapter that decodes with
 * ignore_transformations (which the oriented open needs) gets the STORED planes uncropped; this is the crop.  avifgpu_rect is a rectangle
 * in STORED image coordinates: 0 <= x0, 1 <= width, x0 + width <= desc.width, and likewise in y.  With F the H x W x C array of host samples
 * the un-oriented open of the whole image yields -- avifgpu_read_rows for AVIFGPU_UPSAMPLE_NEAREST, avifgpu_read_rows_upsampled(..., code
 * 1, ...) for the two bilinear modes -- the cropped open of (rect, upsampling, code) is EXACTLY (no tolerance, floats too)
 *     orient(code, F[y0 : y0 + height, x0 : x0 + width])
 * with orient the table above avifgpu_read_rows_oriented: width x height for codes 1-4, height x width for codes 5-8.  The definition is in
 * the PIXEL domain, like the oriented open's: an odd x0 / y0 of a 4:2:0 / 4:2:2 image keeps each pixel the chroma sample it has in the whole
 * image ((x0 + x) >> 1), which advanced plane pointers cannot express, and the bilinear taps of a pixel at the rectangle's edge reach
 * the chroma sample outside it and clamp at the PLANE's edge.  libheif's own crop works on the planes: it is believed to coincide for even
 * x0 / y0 and may differ by one chroma sample's phase for odd ones; that is NOT verified (with the oriented open's two
 * unverified corners). */
typedef struct avifgpu_rect { int32_t x0, y0, width, height; } avifgpu_rect;

/* The rectangle of a clean aperture in a width x height image.  Host only, exact rational arithmetic (128-bit integers).  clap holds
 * cleanApertureWidthN, D, cleanApertureHeightN, D, horizOffN, D, vertOffN, D.  The rule is ISO 14496-12's: pcX = horizOff + (width - 1) / 2,
 * left = pcX - (cleanApertureWidth - 1) / 2, right = pcX + (cleanApertureWidth - 1) / 2, top / bottom the same way; each edge is rounded half
 * up, floor(v + 1/2); then left, top are clamped to >= 0 and right, bottom to <= size - 1; rect = (left, top, right - left + 1, bottom - top
 * + 1).  formatBadParameters for a denominator <= 0, an aperture width or height <= 0 or an empty result (the aperture lies outside the
 * image); 128 bits hold every intermediate of 32-bit operands, so no operand is rejected for its size.  libheif 1.14.0 is believed to compute the same for every aperture whose edges are >= 0;
 * that is NOT verified.  Its rounding of a negative edge truncates toward zero, which after the clamp matters only for an aperture that lies
 * wholly outside the image. */
int32_t avifgpu_clap_to_rect(int32_t width, int32_t height, const int32_t clap[8], avifgpu_rect* out);

/* Fold a crop into a view.  The current view is orient(code, F[current]); crop_in_view is a rectangle in THAT view's coordinates; out is the
 * stored rectangle with orient(code, F[out]) == view[crop_in_view].  Host only.  An adapter folds the file's properties in their listed
 * order, starting from (whole image, code 1): a clap goes through avifgpu_clap_to_rect on the VIEW's size and then through this helper, an
 * irot / imir through avifgpu_orientation_compose.  formatBadParameters for a code outside 1..8, an empty or negative
 * rectangle, a crop outside the view. */
int32_t avifgpu_crop_compose(const avifgpu_rect* current, int32_t code, const avifgpu_rect* crop_in_view, avifgpu_rect* out);

/* Size of the cropped, oriented image: (rect.width, rect.height) for codes 1-4, (rect.height, rect.width) for codes 5-8. */
int32_t avifgpu_read_cropped_geometry(const avifgpu_read_desc* desc, const avifgpu_rect* rect, int32_t orientation, int32_t* out_w, int32_t* out_h);

/* Every cut is legal for the cropped entry; a cut on an odd ABSOLUTE source index of a subsampled direction costs a nearest open one more
 * decoded row / column and a pass of the mover.  Returns the largest onrows <= max_rows (max_rows >= 1) that avoids it where it can:
 * where the cut direction runs forwards, such that the NEXT tile's source region starts on an even absolute index; where it runs backwards
 * (the code flips it), such that THIS tile's does -- the last tile's region starts where the rectangle starts, whatever that is.  All of
 * max_rows, or the rest of the image, where it does not matter (a bilinear mode, an image or a cut direction that is not subsampled).
 * Always > 0 inside the image, so tiles cut with it partition the image for every max_rows; a negative OSErr for bad arguments.  Host only. */
int32_t avifgpu_read_cropped_next_tile(const avifgpu_read_desc* desc, const avifgpu_rect* rect, int32_t upsampling, int32_t orientation,
                                       int32_t orow0, int32_t max_rows);

/* Device scratch that is enough for ANY MEM_DEVICE call of `onrows` output rows.  With the source region of those rows sw x sh (rect.width
 * x onrows for codes 1-4, onrows x rect.height for codes 5-8), s bytes per plane sample and b bytes per host pixel:
 *     a bilinear mode on a 4:2:0 / 4:2:2 image:   2 * align256(sw * s) * sh   +   codes 2-8: align256(sw * b) * sh     (the upsampled open's)
 *     otherwise:                                   align256((sw + px) * b) * (sh + py);    0 for code 1 with px = py = 0
 * px = 1 where the image is subsampled horizontally, sw > 1 and the region may start on an odd column (codes 5-8: always; codes 1-4: x0 is
 * odd), py likewise for rows (codes 1-4: always; codes 5-8: y0 is odd).  A call needs only what ITS region needs (px, py from where it
 * starts; none for a call that degenerates to an existing entry point beyond what that entry needs).  A negative OSErr for an unknown enum,
 * a bad descriptor or rectangle.  Host only: needs no device. */
int64_t avifgpu_read_cropped_scratch_bytes(const avifgpu_read_desc* desc, const avifgpu_rect* rect, int32_t upsampling, int32_t orientation,
                                           int32_t onrows);

/* Open output rows [orow0, orow0 + onrows) of the cropped (upsampled, oriented) image.  src[i] / src_stride[i] are the planes of the WHOLE
 * stored image; everything else as for avifgpu_read_rows_upsampled; bytes of a dst row beyond the output row's pixels are not touched; the
 * bytes of a tile do not depend on the tiling.  How a call is served:
 *   - rect is the whole image (and the cut is one avifgpu_read_rows_upsampled takes): that entry, byte for byte;
 *   - code 1 and no phase problem -- the image is not subsampled YCbCr, or the mode is bilinear, or every subsampled direction of the region
 *     starts even or is a single row / column: the existing kernels write straight into dst from advanced pointers (a bilinear mode gives
 *     chroma_upsample the rectangle); for a nearest call avifgpu_last_kernel_name() is what avifgpu_read_rows reports for an image of the
 *     region's size;
 *   - code 1, nearest, an odd start in a subsampled direction: the existing kernels decode the COVERING rectangle (the start rounded down
 *     to even) into scratch and crop_rows -- a 2-D byte mover, a code object of its own -- moves the rows to dst from one pixel and / or
 *     one row in;
 *   - codes 2-8: decoded into scratch likewise, and the existing orient kernels run from the offset pixel.
 * AVIFGPU_MEM_HOST: scratch is ignored.  A code-1 call with nothing to move whose advanced plane pointers stay on the 16-byte grid is
 * avifgpu_read_rows on the sub-image (every bound context); anything else is staged in tiles through two slots of the library's own on the FIRST bound context: of every plane only the region's part
 * goes up, as a strided copy, plus the covering row / column or the bilinear halo where needed.  The bytes are the same for every number of
 * bound contexts, pinned or pageable memory.  formatBadParameters before anything is launched for a bad rectangle, upsampling, code or row
 * range, too little scratch, too small dst_row_bytes. */
int32_t avifgpu_read_rows_cropped(const avifgpu_read_desc* desc, const avifgpu_rect* rect, int32_t upsampling, int32_t orientation,
                                  int32_t orow0, int32_t onrows,
                                  const void* const src[4], const int64_t src_stride[4],
                                  void* dst, int64_t dst_row_bytes,
                                  void* scratch, int64_t scratch_bytes,
                                  int32_t mem_kind, void* stream);

/* Measuring and testing aid (tools/bench_crop.py): the mover kernel ALONE on device pointers -- `rows` rows of row_payload_bytes bytes from
 * src (any address) to dst (any address, any stride), on `stream`; bytes of a dst row beyond the payload are not touched. */
int32_t avifgpu_probe_crop(const void* src, int64_t src_row_bytes, void* dst, int64_t dst_row_bytes, int64_t row_payload_bytes, int32_t rows,
                           void* stream);

/* ---- grid open: a tiled (grid) image opened from its decoded tiles ----------------------------------------------------------------------
 * Large AVIF / HEIF pictures are stored as a `grid` derived image (ISO 23008-12 6.6.2.3): columns x rows coded tiles of tile_width x
 * tile_height in row-major order, of which the top-left desc.width x desc.height is visible.  libheif assembles the canvas on the CPU
 * inside heif_decode_image; an adapter that decodes the tile items itself hands their planes over as they are.  Every tile has the
 * colourspace, chroma format, bit depth and set of planes of the descriptor; the alpha plane shares the colour planes' tiling (an alpha
 * auxiliary image with a tiling of its own stays the caller's to assemble).  With xs, ys the chroma shifts, a tile's plane pl holds
 * tw_p x th_p samples -- (tile_width, tile_height) for luma, alpha, R, G, B; ((tile_width + xs) >> xs, (tile_height + ys) >> ys) for
 * chroma -- and the ASSEMBLED plane is
 *     P_pl[y, x] = tile[(y / th_p) * columns + (x / tw_p)].plane[pl][y % th_p, x % tw_p]
 * over the canvas's plane extent (chroma: ((W + xs) >> xs) x ((H + ys) >> ys)).  The grid open of (rect, upsampling, code, orow0, onrows)
 * IS avifgpu_read_rows_cropped on the assembled planes, byte for byte, for every descriptor that entry takes: float hosts, padding rules
 * and out-of-range sample rules included.  Assembly comes before upsampling, so bilinear taps cross tile seams as they cross any other
 * sample boundary.  That libheif 1.14.0 assembles a grid exactly this way is believed and NOT verified.
 * Legal grids: 1 <= columns, rows <= 256; columns * tile_width >= width and rows * tile_height >= height (in 64 bits); tile_width even
 * where columns are subsampled and columns > 1; tile_height even where rows are subsampled and rows > 1. */
typedef struct avifgpu_grid      { int32_t columns, rows, tile_width, tile_height; } avifgpu_grid;
typedef struct avifgpu_grid_tile { const void* plane[4]; int64_t stride[4]; } avifgpu_grid_tile;   /* 64 bytes */

/* The ImageGrid item payload, big-endian: version(8) = 0, flags(8), rows_minus_one(8), columns_minus_one(8), output_width and
 * output_height as 16 bits each, or 32 bits each when flags & 1 -- 8 or 12 bytes; trailing bytes are ignored.  formatBadParameters for a
 * null argument, a version other than 0, a short payload, a zero size, a size above INT32_MAX.  Host only: needs no device. */
int32_t avifgpu_grid_parse(const uint8_t* payload, int64_t size, int32_t* rows, int32_t* columns, int32_t* out_w, int32_t* out_h);

/* 0 where desc (its width x height is the canvas) and grid are what avifgpu_read_rows_grid takes; formatBadParameters (or what the
 * descriptor's own check returns) otherwise.  Host only. */
int32_t avifgpu_grid_check(const avifgpu_read_desc* desc, const avifgpu_grid* grid);

/* Device scratch that every MEM_DEVICE call of `onrows` output rows needs -- the entry asks for exactly this value.  rect NULL: the whole
 * canvas.  With the source region of those rows sw x sh (rect.width x onrows for codes 1-4, onrows x rect.height for codes 5-8), s bytes
 * per plane sample, gw = min(width, sw + 38), gh = min(height, sh + 6) (the cropped open's staged rectangle never exceeds that: the
 * region, its covering row / column or bilinear halo, and up to 31 columns in front of it):
 *     256  +  sum over the used planes of  align256(gw_p * s) * gh_p  +  C
 * where (gw_p, gh_p) = (gw, gh), for the chroma planes of a subsampled image ((gw + xs) >> xs, (gh + ys) >> ys), and C is
 * avifgpu_read_cropped_scratch_bytes' formula for sw x sh with px and py both counted.  The 256 let the library start on a 256-byte
 * boundary whatever `scratch` is.  A negative OSErr for an unknown enum, a bad descriptor, grid or rectangle.  Host only. */
int64_t avifgpu_read_grid_scratch_bytes(const avifgpu_read_desc* desc, const avifgpu_grid* grid, const avifgpu_rect* rect, int32_t upsampling,
                                        int32_t orientation, int32_t onrows);

/* Open output rows [orow0, orow0 + onrows) of the cropped (upsampled, oriented) ASSEMBLED image.  Cuts and the output size are the cropped
 * open's (avifgpu_read_cropped_next_tile, avifgpu_read_cropped_geometry on desc): every cut is legal and the bytes of a tile do not depend
 * on the tiling of the output rows.  rect NULL: the whole canvas.  `tiles` holds columns * rows records and lives where mem_kind says:
 *   AVIFGPU_MEM_DEVICE  a device pointer to records of device pointers.  The library never reads it on the host: grid_gather -- one launch
 *     of a byte-moving kernel, a code object of its own -- writes the staged rectangle of every used plane (what the cropped open's host
 *     path would upload for these rows) into the head of scratch, and avifgpu_read_rows_cropped runs on that with the rest of scratch.
 *     Everything is enqueued on `stream`; nothing synchronises.  A 1 x 1 grid gathers too.
 *   AVIFGPU_MEM_HOST    a host array of host pointers; scratch is ignored.  A 1 x 1 grid is avifgpu_read_rows_cropped on tile 0.  Otherwise
 *     the call is staged in tiles through two slots of the library's own on the FIRST bound context: each plane rectangle goes up as one
 *     strided copy per intersecting tile, straight into its place, so the copy engine assembles and no gather kernel runs.  The bytes are
 *     the same for every number of bound contexts, pinned or pageable memory.
 * A tile with no visible sample is never read and its pointers may be NULL; on MEM_HOST a NULL pointer or a stride below the row for a
 * used plane of a visible tile is rejected.  formatBadParameters before anything is launched for an illegal grid, NULL tiles, a bad
 * rectangle, upsampling, code or row range, less scratch than the helper's value, too small dst_row_bytes. */
int32_t avifgpu_read_rows_grid(const avifgpu_read_desc* desc, const avifgpu_grid* grid, const avifgpu_grid_tile* tiles,
                               const avifgpu_rect* rect, int32_t upsampling, int32_t orientation, int32_t orow0, int32_t onrows,
                               void* dst, int64_t dst_row_bytes, void* scratch, int64_t scratch_bytes, int32_t mem_kind, void* stream);

/* Measuring and testing aid (tools/bench_grid.py): the gather kernel ALONE on one plane -- rectangle [x0, x0 + w) x [y0, y0 + h) of the
 * plane assembled from tiles_dev[...].plane[plane] (tile_w_samples x tile_h_samples each, `columns` to a row; the rectangle must lie
 * inside the tiles the table holds) into rows of dst, on `stream`.  dst and dst_row_bytes are multiples of 16; bytes of a dst row beyond
 * the payload are not touched. */
int32_t avifgpu_probe_grid_gather(const avifgpu_grid_tile* tiles_dev, int32_t columns, int32_t plane, int32_t tile_w_samples,
                                  int32_t tile_h_samples, int32_t bytes_per_sample, int32_t x0, int32_t y0, int32_t w, int32_t h,
                                  void* dst, int64_t dst_row_bytes, void* stream);

/* ---- grid save: a save written straight into the padded tiles of a grid -------------------------------------------------------------------
 * The cap on a coded frame that makes large pictures grids on the way in holds on the way out: a document larger than one coded frame
 * reaches the encoder as columns x rows tile images of one size.  The grid save is the exact mirror of avifgpu_read_rows_grid.
 * With desc an avifgpu_write_desc (its width x height is the canvas), P_pl the plane pl the corresponding avifgpu_write_rows* call writes
 * for it -- pw x ph "pixels" of b = bytes_per_sample * samples_per_pixel bytes (avifgpu_write_plane_geometry; b is 1, 2, 3, 4, 6 or 8: the
 * interleaved AVIFGPU_OUT_REFERENCE colour plane moves whole pixels) -- xs, ys the chroma shifts of AVIFGPU_OUT_YCBCR output (0 otherwise)
 * and a tile's plane pl holding tw_p x th_p pixels ((tile_width, tile_height) for luma, alpha and interleaved planes,
 * ((tile_width + xs) >> xs, (tile_height + ys) >> ys) for chroma), the PADDED plane is the canvas plane replicated at its right and
 * bottom edge,
 *     Q_pl[y, x] = P_pl[min(y, ph - 1), min(x, pw - 1)]      over (rows * th_p) x (columns * tw_p),
 * and the tiles are
 *     tile[r * columns + c].plane[pl][y, x] = Q_pl[r * th_p + y, c * tw_p + x].
 * Edge replication is an EXTENSION of this library, like AVIFGPU_DOWNSAMPLE_AVERAGE: the reference writes no grids, and no encoder's own
 * padding rule was verified against it.
 * Legal grids for a save: those of the grid open (above), applied to the write descriptor's shifts, in which every tile also has a visible
 * sample: (columns - 1) * tile_width < width and (rows - 1) * tile_height < height.  Then every sample of every tile is written exactly
 * once per save -- an encoder is never handed a tile nobody wrote.
 * A call converts rows [row0, row0 + nrows) under avifgpu_write_rows' own rule for row0 and nrows and writes, in every used plane, the
 * plane rows of that range over all columns * tw_p pixels; the call whose range ends at `height` also writes the rows below ph.  So the
 * bytes of a tile do not depend on how the rows were cut into calls.  Bytes of a tile row beyond tw_p * b are never touched.
 * Byte equality: the tiles equal, byte for byte, the split of Q built from the plain save of the same descriptor, ICC stage and source into
 * planes whose base and stride are multiples of 256.  (The multiples of 256 matter for one case only: a 32-bit document behind an ICC
 * transform may take the streaming or the generic kernel depending on alignment, which agree within tier 2 -- see avifgpu_set_hot_variant.)
 * An armed code histogram, thumbnail and summary see the canvas, never the padding: what the same arms receive from the plain save. */
enum { AVIFGPU_ICC_KIND_NONE = 0,          /* icc must be NULL */
       AVIFGPU_ICC_KIND_TRANSFORM = 1,     /* const avifgpu_icc_transform*   (avifgpu_write_rows_icc) */
       AVIFGPU_ICC_KIND_SAMPLED = 2,       /* const avifgpu_icc_sampled32*   (avifgpu_write_rows_icc_sampled) */
       AVIFGPU_ICC_KIND_SHAPER8 = 3,       /* const avifgpu_icc_shaper8*     (avifgpu_write_rows_icc8) */
       AVIFGPU_ICC_KIND_CLUT16 = 4,        /* const avifgpu_icc_clut16*      (avifgpu_write_rows_icc16) */
       AVIFGPU_ICC_KIND_CLUT8_TABLE = 5,   /* const avifgpu_icc_clut16*      (avifgpu_write_rows_icc8_table) */
       AVIFGPU_ICC_KIND_PIPELINE32 = 6 };  /* const avifgpu_icc_pipeline32*  (avifgpu_write_rows_icc_pipeline32; must be stamped) */

/* 0 where desc and grid are what avifgpu_write_rows_grid takes; formatBadParameters (or what the descriptor's own check returns) with a
 * message otherwise.  Host only. */
int32_t avifgpu_write_grid_check(const avifgpu_write_desc* desc, const avifgpu_grid* grid);

/* Device scratch that a MEM_DEVICE call of `nrows` rows needs -- the entry asks for exactly this value:
 *     256  +  sum over the used planes of  align256(row bytes of the canvas plane) * plane rows of nrows
 * (plane rows: (nrows + ys) >> ys for chroma).  0 for nrows == 0; a negative OSErr for a bad descriptor or row count.  Host only. */
int64_t avifgpu_write_grid_scratch_bytes(const avifgpu_write_desc* desc, int32_t nrows);

/* The grid with the fewest tiles whose tiles are multiples of `align` and at most max_tile_width x max_tile_height: `columns` is the
 * smallest value for which some multiple of align is at most max_tile_width and at least ceil(width / columns), tile_width the smallest
 * such multiple; align is raised to even where that direction is subsampled and columns > 1; rows alike.  formatBadParameters where none
 * exists or a side would exceed 256.  The result is always legal and minimal: were (columns - 1) * tile_width >= width, tile_width would
 * have qualified columns - 1, which was tried first.  Host only. */
int32_t avifgpu_grid_fit(const avifgpu_write_desc* desc, int32_t max_tile_width, int32_t max_tile_height, int32_t align, avifgpu_grid* grid);

/* The ImageGrid item payload of (grid, width x height), the inverse of avifgpu_grid_parse: 8 bytes, or 12 with flags bit 0 where a size
 * exceeds 65 535.  Returns the byte count; formatBadParameters for a null argument, a side outside 1..256, a size below 1, too little
 * capacity.  Host only. */
int32_t avifgpu_grid_payload(const avifgpu_grid* grid, int32_t width, int32_t height, uint8_t* out, int64_t capacity);

/* Save rows [row0, row0 + nrows) into the tiles.  icc_kind says which prepared structure `icc` points to (NONE: NULL); the checks of the
 * corresponding avifgpu_write_rows* entry apply.  `tiles` holds columns * rows records and lives where mem_kind says:
 *   AVIFGPU_MEM_DEVICE  a device pointer to records of device pointers; the library never reads it on the host.  The unchanged save runs on
 *     `stream` into the head of scratch (planes at 256-byte-aligned bases, pitch align256(row bytes)), any armed statistics behind it on
 *     the caller's device arms, then grid_scatter -- a byte mover, a code object of its own; one launch, two for subsampled chroma --
 *     puts the band of every used plane into the tiles, padding included.  Nothing synchronises.
 *   AVIFGPU_MEM_HOST    a host array of host pointers; scratch is ignored.  The bound contexts' row-tile scheduler converts as for
 *     avifgpu_write_rows, pads in place on the device and sends every band down as one strided copy per tile piece: straight into
 *     page-locked tiles, through the pinned bounce buffer into pageable ones.  The bytes are the same for every number of bound contexts.
 *     A NULL pointer or a stride below the row for a used plane of any tile is refused before anything is queued.
 * Where samples are 16 bits (bit depth above 8) every tile plane and stride is a multiple of 2, as every plane of 16-bit samples in this
 * interface is; MEM_HOST refuses an odd one, a device table is the caller's to keep so.
 * formatBadParameters before anything is launched for an illegal or non-minimal grid, NULL tiles, an unknown kind, a bad row range, less
 * scratch than the helper's value (DEVICE), a bad mem_kind. */
int32_t avifgpu_write_rows_grid(const avifgpu_write_desc* desc, int32_t icc_kind, const void* icc, const avifgpu_grid* grid,
                                const avifgpu_grid_tile* tiles, int32_t row0, int32_t nrows, const void* src, int64_t src_row_bytes,
                                void* scratch, int64_t scratch_bytes, int32_t mem_kind, void* stream);

/* Measuring and testing aid (tools/bench_grid_save.py): the scatter kernel ALONE on one plane.  The plane holds plane_w x plane_h pixels of
 * bytes_per_pixel (1, 2, 3, 4, 6 or 8) bytes; rows [y0, y0 + h) of its PADDED plane (y0 < plane_h; the rows at and below plane_h are row
 * plane_h - 1 again) go to tiles_dev[...].plane[plane] (tile_w_pixels x tile_h_pixels each, `columns` to a row; the table must hold the
 * tile rows those rows touch).  `src` is plane row y0, rows src_row_bytes apart, at any address -- at any EVEN address and
 * row distance, like the tile planes, for the pixel sizes 2, 6 and 8, which are 16-bit samples and are moved as such at seams and in the
 * padding; on `stream`. */
int32_t avifgpu_probe_grid_scatter(const avifgpu_grid_tile* tiles_dev, int32_t columns, int32_t plane, int32_t tile_w_pixels,
                                   int32_t tile_h_pixels, int32_t bytes_per_pixel, int32_t plane_w, int32_t plane_h, int32_t y0, int32_t h,
                                   const void* src, int64_t src_row_bytes, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* AVIFGPU_H */
