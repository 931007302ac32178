// avifgpu_cli -- raw <-> planes converter that drives the FormatRecord tile protocol of include/avifgpu_host.h without
// Photoshop.  The CLI plays the host: advanceState() feeds rows of a raw file (save direction) or
// collects them (open direction), exactly what Photoshop does for the plug-in's row loops (WriteHeifImage.cpp:1017-1029,
// ReadHeifImage.cpp:141-160).  No conversion happens here: every pixel goes through libavifgpu (MI355X or error).
//
//   raw file    : host rows, tightly packed, Photoshop layout (interleaved planes, 8 / 16 [0..32768] / 32-bit float)
//   planes file : the heif_image planes in order 0..3, each with tight rows (width * bytes-per-sample), no header
#include <cerrno>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <utility>
#include <vector>

#include "../../include/avifgpu_host.h"

namespace {

struct Host {                       // the callbacks carry no user pointer in the SDK either: one static host
    avifgpu_FormatRecord fr{};
    FILE* file = nullptr;
    bool saving = false;            // true: host -> plug-in
    int tiles = 0;
} g_host;

avifgpu_OSErr advance_state()
{
    const avifgpu_VRect& r = g_host.fr.theRect32;
    const size_t bytes = (size_t)(r.bottom - r.top) * (size_t)g_host.fr.rowBytes;
    ++g_host.tiles;
    if (fseeko(g_host.file, (off_t)r.top * g_host.fr.rowBytes, SEEK_SET) != 0) return AVIFGPU_readErr;
    if (g_host.saving) return fread(g_host.fr.data, 1, bytes, g_host.file) == bytes ? AVIFGPU_noErr : AVIFGPU_readErr;
    return fwrite(g_host.fr.data, 1, bytes, g_host.file) == bytes ? AVIFGPU_noErr : AVIFGPU_writErr;
}
uint8_t never_abort() { return 0; }

struct Args {
    std::string cmd, in, out, icc, thumb_out;
    int width = 0, height = 0, depth = 8, planes = 3, bits = 8, transfer = AVIFGPU_TRANSFER_CLIP, peak = 1000;
    int alpha = AVIFGPU_ALPHA_NONE, output = AVIFGPU_OUT_REFERENCE, chroma = AVIFGPU_CHROMA_444;
    int matrix = AVIFGPU_MATRIX_BT601, primaries = AVIFGPU_PRIMARIES_BT709, tc = 2, limited = 0, colorspace = AVIFGPU_COLORSPACE_YCBCR;
    int lossless = 0, maxdata = 0, device = 0, hlg_ootf = 0, nclx = 0, keep_profile = 0, light_level = 0, thumb_bbox = 0, summary = 0, orientation = 0, upsampling = AVIFGPU_UPSAMPLE_NEAREST;
    int crop = 0, crop_x0 = 0, crop_y0 = 0, crop_w = 0, crop_h = 0;
    int grid = 0, grid_cols = 0, grid_rows = 0, grid_tw = 0, grid_th = 0;
    float gamma = 1.2f;
    double percentile = 1.0;
};

[[noreturn]] void usage(const char* why)
{
    if (why) fprintf(stderr, "avifgpu_cli: %s\n", why);
    fprintf(stderr,
        "usage: avifgpu_cli write --width W --height H --depth 8|16|32 --planes 1..4 --bits 8|10|12 [--transfer clip|pq|smpte428]\n"
        "                         [--peak NITS] [--alpha none|straight|premultiplied] [--ycbcr 444|422|420] [--matrix N] [--primaries N]\n"
        "                         [--lossless] [--icc PROFILE [--keep-profile]] [--maxdata BYTES] [--device N]\n"
        "                         [--light-level [--percentile P]] [--thumbnail BBOX THUMB.planes] [--summary] [--grid COLSxROWS,TWxTH] IN.raw OUT.planes\n"
        "       avifgpu_cli read  --width W --height H --depth 8|16|32 --bits 8|10|12 --colorspace ycbcr|rgb|mono [--chroma 444|422|420]\n"
        "                         [--alpha none|straight|premultiplied] [--matrix N --primaries N --tc N [--limited]] [--peak NITS]\n"
        "                         [--hlg-ootf --gamma G] [--orientation 1..8] [--chroma-upsampling nearest|bilinear|bilinear-left]\n"
        "                         [--crop X0,Y0,W,H] [--grid COLSxROWS,TWxTH] [--maxdata BYTES] [--device N] IN.planes OUT.raw\n"
        "       --grid: IN.planes holds the tiles' planes, tile after tile in row-major order, each laid out like a whole image of TW x TH;\n"
        "               --width / --height are the canvas.  write --grid saves into padded tiles and writes OUT.planes.tile0, .tile1, ... in that layout\n");
    exit(2);
}

int pick(const char* v, std::initializer_list<std::pair<const char*, int>> tbl, const char* opt)
{
    for (auto& e : tbl) if (!strcmp(v, e.first)) return e.second;
    usage((std::string("bad value for ") + opt + ": " + v).c_str());
}

Args parse(int argc, char** argv)
{
    Args a;
    if (argc < 2) usage(nullptr);
    a.cmd = argv[1];
    if (a.cmd != "write" && a.cmd != "read") usage("first argument must be write or read");
    std::vector<std::string> pos;
    for (int i = 2; i < argc; ++i) {
        const std::string o = argv[i];
        auto val = [&]() -> const char* { if (i + 1 >= argc) usage(("missing value for " + o).c_str()); return argv[++i]; };
        if (o == "--width") a.width = atoi(val());
        else if (o == "--height") a.height = atoi(val());
        else if (o == "--depth") a.depth = atoi(val());
        else if (o == "--planes") a.planes = atoi(val());
        else if (o == "--bits") a.bits = atoi(val());
        else if (o == "--peak") a.peak = atoi(val());
        else if (o == "--matrix") { a.matrix = atoi(val()); a.nclx = 1; }
        else if (o == "--primaries") { a.primaries = atoi(val()); a.nclx = 1; }
        else if (o == "--tc") { a.tc = atoi(val()); a.nclx = 1; }
        else if (o == "--limited") { a.limited = 1; a.nclx = 1; }
        else if (o == "--maxdata") a.maxdata = atoi(val());
        else if (o == "--device") a.device = atoi(val());
        else if (o == "--gamma") a.gamma = (float)atof(val());
        else if (o == "--hlg-ootf") a.hlg_ootf = 1;
        else if (o == "--lossless") a.lossless = 1;
        else if (o == "--keep-profile") a.keep_profile = 1;
        else if (o == "--light-level") a.light_level = 1;
        else if (o == "--percentile") a.percentile = atof(val());
        else if (o == "--thumbnail") { a.thumb_bbox = atoi(val()); a.thumb_out = val(); if (a.thumb_bbox < 1) usage("--thumbnail needs a bounding box >= 1"); }
        else if (o == "--summary") a.summary = 1;
        else if (o == "--icc") a.icc = val();
        else if (o == "--orientation") { a.orientation = atoi(val()); if (a.orientation < 1 || a.orientation > 8) usage("--orientation needs an EXIF code 1..8"); }
        else if (o == "--crop") { a.crop = 1; if (sscanf(val(), "%d,%d,%d,%d", &a.crop_x0, &a.crop_y0, &a.crop_w, &a.crop_h) != 4) usage("--crop needs X0,Y0,W,H"); }
        else if (o == "--chroma-upsampling") a.upsampling = pick(val(), {{"nearest", AVIFGPU_UPSAMPLE_NEAREST}, {"bilinear", AVIFGPU_UPSAMPLE_BILINEAR_CENTER}, {"bilinear-left", AVIFGPU_UPSAMPLE_BILINEAR_LEFT}}, "--chroma-upsampling");
        else if (o == "--transfer") a.transfer = pick(val(), {{"clip", AVIFGPU_TRANSFER_CLIP}, {"pq", AVIFGPU_TRANSFER_PQ}, {"smpte428", AVIFGPU_TRANSFER_SMPTE428}}, "--transfer");
        else if (o == "--alpha") a.alpha = pick(val(), {{"none", AVIFGPU_ALPHA_NONE}, {"straight", AVIFGPU_ALPHA_STRAIGHT}, {"premultiplied", AVIFGPU_ALPHA_PREMULTIPLIED}}, "--alpha");
        else if (o == "--ycbcr") { a.output = AVIFGPU_OUT_YCBCR; a.chroma = pick(val(), {{"444", AVIFGPU_CHROMA_444}, {"422", AVIFGPU_CHROMA_422}, {"420", AVIFGPU_CHROMA_420}}, "--ycbcr"); }
        else if (o == "--chroma") a.chroma = pick(val(), {{"444", AVIFGPU_CHROMA_444}, {"422", AVIFGPU_CHROMA_422}, {"420", AVIFGPU_CHROMA_420}}, "--chroma");
        else if (o == "--colorspace") a.colorspace = pick(val(), {{"ycbcr", AVIFGPU_COLORSPACE_YCBCR}, {"rgb", AVIFGPU_COLORSPACE_RGB}, {"mono", AVIFGPU_COLORSPACE_MONOCHROME}}, "--colorspace");
        else if (o == "--grid") { a.grid = 1; if (sscanf(val(), "%dx%d,%dx%d", &a.grid_cols, &a.grid_rows, &a.grid_tw, &a.grid_th) != 4) usage("--grid needs COLSxROWS,TWxTH"); }
        else if (o == "--help" || o == "-h") usage(nullptr);
        else if (o.rfind("--", 0) == 0) usage(("unknown option " + o).c_str());
        else pos.push_back(o);
    }
    if (pos.size() != 2) usage("need exactly IN and OUT files");
    a.in = pos[0]; a.out = pos[1];
    if (a.width <= 0 || a.height <= 0) usage("--width and --height are required");
    return a;
}

int image_mode(int depth, bool mono)
{
    if (mono) return depth == 8 ? avifgpu_plugInModeGrayScale : depth == 16 ? avifgpu_plugInModeGray16 : avifgpu_plugInModeGray32;
    return depth == 8 ? avifgpu_plugInModeRGBColor : depth == 16 ? avifgpu_plugInModeRGB48 : avifgpu_plugInModeRGB96;
}

void setup_record(const Args& a, int planes)
{
    avifgpu_FormatRecord& fr = g_host.fr;
    fr.abortProc = never_abort; fr.advanceState = advance_state; fr.progressProc = nullptr;
    fr.maxData = a.maxdata;
    fr.depth = (int16_t)a.depth; fr.planes = (int16_t)planes;
    fr.imageMode = (int16_t)image_mode(a.depth, planes <= 2);
    fr.imageSize32 = {a.height, a.width};
    fr.imageSize = {(int16_t)(a.height > 32767 ? 32767 : a.height), (int16_t)(a.width > 32767 ? 32767 : a.width)};
    fr.HostSupports32BitCoordinates = 1; fr.PluginUsing32BitCoordinates = 1;
}

int plane_rows(const avifgpu_image& img, int pl)
{
    const bool sub = img.colorspace == AVIFGPU_COLORSPACE_YCBCR && (pl == 1 || pl == 2) && img.chroma == AVIFGPU_CHROMA_420;
    return sub ? (img.height + 1) >> 1 : img.height;
}
size_t plane_row_bytes(const avifgpu_image& img, int pl)
{
    const int ssz = img.bit_depth > 8 ? 2 : 1;
    if (img.colorspace == AVIFGPU_COLORSPACE_RGB && img.chroma >= 10)
        return (size_t)img.width * ((img.chroma == 11 || img.chroma == 15) ? 4 : 3) * ssz;
    const bool sub = img.colorspace == AVIFGPU_COLORSPACE_YCBCR && (pl == 1 || pl == 2) && img.chroma != AVIFGPU_CHROMA_444;
    return (size_t)(sub ? (img.width + 1) >> 1 : img.width) * ssz;
}

int fail(const char* what, int code)
{
    fprintf(stderr, "avifgpu_cli: %s failed: OSErr %d (%s)\n", what, code, avifgpu_last_error());
    return 1;
}

int do_write(const Args& a)
{
    setup_record(a, a.planes);
    std::vector<uint8_t> profile;
    if (!a.icc.empty()) {
        FILE* f = fopen(a.icc.c_str(), "rb");
        if (!f) { perror(a.icc.c_str()); return 1; }
        uint8_t buf[65536]; size_t n;
        while ((n = fread(buf, 1, sizeof buf, f)) > 0) profile.insert(profile.end(), buf, buf + n);
        fclose(f);
        g_host.fr.iCCprofileData = profile.data(); g_host.fr.iCCprofileSize = (int32_t)profile.size();
    }
    g_host.file = fopen(a.in.c_str(), "rb");
    if (!g_host.file) { perror(a.in.c_str()); return 1; }
    g_host.saving = true;
    avifgpu_SaveUIOptions o{};
    o.imageBitDepth = a.bits; o.hdrTransferFunction = a.transfer; o.pq.nominalPeakBrightness = a.peak;
    o.chromaSubsampling = a.chroma; o.lossless = (uint8_t)a.lossless;
    o.keepColorProfile = (uint8_t)a.keep_profile;
    o.iccDecision = AVIFGPU_ICC_LIKE_PLUGIN;
    if (!a.icc.empty()) {
        // the plug-in's own gate (ColorProfileConversion.cpp:98-157), taken inside the library: HDR saves convert to Rec.2020
        // unless the document already is Rec.2020; 8/16-bit saves convert to sRGB unless it already is sRGB or the profile is
        // kept; 32-bit Clip saves convert to sRGB unless the profile is kept.  Printed here, decided there.
        const int32_t conversion = avifgpu_host_required_conversion_for_record(&g_host.fr, &o);
        if (conversion < 0) return fail("avifgpu_host_required_conversion_for_record", conversion);
        fprintf(stderr, "icc: %s\n", conversion == AVIFGPU_CONVERT_TO_REC2020 ? "convert to Rec.2020"
                                    : conversion == AVIFGPU_CONVERT_TO_SRGB ? "convert to sRGB" : "no conversion");
    }
    // --light-level: the code histogram of the save, armed around the shim's call on this thread (all tiles summed), then MaxCLL / MaxFALL
    std::vector<uint64_t> bins;
    if (a.light_level) {
        if (avifgpu_host_save_wants_light_level(&g_host.fr, &o) != 1) {
            fprintf(stderr, "avifgpu_cli: --light-level applies to 32-bit PQ saves only\n");
            return 1;
        }
        bins.assign((size_t)1 << (a.bits == 12 ? 12 : 10), 0);
        const int hrc = avifgpu_histogram_attach(bins.data(), a.bits, AVIFGPU_MEM_HOST);
        if (hrc) return fail("avifgpu_histogram_attach", hrc);
    }
    // --thumbnail: the box-average thumbnail of the save, its sums armed around the shim's call on this thread (all tiles summed)
    std::vector<uint64_t> tsums;
    avifgpu_write_desc td{};
    int32_t tw = 0, th = 0;
    if (a.thumb_bbox || a.summary) {
        avifgpu_SaveUIOptions n = o;                                // the options the save will run with (Write.cpp:231-258)
        if (avifgpu_host_normalize_save_options(&g_host.fr, &n) != AVIFGPU_noErr) return fail("avifgpu_host_normalize_save_options", AVIFGPU_formatBadParameters);
        td.width = a.width; td.height = a.height; td.depth = a.depth; td.planes = a.planes;
        td.bit_depth = n.imageBitDepth; td.transfer = n.hdrTransferFunction; td.peak_nits = a.peak; td.alpha_state = a.alpha;
        td.output = a.planes <= 2 ? AVIFGPU_OUT_REFERENCE : a.output;
        td.chroma = a.lossless ? AVIFGPU_CHROMA_444 : a.chroma;
        td.matrix_coefficients = a.lossless ? AVIFGPU_MATRIX_RGB_GBR : a.matrix; td.color_primaries = a.primaries;
        td.full_range = 1; td.chroma_downsampling = AVIFGPU_DOWNSAMPLE_AVERAGE; td.chroma_zero_point = AVIFGPU_CHROMA_ZERO_LIBHEIF;
    }
    if (a.thumb_bbox) {
        int trc = avifgpu_thumbnail_fit(&td, a.thumb_bbox, &tw, &th);
        if (trc) return fail("avifgpu_thumbnail_fit", trc);
        tsums.assign((size_t)tw * th * a.planes, 0);
        if ((trc = avifgpu_thumbnail_attach(tsums.data(), tw, th, AVIFGPU_MEM_HOST))) return fail("avifgpu_thumbnail_attach", trc);
    }
    // --summary: the range of every written channel, its counters armed around the shim's call on this thread (all tiles folded in)
    uint32_t counters[AVIFGPU_SUMMARY_COUNTERS] = {};
    if (a.summary) {
        const int src = avifgpu_summary_attach(counters, AVIFGPU_MEM_HOST);
        if (src) return fail("avifgpu_summary_attach", src);
    }
    avifgpu_image img{};
    // --grid: the save goes straight into columns * rows padded tile images (avifgpu_host_create_heif_image_grid), one output file per tile
    std::vector<avifgpu_image> tiles;
    const avifgpu_grid grid = { a.grid_cols, a.grid_rows, a.grid_tw, a.grid_th };
    if (a.grid) {
        if (a.grid_cols < 1 || a.grid_cols > 256 || a.grid_rows < 1 || a.grid_rows > 256 || a.grid_tw < 1 || a.grid_th < 1) { fprintf(stderr, "avifgpu_cli: bad --grid\n"); return 2; }
        tiles.assign((size_t)a.grid_cols * a.grid_rows, avifgpu_image{});
    }
    const int matrix = a.lossless ? AVIFGPU_MATRIX_RGB_GBR : a.matrix;
    const int rc = a.grid ? avifgpu_host_create_heif_image_grid(&g_host.fr, a.alpha, &o, a.output, matrix, a.primaries, &grid, tiles.data())
                          : avifgpu_host_create_heif_image(&g_host.fr, a.alpha, &o, a.output, matrix, a.primaries, &img);
    fclose(g_host.file);
    if (a.light_level) (void)avifgpu_histogram_attach(nullptr, 0, AVIFGPU_MEM_HOST);
    if (a.thumb_bbox) (void)avifgpu_thumbnail_attach(nullptr, 0, 0, AVIFGPU_MEM_HOST);
    if (a.summary) (void)avifgpu_summary_attach(nullptr, AVIFGPU_MEM_HOST);
    if (rc) { for (avifgpu_image& t : tiles) avifgpu_image_free(&t); return fail(a.grid ? "avifgpu_host_create_heif_image_grid" : "avifgpu_host_create_heif_image", rc); }
    if (a.grid) {
        // OUT.tile<k>: the planes of tile k in order 0..3, tight rows -- the layout `read --grid` takes tile after tile
        size_t total = 0;
        for (size_t k = 0; k < tiles.size(); ++k) {
            const std::string name = a.out + ".tile" + std::to_string(k);
            FILE* out = fopen(name.c_str(), "wb");
            if (!out) { perror(name.c_str()); for (avifgpu_image& t : tiles) avifgpu_image_free(&t); return 1; }
            for (int pl = 0; pl < 4; ++pl) {
                if (!tiles[k].plane[pl]) continue;
                const size_t rb = plane_row_bytes(tiles[k], pl);
                for (int y = 0; y < plane_rows(tiles[k], pl); ++y) total += fwrite(tiles[k].plane[pl] + (size_t)y * tiles[k].stride[pl], 1, rb, out);
            }
            fclose(out);
        }
        uint8_t payload[12];
        const int np = avifgpu_grid_payload(&grid, a.width, a.height, payload, sizeof payload);
        fprintf(stderr, "write: %dx%d depth %d -> %d-bit, %d x %d tiles of %d x %d, %d requests, %zu bytes, ImageGrid payload of %d bytes\n", a.width, a.height, a.depth, a.bits,
                a.grid_cols, a.grid_rows, a.grid_tw, a.grid_th, g_host.tiles, total, np);
        for (avifgpu_image& t : tiles) avifgpu_image_free(&t);
    }
    if (a.summary) {
        avifgpu_save_summary sm{};
        const int src = avifgpu_summary_read(&td, counters, &sm);
        if (src) { avifgpu_image_free(&img); return fail("avifgpu_summary_read", src); }
        printf("summary");
        for (int c = 0; c < sm.channels; ++c) printf(" min%d %d max%d %d", c, (int)sm.min_code[c], c, (int)sm.max_code[c]);
        printf(" spread %d alpha_opaque %d neutral %d advice %d\n", (int)sm.spread, (int)sm.alpha_opaque, (int)sm.neutral, (int)sm.advice);
    }
    if (a.thumb_bbox) {
        // the thumbnail planes in the raw form of the main planes: tight rows, plane after plane
        const int ssz = td.bit_depth > 8 ? 2 : 1;
        const bool interleaved = td.output == AVIFGPU_OUT_REFERENCE && a.planes >= 3;
        std::vector<uint8_t> tp[4];
        void* tdst[4] = {}; int64_t tstride[4] = {};
        for (int pl = 0; pl < 4; ++pl) {
            const bool used = interleaved ? pl == 0 : td.output == AVIFGPU_OUT_REFERENCE ? (pl == 0 || (pl == 3 && a.planes == 2)) : (pl < 3 || a.planes == 4);
            if (!used) continue;
            tstride[pl] = (int64_t)tw * (interleaved ? a.planes : 1) * ssz;
            tp[pl].assign((size_t)tstride[pl] * th, 0);
            tdst[pl] = tp[pl].data();
        }
        const int trc = avifgpu_thumbnail_from_sums(&td, tw, th, tsums.data(), tdst, tstride);
        if (trc) { avifgpu_image_free(&img); return fail("avifgpu_thumbnail_from_sums", trc); }
        FILE* tf = fopen(a.thumb_out.c_str(), "wb");
        if (!tf) { perror(a.thumb_out.c_str()); avifgpu_image_free(&img); return 1; }
        for (int pl = 0; pl < 4; ++pl) if (tdst[pl] && fwrite(tp[pl].data(), 1, tp[pl].size(), tf) != tp[pl].size()) { perror(a.thumb_out.c_str()); fclose(tf); avifgpu_image_free(&img); return 1; }
        fclose(tf);
        printf("thumbnail %dx%d\n", (int)tw, (int)th);
    }
    if (a.light_level) {
        avifgpu_content_light_level ll{};
        const int lrc = avifgpu_light_level_from_histogram(bins.data(), a.bits, o.hdrTransferFunction, a.percentile, &ll);
        if (lrc) { avifgpu_image_free(&img); return fail("avifgpu_light_level_from_histogram", lrc); }
        fprintf(stderr, "light-level: MaxCLL %u MaxFALL %u code %d pixels %llu\n", (unsigned)ll.max_cll, (unsigned)ll.max_fall, (int)ll.max_code,
                (unsigned long long)ll.pixels);
    }
    if (a.grid) return 0;
    FILE* out = fopen(a.out.c_str(), "wb");
    if (!out) { perror(a.out.c_str()); return 1; }
    size_t total = 0;
    for (int pl = 0; pl < 4; ++pl) {
        if (!img.plane[pl]) continue;
        const size_t rb = plane_row_bytes(img, pl);
        for (int y = 0; y < plane_rows(img, pl); ++y) total += fwrite(img.plane[pl] + (size_t)y * img.stride[pl], 1, rb, out);
    }
    fclose(out);
    fprintf(stderr, "write: %dx%d depth %d -> %d-bit %s, %d tiles, %zu bytes\n", a.width, a.height, a.depth, a.bits,
            img.colorspace == AVIFGPU_COLORSPACE_YCBCR ? "YCbCr planes" : img.colorspace == AVIFGPU_COLORSPACE_RGB ? "interleaved RGB" : "mono",
            g_host.tiles, total);
    avifgpu_image_free(&img);
    return 0;
}

// --grid: the tiles of a grid image, opened without assembling the canvas on the CPU (avifgpu_host_read_heif_image_grid)
int do_read_grid(const Args& a)
{
    if (a.grid_cols < 1 || a.grid_cols > 256 || a.grid_rows < 1 || a.grid_rows > 256 || a.grid_tw < 1 || a.grid_th < 1) { fprintf(stderr, "avifgpu_cli: bad --grid\n"); return 2; }
    std::vector<avifgpu_image> tiles((size_t)a.grid_cols * a.grid_rows);
    auto release = [&]() { for (avifgpu_image& t : tiles) if (t.owner) avifgpu_image_free(&t); };
    FILE* in = fopen(a.in.c_str(), "rb");
    if (!in) { perror(a.in.c_str()); return 1; }
    for (avifgpu_image& t : tiles) {
        t = avifgpu_image{};
        t.width = a.grid_tw; t.height = a.grid_th; t.colorspace = a.colorspace; t.bit_depth = a.bits;
        t.chroma = a.colorspace == AVIFGPU_COLORSPACE_MONOCHROME ? AVIFGPU_CHROMA_MONOCHROME : a.colorspace == AVIFGPU_COLORSPACE_RGB ? AVIFGPU_CHROMA_444 : a.chroma;
        t.has_alpha = a.alpha != AVIFGPU_ALPHA_NONE; t.premultiplied_alpha = a.alpha == AVIFGPU_ALPHA_PREMULTIPLIED;
        if (avifgpu_image_alloc(&t) != AVIFGPU_noErr) { fprintf(stderr, "avifgpu_cli: out of memory\n"); fclose(in); release(); return 1; }
        for (int pl = 0; pl < 4; ++pl) {
            if (!t.plane[pl]) continue;
            const size_t rb = plane_row_bytes(t, pl);
            for (int y = 0; y < plane_rows(t, pl); ++y)
                if (fread(t.plane[pl] + (size_t)y * t.stride[pl], 1, rb, in) != rb) { fprintf(stderr, "avifgpu_cli: %s is too short\n", a.in.c_str()); fclose(in); release(); return 1; }
        }
    }
    fclose(in);
    const int planes = (a.colorspace == AVIFGPU_COLORSPACE_MONOCHROME ? 1 : 3) + (a.alpha != AVIFGPU_ALPHA_NONE ? 1 : 0);
    setup_record(a, planes);
    const avifgpu_rect rect{a.crop_x0, a.crop_y0, a.crop_w, a.crop_h};
    int vw = a.crop ? a.crop_w : a.width, vh = a.crop ? a.crop_h : a.height;
    if (a.orientation >= 5) std::swap(vw, vh);
    g_host.fr.imageSize32 = {vh, vw};
    g_host.fr.imageSize = {(int16_t)(vh > 32767 ? 32767 : vh), (int16_t)(vw > 32767 ? 32767 : vw)};
    g_host.file = fopen(a.out.c_str(), "wb");
    if (!g_host.file) { perror(a.out.c_str()); release(); return 1; }
    g_host.saving = false;
    avifgpu_nclx nclx{a.primaries, a.tc, a.matrix, (uint8_t)!a.limited};
    avifgpu_LoadUIOptions lo{};
    lo.pq.nominalPeakBrightness = a.peak; lo.hlg.applyOOTF = (uint8_t)a.hlg_ootf; lo.hlg.displayGamma = a.gamma; lo.hlg.nominalPeakBrightness = a.peak;
    const avifgpu_grid grid{a.grid_cols, a.grid_rows, a.grid_tw, a.grid_th};
    const int rc = avifgpu_host_read_heif_image_grid(tiles.data(), &grid, a.width, a.height, a.crop ? &rect : nullptr, a.orientation ? a.orientation : 1, a.upsampling, a.alpha,
                                                     (a.nclx || a.depth == 32) ? &nclx : nullptr, &lo, &g_host.fr);
    fclose(g_host.file);
    release();
    if (rc) return fail("avifgpu_host_read_heif_image_grid", rc);
    fprintf(stderr, "read: %dx%d canvas in %dx%d tiles of %dx%d, %d-bit -> host depth %d, %d planes, %d tiles, maxValue %d\n", a.width, a.height, a.grid_cols, a.grid_rows,
            a.grid_tw, a.grid_th, a.bits, a.depth, planes, g_host.tiles, g_host.fr.maxValue);
    return 0;
}

int do_read(const Args& a)
{
    if (a.grid) return do_read_grid(a);
    avifgpu_image img{};
    img.width = a.width; img.height = a.height; img.colorspace = a.colorspace; img.bit_depth = a.bits;
    img.chroma = a.colorspace == AVIFGPU_COLORSPACE_MONOCHROME ? AVIFGPU_CHROMA_MONOCHROME
               : a.colorspace == AVIFGPU_COLORSPACE_RGB ? AVIFGPU_CHROMA_444 : a.chroma;
    img.has_alpha = a.alpha != AVIFGPU_ALPHA_NONE; img.premultiplied_alpha = a.alpha == AVIFGPU_ALPHA_PREMULTIPLIED;
    if (avifgpu_image_alloc(&img) != AVIFGPU_noErr) { fprintf(stderr, "avifgpu_cli: out of memory\n"); return 1; }
    FILE* in = fopen(a.in.c_str(), "rb");
    if (!in) { perror(a.in.c_str()); return 1; }
    for (int pl = 0; pl < 4; ++pl) {
        if (!img.plane[pl]) continue;
        const size_t rb = plane_row_bytes(img, pl);
        for (int y = 0; y < plane_rows(img, pl); ++y)
            if (fread(img.plane[pl] + (size_t)y * img.stride[pl], 1, rb, in) != rb) { fprintf(stderr, "avifgpu_cli: %s is too short\n", a.in.c_str()); return 1; }
    }
    fclose(in);
    const int planes = (a.colorspace == AVIFGPU_COLORSPACE_MONOCHROME ? 1 : 3) + (img.has_alpha ? 1 : 0);
    setup_record(a, planes);
    // --crop: a rectangle of the STORED image (the clean aperture); OUT.raw is orient(code, crop), composes with the two options below
    const avifgpu_rect rect{a.crop_x0, a.crop_y0, a.crop_w, a.crop_h};
    const int vw = a.crop ? a.crop_w : a.width, vh = a.crop ? a.crop_h : a.height;
    if (a.crop) {
        g_host.fr.imageSize32 = {vh, vw};
        g_host.fr.imageSize = {(int16_t)(vh > 32767 ? 32767 : vh), (int16_t)(vw > 32767 ? 32767 : vw)};
    }
    if (a.orientation >= 5) {                                       // a quarter turn: the document is H wide and W high (avifgpu_read_oriented_geometry)
        g_host.fr.imageSize32 = {vw, vh};
        g_host.fr.imageSize = {(int16_t)(vw > 32767 ? 32767 : vw), (int16_t)(vh > 32767 ? 32767 : vh)};
    }
    g_host.file = fopen(a.out.c_str(), "wb");
    if (!g_host.file) { perror(a.out.c_str()); return 1; }
    g_host.saving = false;
    avifgpu_nclx nclx{a.primaries, a.tc, a.matrix, (uint8_t)!a.limited};
    avifgpu_LoadUIOptions lo{};
    lo.pq.nominalPeakBrightness = a.peak; lo.hlg.applyOOTF = (uint8_t)a.hlg_ootf; lo.hlg.displayGamma = a.gamma; lo.hlg.nominalPeakBrightness = a.peak;
    // --orientation: IN.planes is the STORED image, OUT.raw the oriented one (irot / imir applied on the GPU)
    // --chroma-upsampling: the chroma of a 4:2:x image is interpolated on the GPU (composes with --orientation)
    const int rc = a.crop ? avifgpu_host_read_heif_image_cropped(&img, &rect, a.orientation ? a.orientation : 1, a.upsampling, a.alpha, (a.nclx || a.depth == 32) ? &nclx : nullptr, &lo, &g_host.fr)
                 : a.upsampling != AVIFGPU_UPSAMPLE_NEAREST
                       ? avifgpu_host_read_heif_image_upsampled(&img, a.orientation ? a.orientation : 1, a.upsampling, a.alpha, (a.nclx || a.depth == 32) ? &nclx : nullptr, &lo, &g_host.fr)
                 : a.orientation ? avifgpu_host_read_heif_image_oriented(&img, a.orientation, a.alpha, (a.nclx || a.depth == 32) ? &nclx : nullptr, &lo, &g_host.fr)
                                 : avifgpu_host_read_heif_image(&img, a.alpha, (a.nclx || a.depth == 32) ? &nclx : nullptr, &lo, &g_host.fr);
    fclose(g_host.file);
    avifgpu_image_free(&img);
    if (rc) return fail(a.crop ? "avifgpu_host_read_heif_image_cropped" : a.upsampling != AVIFGPU_UPSAMPLE_NEAREST ? "avifgpu_host_read_heif_image_upsampled" : a.orientation ? "avifgpu_host_read_heif_image_oriented" : "avifgpu_host_read_heif_image", rc);
    fprintf(stderr, "read: %dx%d %d-bit -> host depth %d, %d planes, %d tiles, maxValue %d\n", a.width, a.height, a.bits, a.depth,
            planes, g_host.tiles, g_host.fr.maxValue);
    return 0;
}

} // namespace

int main(int argc, char** argv)
{
    const Args a = parse(argc, argv);
    const int rc = avifgpu_init(a.device);
    if (rc) return fail("avifgpu_init", rc);
    const int r = a.cmd == "write" ? do_write(a) : do_read(a);
    avifgpu_shutdown();
    return r;
}
