// write_dispatch_check -- holds the choice of write kernel (avif-format_amd/csrc/write_dispatch.h) to the record of what the library chose
// before the choice lived in that header: for every case of tests/golden/write_dispatch_labels.json.gz -- handed over as one line of
// tab-separated fields per case, `python tests/write_dispatch_cases.py FIXTURE OUT.tsv` writes them -- it builds the WriteParams
// launch_write() would get (pointers = a 256-byte aligned base + the recorded offset, never dereferenced; of the ICC stage exactly the
// fields the launcher reads) and demands decide_write()'s label, under the case's tuning word and under that word with a block cap of
// 1.  Then, by hand, the cases no small launch reaches: work units at and beyond the 2^31 guard, tiles of 2^29 pixels, footprint groups
// beyond the generic kernel's index.  A stand-alone program with its own main, meant to be built with the sanitizers and run on the CPU
// (no device, no HIP), as the product's first code object sees the header (AG_WRITE_PART=1: the sampled-curve kernels in a part of their own):
//   g++ -std=c++17 -O1 -g -DAG_WRITE_PART=1 -fsanitize=address,undefined -fno-sanitize-recover=all tools/write_dispatch_check.cpp -o write_dispatch_check && ./write_dispatch_check CASES.tsv
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <map>
#include <sstream>
#include <string>
#include <vector>

#include "../avif-format_amd/csrc/write_dispatch.h"

using namespace avifgpu;

static long long g_checks = 0;
#define CHECK(cond) do { ++g_checks; if (!(cond)) { fprintf(stderr, "write_dispatch_check: %s:%d: %s\n", __FILE__, __LINE__, #cond); exit(1); } } while (0)

static uint8_t* fake(uintptr_t base, long long off) { return reinterpret_cast<uint8_t*>(base + (uintptr_t)off); }
constexpr uintptr_t kSrcBase = 0x100000000ull, kDstBase[4] = { 0x200000000ull, 0x300000000ull, 0x400000000ull, 0x500000000ull };
static const int kOne = 1;          // what a non-null table pointer points to: the launcher compares them with nullptr only

// the fields fill_write_params sets that the launcher reads (avifgpu_api.hip), without the ICC stage
static WriteParams params(int depth, int bit_depth, int transfer, int pq, int alpha, int nearest, int w, int rows)
{
    WriteParams p;
    memset(&p, 0, sizeof p);
    p.width = w; p.nrows = rows; p.rows_to_end = rows;
    p.transfer = depth == 32 ? transfer : AVIFGPU_TRANSFER_CLIP;
    p.premultiply = alpha == AVIFGPU_ALPHA_PREMULTIPLIED;
    p.nearest = nearest;
    p.maxv = (1 << bit_depth) - 1;
    p.pq_close = pq != AVIFGPU_PQ_COMPACT;
    return p;
}
// ... and of the ICC stage what fill_icc_params makes of the kind (icc_tables.cpp); bit 6 of the tuning word keeps the tables of the
// " lds" kinds in memory (icc_tables.cpp:153, :217)
static void set_icc(WriteParams& p, const std::string& kind, int word = 0)
{
    const bool lds = !(word & 64);
    auto parametric = [&](bool linear, bool same_simple, int out) {
        for (int c = 0; c < 3; ++c) { p.icc_trc_type[c] = 1; p.icc_trc_linear[c] = linear; }
        p.icc_same_simple = same_simple; p.icc_out = out;
    };
    if (kind == "none") return;
    if (kind == "icc 1") parametric(true, false, 0);
    else if (kind == "icc 2") parametric(false, true, 0);
    else if (kind == "icc 2 mixed") parametric(false, false, 0);
    else if (kind == "icc 4") parametric(true, false, 4);
    else if (kind == "icc 4 curved") parametric(false, true, 4);
    else if (kind == "sampled" || kind == "sampled lds") {
        for (int c = 0; c < 3; ++c) { p.icc_trc_type[c] = 6; p.icc_s_n[c] = (kind == "sampled lds" && lds) ? 256 : 0; }
        p.icc_s_tab = reinterpret_cast<const float*>(&kOne);
        p.icc_s_lds = kind == "sampled lds" && lds;
    } else if (kind == "pipeline32" || kind == "pipeline32 lds") {
        for (int c = 0; c < 3; ++c) p.icc_trc_type[c] = 8;
        p.icc_p8_stages = &kOne;
        p.icc_p8_lds_words = (kind == "pipeline32 lds" && lds) ? 768 : 0;
    } else if (kind == "shaper8") p.icc8_s1 = reinterpret_cast<const int32_t*>(&kOne);
    else if (kind == "clut8-table" || kind == "clut16") p.icc16_clut = reinterpret_cast<const uint16_t*>(&kOne);
    else { fprintf(stderr, "write_dispatch_check: unknown ICC kind '%s'\n", kind.c_str()); exit(1); }
}

struct Decided { WriteLaunch L; WriteParams q; };
static Decided decide(const WriteParams& p, int depth, int planes, int bit_depth, int output, int chroma, int word)
{
    Decided d;
    int xs = 0, ys = 0;                                       // check_write: the hand-offs and gray documents have no chroma shift
    if (output == AVIFGPU_OUT_YCBCR && planes >= 3) { xs = chroma != AVIFGPU_CHROMA_444; ys = chroma == AVIFGPU_CHROMA_420; }
    decide_write(p, depth, planes, bit_depth > 8, output, xs, ys, word, d.q, d.L);
    return d;
}

// ---- the record ---------------------------------------------------------------------------------------------------------------------------
static long long replay(const char* path)
{
    std::ifstream in(path);
    if (!in) { fprintf(stderr, "write_dispatch_check: cannot read %s\n", path); exit(1); }
    std::string line;
    long long n = 0;
    std::map<std::string, long long> taken;
    while (std::getline(in, line)) {
        std::vector<std::string> f;
        std::stringstream ss(line);
        for (std::string t; std::getline(ss, t, '\t');) f.push_back(t);
        CHECK(f.size() == 25);
        auto num = [&](int i) { return atoll(f[i].c_str()); };
        // depth planes bit_depth transfer pq alpha output chroma nearest icc word w rows src ss d0..d3 ds0..ds3 label label_cap
        const int depth = (int)num(0), planes = (int)num(1), bit_depth = (int)num(2), output = (int)num(6), chroma = (int)num(7), word = (int)num(10);
        WriteParams p = params(depth, bit_depth, (int)num(3), (int)num(4), (int)num(5), (int)num(8), (int)num(11), (int)num(12));
        set_icc(p, f[9], word);
        p.src = fake(kSrcBase, num(13)); p.src_row_bytes = num(14);
        for (int pl = 0; pl < 4; ++pl) {
            p.dst[pl] = num(15 + pl) < 0 ? nullptr : fake(kDstBase[pl], num(15 + pl));
            p.dst_stride[pl] = num(19 + pl);
        }
        for (int capped = 0; capped < 2; ++capped) {
            const Decided d = decide(p, depth, planes, bit_depth, output, chroma, capped ? (word | 1 << 8) : word);
            const std::string& want = f[23 + capped];
            if (d.L.invalid || d.L.kernel == kWkEmpty || want != d.L.label) {
                fprintf(stderr, "write_dispatch_check: case %lld (%s): recorded '%s', decided '%s'%s\n", n, line.c_str(), want.c_str(), d.L.label, d.L.invalid ? " (invalid)" : "");
                exit(1);
            }
            ++g_checks;
            CHECK(d.L.blocks >= 1 && d.L.blocks <= d.L.need && d.L.blocks <= d.L.cap);
            CHECK((strstr(d.L.label, " cap=") != nullptr) == (capped && d.L.need > 1));
            CHECK(d.L.flat == (strstr(d.L.label, " flat") != nullptr && d.L.kernel != kWkCopyRows));
        }
        ++n;
    }
    return n;
}

// ---- what no small launch reaches ---------------------------------------------------------------------------------------------------------
static WriteParams tile(int depth, int planes, int bit_depth, int w, int rows, long long src_pad, int nplanes_out, long long plane_row_bytes, long long dst_pad)
{
    WriteParams p = params(depth, bit_depth, AVIFGPU_TRANSFER_PQ, AVIFGPU_PQ_AUTO, AVIFGPU_ALPHA_NONE, 0, w, rows);
    p.src = fake(kSrcBase, 0); p.src_row_bytes = (long long)w * planes * (depth / 8) + src_pad;
    for (int pl = 0; pl < nplanes_out; ++pl) { p.dst[pl] = fake(kDstBase[pl], 0); p.dst_stride[pl] = plane_row_bytes + dst_pad; }
    return p;
}

static void by_hand()
{
    const int word = kHotDefault;
    // Work units at and beyond the guard `units + 8 * 65536 * 4 < 0x7fffffff` (parent write_kernels.hip:4501, the f32 hand-off; every
    // streaming block carried the same line): the candidate takes 2 145 383 424 waves and hands 2 145 386 496 on -- to the generic kernel,
    // whose footprint groups then exceed its own index: hipErrorInvalidValue (parent :3564).
    {
        const int w = 1 << 20;                                  // 3 Mi samples a row: 3072 waves
        for (int over = 0; over < 2; ++over) {
            const int rows = 698367 + over;
            const WriteParams p = tile(32, 3, 10, w, rows, 16, 1, (long long)w * 3 * 2, 16);
            const Decided d = decide(p, 32, 3, 10, AVIFGPU_OUT_REFERENCE, AVIFGPU_CHROMA_444, word);
            const WriteAsk a = { p, 32, 3, true, AVIFGPU_OUT_REFERENCE, 0, 0, word };
            WriteLaunch one;
            CHECK(cand_f32_ref(a, one) == !over);
            if (!over) {
                CHECK(d.L.kernel == kWkF32Ref && !d.L.invalid && d.L.units == 3072LL * rows && d.L.units + 8LL * 65536 * 4 == 0x7fffffffLL - 3071);
                CHECK(d.L.need == d.L.units && d.L.blocks == AG_STREAM_BLOCK_CAP * 4 / kF32RefWaves);
                CHECK(strcmp(d.L.label, "write_f32_ref_stream<transfer=0,planes=3>") == 0);
            } else {
                CHECK(d.L.kernel == kWkPx && d.L.invalid);
            }
        }
        // the same at a candidate behind which another one stands: the 8-bit copy hands on to the integer hand-off (parent :3803, :3813)
        const int w8 = 1 << 19, rows8 = 2095105;                // RGBA8, 2 MiB a row: 1024 waves of the copy, 512 of the hand-off
        WriteParams p = tile(8, 4, 8, w8, rows8, 16, 1, (long long)w8 * 4, 16);
        Decided d = decide(p, 8, 4, 8, AVIFGPU_OUT_REFERENCE, AVIFGPU_CHROMA_444, word);
        CHECK(d.L.kernel == kWkIntRef && !d.L.invalid && d.L.units == 512LL * rows8);
        CHECK(strcmp(d.L.label, "write_int_ref_stream<depth=8,planes=4,dst16=0>") == 0 && !d.L.one);
        p.nrows = 2095104 - 1;                                  // 1024 x 2 095 103 + 2^21 = 0x7fffffff - 1023: the copy's own
        d = decide(p, 8, 4, 8, AVIFGPU_OUT_REFERENCE, AVIFGPU_CHROMA_444, word);
        CHECK(d.L.kernel == kWkCopyRows && d.L.units == 1024LL * p.nrows);
    }
    // FLAT needs px < 2^29 (parent write_kernels.hip:4433-4434): 32768 x 16383 contiguous RGB f32 pixels are one row, 32768 x 16384 are not
    for (int over = 0; over < 2; ++over) {
        const int w = 32768, rows = 16383 + over;
        const WriteParams p = tile(32, 3, 10, w, rows, 0, 3, (long long)w * 2, 0);
        const Decided d = decide(p, 32, 3, 10, AVIFGPU_OUT_YCBCR, AVIFGPU_CHROMA_444, word);
        CHECK(d.L.kernel == kWkRgb32 && d.L.flat == !over && d.L.lines);
        CHECK(strcmp(d.L.label, over ? "write_rgb32_ycbcr444_hot<transfer=0,pxl=8,nt=1>" : "write_rgb32_ycbcr444_hot<transfer=0,pxl=8,nt=1> flat") == 0);
        CHECK(d.L.units == 64LL * rows && d.L.waves == AG_HOT444_BLOCK_LINES / 64);
        if (!over) CHECK(d.q.width == w * rows && d.q.nrows == 1 && d.q.rows_to_end == 1 && d.q.src_row_bytes == 12LL * w * rows && d.q.dst_stride[2] == 2LL * w * rows && d.q.dst_stride[3] == 0);
    }
    // write_px: groups >= 0x7fffffff - 256 * 65536 is hipErrorInvalidValue (parent write_kernels.hip:3564).  RGB16 -> u16 planes owns 4
    // pixels a thread: 12 pixels a row, 710 235 477 rows are 2 130 706 431 groups, the first count refused; one row less is launched.
    for (int over = 0; over < 2; ++over) {
        const int rows = 710235476 + over;
        const WriteParams p = tile(16, 3, 12, 12, rows, 8, 3, 24, 8);
        const Decided d = decide(p, 16, 3, 12, AVIFGPU_OUT_YCBCR, AVIFGPU_CHROMA_444, 0);
        CHECK(d.L.kernel == kWkPx && d.L.invalid == (over != 0));
        if (!over) {
            CHECK(d.L.units == 3LL * rows && d.L.units == 0x7fffffffLL - 256LL * 65536 - 3 && d.L.blocks == AG_WRITE_BLOCK_CAP && d.L.need == (d.L.units + 255) / 256);
            CHECK(strcmp(d.L.label, "write_px<depth=16,planes=3,out=2,dst16=1,xs=0,ys=0,transfer=3,aligned=1>") == 0);
        }
    }
    // a 32-bit document is never saved at 8 bit (parent :3704); the sRGB output curve goes with Clip (parent :3648)
    {
        WriteParams p = tile(32, 3, 8, 64, 2, 0, 3, 64, 0);
        CHECK(decide(p, 32, 3, 8, AVIFGPU_OUT_YCBCR, AVIFGPU_CHROMA_444, 0).L.invalid);
        p = tile(32, 3, 10, 64, 2, 0, 3, 128, 0);
        set_icc(p, "icc 4");
        CHECK(decide(p, 32, 3, 10, AVIFGPU_OUT_YCBCR, AVIFGPU_CHROMA_444, 0).L.invalid);      // transfer PQ
        p.transfer = AVIFGPU_TRANSFER_CLIP;
        CHECK(!decide(p, 32, 3, 10, AVIFGPU_OUT_YCBCR, AVIFGPU_CHROMA_444, 0).L.invalid);
    }
    // an empty tile launches nothing, whoever would have taken it (parent :3555 and every `if (spans == 0) return hipSuccess`)
    {
        const WriteParams p = tile(32, 3, 10, 64, 0, 0, 3, 128, 0);
        CHECK(decide(p, 32, 3, 10, AVIFGPU_OUT_YCBCR, AVIFGPU_CHROMA_444, word).L.kernel == kWkEmpty);
        CHECK(decide(p, 32, 3, 10, AVIFGPU_OUT_YCBCR, AVIFGPU_CHROMA_444, 0).L.kernel == kWkEmpty);
    }
}

int main(int argc, char** argv)
{
    if (argc != 2) { fprintf(stderr, "usage: write_dispatch_check CASES.tsv\n"); return 2; }
    const long long n = replay(argv[1]);
    by_hand();
    printf("write_dispatch_check: %lld recorded cases, %lld checks passed\n", n, g_checks);
    return 0;
}
