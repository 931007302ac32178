// icc_tables_check -- checks the parts of the ICC device-table cache that make no HIP call (avif-format_amd/csrc/icc_tables.h) on the host:
// the node-pair tables of a seeded 33^3 table against a direct restatement, entry by entry; the staleness decision on its full truth
// table; what table_fingerprint reads and what it does not.  A stand-alone program with its own main, meant to be built with the
// sanitizers and run on the CPU (no device, no HIP):
//   g++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all tools/icc_tables_check.cpp -o icc_tables_check && ./icc_tables_check
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../avif-format_amd/csrc/icc_tables.h"

using namespace avifgpu;

static long long g_checks = 0;
#define CHECK(cond) do { ++g_checks; if (!(cond)) { fprintf(stderr, "icc_tables_check: %s:%d: %s\n", __FILE__, __LINE__, #cond); exit(1); } } while (0)

static uint32_t g_rng = 20261020u;
static uint32_t rnd() { g_rng ^= g_rng << 13; g_rng ^= g_rng >> 17; g_rng ^= g_rng << 5; return g_rng; }

// ---- the node-pair tables (layout 2) ----------------------------------------------------------------------------------------------------------
static void check_pair_tables()
{
#if AG_ICC16_DOT2 == 2
    constexpr int G = AVIFGPU_ICC_CLUT_GRID;
    static_assert(kIcc16DeviceBytes == kIcc16PairTablesBytes, "layout 2 is the node-pair tables");
    CHECK(kIcc16PairTablesBytes == (uint32_t)G * G * G * 12u + ((uint32_t)G * G * G + (uint32_t)G * G) * 3u * 12u);
    // exact-size heap buffers: one word too far is the sanitizer's
    std::vector<uint16_t> table((size_t)G * G * G * 4), out(kIcc16DeviceBytes / 2, 0);
    for (uint16_t& w : table) w = (uint16_t)(rnd() | 1u);        // no node word is 0: a zero in the image is a node beyond the grid
    icc16_device_image(reinterpret_cast<const uint16_t (*)[4]>(table.data()), out.data());
    auto node = [&](int r, int g, int b, int ch) -> uint16_t {
        return (r < G && g < G && b < G) ? table[(((size_t)r * G + g) * G + b) * 4 + ch] : 0;
    };
    const uint16_t* A = out.data();
    const uint16_t* B = out.data() + (size_t)G * G * G * 6;
    const int e[3][3] = { { 1, 0, 0 }, { 0, 1, 0 }, { 0, 0, 1 } };
    for (int r = 0; r < G; ++r) for (int g = 0; g < G; ++g) for (int b = 0; b < G; ++b) {
        const size_t n = ((size_t)r * G + g) * G + b;
        for (int ch = 0; ch < 3; ++ch) {
            CHECK(A[6 * n + 2 * ch] == node(r, g, b, ch) && A[6 * n + 2 * ch + 1] == node(r + 1, g + 1, b + 1, ch));
            for (int k = 0; k < 3; ++k)
                CHECK(B[6 * (3 * n + k) + 2 * ch] == node(r, g, b, ch) && B[6 * (3 * n + k) + 2 * ch + 1] == node(r + e[k][0], g + e[k][1], b + e[k][2], ch));
        }
    }
    // table B runs one slab past the last node (m = n + stride(amax), kernel_params.h): zeros, up to the last byte of the image
    for (size_t i = (size_t)G * G * G * 6 * 4; i < out.size(); ++i) CHECK(out[i] == 0);
    CHECK(out.size() * 2 == kIcc16PairTablesBytes);
#endif
}

// ---- the staleness decision: same or other address, fingerprint, epoch and size, under both policies ------------------------------------------------
static void check_staleness()
{
    static const char here = 0, there = 0;
    const IccStamp rec = { &here, 77, 5, 1000 };
    for (int m = 0; m < 16; ++m) {
        IccStamp call = rec;
        if (m & 1) call.src = &there;
        if (m & 2) call.fp = 78;
        if (m & 4) call.epoch = 6;
        if (m & 8) call.size = 1004;
        const IccStale once = icc_staleness(rec, call, IccVerify::OncePerEpoch), every = icc_staleness(rec, call, IccVerify::EveryCall);
        CHECK(once == ((m & 8) ? IccStale::Upload : m == 0 ? IccStale::Trusted : IccStale::CompareBytes));
        CHECK(every == ((m & 8) ? IccStale::Upload : IccStale::CompareBytes));   // never trusted, whatever matches
    }
    // a record that has never been uploaded: no image is empty
    const IccStamp fresh;
    IccStamp call = { &here, 1, 1, 2048 };
    CHECK(icc_staleness(fresh, call, IccVerify::OncePerEpoch) == IccStale::Upload && icc_staleness(fresh, call, IccVerify::EveryCall) == IccStale::Upload);
}

// ---- the fingerprint: a sampled word changes it, an unsampled one does not (what the epoch tests rely on) ----------------------------------------
static void check_fingerprint_of(size_t bytes)
{
    const size_t n = bytes / 4, step = n / 4096 ? n / 4096 : 1;
    std::vector<uint32_t> w(n);                                  // exact size; n == 0: data() may be null and is not read
    for (uint32_t& x : w) x = rnd();
    const uint64_t h = table_fingerprint(w.data(), bytes);
    CHECK(h == table_fingerprint(w.data(), bytes));
    if (bytes >= 4) CHECK(h != table_fingerprint(w.data(), bytes - 4));              // the size is part of it
    size_t sampled = 0;
    for (size_t i = 0; i < n; ++i) {
        const bool read = i % step == 0 || i == n - 1;
        sampled += read;
        if (!read && n > 3 * 4096 && i > 64 && rnd() % 32) continue;                // the large tables: every word read, a 32nd of the others
        w[i] ^= 0x4000u;
        CHECK((table_fingerprint(w.data(), bytes) != h) == read);
        w[i] ^= 0x4000u;
    }
    CHECK(sampled == (n ? (n - 1) / step + 1 + ((n - 1) % step != 0) : 0));
    if (step > 1) CHECK(sampled < n);
}

static void check_fingerprint()
{
    CHECK(table_fingerprint(nullptr, 0) == table_fingerprint(nullptr, 0));
    const size_t sizes[] = { 0, 4, 4096 * 4 - 4, 4096 * 4, 4096 * 4 + 4, 8192 * 4 - 4, 8192 * 4, 8192 * 4 + 4,
                             sizeof(avifgpu_icc_clut16::table),                      // stride 17: word 1 is not read (tests/test_icc16.py)
                             sizeof(avifgpu_icc_sampled32::curve) + sizeof(avifgpu_icc_sampled32::table16) };   // stride 49
    for (size_t s : sizes) check_fingerprint_of(s);
    CHECK(sizeof(avifgpu_icc_clut16::table) / 4 / 4096 == 17);
    CHECK((sizeof(avifgpu_icc_sampled32::curve) + sizeof(avifgpu_icc_sampled32::table16)) / 4 / 4096 == 49);
}

int main()
{
    check_pair_tables();
    check_staleness();
    check_fingerprint();
    printf("icc_tables_check: ok, %lld checks\n", g_checks);
    return 0;
}
