"""The choice of write kernel (csrc/write_dispatch.h) on the CPU: tools/write_dispatch_check.cpp, built with the sanitizers, replays the
record of what the library chose before the choice lived in that header (tests/golden/write_dispatch_labels.json.gz) and the cases
no small launch reaches; and the record itself is counted -- from the fixture alone, with the rules restated here -- to hold, for
every launch candidate, a case that takes it and, for every clause of its rule, a case that fails that clause alone and lands elsewhere."""
import os
import re
import shutil
import subprocess

import write_dispatch_cases as wc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
pkg = wc.pkg
CASES, BIG = wc.load_fixture()


def test_decision_equals_the_record_under_sanitizers(tmp_path):
    cxx = shutil.which("g++") or shutil.which("c++")
    assert cxx, "a host C++ compiler is part of the toolchain this project builds with"
    exe, tsv = tmp_path / "write_dispatch_check", tmp_path / "cases.tsv"
    wc.write_tsv(CASES + BIG, str(tsv))
    # the sanitizer runtimes are linked into the program itself, so it runs as it is wherever it is started
    r = subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-DAG_WRITE_PART=1", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-static-libasan",
                        "-static-libubsan", os.path.join(ROOT, "tools", "write_dispatch_check.cpp"), "-o", str(exe)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr
    r = subprocess.run([str(exe), str(tsv)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    assert f"{len(CASES) + len(BIG)} recorded cases" in r.stdout and "checks passed" in r.stdout


def test_every_capped_label_shows_its_grid():
    for c in CASES + BIG:
        base = re.sub(r" cap=1/\d+", "", c["label_cap"])
        assert base == c["label"] and " cap=" not in c["label"], (c["label"], c["label_cap"])
    assert sum(" cap=1/" in c["label_cap"] for c in CASES) > 2000


# ---- the coverage of the record, counted from the record ---------------------------------------------------------------------------------
class Seen:
    """What the launcher sees of a case: the tile after the FLAT rule, the ICC kind after the word's bit 6."""

    def __init__(self, c):
        self.c = c
        self.depth, self.planes, self.out, self.word = c["depth"], c["planes"], c["output"], c["word"]
        self.dst16, self.maxv = c["bit_depth"] > 8, (1 << c["bit_depth"]) - 1
        self.xs, self.ys = wc.shifts(c)
        self.ycc = self.out == wc.YCC
        self.premul, self.nearest = c["alpha"] == pkg.ALPHA_PREMULTIPLIED, c["nearest"]
        self.clip = c["depth"] != 32 or c["transfer"] == wc.CLIP
        self.w, self.rows, self.src, self.ss = c["w"], c["rows"], c["src"], c["ss"]
        self.d, self.ds = [v or 0 for v in c["d"]], list(c["ds"])
        self.has = [v is not None for v in c["d"]]
        self.icc = c["icc"]
        self.stream = bool(self.word & 1)
        self.flat = self._flat()

    def _flat(self):
        h422 = self.xs == 1 and self.ys == 0 and self.w % 2 == 0 and self.ycc
        ssz, dsz = self.depth // 8, 2 if self.dst16 else 1
        self.flat_clauses = [
            ("word bit 0", self.stream), ("word bit 4 clear", not self.word & 16), ("more than one row", self.rows > 1), ("colour", self.planes >= 3),
            ("16- or 32-bit document", self.depth in (16, 32)), ("no vertical sub-sampling", self.ys == 0), ("4:4:4 or even-width 4:2:2", self.xs == 0 or h422),
            ("contiguous source", self.ss == self.w * self.planes * ssz),
            ("contiguous planes", self.ds[0] == self.w * self.planes * dsz if self.out == wc.REF else
             all(self.has[pl] and self.ds[pl] == (self.w // 2 if h422 and pl in (1, 2) else self.w) * dsz for pl in range(4 if self.planes == 4 else 3)))]
        if not all(ok for _, ok in self.flat_clauses):
            return False
        px = self.w * self.rows
        self.w, self.rows, self.ss = px, 1, px * self.planes * ssz
        for pl in range(4):
            if self.has[pl]:
                self.ds[pl] = (px * self.planes if self.out == wc.REF else (px // 2 if h422 and pl in (1, 2) else px)) * dsz
        return True

    def src_ok(self, mask):
        return (self.src | self.ss) & mask == 0

    def planes_ok(self, planes, mask):
        return all((self.d[pl] | self.ds[pl]) & mask == 0 for pl in planes)

    @property
    def trc(self):                                   # icc_trc_type[0] != 0
        return self.icc.startswith(("icc", "sampled", "pipeline32"))

    @property
    def stream_icc(self):                            # a stage the streaming kernels carry: 1, 4 (Clip), 2
        return self.icc in ("icc 1", "icc 2") or (self.icc == "icc 4" and self.clip)


def rules(s):
    """{candidate: (label pattern, [(clause, holds)])} in the launcher's order, restated from the rules of csrc/write_dispatch.h."""
    on = ("word bit 0", s.stream)
    ref, ycc = ("interleaved hand-off", s.out == wc.REF), ("Y, Cb, Cr planes", s.ycc)
    c444, sub = ("4:4:4", s.xs == 0 and s.ys == 0), ("4:2:2 / 4:2:0", s.xs == 1)
    w8 = ("whole 8-pixel groups", s.w % 8 == 0)
    no8 = ("no 8-bit shaper", s.icc != "shaper8")
    no8t = ("no 8-bit table profile", s.icc != "clut8-table")
    no16 = ("no 16-bit table", s.icc != "clut16")
    u8out, u16out = ("u8 planes", not s.dst16), ("u16 planes", s.dst16)
    d = lambda n: ("%d-bit document" % n, s.depth == n)                         # noqa: E731
    pl = lambda *n: ("planes in %s" % (n,), s.planes in n)                      # noqa: E731
    src = lambda m: ("source aligned to %d" % (m + 1), s.src_ok(m))             # noqa: E731
    dst = lambda p, m: ("planes %s aligned to %d" % (p, m + 1), s.planes_ok(p, m))      # noqa: E731
    no_icc = ("no ICC stage", not s.trc)
    R = {}
    R["copy"] = (r"^write_copy_rows_stream", [on, no8, no8t, d(8), u8out, ref, ("gray, RGB or straight RGBA", s.planes in (1, 3) or (s.planes == 4 and not s.premul)),
                 ("rows of whole dwords", s.w * s.planes % 4 == 0), src(3), dst((0,), 3)])
    R["int_ref"] = (r"^write_int_ref_stream", [on, no16, no8, no8t, ("16-bit document or RGBA8", s.depth == 16 or (s.depth == 8 and s.planes == 4)),
                    ("hand-off of a colour document, or Gray16", (s.planes >= 3 and s.out == wc.REF) or (s.planes == 1 and s.depth == 16)),
                    ("rows of whole 16-byte vectors", s.w * s.planes * (s.depth // 8) % 16 == 0), src(15), dst((0,), 15)])
    R["ga16"] = (r"^write_ga_stream<depth=16>", [on, d(16), pl(2), u16out, ("whole 4-pixel vectors", s.w % 4 == 0), src(3), dst((0, 3), 3)])
    R["rgb8"] = (r"^write_rgb8_ycbcr_hot", [on, no8, no8t, d(8), pl(3), u8out, ycc, w8, src(3), dst((0, 1, 2), 3)])
    R["rgb8_to16"] = (r"^write_rgb8_ycbcr16_hot", [on, no8, no8t, d(8), pl(3), u16out, ycc, w8, src(3), dst((0, 1, 2), 3)])
    R["rgba8"] = (r"^write_rgba8_ycbcra_hot", [on, no8, no8t, d(8), pl(4), u8out, ycc, w8, src(3), dst((0, 1, 2, 3), 3)])
    to8 = ("u16 planes or 8-bit planes", s.dst16 or s.maxv == 255)
    R["rgb16"] = (r"^write_rgb16_ycbcr444_hot", [on, no16, d(16), pl(3), to8, ycc, c444, w8, src(15), dst((0, 1, 2), 15)])
    R["rgba16"] = (r"^write_rgba16_ycbcra444_hot", [on, no16, d(16), pl(4), to8, ycc, c444, w8, src(15), dst((0, 1, 2, 3), 15)])
    R["rgba16_sub"] = (r"^write_rgba16_ycbcra_sub_hot", [on, no16, d(16), pl(4), to8, ycc, sub, w8, src(15), dst((0, 3), 15), dst((1, 2), 7)])
    R["rgb16_sub"] = (r"^write_rgb16_ycbcr_sub_hot", [on, no16, d(16), pl(3), to8, ycc, sub, w8, src(15), dst((0, 1, 2), 15)])
    R["ga32"] = (r"^write_ga_stream<depth=32", [on, d(32), pl(2), u16out, ("even width", s.w % 2 == 0), src(3), dst((0, 3), 3)])
    R["rgba32_sub"] = (r"^write_rgba32_ycbcra_sub_hot", [on, no_icc, d(32), pl(4), u16out, ycc, sub, src(3), dst((0, 1, 2, 3), 3)])
    R["rgba32"] = (r"^write_rgba32_ycbcra444_hot", [on, ("no ICC stage or a streaming one", not s.trc or s.stream_icc), d(32), pl(4), u16out, ycc, c444, src(15),
                   dst((0, 1, 2, 3), 15)])
    R["rgb32_sub"] = (r"^write_rgb32_ycbcr_sub_hot", [on, ("no ICC stage or a streaming one", not s.trc or s.stream_icc), d(32), pl(3), u16out, ycc, sub, src(3),
                      dst((0, 1, 2), 3)])
    R["rgb32_icc_ref"] = (r"^write_rgb32_icc1_ycbcr444_hot<transfer=\d,out=ref>", [on, ("a streaming ICC stage", s.stream_icc), d(32), pl(3), u16out, ref, src(3), dst((0,), 15)])
    R["f32_ref"] = (r"^write_f32_ref_stream", [on, no_icc, d(32), ("hand-off of a colour document, or gray", (s.planes >= 3 and s.out == wc.REF) or s.planes == 1), u16out,
                    ("rows of whole 4-sample vectors", s.w * s.planes % 4 == 0), src(15), dst((0,), 7)])
    R["rgb32_icc"] = (r"^write_rgb32_icc1_ycbcr444_hot<transfer=\d>", [on, ("a streaming ICC stage", s.stream_icc), d(32), pl(3), u16out, ycc, c444, src(3), dst((0, 1, 2), 3)])
    R["rgb32"] = (r"^write_rgb32_ycbcr444_hot", [on, no_icc, d(32), pl(3), u16out, ycc, c444, src(3), dst((0, 1, 2), 3)])
    return R


# Clauses the rules above do not restate, because no call can make them fail alone -- by name, with the reason.
NOT_RESTATED = {
    "p.dst[3] != nullptr (ga16, rgba8, rgba16, rgba16_sub, ga32, rgba32_sub, rgba32)": "check_write_buffers refuses a null plane the descriptor writes",
    "p.maxv == 255 / 1023 / 4095 (copy, rgb8, rgb8_to16, rgba8)": "fill_write_params derives maxv from bit_depth, which dst16 is derived from too",
    "width x rows >= AG_RGB16_MIN_PX / AG_RGBA16_MIN_PX, or word bit 3 (rgb16, rgba16)": "both gates are 0 in the product: always true",
    "p.icc_s_tab == nullptr (rgba32_sub)": "fill_icc_params sets icc_trc_type[0] with every sampled profile: 'no ICC stage' fails with it",
    "px < 2^29 (FLAT)": "a tile of 2^29 pixels: tools/write_dispatch_check.cpp, by hand",
    "units + 8 x 65536 x 4 < 0x7fffffff (every candidate)": "tiles of 2^31 work units: tools/write_dispatch_check.cpp, by hand",
    "AG_COPY8, AG_IREF8, AG_RGB8_HOT, AG_RGBA16_TO8, AG_ICC1_HOT, AG_ICC2_HOT, AG_ICC_FASTPOW, AG_RGBA_HOT_ENABLE, AG_FLAT": "compile-time switches, all on in the product",
}
# ... and the restated clauses that no case of the record fails alone, each with the reason: the count below demands exactly these
F32_CANDIDATES = ("ga32", "rgba32_sub", "rgba32", "rgb32_sub", "rgb32_icc_ref", "f32_ref", "rgb32_icc", "rgb32")
NOT_ALONE = {}
for _c in ("rgb16", "rgba16", "rgba16_sub", "rgb16_sub"):
    NOT_ALONE[(_c, "u16 planes or 8-bit planes")] = "always holds: planes that are not u16 are 8-bit (fill_write_params derives maxv from bit_depth)"
for _c in F32_CANDIDATES:
    NOT_ALONE[(_c, "u16 planes")] = "check_write refuses a 32-bit document saved at 8 bit"
for _c in ("rgba16_sub", "rgb16_sub", "rgba32_sub", "rgb32_sub"):
    NOT_ALONE[(_c, "Y, Cb, Cr planes")] = "the hand-off has no chroma shift (check_write): '4:2:2 / 4:2:0' fails with it"
for _c in ("rgb32_icc_ref", "rgb32_icc"):
    NOT_ALONE[(_c, "32-bit document")] = "fill_icc_params refuses the ICC transform of 32-bit documents at any other depth"
for _c in ("ga32", "rgba32_sub", "rgb32_sub", "rgb32_icc_ref", "rgb32_icc", "rgb32"):
    NOT_ALONE[(_c, "source aligned to 4")] = "floats off their natural alignment are not issued: the kernels load them as dwords"


def test_record_covers_every_candidate_and_every_clause():
    taken, failed_alone = {}, {}
    flat_taken, flat_failed = 0, {}
    for c in CASES + BIG:
        s = Seen(c)
        flat_taken += s.flat
        assert s.flat == (c["label"].endswith(" flat") and not c["label"].startswith("write_copy_rows_stream")), c
        bad = [n for n, ok in s.flat_clauses if not ok]
        if len(bad) == 1:
            flat_failed[bad[0]] = flat_failed.get(bad[0], 0) + 1
        first = None
        for name, (pattern, clauses) in rules(s).items():
            is_it = re.search(pattern, c["label"]) is not None
            bad = [n for n, ok in clauses if not ok]
            if not bad and first is None:
                first = name
                assert is_it, (name, c)                          # every clause holds and no earlier candidate took it: it is taken
                taken[name] = taken.get(name, 0) + 1
            elif len(bad) == 1 and not is_it:
                failed_alone[(name, bad[0])] = failed_alone.get((name, bad[0]), 0) + 1
            assert not (bad and is_it), (name, bad, c)           # a failed clause: never taken
        if first is None:
            assert c["label"].startswith("write_px<"), c
    s0 = Seen(CASES[0])
    missing = []
    for name, (_, clauses) in rules(s0).items():
        assert taken.get(name, 0) > 0, (name, "no case takes it")
        for n, _ in clauses:
            if failed_alone.get((name, n), 0) == 0:
                missing.append((name, n))
    assert sorted(missing) == sorted(NOT_ALONE), (sorted(set(missing) - set(NOT_ALONE)), sorted(set(NOT_ALONE) - set(missing)))
    assert flat_taken > 0
    # (FLAT's `ys == 0` never fails alone: 4:2:0 is not the even-width 4:2:2 the next clause asks for either)
    assert [n for n, _ in s0.flat_clauses if flat_failed.get(n, 0) == 0] == ["no vertical sub-sampling"]
    # the generic kernel: every ICC branch, aligned and not
    for icc in ("", ",icc=1", ",icc=2", ",icc=3", ",icc=4", ",icc=5", ",icc=6", ",icc=7", ",icc=8"):
        for aligned in (0, 1):
            assert any(re.search(r"^write_px<.*aligned=%d%s>" % (aligned, icc), c["label"]) for c in CASES), (icc, aligned)
    assert any(c["label"].endswith(",icc=6> lds") for c in CASES) and any(",icc=8> lds" in c["label"] for c in CASES)
    assert any(re.search(r",icc=6>( flat)?$", c["label"]) for c in CASES) and any(re.search(r",icc=8>( flat)?$", c["label"]) for c in CASES)
