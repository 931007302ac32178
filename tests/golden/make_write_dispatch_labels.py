#!/usr/bin/env python3
"""Generates tests/golden/write_dispatch_labels.json.gz ON A GPU, from the library the package loads (AVIFGPU_LIB or the tree's): for
every case of cases() -- everything the write launcher reads, tests/write_dispatch_cases.py -- the label avifgpu_last_kernel_name()
returns for its save under the case's tuning word ("label") and under that word with a block cap of 1 ("label_cap", which ends in
" cap=1/M", M the launcher's one-trip grid).

Shapes: every document kind at one aligned shape (descriptors), and around one descriptor per launch candidate (geometry_bases) the
widths, rows, offsets and stride pads below, each moved alone; beyond those sets, rows rounded up to 16 bytes and offsets / pads of 1
and 2 bytes where every sample stays on its natural alignment -- without them no width clause and no dword-alignment clause of a rule
fails ALONE (tests/test_write_dispatch.py counts that).  One pair of 512 x 32767 / 32768 tiles for the two-spans-per-wave rule.

The committed fixture was recorded from the build BEFORE the choice of kernel moved to csrc/write_dispatch.h;
tools/write_dispatch_check.cpp (CPU) and tests/test_zzzzzzz_gpu_write_dispatch.py hold the launcher to it.  Run it again only from a
build whose choices are meant to become the new record."""
import gzip
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "..", ".."))
sys.path.insert(0, os.path.join(HERE, ".."))

WIDTHS = (1, 2, 4, 6, 7, 8, 9, 24, 256, 257, 512, 520, 1024, 1032)
ROWS = (1, 2, 3)
OFFSETS = (4, 8, 16, 64)
PADS = (4, 16, 128)


def descriptors(wc):
    """Every document kind at one aligned shape: (depth, planes, bit_depth, output, chroma, transfer, icc, extra)."""
    out = []
    for depth, bits_of in ((8, (8, 10, 12)), (16, (8, 10, 12)), (32, (10, 12))):
        kinds = [k for k, d in wc.ICC_KINDS.items() if d in (None, depth)]
        for planes in (1, 2, 3, 4):
            for bits in bits_of:
                outs = [(wc.REF, wc.C444)] + ([(wc.YCC, c) for c in (wc.C444, wc.C422, wc.C420)] if planes >= 3 else [])
                for output, chroma in outs:
                    for icc in (kinds if planes >= 3 else ["none"]):
                        transfers = [wc.CLIP]
                        if depth == 32 and "4" not in icc.split():
                            transfers = [wc.PQ, wc.CLIP] if planes < 3 else [wc.PQ, wc.HLG, wc.S428, wc.CLIP]
                        for tr in transfers:
                            out.append(dict(depth=depth, planes=planes, bit_depth=bits, output=output, chroma=chroma, transfer=tr, icc=icc))
    return out


def geometry_bases(wc):
    """One descriptor per launch candidate (and per write_px ICC branch), the ones whose geometry is perturbed clause by clause."""
    D = wc.DEFAULT_WORD
    b = [dict(depth=8, planes=3, bit_depth=8), dict(depth=8, planes=1, bit_depth=8), dict(depth=8, planes=4, bit_depth=8),         # the copy
         dict(depth=8, planes=4, bit_depth=8, alpha=wc.pkg.ALPHA_PREMULTIPLIED), dict(depth=16, planes=3, bit_depth=12),            # the integer hand-off
         dict(depth=16, planes=1, bit_depth=10), dict(depth=16, planes=4, bit_depth=8),
         dict(depth=16, planes=2, bit_depth=12), dict(depth=32, planes=2, bit_depth=10, transfer=wc.PQ),                           # gray + alpha
         dict(depth=32, planes=1, bit_depth=10, transfer=wc.PQ), dict(depth=32, planes=3, bit_depth=12, transfer=wc.HLG),           # the f32 hand-off
         dict(depth=32, planes=4, bit_depth=10, transfer=wc.CLIP),
         dict(depth=32, planes=3, bit_depth=10, transfer=wc.PQ, icc="icc 1"), dict(depth=32, planes=3, bit_depth=10, transfer=wc.CLIP, icc="icc 4")]
    for chroma in (wc.C444, wc.C422, wc.C420):
        y = dict(output=wc.YCC, chroma=chroma)
        b += [dict(y, depth=8, planes=3, bit_depth=8), dict(y, depth=8, planes=3, bit_depth=10), dict(y, depth=8, planes=4, bit_depth=8),
              dict(y, depth=16, planes=3, bit_depth=12), dict(y, depth=16, planes=3, bit_depth=8), dict(y, depth=16, planes=4, bit_depth=12),
              dict(y, depth=16, planes=4, bit_depth=8), dict(y, depth=32, planes=3, bit_depth=10, transfer=wc.PQ),
              dict(y, depth=32, planes=4, bit_depth=10, transfer=wc.PQ), dict(y, depth=32, planes=3, bit_depth=12, transfer=wc.PQ, icc="icc 2"),
              dict(y, depth=32, planes=4, bit_depth=12, transfer=wc.CLIP, icc="icc 4")]
    # the generic kernel's own branches: the word's bit 0 off
    b += [dict(depth=8, planes=3, bit_depth=8, output=wc.YCC, chroma=wc.C420, icc="shaper8", word=0),
          dict(depth=8, planes=4, bit_depth=8, output=wc.YCC, chroma=wc.C422, icc="clut8-table", word=D),
          dict(depth=16, planes=3, bit_depth=12, output=wc.YCC, chroma=wc.C444, icc="clut16", word=D),
          dict(depth=32, planes=3, bit_depth=10, output=wc.YCC, chroma=wc.C420, transfer=wc.PQ, icc="pipeline32 lds", word=D),
          dict(depth=32, planes=4, bit_depth=10, output=wc.YCC, chroma=wc.C444, transfer=wc.PQ, icc="sampled lds", word=D),
          dict(depth=32, planes=3, bit_depth=10, output=wc.YCC, chroma=wc.C444, transfer=wc.CLIP, icc="icc 4", word=0),
          dict(depth=32, planes=3, bit_depth=10, output=wc.YCC, chroma=wc.C422, transfer=wc.PQ, icc="icc 1", word=0),
          dict(depth=32, planes=3, bit_depth=10, output=wc.YCC, chroma=wc.C420, transfer=wc.PQ, icc="icc 2 mixed", word=D),
          dict(depth=32, planes=3, bit_depth=10, output=wc.YCC, chroma=wc.C444, transfer=wc.PQ, word=0),
          dict(depth=16, planes=3, bit_depth=12, output=wc.YCC, chroma=wc.C420, word=0),
          dict(depth=8, planes=2, bit_depth=8, word=D)]
    return b


def cases(wc):
    D = wc.DEFAULT_WORD
    out = []
    for kw in descriptors(wc):
        out.append(wc.make_case(**kw))
        out.append(wc.make_case(**kw, src_pad=16, pad=(16, 16, 16, 16)))           # not FLAT
        if kw["planes"] in (2, 4):
            out.append(wc.make_case(**kw, alpha=wc.pkg.ALPHA_PREMULTIPLIED))
        if kw["output"] == wc.YCC and kw["chroma"] != wc.C444:
            out.append(wc.make_case(**kw, nearest=1, src_pad=16))
        if kw["depth"] == 32 and kw["transfer"] == wc.PQ:
            out.append(wc.make_case(**kw, pq=wc.pkg.PQ_COMPACT))
        out.append(wc.make_case(**kw, word=D & ~1))                                  # streaming kernels off
        if kw["icc"] in ("sampled lds", "pipeline32 lds"):
            out.append(wc.make_case(**kw, word=D | 64))                              # the tables stay in memory
    for kw in geometry_bases(wc):
        word = kw.get("word", D)
        ssz, dsz = kw["depth"] // 8, 2 if kw["bit_depth"] > 8 else 1
        for w in WIDTHS:
            for rows in ROWS:
                out.append(wc.make_case(**dict(kw, w=w, rows=rows)))
                out.append(wc.make_case(**dict(kw, w=w, rows=rows, src_pad=16, pad=(16, 16, 16, 16))))
                # rows rounded up to 16 bytes, as a caller with aligned rows has them: what a width clause fails ALONE on
                tight = wc.make_case(**dict(kw, w=w, rows=rows))
                out.append(wc.make_case(**dict(kw, w=w, rows=rows, src_pad=-tight["ss"] % 16, pad=tuple(-v % 16 for v in tight["ds"]))))
        # below the issue's offsets and pads, as far as a sample stays on its natural alignment: what a dword clause fails alone on
        for o in (1, 2):
            k = dict(kw, w=1024)
            if o % ssz == 0:
                out += [wc.make_case(**k, src=o), wc.make_case(**k, src=o, src_pad=128, pad=(128, 128, 128, 128)),
                        wc.make_case(**k, src_pad=o), wc.make_case(**k, src_pad=128 + o, pad=(128, 128, 128, 128))]
            if o % dsz == 0:
                for pl in range(4):
                    off, pad = tuple(o if i == pl else 0 for i in range(4)), tuple(128 + o if i == pl else 128 for i in range(4))
                    out += [wc.make_case(**k, off=off), wc.make_case(**k, off=off, src_pad=128, pad=(128, 128, 128, 128)),
                            wc.make_case(**k, pad=tuple(o if i == pl else 0 for i in range(4))), wc.make_case(**k, src_pad=128, pad=pad)]
        for w in (1024, 512):
            k = dict(kw, w=w)
            out += [wc.make_case(**dict(k, word=word | 16)), wc.make_case(**dict(k, word=word & ~2)), wc.make_case(**dict(k, word=word & ~4)),
                    wc.make_case(**dict(k, word=word | 8))]
            for o in OFFSETS:
                out.append(wc.make_case(**k, src=o))
                out.append(wc.make_case(**k, src=o, src_pad=128, pad=(128, 128, 128, 128)))
                for pl in range(4):
                    off = tuple(o if i == pl else 0 for i in range(4))
                    out.append(wc.make_case(**k, off=off))
                    out.append(wc.make_case(**k, off=off, src_pad=128, pad=(128, 128, 128, 128)))
            for p in PADS:
                out.append(wc.make_case(**k, src_pad=p))
                out.append(wc.make_case(**k, src_pad=p, pad=(128, 128, 128, 128)))
                for pl in range(4):
                    pad = tuple(p if i == pl else 0 for i in range(4))
                    out.append(wc.make_case(**k, pad=pad))
                    out.append(wc.make_case(**k, src_pad=128, pad=tuple(p if i == pl else 128 for i in range(4))))
            # every plane on a 128-byte line or not: the headline kernel's two workgroup shapes
            out += [wc.make_case(**k, rows=3, src_pad=128, pad=(128, 128, 128, 128)), wc.make_case(**k, rows=1, src=64), wc.make_case(**k, rows=1, off=(0, 64, 0, 0))]
    seen, uniq = set(), []
    for c in out:                                                                     # (a perturbation of a plane the descriptor does not write changes nothing)
        key = json.dumps(c, sort_keys=True)
        if key not in seen:
            seen.add(key)
            uniq.append(c)
    return uniq


def main():
    import write_dispatch_cases as wc
    gpu = wc.pkg.AvifGpu(0)
    arena = wc.Arena(gpu)
    todo = cases(wc)
    for c in todo:
        c["label"] = wc.run_case(gpu, arena, c, c["word"])
        c["label_cap"] = wc.run_case(gpu, arena, c, c["word"] | wc.CAP1)
    arena.sync()
    del arena
    big = wc.big_arena(gpu)
    pair = wc.big_pair()
    for c in pair:
        c["label"] = wc.run_case(gpu, big, c, c["word"])
        c["label_cap"] = wc.run_case(gpu, big, c, c["word"] | wc.CAP1)
    big.sync()
    path = os.path.join(HERE, "write_dispatch_labels.json.gz")
    with open(path, "wb") as f, gzip.GzipFile(fileobj=f, mode="wb", mtime=0) as z:
        z.write(json.dumps({"cases": todo, "big": pair}, separators=(",", ":")).encode())
    kernels = sorted({c["label"].split("<")[0].split(" ")[0] for c in todo + pair})
    print("written", len(todo), "+", len(pair), "cases,", os.path.getsize(path), "bytes, from", wc.pkg.LIB_PATH)
    print("kernels:", " ".join(kernels))


if __name__ == "__main__":
    main()
