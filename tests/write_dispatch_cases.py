"""What tests/golden/make_write_dispatch_labels.py records and tests/test_zzzzzzz_gpu_write_dispatch.py replays: one save per CASE, a dict
of everything the write launcher reads --
    depth, planes, bit_depth, transfer, peak, alpha, output, chroma, nearest, pq    the descriptor
    icc                     the ICC kind by name (ICC_KINDS)
    word                    the tuning word
    w, rows                 the tile (the image is the tile: row0 = 0, height = rows)
    src, ss                 byte offset of the source from a 256-byte-aligned base, its row stride
    d[4], ds[4]             the same per plane; None / 0 for a plane the descriptor does not write
-- issued on device pointers into one arena, nothing but the label looked at.  The ICC structures are built by hand (no profile, no
lcms2): the launcher reads what fill_icc_params makes of them, not their curves."""
import functools
import gzip
import json
import os
import sys

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))      # (run as a program: the repository's root)

import harness  # noqa: E402
import icc32_programs as progs  # noqa: E402

pkg = harness.pkg

REF, YCC = pkg.OUT_REFERENCE, pkg.OUT_YCBCR
C420, C422, C444 = pkg.CHROMA_420, pkg.CHROMA_422, pkg.CHROMA_444
PQ, HLG, S428, CLIP = pkg.TRANSFER_PQ, pkg.TRANSFER_HLG, pkg.TRANSFER_SMPTE428, pkg.TRANSFER_CLIP
DEFAULT_WORD = 1 | 2 | 4
CAP1 = 1 << 8

# name -> the depth of the documents it goes with
ICC_KINDS = {"none": None, "icc 1": 32, "icc 2": 32, "icc 2 mixed": 32, "icc 4": 32, "icc 4 curved": 32, "sampled": 32, "sampled lds": 32,
             "pipeline32": 32, "pipeline32 lds": 32, "shaper8": 8, "clut8-table": 8, "clut16": 16}
SRGB_INVERSE = [2.4, 1 / 1.055, 0.055 / 1.055, 1 / 12.92, 0.04045, 0.04045 / 12.92, 1 / 2.4, 0.0]


def _transform(gammas, out_curve):
    t = pkg.IccTransform()
    for c in range(3):
        t.trc_type[c] = 1
        t.trc_params[c][0] = gammas[c]
        t.matrix[4 * c] = 1.0
    t.out_curve = out_curve
    if out_curve:
        for k, v in enumerate(SRGB_INVERSE):
            t.out_params[k] = v
    return t


def _sampled(entries):
    t = pkg.IccSampled32()
    for c in range(3):
        t.base.matrix[4 * c] = 1.0
        t.entries[c] = entries
    return t


@functools.lru_cache(maxsize=None)
def icc_of(kind):
    """The icc argument of AvifGpu.write_rows for an ICC kind (kept alive: the library caches by address and content)."""
    if kind == "none":
        return None
    if kind == "icc 1":
        return _transform((1.0, 1.0, 1.0), 0)
    if kind == "icc 2":
        return _transform((2.2, 2.2, 2.2), 0)                       # one simple curve for R, G, B: icc_same_simple
    if kind == "icc 2 mixed":
        return _transform((2.2, 1.8, 2.2), 0)                       # not the same curve: the generic kernel's icc = 2
    if kind == "icc 4":
        return _transform((1.0, 1.0, 1.0), 4)
    if kind == "icc 4 curved":
        return _transform((2.2, 2.2, 2.2), 4)
    if kind == "sampled":
        return _sampled(0)                                          # no table of the profile's own: curve[] in memory
    if kind == "sampled lds":
        return _sampled(256)
    if kind == "pipeline32":
        return progs.stamp(progs.build([("matrix", progs.M_SMALL, None), progs.TAIL]))      # no words: nothing for LDS
    if kind == "pipeline32 lds":
        return progs.stamp(progs.build([("tables", [progs.seeded_table(256, 3 + c) for c in range(3)], 0), progs.TAIL]))
    if kind == "shaper8":
        return pkg.IccShaper8()
    if kind in ("clut8-table", "clut16"):
        t = pkg.IccClut16()
        t.grid_points = 33
        return t
    raise ValueError(kind)


def shifts(case):
    return harness.chroma_shift(case["chroma"]) if (case["output"] == YCC and case["planes"] >= 3) else (0, 0)


def desc_of(case):
    return pkg.WriteDesc(width=case["w"], height=case["rows"], depth=case["depth"], planes=case["planes"], bit_depth=case["bit_depth"],
                         transfer=case["transfer"], peak_nits=case["peak"], alpha_state=case["alpha"], output=case["output"],
                         chroma=case["chroma"], chroma_downsampling=case["nearest"], pq_evaluation=case["pq"])


def plane_rows(case, pl):
    ys = shifts(case)[1]
    return (case["rows"] + ys) >> ys if pl in (1, 2) else case["rows"]


def make_case(depth, planes, bit_depth, output=REF, chroma=C444, w=1024, rows=2, transfer=CLIP, icc="none", word=DEFAULT_WORD, alpha=None,
              nearest=0, pq=pkg.PQ_AUTO, peak=1000, src=0, src_pad=0, off=(0, 0, 0, 0), pad=(0, 0, 0, 0)):
    """A case with tight strides plus the pads, the planes at `off`."""
    if alpha is None:
        alpha = pkg.ALPHA_STRAIGHT if planes in (2, 4) else pkg.ALPHA_NONE
    if planes < 3:
        output, chroma = REF, C444
    c = dict(depth=depth, planes=planes, bit_depth=bit_depth, transfer=transfer if depth == 32 else CLIP, peak=peak, alpha=alpha,
             output=output, chroma=chroma, nearest=nearest, pq=pq, icc=icc, word=word, w=w, rows=rows, src=src,
             ss=w * planes * (depth // 8) + src_pad)
    ssz = 2 if bit_depth > 8 else 1
    used = harness.write_planes(desc_of(c))
    c["d"] = [off[pl] if pl in used else None for pl in range(4)]
    c["ds"] = [used[pl][0] * ssz + pad[pl] if pl in used else 0 for pl in range(4)]
    return c


class Arena:
    """One source and four plane buffers on the device, each on a 256-byte boundary, large enough for every small case."""
    BYTES = 1 << 20

    def __init__(self, gpu, nbytes=None):
        import torch
        self.torch, self.dev = torch, f"cuda:{gpu.device}"
        self.nbytes = nbytes or [self.BYTES] * 5
        self.bufs = [torch.zeros(n + 256, dtype=torch.uint8, device=self.dev) for n in self.nbytes]
        self.base = [(b.data_ptr() + 255) & ~255 for b in self.bufs]

    def pointers(self, case):
        """(src, [dst]) of a case, after checking that every byte the save may touch lies inside the arena."""
        need = case["src"] + case["ss"] * case["rows"]
        assert need <= self.nbytes[0], ("source", need)
        dst = []
        for pl in range(4):
            if case["d"][pl] is None:
                dst.append(None)
                continue
            need = case["d"][pl] + case["ds"][pl] * plane_rows(case, pl)
            assert need <= self.nbytes[1 + pl], ("plane", pl, need)
            dst.append(self.base[1 + pl] + case["d"][pl])
        return self.base[0] + case["src"], dst

    def sync(self):
        self.torch.cuda.synchronize(self.dev)


def run_case(gpu, arena, case, word):
    """The label of the case's save under `word`."""
    src, dst = arena.pointers(case)
    gpu.lib.avifgpu_set_hot_variant(word)
    try:
        gpu.write_rows(desc_of(case), 0, case["rows"], src, case["ss"], dst, case["ds"], mem=pkg.MEM_DEVICE, icc=icc_of(case["icc"]))
    finally:
        gpu.lib.avifgpu_set_hot_variant(DEFAULT_WORD)
    return gpu.last_kernel()


def big_pair():
    """write_rgb32_ycbcr_sub_hot takes two spans per wave from 32 768 whole spans on: a flat 4:2:2 tile one row short of that, and at it."""
    return [make_case(32, 3, 10, YCC, C422, w=512, rows=r, transfer=PQ) for r in (32767, 32768)]


def big_arena(gpu):
    c = big_pair()[1]
    return Arena(gpu, [c["ss"] * c["rows"]] + [max(c["ds"][pl] * c["rows"], 256) for pl in range(4)])


# ---- the fixture, and its cases as lines of tab-separated fields for tools/write_dispatch_check.cpp -------------------------------------
FIXTURE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "write_dispatch_labels.json.gz")
TSV_FIELDS = ("depth", "planes", "bit_depth", "transfer", "pq", "alpha", "output", "chroma", "nearest", "icc", "word", "w", "rows", "src", "ss")


def load_fixture(path=FIXTURE):
    """(the small cases, the pair at 512 x 32767 / 32768)"""
    with gzip.open(path, "rb") as f:
        d = json.loads(f.read().decode())
    return d["cases"], d["big"]


def write_tsv(cases, path):
    with open(path, "w") as f:
        for c in cases:
            row = [c[k] for k in TSV_FIELDS] + [-1 if v is None else v for v in c["d"]] + c["ds"] + [c["label"], c["label_cap"]]
            f.write("\t".join(str(v) for v in row) + "\n")


if __name__ == "__main__":
    small, big = load_fixture(sys.argv[1])
    write_tsv(small + big, sys.argv[2])
