"""The grid save on the GPU (include/avifgpu.h "grid save", csrc/grid_save_kernels.hip, the grid destination of csrc/pipeline.hip).

The definition is exact (tests/grid_save_truth.py): the tiles are split(pad(planes)) of the plain save.  For 8- and 16-bit documents the
planes are the oracle's; for 32-bit documents and behind an ICC stage they are the library's own plain save into planes whose base and
stride are multiples of 256 -- existing code that the existing suites hold to the oracle.  A grid save is never compared with a grid save.
Every comparison is array_equal on bytes.

Tiles are pre-filled with a sentinel, their strides differ from tile to tile and some bases are off the 16-byte grid; the sentinel must
survive in every stride tail, in front of every tile and behind it.

Shapes are the smallest at which the movers can go wrong: a lane of grid_scatter owns 16 bytes of a padded row and takes the one-word path
only where they lie inside one tile and inside the canvas, so tiles narrower than 16 bytes, seams off the 16-byte grid, pixels of 3 and 6
bytes, pad widths of 1 and of tile_width - 1, pure padding and more rows than grid.y holds are each a path of their own.

The file sorts behind every other test file, as the suite's other late additions do."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

import grid_save_truth as truth
import grid_truth
import harness
import icc32_programs as ip
import icc_profiles
from fake_host import FakeHost

pkg = harness.pkg
H = pkg.host
pytestmark = pytest.mark.gpu

SENTINEL = 0xA5
BAD = pkg.formatBadParameters


def ssz_of(desc):
    return 2 if desc.bit_depth > 8 else 1


class Tiles:
    """columns * rows tiles in ONE flat buffer: every tile plane starts at a 256-byte slot plus 0, 1 or 3 samples, has a stride of its
    own, and the whole buffer is the sentinel.  On the device the buffer is uploaded as it is, so every offset from the 16-byte grid stays."""

    def __init__(self, desc, grid, gpu=None, pinned=False):
        self.desc, self.grid, self.geo = desc, grid, truth.geometry(desc, grid)
        s = ssz_of(desc)
        self.where, at = {}, 0
        for k in range(grid[0] * grid[1]):
            for pl, (pw, ph, twp, thp, spp) in self.geo.items():
                rb = twp * spp * s
                stride = rb + (1 + (k * 5 + pl * 3) % 11) * s
                off = (0, 1, 3)[k % 3] * s
                self.where[(k, pl)] = (at + off, stride, rb, thp)
                at += harness.align(off + thp * stride + 16, 256)
        self.size = at
        self.dev = None
        if gpu is not None:
            import torch
            self.dev = f"cuda:{gpu.device}"
            self.data = torch.full((at,), SENTINEL, dtype=torch.uint8, device=self.dev)
            base = self.data.data_ptr()
            assert base % 256 == 0
        elif pinned:
            import torch
            self.keep = torch.full((at,), SENTINEL, dtype=torch.uint8).pin_memory()
            self.flat = self.keep.numpy()
            base = self.flat.ctypes.data
        else:
            self.flat = np.full((at + 256,), SENTINEL, dtype=np.uint8)
            base = self.flat.ctypes.data + (-self.flat.ctypes.data) % 256
            self.flat = self.flat[base - self.flat.ctypes.data:][:at]
        self.table = (pkg.GridTile * (grid[0] * grid[1]))()
        for (k, pl), (o, stride, rb, thp) in self.where.items():
            self.table[k].plane[pl] = base + o
            self.table[k].stride[pl] = stride
        strides = {w[1] for (k, pl), w in self.where.items() if pl == 0}
        assert len(self.table) < 3 or (len(strides) > 1 and any((base + w[0]) % 16 for w in self.where.values()))
        if gpu is not None:
            import torch
            self.dtable = torch.from_numpy(np.frombuffer(bytes(self.table), dtype=np.uint8).copy()).to(self.dev)
            self.ptr = self.dtable.data_ptr()
        else:
            self.ptr = ctypes.addressof(self.table)

    def read(self):
        """[{plane: (th_p, tw_p * samples per pixel) array}] -- and every byte outside the tile rows is still the sentinel"""
        flat = self.data.cpu().numpy() if self.dev else self.flat
        dt = np.uint16 if ssz_of(self.desc) == 2 else np.uint8
        mask = np.ones(flat.shape, dtype=bool)
        out = [dict() for _ in range(self.grid[0] * self.grid[1])]
        for (k, pl), (o, stride, rb, thp) in self.where.items():
            rows = np.lib.stride_tricks.as_strided(flat[o:], shape=(thp, rb), strides=(stride, 1))
            out[k][pl] = np.ascontiguousarray(rows).view(dt)
            np.lib.stride_tricks.as_strided(mask[o:], shape=(thp, rb), strides=(stride, 1))[:] = False
        assert (flat[mask] == SENTINEL).all(), "bytes outside the tile rows were touched"
        return out


def same_tiles(got, want):
    for k, (g, w) in enumerate(zip(got, want)):
        assert set(g) == set(w)
        for pl in w:
            if not np.array_equal(g[pl], w[pl]):
                return False
    return True


def whole(desc):
    return [(0, desc.height)]


def grid_save(gpu, desc, grid, src, mem="device", cuts=None, icc=None, pinned=False):
    """the grid save of src as a list of tiles, rows cut as `cuts` says ([(row0, nrows)]); device: every call gets exactly the helper's
    scratch and a sentinel region behind it stays untouched"""
    cuts = cuts or whole(desc)
    if mem == "device":
        import torch
        dev = f"cuda:{gpu.device}"
        t = Tiles(desc, grid, gpu=gpu)
        d_src = torch.from_numpy(np.ascontiguousarray(src).view(np.uint8).reshape(-1)).to(dev)
        needs = [pkg.write_grid_scratch_bytes(desc, n) for _, n in cuts]
        scratch = torch.full((max(needs) + 4096 + 16,), 0x5A, dtype=torch.uint8, device=dev)
        stream = torch.cuda.current_stream(dev).cuda_stream
        for (r0, n), need in zip(cuts, needs):
            gpu.write_rows_grid(desc, grid, t.ptr, r0, n, d_src.data_ptr() + r0 * src.strides[0], src.strides[0], scratch.data_ptr() + 16, need,
                                mem=pkg.MEM_DEVICE, stream=stream, icc=icc)
        torch.cuda.synchronize(dev)
        assert bool((scratch[16 + max(needs):] == 0x5A).all()) and bool((scratch[:16] == 0x5A).all()), "bytes outside the scratch were touched"
        return t.read()
    t = Tiles(desc, grid, pinned=pinned)
    for r0, n in cuts:
        gpu.write_rows_grid(desc, grid, t.ptr, r0, n, src.ctypes.data + r0 * src.strides[0], src.strides[0], mem=pkg.MEM_HOST, icc=icc)
    return t.read()


def plain_save_256(gpu, desc, src, icc=None):
    """the library's plain save into device planes whose base and stride are multiples of 256, trimmed to the canvas"""
    import torch
    dev = f"cuda:{gpu.device}"
    s = ssz_of(desc)
    dt = np.uint16 if s == 2 else np.uint8
    bufs, ptrs, strides = {}, [None] * 4, [0] * 4
    for pl, (w, xs, ys) in harness.write_planes(desc).items():
        h = (desc.height + ys) >> ys
        pitch = harness.align(w * s, 256)
        bufs[pl] = (torch.full((h * pitch,), SENTINEL, dtype=torch.uint8, device=dev), h, w, pitch)
        assert bufs[pl][0].data_ptr() % 256 == 0
        ptrs[pl], strides[pl] = bufs[pl][0].data_ptr(), pitch
    d_src = torch.from_numpy(np.ascontiguousarray(src).view(np.uint8).reshape(-1)).to(dev)
    gpu.write_rows(desc, 0, desc.height, d_src.data_ptr(), src.strides[0], ptrs, strides, mem=pkg.MEM_DEVICE,
                   stream=torch.cuda.current_stream(dev).cuda_stream, icc=icc)
    torch.cuda.synchronize(dev)
    return {pl: np.ascontiguousarray(b.cpu().numpy().reshape(h, pitch)[:, :w * s]).view(dt) for pl, (b, h, w, pitch) in bufs.items()}


_truths = {}


def case(gpu, name, kw, grid, icc=None, seed=7):
    """(desc, src, the tiles the definition gives), computed once per case and shared"""
    key = (name, grid, id(icc))
    if key not in _truths:
        desc = pkg.WriteDesc(**kw)
        pkg.write_grid_check(desc, grid)
        src = harness.make_write_source(desc, seed=seed)
        if icc is not None:
            src = np.abs(src)
        exact = desc.depth != 32 and icc is None
        planes = harness.oracle_write(desc, src) if exact else plain_save_256(gpu, desc, src, icc)
        want = truth.tiles_of(planes, desc, grid)
        for t in want:
            for a in t.values():
                a.setflags(write=False)
        _truths[key] = (desc, src, want)
    return _truths[key]


YCC = dict(alpha_state=pkg.ALPHA_NONE, output=pkg.OUT_YCBCR, matrix_coefficients=pkg.MATRIX_BT709, planes=3)
REF = dict(output=pkg.OUT_REFERENCE)
PQ32 = dict(depth=32, transfer=pkg.TRANSFER_PQ, peak_nits=1000, matrix_coefficients=pkg.MATRIX_BT2020_NCL, color_primaries=pkg.PRIMARIES_BT2020)
SHAPES = [
    ("420-8-seams-inside-a-lane", dict(YCC, width=37, height=23, depth=8, bit_depth=8, chroma=pkg.CHROMA_420), (3, 2, 14, 12)),
    ("420-8-one-sample-chroma-tiles", dict(YCC, width=37, height=23, depth=8, bit_depth=8, chroma=pkg.CHROMA_420), (19, 12, 2, 2)),
    ("422-12", dict(YCC, width=70, height=41, depth=16, bit_depth=12, chroma=pkg.CHROMA_422), (3, 3, 32, 16)),
    ("444-10", dict(YCC, width=67, height=45, depth=16, bit_depth=10, chroma=pkg.CHROMA_444), (3, 3, 32, 16)),
    ("444-10-alpha-f32-pq", dict(YCC, **PQ32, width=67, height=45, bit_depth=10, chroma=pkg.CHROMA_444, planes=4, alpha_state=pkg.ALPHA_STRAIGHT), (3, 3, 32, 16)),
    ("rgb8", dict(REF, width=37, height=23, depth=8, bit_depth=8, planes=3, alpha_state=pkg.ALPHA_NONE), (3, 2, 14, 12)),
    ("rgb10", dict(REF, width=37, height=23, depth=16, bit_depth=10, planes=3, alpha_state=pkg.ALPHA_NONE), (3, 2, 14, 12)),
    ("rgba16-to-8", dict(REF, width=37, height=23, depth=16, bit_depth=8, planes=4, alpha_state=pkg.ALPHA_PREMULTIPLIED), (5, 3, 9, 8)),
    ("rgba12", dict(REF, width=37, height=23, depth=16, bit_depth=12, planes=4, alpha_state=pkg.ALPHA_STRAIGHT), (3, 2, 14, 12)),
    ("gray-alpha-12", dict(REF, width=77, height=33, depth=8, bit_depth=12, planes=2, alpha_state=pkg.ALPHA_STRAIGHT), (3, 2, 32, 20)),
    ("one-tile-larger-than-the-canvas", dict(YCC, width=21, height=9, depth=8, bit_depth=8, chroma=pkg.CHROMA_420), (1, 1, 39, 23)),
    ("pad-width-1", dict(YCC, width=31, height=9, depth=8, bit_depth=8, chroma=pkg.CHROMA_444), (2, 2, 16, 5)),
    ("pad-width-tile-minus-1", dict(YCC, width=17, height=6, depth=8, bit_depth=8, chroma=pkg.CHROMA_444), (2, 1, 16, 6)),
]
IDS = [s[0] for s in SHAPES]


# ---- 1. the kernel alone ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("B", [1, 2, 3, 4, 6, 8])
def test_scatter_alone_against_numpy(gpu, B):
    """one plane of pixels of B bytes through avifgpu_probe_grid_scatter, every row cut: tiles narrower and wider than a lane's 16 bytes, a
    padded row of more than one workgroup, a source at any address"""
    import torch
    dev = f"cuda:{gpu.device}"
    rng = np.random.default_rng(B)
    n = 0
    for pw, ph, cols, rows, tw, th in ((37, 23, 3, 2, 14, 12), (37, 23, 19, 12, 2, 2), (5, 3, 1, 1, 9, 7), (31, 9, 2, 2, 16, 5), (17, 6, 2, 1, 16, 6),
                                       (4200 // B + 3, 5, 3, 2, (4200 // B + 3) // 3 + 2, 3)):
        P = rng.integers(0, 256, size=(ph, pw, B), dtype=np.uint8)
        Q = P[np.minimum(np.arange(rows * th), ph - 1)][:, np.minimum(np.arange(cols * tw), pw - 1)]
        pitch = pw * B + (6 if B % 2 == 0 else 5)                # 16-bit pixel sizes: an even row distance, as the header asks
        flat = np.full((ph * pitch + 3,), 0x3C, dtype=np.uint8)
        srcv = np.lib.stride_tricks.as_strided(flat[2 if B % 2 == 0 else 3:], shape=(ph, pw * B), strides=(pitch, 1))
        srcv[:] = P.reshape(ph, pw * B)
        d_src = torch.from_numpy(flat).to(dev)
        src0 = d_src.data_ptr() + (2 if B % 2 == 0 else 3)
        # the tiles hold B-byte pixels: lay them out as a gray plane of tw * B / s samples of s bytes, so that 16-bit pixel sizes get the
        # natural alignment their samples have
        s = 2 if B % 2 == 0 else 1
        d = pkg.WriteDesc(width=pw, height=ph, depth=8 * s, bit_depth=8 if s == 1 else 12, planes=1, alpha_state=pkg.ALPHA_NONE, output=pkg.OUT_REFERENCE)
        bands = [(y, 2) for y in range(0, ph - 2, 2)]
        last = bands[-1][0] + 2 if bands else 0
        bands.append((last, rows * th - last))                   # the band that ends the plane also writes the rows below it
        for cuts in ([(0, rows * th)], bands):
            t = Tiles(d, (cols, rows, tw * B // s, th), gpu=gpu)
            for y0, h in cuts:
                gpu.probe_grid_scatter(t.ptr, cols, 0, tw, th, B, pw, ph, y0, h, src0 + y0 * pitch, pitch, None)
            torch.cuda.synchronize(dev)
            got = t.read()
            for k in range(cols * rows):
                c, r = k % cols, k // cols
                want = Q[r * th:(r + 1) * th, c * tw:(c + 1) * tw].reshape(th, tw * B)
                assert np.array_equal(got[k][0].view(np.uint8), want), (B, pw, ph, cols, rows, tw, th, k, cuts)
            n += 1
    assert n == 12


# ---- 2. more rows than grid.y holds -------------------------------------------------------------------------------------------------------------
def test_scatter_row_wrap(gpu):
    import torch
    dev = f"cuda:{gpu.device}"
    rng = np.random.default_rng(65600)
    pw, ph, tw, th, cols, rows = 8, 65600, 4, 257, 2, 256
    assert rows * th > ph > 65535
    P = rng.integers(0, 256, size=(ph, pw), dtype=np.uint8)
    d_src = torch.from_numpy(P).to(dev)
    stride = 7
    d_tiles = torch.full((cols * rows * th * stride + 16,), SENTINEL, dtype=torch.uint8, device=dev)
    table = (pkg.GridTile * (cols * rows))()
    for k in range(cols * rows):
        table[k].plane[0] = d_tiles.data_ptr() + 1 + k * th * stride
        table[k].stride[0] = stride
    d_table = torch.from_numpy(np.frombuffer(bytes(table), dtype=np.uint8).copy()).to(dev)
    gpu.probe_grid_scatter(d_table.data_ptr(), cols, 0, tw, th, 1, pw, ph, 0, rows * th, d_src.data_ptr(), pw, None)
    torch.cuda.synchronize(dev)
    flat = d_tiles.cpu().numpy()
    got = flat[1:1 + cols * rows * th * stride].reshape(rows, cols, th, stride)
    assert flat[0] == SENTINEL and (flat[1 + cols * rows * th * stride:] == SENTINEL).all() and (got[..., tw:] == SENTINEL).all()
    Q = P[np.minimum(np.arange(rows * th), ph - 1)]
    want = Q.reshape(rows, th, cols, tw).transpose(0, 2, 1, 3)
    assert np.array_equal(got[..., :tw], want)


# ---- 3. the entry, every shape, both memory kinds -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,kw,grid", SHAPES, ids=IDS)
def test_entry_device_and_host(gpu, name, kw, grid):
    desc, src, want = case(gpu, name, kw, grid)
    assert same_tiles(grid_save(gpu, desc, grid, src), want), (name, "device")
    assert same_tiles(grid_save(gpu, desc, grid, src, mem="host"), want), (name, "host")


# ---- 4. row cuts ------------------------------------------------------------------------------------------------------------------------------------
def cuts_of(desc, step=None, steps=None):
    out, r = [], 0
    i = 0
    while r < desc.height:
        n = min(step if step else steps[i % len(steps)], desc.height - r)
        out.append((r, n))
        r += n
        i += 1
    return out


@pytest.mark.parametrize("name,kw,grid", [SHAPES[0], SHAPES[2], SHAPES[4], SHAPES[6], SHAPES[10]], ids=[IDS[i] for i in (0, 2, 4, 6, 10)])
def test_row_cuts_give_identical_tiles(gpu, name, kw, grid):
    desc, src, want = case(gpu, name, kw, grid)
    uneven = cuts_of(desc, steps=(6, 2, 14, 4, 10))              # crosses tile rows off their boundaries; even starts for 4:2:0
    assert len(uneven) > 1 or desc.height < 7
    for cuts in (cuts_of(desc, step=2), uneven):
        assert same_tiles(grid_save(gpu, desc, grid, src, cuts=cuts), want), (name, "device", cuts)
        assert same_tiles(grid_save(gpu, desc, grid, src, mem="host", cuts=cuts), want), (name, "host", cuts)


# ---- 5. memory kinds ----------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,kw,grid", [SHAPES[0], SHAPES[3], SHAPES[8]], ids=[IDS[i] for i in (0, 3, 8)])
def test_memory_kinds_give_identical_tiles(gpu, name, kw, grid):
    desc, src, want = case(gpu, name, kw, grid)
    try:
        for nctx in (1, 2):
            g = pkg.AvifGpu(devices=[gpu.device] * nctx)
            for pinned in (False, True):
                assert same_tiles(grid_save(g, desc, grid, src, mem="host", pinned=pinned), want), (name, nctx, pinned)
                assert same_tiles(grid_save(g, desc, grid, src, mem="host", pinned=pinned, cuts=cuts_of(desc, steps=(6, 2, 14))), want), (name, nctx, pinned, "cut")
            assert same_tiles(grid_save(g, desc, grid, src), want), (name, nctx, "device")
    finally:
        pkg.AvifGpu(gpu.device)                                  # the session's binding


# ---- 6. statistics see the canvas, never the padding ------------------------------------------------------------------------------------------------------
def test_statistics_equal_the_plain_saves(gpu):
    import torch
    dev = f"cuda:{gpu.device}"
    name, kw, grid = SHAPES[4]
    desc, src, want = case(gpu, name, kw, grid)
    tw, th = pkg.thumbnail_fit(desc, 16)
    nb = 1 << desc.bit_depth

    def host_arms():
        return np.zeros(nb, np.uint64), np.zeros(tw * th * desc.planes, np.uint64), np.zeros(pkg.SUMMARY_COUNTERS, np.uint32)

    def dev_arms():
        return (torch.zeros(nb, dtype=torch.int64, device=dev), torch.zeros(tw * th * desc.planes, dtype=torch.int64, device=dev),
                torch.zeros(pkg.SUMMARY_COUNTERS, dtype=torch.int32, device=dev))

    def armed(arms, mem, fn):
        with pkg.code_histogram(arms[0], desc.bit_depth, mem), pkg.thumbnail_sums(arms[1], tw, th, mem), pkg.plane_summary(arms[2], mem):
            out = fn()
        torch.cuda.synchronize(dev)
        return out

    plain_h, plain_d, grid_h, grid_d = host_arms(), dev_arms(), host_arms(), dev_arms()
    armed(plain_h, pkg.MEM_HOST, lambda: harness.gpu_write(gpu, desc, src, mem="host"))
    armed(plain_d, pkg.MEM_DEVICE, lambda: plain_save_256(gpu, desc, src))
    assert plain_h[0].any() and plain_h[1].any() and plain_h[2].any()
    got = armed(grid_h, pkg.MEM_HOST, lambda: grid_save(gpu, desc, grid, src, mem="host", cuts=cuts_of(desc, steps=(6, 2, 14))))
    assert same_tiles(got, want)
    got = armed(grid_d, pkg.MEM_DEVICE, lambda: grid_save(gpu, desc, grid, src, cuts=cuts_of(desc, steps=(6, 2, 14))))
    assert same_tiles(got, want)
    for k in range(3):
        assert np.array_equal(grid_h[k], plain_h[k]), ("host", k)
        assert np.array_equal(grid_d[k].cpu().numpy(), plain_d[k].cpu().numpy()), ("device", k)


# ---- 7. one ICC stage of each kind ----------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def icc_tables(gpu):
    icc = icc_profiles.profile_bytes("adobergb-gamma2.2")
    t = {"transform": (32, icc_profiles.prepared("adobergb-gamma2.2", icc_profiles.REC2020)),
         "sampled": (32, icc_profiles.prepared("p3-sampled-srgb-1024", icc_profiles.REC2020)),
         "shaper8": (8, gpu.icc_prepare_shaper8(icc)),
         "clut16": (16, gpu.icc_prepare_clut16(icc)),
         "pipeline32": (32, ip.stamp(ip.build(ip.tier_a_programs()["clut 9x9x9"][0])))}
    t["clut8_table"] = (8, type(t["clut16"][1]).from_buffer_copy(t["clut16"][1]))
    return t


@pytest.mark.parametrize("kind", ["transform", "sampled", "shaper8", "clut16", "clut8_table", "pipeline32"])
def test_icc_stage_of_each_kind(gpu, icc_tables, kind):
    depth, table = icc_tables[kind]
    want_kind = getattr(pkg, "ICC_KIND_" + kind.upper())
    kw = dict(REF, width=67, height=21, depth=depth, bit_depth=8 if depth == 8 else 12, planes=3, alpha_state=pkg.ALPHA_NONE)
    if depth == 32:
        kw.update(transfer=pkg.TRANSFER_CLIP, peak_nits=1000)
    grid = (3, 2, 24, 12)
    desc, src, want = case(gpu, "icc-" + kind, kw, grid, icc=table)
    assert pkg.icc_kind_of(table, desc) == want_kind
    if depth != 32:
        assert not same_tiles(want, case(gpu, "icc-none-" + kind, kw, grid)[2]), "the ICC stage changes nothing: the case shows nothing"
    assert same_tiles(grid_save(gpu, desc, grid, src, icc=table), want), (kind, "device")
    assert same_tiles(grid_save(gpu, desc, grid, src, mem="host", icc=table, cuts=cuts_of(desc, steps=(6, 2, 14))), want), (kind, "host")


# ---- 8. round trip with the grid open -----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,kw,grid", [SHAPES[0], SHAPES[2]], ids=[IDS[0], IDS[2]])
def test_round_trip_with_the_grid_open(gpu, name, kw, grid):
    """grid save, then avifgpu_read_rows_grid of those tiles == plain save, then avifgpu_read_rows, on the canvas"""
    desc, src, want = case(gpu, name, kw, grid)
    rd = pkg.ReadDesc(width=desc.width, height=desc.height, colorspace=pkg.COLORSPACE_YCBCR, chroma=desc.chroma, bit_depth=desc.bit_depth, depth=desc.depth,
                      alpha_state=pkg.ALPHA_NONE, has_nclx=1, matrix_coefficients=desc.matrix_coefficients, color_primaries=pkg.PRIMARIES_BT709,
                      transfer_characteristics=13, full_range_flag=1)
    plain = harness.gpu_write(gpu, desc, src, mem="device", return_raw=True)
    expect = harness.gpu_read(gpu, rd, plain, mem="host")
    t = Tiles(desc, grid)
    gpu.write_rows_grid(desc, grid, t.ptr, 0, desc.height, src.ctypes.data, src.strides[0], mem=pkg.MEM_HOST)
    nch = harness.read_channels(rd)
    row_bytes = desc.width * nch * (desc.depth // 8)
    out = np.full((desc.height, harness.align(row_bytes, 16)), SENTINEL, dtype=np.uint8)
    gpu.read_rows_grid(rd, grid, t.table, None, pkg.UPSAMPLE_NEAREST, 1, 0, desc.height, out.ctypes.data, out.strides[0], mem=pkg.MEM_HOST)
    got = np.ascontiguousarray(out[:, :row_bytes]).view(harness.src_dtype(desc.depth)).reshape(np.asarray(expect).shape)
    assert np.array_equal(got, np.asarray(expect))


# ---- 9. the FormatRecord shim ----------------------------------------------------------------------------------------------------------------------------------------
def test_shim_saves_into_grid_tiles(gpu):
    kw = dict(YCC, width=64, height=48, depth=8, bit_depth=8, chroma=pkg.CHROMA_420, matrix_coefficients=pkg.MATRIX_BT601, chroma_downsampling=pkg.DOWNSAMPLE_NEAREST)
    grid = (2, 2, 34, 26)
    desc, src, want = case(gpu, "shim-420", kw, grid)
    entry = grid_save(gpu, desc, grid, src, mem="host")
    assert same_tiles(entry, want)

    def save(abort_after=None, g=grid, imgs=None):
        host = FakeHost(desc.width, desc.height, desc.depth, desc.planes, max_data=desc.width * 3 * 8, image=src, abort_after=abort_after)
        opts = H.SaveUIOptions(imageBitDepth=8, hdrTransferFunction=desc.transfer, pq=H.PQOptions(desc.peak_nits), chromaSubsampling=pkg.CHROMA_420, lossless=0)
        imgs = imgs if imgs is not None else (H.Image * (g[0] * g[1]))()
        code = gpu.lib.avifgpu_host_create_heif_image_grid(ctypes.byref(host.fr), desc.alpha_state, ctypes.byref(opts), pkg.OUT_YCBCR, pkg.MATRIX_BT601,
                                                           pkg.PRIMARIES_BT709, ctypes.byref(pkg.Grid(*g)), imgs)
        return host, imgs, code

    host, imgs, code = save()
    assert code == 0, gpu.lib.avifgpu_last_error()
    assert len(host.rects) == 6 and host.rects[0][0] == 0 and host.rects[-1][2] == desc.height and host.polls == len(host.rects)
    geo = truth.geometry(desc, grid)
    for k in range(4):
        assert (imgs[k].width, imgs[k].height, imgs[k].colorspace, imgs[k].chroma, imgs[k].bit_depth) == (34, 26, pkg.COLORSPACE_YCBCR, pkg.CHROMA_420, 8)
        for pl, (pw, ph, twp, thp, spp) in geo.items():
            rows = np.ctypeslib.as_array((ctypes.c_uint8 * (imgs[k].stride[pl] * thp)).from_address(imgs[k].plane[pl])).reshape(thp, imgs[k].stride[pl])
            assert np.array_equal(rows[:, :twp], entry[k][pl]), (k, pl)
        gpu.lib.avifgpu_image_free(ctypes.byref(imgs[k]))
    host, imgs, code = save(abort_after=3)                       # abortProc is honoured
    assert code == pkg.userCanceledErr and len(host.rects) == 3
    for k in range(4):
        gpu.lib.avifgpu_image_free(ctypes.byref(imgs[k]))
    host, imgs, code = save(g=(3, 2, 34, 26))                    # not minimal: nothing is requested from the host
    assert code == BAD and not host.rects and b"not minimal" in gpu.lib.avifgpu_last_error()
    # preset tiles are the caller's: a NULL plane or a short stride of one of them is refused before the host is asked for a row
    for defect, text in (("null", b"plane 1 of tile 2 is null"), ("thin", b"stride 16 of plane 2 of tile 3 < 17")):
        t = Tiles(desc, grid)
        preset = (H.Image * 4)()
        for k in range(4):
            for pl in range(3):
                preset[k].plane[pl] = t.table[k].plane[pl]
                preset[k].stride[pl] = t.table[k].stride[pl]
        if defect == "null":
            preset[2].plane[1] = None
        else:
            preset[3].stride[2] = 16
        host, imgs, code = save(imgs=preset)
        assert code == BAD and not host.rects and host.polls == 0 and text in gpu.lib.avifgpu_last_error(), (defect, gpu.lib.avifgpu_last_error())
        assert (t.flat == SENTINEL).all()
    # ... and good preset tiles are written in place
    t = Tiles(desc, grid)
    preset = (H.Image * 4)()
    for k in range(4):
        for pl in range(3):
            preset[k].plane[pl] = t.table[k].plane[pl]
            preset[k].stride[pl] = t.table[k].stride[pl]
    host, imgs, code = save(imgs=preset)
    assert code == 0 and same_tiles(t.read(), want) and all(not imgs[k].owner for k in range(4))


# ---- 10. the CLI --------------------------------------------------------------------------------------------------------------------------------------------------------
def test_cli_write_grid(gpu, tmp_path):
    cli = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "avif-format_amd", "avifgpu_cli")
    kw = dict(YCC, width=64, height=48, depth=8, bit_depth=8, chroma=pkg.CHROMA_420, matrix_coefficients=pkg.MATRIX_BT601, chroma_downsampling=pkg.DOWNSAMPLE_NEAREST)
    grid = (2, 2, 34, 26)
    desc, src, want = case(gpu, "shim-420", kw, grid)
    (tmp_path / "in.raw").write_bytes(src.tobytes())
    r = subprocess.run([cli, "write", "--width", "64", "--height", "48", "--depth", "8", "--planes", "3", "--bits", "8", "--ycbcr", "420",
                        "--grid", "2x2,34x26", "--maxdata", str(64 * 3 * 8), str(tmp_path / "in.raw"), str(tmp_path / "out.planes")], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    for k in range(4):
        blob = np.frombuffer((tmp_path / f"out.planes.tile{k}").read_bytes(), dtype=np.uint8)
        at = 0
        for pl in sorted(want[k]):
            n = want[k][pl].size
            assert np.array_equal(blob[at:at + n].reshape(want[k][pl].shape), want[k][pl]), (k, pl)
            at += n
        assert at == blob.size


# ---- 11. rejections leave the tiles untouched -------------------------------------------------------------------------------------------------------------------------------
def test_rejections_leave_the_tiles_untouched(gpu):
    import torch
    dev = f"cuda:{gpu.device}"
    name, kw, grid = SHAPES[0]
    desc, src, want = case(gpu, name, kw, grid)
    t = Tiles(desc, grid, gpu=gpu)
    d_src = torch.from_numpy(src.view(np.uint8).reshape(-1)).to(dev)
    need = pkg.write_grid_scratch_bytes(desc, desc.height)
    scratch = torch.zeros((need,), dtype=torch.uint8, device=dev)
    good = dict(grid=grid, tiles=t.ptr, r0=0, n=desc.height, sb=need, mem=pkg.MEM_DEVICE)
    for kw2 in (dict(grid=(3, 2, 13, 12)), dict(grid=(2, 2, 14, 12)), dict(grid=(4, 2, 14, 12)), dict(grid=(3, 3, 14, 12)), dict(tiles=None), dict(sb=need - 1),
                dict(r0=1, n=2), dict(r0=2, n=22), dict(mem=5)):
        a = dict(good); a.update(kw2)
        with pytest.raises(pkg.AvifGpuError) as e:
            gpu.write_rows_grid(desc, a["grid"], a["tiles"], a["r0"], a["n"], d_src.data_ptr(), src.strides[0], scratch.data_ptr(), a["sb"], mem=a["mem"])
        assert e.value.code == BAD, kw2
    torch.cuda.synchronize(dev)
    assert bool((t.data == SENTINEL).all()), "a rejected call wrote to a tile"
    th = Tiles(desc, grid)
    th.table[4].plane[1] = None
    with pytest.raises(pkg.AvifGpuError) as e:
        gpu.write_rows_grid(desc, grid, th.ptr, 0, desc.height, src.ctypes.data, src.strides[0], mem=pkg.MEM_HOST)
    assert e.value.code == BAD and (th.flat == SENTINEL).all()
