"""The batch calls' memory contract on the device at hostile layouts (tests/layouts.py; the same families run on the CPU wave emulator
in tests/test_emu_layout.py): exact slots -- kmp_zstd_compress_bound(len) + 8, kmp_deflate_bound(len), kmp_deflate_bound_params(...),
d_out_cap equal to the content size -- with canary gaps of 1 .. 63 bytes, slot and slice starts on every residue modulo 64 in permuted
order; slices whose surroundings tempt a compare to leave them; aliased, overlapping and empty entries; every layout twice with
complementary filler.  Through the C ABI with dst= / out_off= of the existing ZstdBatch methods: the real launch code (chunks, pieces,
team strides, the XCD-aware mapping, the 64 KiB spans of DEFLATE).  Every frame against the oracle / zlib, every byte outside the
entries against the canary; bit-exact, no tolerance.  Nothing here asks for memory outside its tensors, retries, or is made to fault."""
import struct

import numpy as np
import pytest

import helpers
import layouts as LY
from layouts import SIZES, EDGES, NONEMPTY, BODIES, with_large, families, n_entries, zlib_ref

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

FAMILIES = ("exact", "tempting", "aliased")
FMT = ("raw", "zlib", "gzip", "auto")


def ctx(**kw):
    from kompressor_amd.batch import ZstdBatch
    assert torch.cuda.is_available(), "these tests need the MI355X"
    return ZstdBatch(**kw)


def dev(L):
    return (torch.from_numpy(L.src).cuda(), torch.from_numpy(L.in_off).cuda(), torch.from_numpy(L.in_len).cuda(),
            torch.from_numpy(L.new_dst()).cuda(), torch.from_numpy(L.out_off).cuda())


def check_compress(b, make, run, ref, bound=None, residues=64, refused=None, bits=0):
    """Both twins of a layout through run(src, in_off, in_len, dst, out_off) -> out_len; every entry against ref(data) -- refused on purpose
    (out_len 0, status bit `bits`) only where `refused` names it --, every byte outside against the canary.  bound: the room the header
    promises on the zstd calls (the reference must fit: asserted on the CPU before the device runs); None = DEFLATE: the slot is the bound,
    nothing behind the stream may change.  -> entries compared"""
    layouts = LY.twins(make)
    want = []
    for i, d in enumerate(layouts[0].datas):
        w = ref(d)
        if refused is not None and refused(d):
            assert not w, (i, len(d))
            w = b""
        else:
            assert w, ("the reference does not serve this entry", i, len(d))
            if bound is not None:
                assert len(w) <= bound(len(d)), ("the reference's frame exceeds the promised room", len(d), len(w))
        want.append(w)
    results = []
    for L in layouts:
        L.check_residues(residues)
        LY.check_content_mix(L.datas)
        src, io, il, dst, oo = dev(L)
        ol = run(src, io, il, dst, oo)
        torch.cuda.synchronize()
        rc, got_bits = b.status()
        assert got_bits == bits and (rc == 0) == (bits == 0), (rc, got_bits)
        dst, ol = dst.cpu().numpy(), ol.cpu().numpy()
        frames = L.frames(dst, ol)
        for i, (d, f, w) in enumerate(zip(L.datas, frames, want)):
            assert f == w, (i, len(d), len(f), len(w), int(L.in_off[i]) % 64, int(L.out_off[i]) % 64)
        bad = L.check(dst, ol, slot_tail_ok=bound is not None)
        assert not bad, "\n".join(bad)
        results.append(frames)
    assert results[0] == results[1], "the frames depend on the filler outside the slices"
    return layouts[0].n


def zstd_run(b, **kw):
    return lambda src, io, il, dst, oo: b.compress(src, io, il, dst=dst, out_off=oo, **kw)[2]


def deflate_run(b, **kw):
    return lambda src, io, il, dst, oo: b.deflate(src, io, il, dst=dst, out_off=oo, **kw)[2]


# -------------------------------------------------------------------------------------------------- zstd compressors ----
@pytest.mark.parametrize("family", FAMILIES)
def test_level_3(family):
    o = helpers.oracle()
    b = ctx(max_slices=256, max_slice_bytes=131072)
    try:
        n = check_compress(b, families(LY.zstd_slot, 100, sizes=EDGES)[family], zstd_run(b), o.compress, LY.zstd_bound)
        assert n == n_entries(family)
    finally:
        b.close()


def test_level_3_in_chunks_at_another_team_width():
    """team_lanes = 64: one team per wave, so a batch of more slices than the device has team slots goes through in two chunks, the
    entropy kernel of the first beside the match kernel of the second; 4 224 entries of up to 16 KiB + 1 in exact slots."""
    o = helpers.oracle()
    sizes = SIZES * 66
    b = ctx(max_slices=len(sizes), max_slice_bytes=16384 + 64, team_lanes=64)
    try:
        n = check_compress(b, families(LY.zstd_slot, 110, sizes=sizes)["exact"], zstd_run(b), o.compress, LY.zstd_bound)
        assert n == 4224 and b.last_chunks() > 1, b.last_chunks()
    finally:
        b.close()


def test_level_3_in_pieces():
    """kmp_zstd_compress_batch_pieces: 8 parts side by side on streams of their own, exact slots."""
    o = helpers.oracle()
    sizes = EDGES * 4
    b = ctx(max_slices=len(sizes), max_slice_bytes=131072)
    streams = [torch.cuda.Stream() for _ in range(8)]

    def run(src, io, il, dst, oo):
        ol = torch.zeros(il.numel(), dtype=torch.int32, device="cuda")
        torch.cuda.synchronize()
        b.compress_pieces(src, io, il, dst, oo, ol, streams)
        return ol
    try:
        assert check_compress(b, families(LY.zstd_slot, 120, sizes=sizes)["exact"], run, o.compress, LY.zstd_bound) == 256
    finally:
        b.close()


@pytest.mark.parametrize("level,family", [(1, "exact"), (1, "tempting"), (1, "aliased"), (2, "exact"), (2, "tempting"), (2, "aliased"), (-1, "exact"), (-1, "tempting"),
                                          (-1, "aliased"), (-5, "exact"), (-5, "tempting"), (-5, "aliased"), (-1000, "exact"), (-1000, "tempting"), (-1000, "aliased")])
def test_fast_levels(level, family):
    o = helpers.oracle()
    b = ctx(max_slices=256, max_slice_bytes=131072)
    try:
        n = check_compress(b, families(LY.zstd_slot, 2000 + level, sizes=EDGES)[family], zstd_run(b, level=level), lambda d: o.compress_level(d, level), LY.zstd_bound)
        assert n == n_entries(family)
    finally:
        b.close()


L4_SIZES = with_large(EDGES[:-5], 24000, 50000, 17000, 100000, 30000, 20000, 40000) + EDGES[-5:]
L4_BODIES = BODIES + (70000,)


@pytest.mark.parametrize("family", FAMILIES)
def test_level_4(family):
    """above 16 KiB the double-fast parse, 16 KiB and less (strategy "greedy": the kernels of levels 5 .. 10) beside them"""
    o = helpers.oracle()
    ref = lambda d: o.compress_level(d, 4) if len(d) > 16384 else o.compress_lazy(d, 4) if d else LY.empty_frame()      # noqa: E731
    b = ctx(max_slices=256, max_slice_bytes=131072)
    try:
        n = check_compress(b, families(LY.zstd_slot, 140, sizes=L4_SIZES, bodies=L4_BODIES)[family], zstd_run(b, level=4), ref, LY.zstd_bound)
        assert n == n_entries(family, L4_SIZES, L4_BODIES)
    finally:
        b.close()


@pytest.mark.parametrize("level,family", [(5, "exact"), (5, "tempting"), (5, "aliased"), (6, "exact"), (6, "tempting"), (6, "aliased"), (7, "exact"), (7, "tempting"), (7, "aliased")])
def test_lazy_levels(level, family):
    o = helpers.oracle()
    b = ctx(max_slices=256, max_slice_bytes=131072)
    try:
        n = check_compress(b, families(LY.zstd_slot, 300 + level, sizes=EDGES)[family], zstd_run(b, level=level),
                           lambda d: o.compress_lazy(d, level) if d else LY.empty_frame(), LY.zstd_bound)
        assert n == n_entries(family)
    finally:
        b.close()


L10_SIZES = (1, 5, 7, 16385, 17000, 20000, 6, 30000, 3, 18000, 24000, 40000, 4, 16500, 2, 65537, 131072, 65536, 131071, 65535,            # served
             8, 9, 16384, 300)                                                                                                              # refused
L10_BODIES = (70000, 40000, 7, 20000)


@pytest.mark.parametrize("family", FAMILIES)
def test_level_10_serves_its_sizes_and_refuses_the_others_in_place(family):
    """Level 10 is another strategy for 8 bytes .. 16 KiB: those entries come back refused (out_len 0, KMP_STATUS_LEVEL_SIZE) -- named here
    on purpose --, their slots untouched, beside the sizes the level serves."""
    o = helpers.oracle()
    refused = lambda d: 8 <= len(d) <= 16384                                                                                                # noqa: E731
    b = ctx(max_slices=256, max_slice_bytes=131072)
    try:
        n = check_compress(b, families(LY.zstd_slot, 310, sizes=L10_SIZES, bodies=L10_BODIES)[family], zstd_run(b, level=10),
                           lambda d: o.compress_lazy(d, 10) if d else LY.empty_frame(), LY.zstd_bound, residues=16, refused=refused, bits=4)
        assert n == n_entries(family, L10_SIZES, L10_BODIES)
    finally:
        b.close()


def dictionaries():
    """(name, dictionary, ID): a raw-content one (helpers.dict_compress_cases) and two in zstd's own format (helpers.formatted_dict_built,
    helpers.formatted_dict_cases)"""
    raw = next(d for d, _ in helpers.dict_compress_cases() if len(d) == 3000)
    out = [("raw", raw, 0)]
    name, d, _ = helpers.formatted_dict_built()[1]
    out.append((name, d, struct.unpack("<I", d[4:8])[0]))
    name, d, _, _ = helpers.formatted_dict_cases()[0]
    out.append((name, d, struct.unpack("<I", d[4:8])[0]))
    return out


@pytest.mark.parametrize("which,family", [(0, "exact"), (0, "tempting"), (0, "aliased"), (1, "exact"), (1, "tempting"), (1, "aliased"), (2, "exact"), (2, "tempting"), (2, "aliased")])
def test_dictionary(which, family):
    """which 2, the dictionary ZDICT trained: its Huffman table codes every byte value and is used unseen on literals of 6 .. 1 024 bytes.
    On incompressible slices the coded literals went behind the slot before they were discarded -- found here, fixed in khuf_encode_streams
    (zstd_entropy.h), which now stops before it writes what its caller would not keep."""
    o = helpers.oracle()
    name, dic, did = dictionaries()[which]
    ref = lambda d: o.compress_dict(d, dic)[0] if d else LY.empty_frame(did)      # noqa: E731
    b = ctx(max_slices=256, max_slice_bytes=131072)
    try:
        n = check_compress(b, families(LY.zstd_slot, 400 + which, sizes=EDGES)[family], zstd_run(b, dictionary=dic), ref, LY.zstd_bound)
        assert n == n_entries(family)
    finally:
        b.close()


BIG_SIZES = LY.BIG_EDGE_SIZES + (140000, 9, 300000, 700, 17, 4097, 0, 131072, 3000, 1, 64, 16385, 255, 8, 1000, 65537, 500000, 100, 30000)          # 24 entries
BIG_BODIES = (150000, 3000, 4097, 280000, 20, 700)


@pytest.mark.parametrize("level,kw,family", [(3, {}, "exact"), (3, {}, "tempting"), (3, {}, "aliased"), (3, {"streaming": "data"}, "tempting"), (3, {"streaming": "empty"}, "exact"),
                                             (3, {"reference": True}, "tempting"), (1, {}, "tempting"), (1, {"streaming": "data"}, "exact"), (1, {"reference": True}, "aliased"),
                                             (2, {}, "tempting"), (2, {"streaming": "empty"}, "aliased"), (2, {"reference": True}, "exact")])
def test_frames_of_several_blocks(level, kw, family):
    """A context for slices above 128 KiB (the block-chain kernels): ZSTD_compress2's frames, streamed frames closed with / without data,
    the reference's one-shot driver; levels 1, 2, 3; at level 1 a slice beyond the level's window of 512 KiB; small slices beside them."""
    o = helpers.oracle()
    mode = 3 if kw.get("reference") else {None: 0, "data": 1, "empty": 2}[kw.get("streaming")]
    if level == 3:
        ref = {0: lambda d: o.compress_buffered(d, 2), 1: lambda d: o.compress_buffered(d, False), 2: lambda d: o.compress_buffered(d, False, empty_end=True),
               3: lambda d: o.compress_buffered(d, True)}[mode]
    else:
        ref = lambda d: o.compress_fast_buffered(d, level, stream=mode)      # noqa: E731
    sizes = BIG_SIZES + ((700001,) if level == 1 else ())
    b = ctx(max_slices=128, max_slice_bytes=1 << 20)
    try:
        n = check_compress(b, families(LY.zstd_slot, 500 + 10 * level + mode, sizes=sizes, bodies=BIG_BODIES)[family], zstd_run(b, level=level, **kw), ref, LY.zstd_bound, residues=16)
        assert n == n_entries(family, sizes, BIG_BODIES)
    finally:
        b.close()


def test_level_4_frames_of_several_blocks():
    """level 4 on such a context serves above 16 KiB .. 128 KiB and above 256 KiB (double-fast there); only those sizes here"""
    o = helpers.oracle()
    sizes = (262145, 17000, 300000, 131072, 65537, 20000, 393217, 40000, 16385, 30000, 100000, 24000, 50000, 131071, 500000, 65536)
    ref = lambda d: o.compress_buffered(d, 2, level=4) if len(d) > 131072 else o.compress_level(d, 4)      # noqa: E731
    b = ctx(max_slices=64, max_slice_bytes=1 << 20)
    try:
        cs = LY.contents(sizes, 560)
        make = lambda f: LY.tempting([d for d, _ in cs], [p for _, p in cs], [LY.zstd_slot(len(d)) for d, _ in cs], 560, f)      # noqa: E731
        assert check_compress(b, make, zstd_run(b, level=4), ref, LY.zstd_bound, residues=16) == 16
    finally:
        b.close()


# ---------------------------------------------------------------------------------------------------------- DEFLATE ----
DEFLATE_SIZES = with_large(SIZES, 65536, 65535, 40000)


@pytest.mark.parametrize("level,fmt,family", [(1, 0, "exact"), (1, 1, "tempting"), (1, 2, "aliased"), (4, 2, "exact"), (4, 0, "tempting"), (4, 1, "aliased"), (6, 1, "exact"),
                                              (6, 0, "tempting"), (6, 2, "aliased"), (9, 2, "exact"), (9, 1, "tempting"), (9, 0, "aliased")])
def test_deflate(level, fmt, family):
    b = ctx(max_slices=256, max_slice_bytes=65536)
    try:
        n = check_compress(b, families(LY.deflate_bound, 600 + 10 * level + fmt, sizes=DEFLATE_SIZES)[family], deflate_run(b, level=level, format=FMT[fmt]), zlib_ref(level, fmt))
        assert n == n_entries(family)
    finally:
        b.close()


@pytest.mark.parametrize("level,wb,ml,fmt,family", [(6, 12, 5, 1, "exact"), (2, 9, 1, 2, "tempting"), (9, 10, 9, 0, "aliased")])
def test_deflate_window_bits_and_mem_level(level, wb, ml, fmt, family):
    b = ctx(max_slices=256, max_slice_bytes=65536)
    try:
        n = check_compress(b, families(lambda n: LY.deflate_bound_params(n, wb, ml), 700 + level, sizes=DEFLATE_SIZES)[family],
                           deflate_run(b, level=level, format=FMT[fmt], window_bits=wb, mem_level=ml), zlib_ref(level, fmt, wb, ml))
        assert n == n_entries(family)
    finally:
        b.close()


SPAN_SIZES = (98305, 65537, 9, 140000, 700, 17, 4097, 0, 65536, 3000, 1, 64, 16385, 255, 8, 1000, 300000, 98304, 100, 200000)          # above 64 KiB: taken in 64 KiB spans
SPAN_BODIES = (70000, 300, 4097, 150000)


@pytest.mark.parametrize("level,wb,ml,fmt,family", [(6, 15, 8, 0, "tempting"), (4, 15, 8, 1, "exact"), (9, 12, 5, 2, "aliased"), (1, 15, 8, 0, "tempting"), (6, 15, 8, 2, "aliased")])
def test_deflate_spans_above_64_kib(level, wb, ml, fmt, family):
    b = ctx(max_slices=128, max_slice_bytes=300000)
    try:
        n = check_compress(b, families(lambda n: LY.deflate_bound_params(n, wb, ml), 800 + level, sizes=SPAN_SIZES, bodies=SPAN_BODIES)[family],
                           deflate_run(b, level=level, format=FMT[fmt], window_bits=wb, mem_level=ml), zlib_ref(level, fmt, wb, ml), residues=16)
        assert n == n_entries(family, SPAN_SIZES, SPAN_BODIES)
    finally:
        b.close()


def test_compact_into_a_destination_of_exactly_the_total():
    """kmp_compact_batch: the frames of a batch at exact-layout offsets packed into a destination of exactly their total (canaries in front
    and behind), the n + 1 prefix sums against numpy."""
    o = helpers.oracle()
    b = ctx(max_slices=256, max_slice_bytes=131072)
    try:
        L = families(LY.zstd_slot, 130, sizes=EDGES)["exact"]("random")
        src, io, il, dst, oo = dev(L)
        ol = b.compress(src, io, il, dst=dst, out_off=oo)[2]
        torch.cuda.synchronize()
        lens = ol.cpu().numpy().astype(np.int64)
        total = int(lens.sum())
        rng = np.random.default_rng(131)
        can = rng.integers(0, 256, total + 2 * LY.MARGIN, dtype=np.uint8)
        dense = torch.from_numpy(can.copy()).cuda()
        offs = torch.full((L.n + 2,), -7, dtype=torch.int64, device="cuda")
        b.compact_into(dst, oo, ol, dense[LY.MARGIN:LY.MARGIN + total], offs[:L.n + 1])
        torch.cuda.synchronize()
        assert b.status() == (0, 0)
        offs, dense = offs.cpu().numpy(), dense.cpu().numpy()
        assert np.array_equal(offs[:L.n + 1], np.concatenate([[0], np.cumsum(lens)])) and offs[L.n + 1] == -7
        assert np.array_equal(dense[:LY.MARGIN], can[:LY.MARGIN]) and np.array_equal(dense[LY.MARGIN + total:], can[LY.MARGIN + total:])
        body = dense[LY.MARGIN:LY.MARGIN + total]
        n = 0
        for i, d in enumerate(L.datas):
            assert body[int(offs[i]):int(offs[i + 1])].tobytes() == o.compress(d), i
            n += 1
        assert n == 64 and not L.check(dst.cpu().numpy(), ol.cpu().numpy(), slot_tail_ok=True)
    finally:
        b.close()


# --------------------------------------------------------------------------------------------------------- decoders ----
def check_decode(b, entries, plains, behind, run, seed, short=(), short_status=70, residues=64):
    """Both twins; right behind every entry lies `behind`, a VALID frame / stream of other content (a decoder that ran past d_in_len would
    append it or report that the room ran out); d_out_cap = the content size exactly (entries in `short`: one byte less -> the status,
    out_len 0, nothing outside [out_off, +cap) touched, the neighbours right).  -> entries compared"""
    caps = [len(p) - (1 if i in short else 0) for i, p in enumerate(plains)]
    for i in short:
        assert len(plains[i]) > 0
    results = []
    a, a2 = LY.twins(lambda f: LY.decode_layout(entries, behind, caps, seed, f))
    for L in (a, a2):
        L.check_residues(residues)
        src, io, il, dst, oo = dev(L)
        cap = torch.tensor(caps, dtype=torch.int32).cuda()
        _, _, ol, st = run(src, io, il, cap, dst, oo)
        torch.cuda.synchronize()
        assert b.status() == (0, 0)
        dst, ol, st = dst.cpu().numpy(), ol.cpu().numpy(), st.cpu().numpy()
        outs = L.frames(dst, ol)
        for i, p in enumerate(plains):
            if i in short:
                assert (int(st[i]), int(ol[i])) == (short_status, 0), (i, int(st[i]), int(ol[i]))
            else:
                assert int(st[i]) == 0 and outs[i] == p, (i, int(st[i]), len(p), int(L.in_off[i]) % 64)
        bad = L.check(dst, ol, allowed=[c if i in short else int(ol[i]) for i, c in enumerate(caps)])
        assert not bad, "\n".join(bad)
        results.append((outs, [int(x) for x in st]))
    assert results[0] == results[1], "the decoder's result depends on the filler outside the entries"
    return a.n


def zstd_decode_cases(b, repeat=1):
    """(entries, plains): frames the device compressed in this module's own way (checked against the oracle), frames of the oracle at
    other levels, tests/golden/foreign_frames.bin, entries of several frames and a skippable one"""
    o = helpers.oracle()
    cs = [d for d, _ in LY.contents(EDGES * repeat, 900)]
    L = LY.exact(cs, [LY.zstd_slot(len(d)) for d in cs], 900)
    src, io, il, dst, oo = dev(L)
    ol = b.compress(src, io, il, dst=dst, out_off=oo)[2]
    torch.cuda.synchronize()
    own = L.frames(dst.cpu().numpy(), ol.cpu().numpy())
    frames = []
    for i, d in enumerate(cs):
        k = i % 5
        if k == 0:
            assert own[i] == o.compress(d), i
        frames.append(own[i] if k == 0 else o.compress_level(d, 1) if k == 1 else o.compress_level(d, -5) if k == 2
                      else (o.compress_lazy(d, 7) if d else LY.empty_frame()) if k == 3 else o.compress_buffered(d, False))
    plains = list(cs)
    foreign = [r for r in helpers.foreign_frames() if len(r[2]) <= 131072]
    frames += [f for _, f, _ in foreign]; plains += [p for _, _, p in foreign]
    skip = struct.pack("<II", 0x184D2A53, 7) + b"ignored"
    for x, y in ((3, 40), (50, 41), (58, 7)):
        frames.append(frames[x] + skip + frames[y] + frames[x]); plains.append(plains[x] + plains[y] + plains[x])
    return frames, plains


@pytest.mark.parametrize("pre", [True, False])
def test_zstd_decoder(pre, monkeypatch):
    """pre: with the pre-decode kernels (KMP_PRE_MIN_BATCH = 1, tests/conftest.py) / without them (the ablation build's KMP_DECODE_PRE = 0)"""
    o = helpers.oracle()
    if not pre:
        monkeypatch.setenv("KMP_DECODE_PRE", "0")
    b = ctx(max_slices=512, max_slice_bytes=1 << 18, ablations=not pre)
    try:
        frames, plains = zstd_decode_cases(b)
        behind = o.compress(b"INTRUDER " * 30)
        short = {5, 17, 33, 63, len(frames) - 1}
        run = lambda src, io, il, cap, dst, oo: b.decompress(src, io, il, cap, dst=dst, out_off=oo)      # noqa: E731
        n = check_decode(b, frames, plains, behind, run, 901 + pre, short=short)
        assert n == len(frames) and n > 64 + 3
    finally:
        b.close()


def test_zstd_decoder_default_batch_path(monkeypatch):
    """more than 256 entries with KMP_PRE_MIN_BATCH at its default: the path a caller's batch takes"""
    o = helpers.oracle()
    monkeypatch.delenv("KMP_PRE_MIN_BATCH", raising=False)
    b = ctx(max_slices=1024, max_slice_bytes=1 << 18)
    try:
        frames, plains = zstd_decode_cases(b, repeat=4)
        assert len(frames) > 256
        run = lambda src, io, il, cap, dst, oo: b.decompress(src, io, il, cap, dst=dst, out_off=oo)      # noqa: E731
        assert check_decode(b, frames, plains, o.compress(b"INTRUDER " * 30), run, 905, short={5, 100, 255, 300}) == len(frames)
    finally:
        b.close()


@pytest.mark.parametrize("which", [0, 1, 2])
def test_zstd_decoder_with_a_dictionary(which):
    o = helpers.oracle()
    name, dic, did = dictionaries()[which]
    dd = torch.from_numpy(np.frombuffer(dic, dtype=np.uint8).copy()).cuda()
    plains = [d for d, _ in LY.contents(NONEMPTY, 910 + which)]
    frames = [o.compress_dict(d, dic)[0] for d in plains]
    behind = o.compress_dict(b"INTRUDER " * 30, dic)[0]
    b = ctx(max_slices=256, max_slice_bytes=131072)
    try:
        run = lambda src, io, il, cap, dst, oo: b.decompress(src, io, il, cap, dst=dst, out_off=oo, dictionary=dd)      # noqa: E731
        assert check_decode(b, frames, plains, behind, run, 911 + which, short={2, 30}) == 64
    finally:
        b.close()


@pytest.mark.parametrize("fmt", [0, 1, 2, 3])
def test_inflate(fmt):
    """formats raw / zlib / gzip / auto (zlib or gzip per stream); behind every stream lies another valid stream -- for raw DEFLATE a
    further block that a decoder which missed the final bit would take as its own."""
    plains = [d for d, _ in LY.contents(with_large(SIZES, 65536, 40000, 65535, 20000), 920 + fmt)]
    streams = [zlib_ref((1, 4, 6, 9)[i % 4], fmt if fmt < 3 else 1 + i % 2)(d) for i, d in enumerate(plains)]
    behind = zlib_ref(6, fmt if fmt < 3 else 1)(b"INTRUDER " * 30)
    b = ctx(max_slices=256, max_slice_bytes=65536)
    try:
        run = lambda src, io, il, cap, dst, oo: b.inflate(src, io, il, cap, dst=dst, out_off=oo, format=FMT[fmt])      # noqa: E731
        assert check_decode(b, streams, plains, behind, run, 921 + fmt, short={5, 17, 33, 59}, short_status=-5) == 64
    finally:
        b.close()
