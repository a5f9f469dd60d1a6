"""The batch calls' memory contract at hostile layouts (tests/layouts.py), kernel bodies on the CPU wave emulator, n > 1: exact slots
with canary gaps at every residue modulo 64 in permuted order, slices whose surroundings tempt a compare to leave them, aliased and
overlapping and empty entries -- each run twice with complementary filler.  Every frame is compared with the oracle / zlib, every
byte outside the entries with the canary.  The same families run on the device in tests/test_gpu_layout.py; the guard-page runs
(tests/guard_pages_compress.py) stay what they are: one slice at a time, against PROT_NONE pages."""
import struct

import numpy as np
import pytest

import helpers
import layouts as LY
from layouts import SIZES, EDGES, NONEMPTY, BODIES, with_large, families, n_entries, zlib_ref

vp = helpers._vp
FAMILIES = ("exact", "tempting", "aliased")


def run(L, call):
    io, il, oo = L.in_off.astype(np.uint64), L.in_len.astype(np.uint32), L.out_off.astype(np.uint64)
    dst = L.new_dst()
    ol = np.zeros(L.n, dtype=np.uint32)
    r = call(vp(L.src), vp(io), vp(il), L.n, vp(dst), vp(oo), vp(ol))
    assert r == 0, f"emulator reported {r}"
    return dst, ol


def check_compress(make, call, ref, bound=None, residues=64, refused=None):
    """Both twins of a layout through `call`; every entry against ref(data) -- refused on purpose (out_len 0) only where `refused`
    names the entry --, every byte outside against the canary.  bound: the room the header promises (the reference must fit: checked
    here, on the CPU); None = DEFLATE, whose slot is the bound and nothing behind the stream may change.  -> entries compared"""
    a, b = LY.twins(make)
    results = []
    for L in (a, b):
        L.check_residues(residues)
        LY.check_content_mix(L.datas)
        dst, ol = run(L, call)
        frames = L.frames(dst, ol)
        for i, (d, f) in enumerate(zip(L.datas, frames)):
            w = ref(d)
            if refused is not None and refused(d):
                assert not w and f == b"", (i, len(d))
                continue
            assert w, ("the reference does not serve this entry", i, len(d))
            if bound is not None:
                assert len(w) <= bound(len(d)), ("the reference's frame exceeds the promised room", len(d), len(w))
            assert f == w, (i, len(d), int(L.in_off[i]) % 64, int(L.out_off[i]) % 64)
        bad = L.check(dst, ol, slot_tail_ok=bound is not None)
        assert not bad, "\n".join(bad)
        results.append(frames)
    assert results[0] == results[1], "the frames depend on the filler outside the slices"
    return a.n


# ------------------------------------------------------------------------------------------------ the helper itself ----
def test_the_checker_sees_every_kind_of_damage():
    """layouts.py on its own: a byte behind a frame, in a gap, in a margin are all findings; the slot's tail is one unless the caller
    allows it; writes inside [out_off, +out_len) are not.  The twins differ in every byte outside the slices and in none inside."""
    cs = LY.contents(SIZES, 1)
    make = lambda f: LY.exact([d for d, _ in cs], [LY.zstd_slot(len(d)) for d, _ in cs], 1, f)      # noqa: E731
    L, twin = LY.twins(make)
    L.check_residues(64)
    ol = [min(9, int(s)) for s in L.slot]
    dst = L.new_dst()
    assert L.check(dst, ol) == []
    for i in range(L.n):
        dst[int(L.out_off[i]):int(L.out_off[i]) + ol[i]] ^= 0xFF
    assert L.check(dst, ol) == []
    i = int(np.argmax(L.out_off))
    for at, tail_ok in ((int(L.out_off[i]) + ol[i], False), (int(L.out_off[i]) + int(L.slot[i]), True), (int(L.out_off[i]) - 1, True), (5, True), (L.dst_size - 1, True)):
        d2 = dst.copy(); d2[at] ^= 1
        assert L.check(d2, ol, slot_tail_ok=tail_ok), at
    d2 = dst.copy(); d2[int(L.out_off[i]) + ol[i]] ^= 1
    assert L.check(d2, ol, slot_tail_ok=True) == []               # the tail of a zstd slot may be written
    inside = np.zeros(len(L.src), dtype=bool)
    for o_, l_ in zip(L.in_off, L.in_len):
        inside[int(o_):int(o_) + int(l_)] = True
    assert np.array_equal(L.src[inside], twin.src[inside]) and np.array_equal(L.src[~inside], ~twin.src[~inside])
    assert list(np.argsort(L.in_off)) != list(range(L.n)) and list(np.argsort(L.out_off)) != list(range(L.n))
    # a tempting region: what follows the slice is its own continuation, what precedes it precedes its first match source
    r = LY.tempting_region((b"abcdefg" * 40)[:250], 7)
    whole = r.pre + r.body + r.post
    assert all(whole[k] == whole[k + 7] for k in range(len(whole) - 7)) and len(r.pre) == 256 and len(r.post) == 512


# -------------------------------------------------------------------------------------------------- zstd compressors ----
@pytest.mark.parametrize("family", FAMILIES)
def test_level_3(family):
    o = helpers.oracle()
    G = {"exact": 8, "tempting": 4, "aliased": 16}[family]
    call = lambda s, io, il, n, d, oo, ol: helpers.emu().emu_zstd_compress(s, io, il, n, G, 2, d, oo, ol, 131072)      # noqa: E731
    n = check_compress(families(LY.zstd_slot, 100, sizes=EDGES)[family], call, o.compress, LY.zstd_bound)
    assert n == n_entries(family)


L4_SIZES = (16385, 131072, 17000, 65535, 20000, 65536, 24000, 65537, 30000, 131071, 40000, 16500, 50000, 18000, 100000, 70000)
L4_BODIES = (70000, 40000, 20000, 131072)


@pytest.mark.parametrize("family", FAMILIES)
def test_level_4_above_16_kib(family, monkeypatch):
    """level 4's double-fast row (KXEMU_LEVEL = 4 makes emu_zstd_compress run it): the size class it serves here, above 16 KiB; the
    greedy class below it is parsed by the kernels of test_lazy_levels and runs beside these on the device (tests/test_gpu_layout.py)"""
    o = helpers.oracle()
    monkeypatch.setenv("KXEMU_LEVEL", "4")
    cs = LY.contents(L4_SIZES, 150)
    bo = [d for d, _ in LY.contents(L4_BODIES, 152)]
    make = {"exact": lambda f: LY.exact([d for d, _ in cs], [LY.zstd_slot(len(d)) for d, _ in cs], 150, f),
            "tempting": lambda f: LY.tempting([d for d, _ in cs], [p for _, p in cs], [LY.zstd_slot(len(d)) for d, _ in cs], 151, f),
            "aliased": lambda f: LY.build([LY.Region(b) for b in bo], [(i, a, len(b) - a - c) for i, b in enumerate(bo) for a, c in ((0, 0), (0, 0), (0, 1000), (1000, 0), (700, 900))],
                                          [LY.zstd_slot(len(b) - a - c) for b in bo for a, c in ((0, 0), (0, 0), (0, 1000), (1000, 0), (700, 900))], 152, f)}[family]
    call = lambda s, io, il, n, d, oo, ol: helpers.emu().emu_zstd_compress(s, io, il, n, 8, 2, d, oo, ol, 131072)      # noqa: E731
    n = check_compress(make, call, lambda d: o.compress_level(d, 4), LY.zstd_bound, residues=16 if family != "aliased" else 4)
    assert n == (20 if family == "aliased" else 16)


@pytest.mark.parametrize("level,family", [(1, "exact"), (1, "tempting"), (1, "aliased"), (2, "tempting"), (-1, "exact"), (-5, "tempting"), (-1000, "aliased")])
def test_fast_levels(level, family):
    o = helpers.oracle()
    G = {1: 4, 2: 2, -1: 8, -5: 16, -1000: 4}[level]
    call = lambda s, io, il, n, d, oo, ol: helpers.emu().emu_zstd_compress_level(s, io, il, n, G, 2, d, oo, ol, 131072, level)      # noqa: E731
    n = check_compress(families(LY.zstd_slot, 2000 + level, sizes=EDGES)[family], call, lambda d: o.compress_level(d, level), LY.zstd_bound)
    assert n == n_entries(family)


@pytest.mark.parametrize("level,family", [(7, "exact"), (7, "tempting"), (7, "aliased"), (5, "tempting"), (6, "exact")])
def test_lazy_levels(level, family):
    o = helpers.oracle()
    sizes = EDGES
    cap = max(max(sizes), max(BODIES))
    call = lambda s, io, il, n, d, oo, ol: helpers.emu().emu_zstd_compress_lazy(s, io, il, n, 2, d, oo, ol, cap, level)      # noqa: E731
    n = check_compress(families(LY.zstd_slot, 300 + level, sizes=sizes)[family], call, lambda d: o.compress_lazy(d, level) if d else LY.empty_frame(), LY.zstd_bound)
    assert n == n_entries(family)


def test_level_10_serves_its_sizes_and_refuses_the_others_in_place():
    """Level 10 is another strategy for 8 bytes .. 16 KiB: those entries come back refused (out_len 0) -- named here on purpose --, their
    slots untouched, beside the sizes the level serves."""
    o = helpers.oracle()
    sizes = (1, 5, 7, 16385, 17000, 20000, 6, 30000, 3, 18000, 24000, 40000, 4, 16500, 2, 65537,            # served
             8, 9, 16384, 300)                                                                                # refused
    refused = lambda d: 8 <= len(d) <= 16384                                                                  # noqa: E731
    cs = LY.contents(sizes, 310)
    make = lambda f: LY.tempting([d for d, _ in cs], [p for _, p in cs], [LY.zstd_slot(len(d)) for d, _ in cs], 310, f)      # noqa: E731
    call = lambda s, io, il, n, d, oo, ol: helpers.emu().emu_zstd_compress_lazy(s, io, il, n, 2, d, oo, ol, 65537, 10)      # noqa: E731
    assert check_compress(make, call, lambda d: o.compress_lazy(d, 10), LY.zstd_bound, residues=16, refused=refused) == 20


def dictionaries():
    """(name, dictionary, ID): a raw-content one and two in zstd's own format"""
    raw = next(d for d, _ in helpers.dict_compress_cases() if len(d) == 3000)
    out = [("raw", raw, 0)]
    for name, d, _ in helpers.formatted_dict_built()[1:3]:
        out.append((name, d, struct.unpack("<I", d[4:8])[0]))
    name, d, _, _ = helpers.formatted_dict_cases()[0]        # trained by ZDICT: a Huffman table that codes every byte value
    out.append((name, d, struct.unpack("<I", d[4:8])[0]))
    return out


@pytest.mark.parametrize("which,family", [(0, "exact"), (0, "tempting"), (1, "aliased"), (2, "tempting"), (3, "exact"), (3, "tempting"), (3, "aliased")])
def test_dictionary(which, family):
    """which 3, the trained dictionary: its Huffman table is used unseen on literals of 6 .. 1 024 bytes; on incompressible slices the
    coded literals were written behind the slot before they were discarded (found by these layouts on the device; khuf_encode_streams
    now stops before it writes)."""
    o = helpers.oracle()
    name, dic, did = dictionaries()[which]
    dbuf = np.frombuffer(dic, dtype=np.uint8).copy()
    sizes = with_large(SIZES, 40000, 20000)                  # both sides of the 16 KiB attach / copy cut-off
    call = lambda s, io, il, n, d, oo, ol: helpers.emu().emu_zstd_compress_dict(s, io, il, n, 4, 2, d, oo, ol, 131072, vp(dbuf), len(dic))      # noqa: E731
    ref = lambda d: o.compress_dict(d, dic)[0] if d else LY.empty_frame(did)      # noqa: E731
    n = check_compress(families(LY.zstd_slot, 400 + which, sizes=sizes)[family], call, ref, LY.zstd_bound)
    assert n == n_entries(family)


BIG_SIZES = LY.BIG_EDGE_SIZES + (140000, 9, 700, 17, 4097, 0, 131072, 3000, 1, 64, 16385, 255, 8, 1000, 100)          # 20 entries: six frames of several blocks
BIG_BODIES = (150000, 300, 4097, 20)


@pytest.mark.parametrize("level,stream,family", [(3, 0, "exact"), (3, 1, "tempting"), (3, 2, "aliased"), (3, 3, "tempting"), (1, 0, "tempting"), (1, 1, "exact"), (2, 0, "exact")])
def test_frames_of_several_blocks(level, stream, family):
    """emu_zstd_compress_big_ex2: the block-chain kernel (what a context for slices above 128 KiB runs), ZSTD_compress2's frames (0),
    streamed frames closed with / without data (1 / 2), the reference's one-shot driver (3); small slices beside the large ones."""
    o = helpers.oracle()
    if level == 3:
        ref = {0: lambda d: o.compress_buffered(d, 2), 1: lambda d: o.compress_buffered(d, False), 2: lambda d: o.compress_buffered(d, False, empty_end=True),
               3: lambda d: o.compress_buffered(d, True)}[stream]
    else:
        ref = lambda d: o.compress_fast_buffered(d, level, stream=stream)      # noqa: E731
    flags = stream | ((level if level in (1, 2) else 0) << 8)
    call = lambda s, io, il, n, d, oo, ol: helpers.emu().emu_zstd_compress_big_ex2(s, io, il, n, 8, 2, d, oo, ol, None, flags, 0, 0)      # noqa: E731
    n = check_compress(families(LY.zstd_slot, 500 + 10 * level + stream, sizes=BIG_SIZES, bodies=BIG_BODIES)[family], call, ref, LY.zstd_bound, residues=16)
    assert n == n_entries(family, BIG_SIZES, BIG_BODIES)


# ---------------------------------------------------------------------------------------------------------- DEFLATE ----
@pytest.mark.parametrize("fmt,family", [(0, "exact"), (1, "tempting"), (2, "aliased")])
def test_deflate_level_6(fmt, family):
    sizes = with_large(SIZES, 65536, 65535) if family == "tempting" else SIZES
    call = lambda s, io, il, n, d, oo, ol: helpers.emu().emu_deflate(s, io, il, n, d, oo, ol, None, None, fmt)      # noqa: E731
    n = check_compress(families(LY.deflate_bound, 600 + fmt, tempting_sizes=sizes)[family], call, zlib_ref(6, fmt))
    assert n == n_entries(family)


@pytest.mark.parametrize("level,wb,ml,fmt,family", [(1, 15, 8, 1, "tempting"), (4, 15, 8, 2, "exact"), (9, 15, 8, 0, "tempting"), (6, 12, 5, 1, "exact"),
                                                     (2, 9, 1, 2, "tempting"), (9, 10, 9, 0, "aliased")])
def test_deflate_levels_and_params(level, wb, ml, fmt, family):
    slot_of = lambda n: LY.deflate_bound_params(n, wb, ml)      # noqa: E731
    call = lambda s, io, il, n, d, oo, ol: helpers.emu().emu_deflate_params(s, io, il, n, d, oo, ol, None, None, fmt, level, wb, ml, 0)      # noqa: E731
    n = check_compress(families(slot_of, 700 + 10 * level + wb, tempting_sizes=with_large(SIZES, 65536))[family], call, zlib_ref(level, fmt, wb, ml))
    assert n == n_entries(family)


SPAN_SIZES = (98305, 65537, 9, 140000, 700, 17, 4097, 0, 65536, 3000, 1, 64, 16385, 255, 8, 1000)          # above 64 KiB: the kernels take the slice in 64 KiB spans
SPAN_BODIES = (70000, 300, 4097, 20)


@pytest.mark.parametrize("level,wb,ml,fmt,family", [(6, 15, 8, 0, "tempting"), (4, 15, 8, 1, "exact"), (9, 12, 5, 2, "aliased"), (1, 15, 8, 0, "tempting")])
def test_deflate_spans_above_64_kib(level, wb, ml, fmt, family):
    slot_of = lambda n: LY.deflate_bound_params(n, wb, ml)      # noqa: E731
    call = lambda s, io, il, n, d, oo, ol: helpers.emu().emu_deflate_params(s, io, il, n, d, oo, ol, None, None, fmt, level, wb, ml, 0)      # noqa: E731
    n = check_compress(families(slot_of, 800 + level, sizes=SPAN_SIZES, bodies=SPAN_BODIES)[family], call, zlib_ref(level, fmt, wb, ml), residues=16)
    assert n == n_entries(family, SPAN_SIZES, SPAN_BODIES)


# --------------------------------------------------------------------------------------------------------- decoders ----
def check_decode(entries, plains, behind, call, seed, short=(), short_status=70, residues=64):
    """Both twins; exact capacities (entries in `short`: one byte less: the status, out_len 0, nothing outside the slot touched).
    -> entries compared"""
    caps = [len(p) - (1 if i in short else 0) for i, p in enumerate(plains)]
    for i in short:
        assert len(plains[i]) > 0
    a, b = LY.twins(lambda f: LY.decode_layout(entries, behind, caps, seed, f))
    results = []
    for L in (a, b):
        L.check_residues(residues)
        io, il, oo = L.in_off.astype(np.uint64), L.in_len.astype(np.uint32), L.out_off.astype(np.uint64)
        cap = np.array(caps, dtype=np.uint32)
        dst = L.new_dst(); ol = np.zeros(L.n, dtype=np.uint32); st = np.zeros(L.n, dtype=np.int32)
        r = call(vp(L.src), vp(io), vp(il), L.n, vp(dst), vp(oo), vp(cap), vp(ol), vp(st))
        assert r == 0, f"emulator reported {r}"
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


def zstd_decode_cases():
    """(entries, plains): frames of the oracle at several levels, foreign frames (tests/golden/foreign_frames.bin), entries of several
    frames and a skippable one"""
    o = helpers.oracle()
    cs = [d for d, _ in LY.contents(with_large(SIZES, 65537, 40000), 900)]
    frames = []
    for i, d in enumerate(cs):
        k = i % 5
        frames.append(o.compress(d) if k == 0 else o.compress_level(d, 1) if k == 1 else o.compress_level(d, -5) if k == 2
                      else o.compress_lazy(d, 7) if k == 3 else o.compress_buffered(d, False))
    plains = list(cs)
    foreign = sorted(helpers.foreign_frames(), key=lambda r: len(r[2]))[:12]
    frames += [f for _, f, _ in foreign]; plains += [p for _, _, p in foreign]
    skip = struct.pack("<II", 0x184D2A53, 7) + b"ignored"
    for a, b in ((3, 40), (50, 41), (62, 7)):
        frames.append(frames[a] + skip + frames[b] + frames[a]); plains.append(plains[a] + plains[b] + plains[a])
    return frames, plains


@pytest.mark.parametrize("pre", [True, False])
def test_zstd_decoder(pre, monkeypatch):
    o = helpers.oracle()
    if not pre:
        monkeypatch.setenv("KXEMU_NO_PRE", "1")
    frames, plains = zstd_decode_cases()
    behind = o.compress(b"INTRUDER " * 30)
    short = {5, 17, 33, 63, len(frames) - 1}
    call = lambda s, io, il, n, d, oo, cap, ol, st: helpers.emu().emu_zstd_decompress(s, io, il, n, 2, d, oo, cap, ol, st, 128 * 1024 + 64)      # noqa: E731
    assert check_decode(frames, plains, behind, call, 901 + pre, short=short) == 64 + 12 + 3


@pytest.mark.parametrize("which", [0, 1, 3])
def test_zstd_decoder_with_a_dictionary(which):
    o = helpers.oracle()
    name, dic, did = dictionaries()[which]
    dbuf = np.frombuffer(dic, dtype=np.uint8).copy()
    plains = [d for d, _ in LY.contents(with_large(NONEMPTY[:-5] + (7000, 8000, 9000, 40000, 20000)), 910 + which)]
    frames = [o.compress_dict(d, dic)[0] for d in plains]
    behind = o.compress_dict(b"INTRUDER " * 30, dic)[0]
    call = lambda s, io, il, n, d, oo, cap, ol, st: helpers.emu().emu_zstd_decompress_dict(s, io, il, n, 2, d, oo, cap, ol, st, 128 * 1024 + 64, vp(dbuf), len(dic))      # noqa: E731
    assert check_decode(frames, plains, behind, call, 911 + which, short={2, 30}) == 64


@pytest.mark.parametrize("fmt", [0, 1, 2, 3])
def test_inflate(fmt):
    """formats raw / zlib / gzip / auto (zlib or gzip per stream); behind every stream lies another valid stream -- for raw DEFLATE a
    further block that a decoder which missed the final bit would take as its own.  Both the one-kernel inflate and the pre-decoder +
    executor pair."""
    plains = [d for d, _ in LY.contents(with_large(SIZES, 65536, 40000), 920 + fmt)]
    streams = [zlib_ref((1, 4, 6, 9)[i % 4], fmt if fmt < 3 else 1 + i % 2)(d) for i, d in enumerate(plains)]
    behind = zlib_ref(6, fmt if fmt < 3 else 1)(b"INTRUDER " * 30)
    short = {5, 17, 33, 63}
    call = lambda s, io, il, n, d, oo, cap, ol, st: helpers.emu().emu_inflate(s, io, il, n, d, oo, cap, ol, st, fmt)      # noqa: E731
    assert check_decode(streams, plains, behind, call, 921 + fmt, short=short, short_status=-5) == 64
    cov = np.zeros(64, dtype=np.uint32)
    call = lambda s, io, il, n, d, oo, cap, ol, st: helpers.emu().emu_inflate_pre(s, io, il, n, d, oo, cap, ol, st, fmt, 65536, vp(cov))      # noqa: E731
    assert check_decode(streams, plains, behind, call, 931 + fmt, short=short, short_status=-5) == 64
