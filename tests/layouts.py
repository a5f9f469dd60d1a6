"""Hostile memory layouts for the batched calls (TEST INFRASTRUCTURE; numpy only, no GPU): where a kernel reads and writes,
not which bytes it makes.  include/kompressor_hip.h promises that slice i is src[in_off[i] .. +in_len[i]) and nothing else, that
its output stays inside its slot, and asks for no alignment, order or spacing of the offsets.  build() lays entries out so that
a kernel that breaks the promise changes a frame or damages a canary (it never leaves the buffers):

  * every slice and every slot lies inside its allocation, with MARGIN (4 KiB) and more of canary in front of the first and
    behind the last one, in source and destination alike; entries of length zero point inside the buffer too;
  * slots and slices stand in a seeded permutation of the entry order (offsets are not monotonic), a gap of 1 .. 63 canary
    bytes behind each, their starts walking through the residues modulo 64 (check_residues asserts the coverage);
  * the destination is a seeded non-constant pattern, and Layout.check compares EVERY byte outside [out_off, +out_len)
    (or outside the slot where the contract allows the slot's tail to be written);
  * "tempting" regions carry chosen bytes right in front of and behind a slice (its own continuation: tempting_region), so
    that a compare that runs past the slice end, or a backward extension that steps before its start, pays off and changes the
    frame;
  * "aliased" entries name the same source range, prefixes, suffixes and overlapping middles of it, and empty ranges;
  * every layout can be built twice, filler="random" and filler="complement" (the byte-wise complement outside slices and
    slots): the results of the two runs must be the same bytes and the same status words.
"""
import zlib

import numpy as np

MARGIN = 4096

# the sizes where parsers switch behaviour (one block)
EDGE_SIZES = (1, 7, 8, 9, 16, 17, 4095, 4096, 4097, 16384, 16385, 65535, 65536, 65537, 131071, 131072)
# around multiples of 128 KiB: the paths for frames of several blocks
BIG_EDGE_SIZES = (131073, 262143, 262144, 262145, 393217)
# what fills a batch up to 64 entries and more at little cost
SMALL_SIZES = (0, 2, 3, 5, 6, 10, 15, 31, 33, 63, 64, 65, 100, 127, 129, 200, 255, 256, 257, 300, 511, 513, 700, 1000, 1023, 1025, 1500, 2000, 2500, 3000)


def zstd_bound(n):
    """kmp_zstd_compress_bound (ZSTD_compressBound)"""
    return n + (n >> 8) + ((((128 << 10) - n) >> 11) if n < (128 << 10) else 0)


def zstd_slot(n):
    """the room the header asks for behind d_out_off[i] on the zstd compress calls"""
    return zstd_bound(n) + 8


def deflate_bound(n):
    """kmp_deflate_bound (windowBits 15, memLevel 8; covers the gzip wrapper's 18 bytes)"""
    return n + (n >> 12) + (n >> 14) + (n >> 25) + 7 + 18


def deflate_bound_params(n, window_bits, mem_level):
    """kmp_deflate_bound_params (zlib's deflateBound for other settings: an eighth and a 64th more)"""
    if (window_bits, mem_level) == (15, 8):
        return deflate_bound(n)
    return n + ((n + 7) >> 3) + ((n + 63) >> 6) + 5 + 18


class Region:
    """A run of source bytes that entries are cut from: `pre` and `post` are placed right in front of and behind `body` (chosen
    bytes, not filler: they survive the filler twin).  len(pre) is a multiple of 64, so that the body starts on the residue the
    region was placed at."""

    def __init__(self, body, pre=b"", post=b""):
        assert len(pre) % 64 == 0
        self.body, self.pre, self.post = bytes(body), bytes(pre), bytes(post)


class Layout:
    def __init__(self):
        self.src = None; self.in_off = None; self.in_len = None
        self.dst_size = 0; self.out_off = None; self.slot = None; self.canary = None
        self.datas = None
        self.body_at = None                     # where each region's body starts in src

    @property
    def n(self):
        return len(self.in_len)

    def new_dst(self):
        """the destination buffer as it must be handed to the call: canary bytes everywhere"""
        return self.canary.copy()

    def frames(self, dst, out_len):
        return [dst[int(o):int(o) + int(l)].tobytes() for o, l in zip(self.out_off, out_len)]

    def check(self, dst, out_len, slot_tail_ok=False, allowed=None):
        """-> list of findings (empty = nothing outside the entries' own bytes changed).  Every byte outside [out_off[i], +out_len[i])
        is compared with the canary; slot_tail_ok: the whole slot may have been written (the zstd compressors' bound + 8); allowed:
        per-entry byte counts that may have been written, where the caller knows better (a decoder that ran out of capacity)."""
        dst = np.asarray(dst)
        assert dst.shape == self.canary.shape and dst.dtype == np.uint8
        out_len = [int(x) for x in out_len]
        assert len(out_len) == self.n
        bad = []
        keep = np.ones(self.dst_size, dtype=bool)
        for i in range(self.n):
            if out_len[i] > int(self.slot[i]):
                bad.append(f"entry {i}: out_len {out_len[i]} above its slot of {int(self.slot[i])}")
            w = int(self.slot[i]) if slot_tail_ok else out_len[i] if allowed is None else int(allowed[i])
            w = min(w, int(self.slot[i]))
            keep[int(self.out_off[i]):int(self.out_off[i]) + w] = False
        hit = np.flatnonzero((dst != self.canary) & keep)
        if hit.size:
            order = np.argsort(self.out_off, kind="stable")
            starts = self.out_off[order]
            for p in hit[:8]:
                k = int(np.searchsorted(starts, p, side="right")) - 1
                if k < 0:
                    bad.append(f"byte {int(p)} changed: in the margin in front of the first slot")
                else:
                    i = int(order[k])
                    bad.append(f"byte {int(p)} changed: {int(p) - int(self.out_off[i])} bytes behind the start of entry {i}'s slot of {int(self.slot[i])} "
                               f"(out_len {out_len[i]}, in_len {int(self.in_len[i])}, out_off {int(self.out_off[i])} = {int(self.out_off[i]) % 64} mod 64)")
            bad.append(f"{hit.size} bytes outside the entries changed in all")
        return bad

    def residues(self):
        """(slice-start residues, slot-start residues) modulo 64, as sets"""
        return {int(x) % 64 for x in self.in_off}, {int(x) % 64 for x in self.out_off}

    def check_residues(self, at_least=64):
        """Each batch covers every residue 0 .. 63 of slice starts and of slot starts; batches of few large entries at_least 16
        distinct ones of each, 0, 1 and 63 among them."""
        for what, r in zip(("slice", "slot"), self.residues()):
            assert len(r) >= at_least, f"{what} starts cover {len(r)} residues modulo 64, {at_least} wanted"
            assert {0, 1, 63} <= r, f"{what} starts miss one of the residues 0, 1, 63"

    def check_inside(self):
        """the layout's own invariants: what keeps a wrong kernel inside the test's buffers"""
        n_src = len(self.src)
        for i in range(self.n):
            a, l = int(self.in_off[i]), int(self.in_len[i])
            assert MARGIN <= a and a + l <= n_src - MARGIN, ("slice", i)
            a, l = int(self.out_off[i]), int(self.slot[i])
            assert MARGIN <= a and a + l <= self.dst_size - MARGIN, ("slot", i)
        order = np.argsort(self.out_off, kind="stable")
        for a, b in zip(order[:-1], order[1:]):
            gap = int(self.out_off[b]) - int(self.out_off[a]) - int(self.slot[a])
            assert 1 <= gap <= 63, ("gap behind slot", int(a), gap)
        assert len(np.unique(self.canary[:MARGIN])) > 16


def _walk(rng, sizes, order, first_residues=(0, 1, 63)):
    """Places items of the given sizes one behind the other in `order`, a gap of 1 .. 63 bytes behind each, starts walking through the
    residues modulo 64 (0, 1 and 63 first, then the others in seeded order, again and again).  -> (starts, total size)"""
    rest = [r for r in range(64) if r not in first_residues]
    rng.shuffle(rest)
    pos0 = MARGIN + int(rng.integers(0, 512))
    tail = 1 + int(rng.integers(0, 63)) + MARGIN + int(rng.integers(0, 512))
    for attempt in range(len(rest)):        # (an order that leaves a residue out of the first round is rotated)
        cycle = list(first_residues) + rest[attempt:] + rest[:attempt]
        pool = list(cycle)
        pos = pos0
        starts = [0] * len(sizes)
        for k, i in enumerate(order):
            if not pool:
                pool = list(cycle)
            pick = next((r for r in pool if k == 0 or (r - pos) % 64 != 0), None)
            if pick is None:                # only the residue the previous item ended on is left: it waits for the next round
                pick = next(r for r in cycle if (r - pos) % 64 != 0)
            else:
                pool.remove(pick)
            pos += (pick - pos) % 64
            starts[i] = pos
            pos += int(sizes[i])
        if len({s % 64 for s in starts}) >= min(64, len(sizes)):
            break
    return starts, pos + tail


def build(regions, entries, slots, seed, filler="random"):
    """regions: [Region]; entries: [(region index, start in its body, length)]; slots: per-entry slot sizes (the documented room).
    seed fixes the permutations, the gaps and the filler; filler "random" / "complement" are the two twins (same offsets, every
    byte outside regions and slots complemented)."""
    assert filler in ("random", "complement")
    rng = np.random.default_rng(seed)
    L = Layout()
    n = len(entries)
    assert len(slots) == n and n > 0
    # source: the regions in a seeded order (pre lengths are multiples of 64: the bodies start on the residues of the walk)
    rorder = [int(x) for x in rng.permutation(len(regions))]
    starts, total = _walk(rng, [len(r.pre) + len(r.body) + len(r.post) for r in regions], rorder)
    src = rng.integers(0, 256, total, dtype=np.uint8)
    if filler == "complement":
        src = ~src
    for r, s in zip(regions, starts):
        blob = r.pre + r.body + r.post
        src[s:s + len(blob)] = np.frombuffer(blob, dtype=np.uint8)
    for ri, st, ln in entries:
        assert 0 <= st and 0 <= ln and st + ln <= len(regions[ri].body)
    L.src = src
    L.body_at = [s + len(r.pre) for r, s in zip(regions, starts)]
    L.in_off = np.array([starts[ri] + len(regions[ri].pre) + st for ri, st, ln in entries], dtype=np.int64)
    L.in_len = np.array([ln for ri, st, ln in entries], dtype=np.int32)
    L.datas = [regions[ri].body[st:st + ln] for ri, st, ln in entries]
    # destination: the slots in another seeded order
    ostarts, osize = _walk(rng, slots, [int(x) for x in rng.permutation(n)])
    L.out_off = np.array(ostarts, dtype=np.int64)
    L.slot = np.array(slots, dtype=np.int64)
    L.dst_size = osize
    can = rng.integers(0, 256, osize, dtype=np.uint8)
    L.canary = ~can if filler == "complement" else can
    L.check_inside()
    for i, d in enumerate(L.datas):
        assert L.src[int(L.in_off[i]):int(L.in_off[i]) + len(d)].tobytes() == d
    return L


def exact(datas, slots, seed, filler="random"):
    """Every entry a region of its own, exact slots."""
    return build([Region(d) for d in datas], [(i, 0, len(d)) for i, d in enumerate(datas)], slots, seed, filler)


def tempting_region(d, period=None):
    """The slice `d` with the bytes around it that make an out-of-range compare pay off.  period: d is periodic with that period (a
    cut out of a longer periodic buffer): the period goes on behind the end (a match running at the slice end would run on for 512
    bytes more), and the 256 bytes in front of the start are those in front of the first match source one period on (a backward
    extension of that match would step out of the slice).  None: the same with the slice as the period -- its start follows its end
    and its end stands in front of its start, which gives a probe past the end something to find."""
    if len(d) == 0:
        return Region(d)
    p = period if period and period < len(d) else len(d)
    unit = d[:p]
    shift = len(d) % p
    cont = unit[shift:] + unit[:shift]                  # the period as it goes on behind d
    post = (cont * (512 // p + 2))[:512]
    pre = unit * (256 // p + 2)
    return Region(d, pre[len(pre) - 256:], post)


def tempting(datas, periods, slots, seed, filler="random"):
    return build([tempting_region(d, p) for d, p in zip(datas, periods)], [(i, 0, len(d)) for i, d in enumerate(datas)], slots, seed, filler)


def aliased_entries(bodies, seed):
    """Entries over a few bodies: the whole body several times, a proper prefix and a proper suffix of it, two ranges that overlap in
    the middle, empty ranges between the others.  -> [(region index, start, length)] in a seeded order"""
    rng = np.random.default_rng(seed)
    out = []
    for ri, b in enumerate(bodies):
        n = len(b)
        out += [(ri, 0, n), (ri, 0, n)]
        if n >= 4:
            cut = int(rng.integers(1, n))
            out += [(ri, 0, cut), (ri, n - cut, cut), (ri, n // 4, n // 2), (ri, n // 3, n // 2)]
        out.append((ri, int(rng.integers(0, n + 1)), 0))
    return [out[int(k)] for k in rng.permutation(len(out))]


def aliased(bodies, slot_of, seed, filler="random"):
    """slot_of(length) -> the exact slot of an entry of that length.  Behind the entries of aliased_entries come 64 more, one starting
    on each residue modulo 64, cut out of the middle of the bodies of 192 bytes and more (they overlap the others and each other)."""
    entries = aliased_entries(bodies, seed)
    regions = [Region(b) for b in bodies]
    first = build(regions, entries, [slot_of(ln) for _, _, ln in entries], seed + 1, filler)      # (where the bodies come to lie)
    rng = np.random.default_rng(seed + 2)
    big = [ri for ri, b in enumerate(bodies) if len(b) >= 192]
    for r in range(64):
        ri = big[r % len(big)]
        st = (r - first.body_at[ri]) % 64 + 64 * int(rng.integers(0, (len(bodies[ri]) - 64) // 64))
        entries.append((ri, st, min(len(bodies[ri]) - st, 1 + int(rng.integers(0, 2000)))))
    L = build(regions, entries, [slot_of(ln) for _, _, ln in entries], seed + 1, filler)
    assert L.body_at == first.body_at
    return L


_WORDS = None


def contents(sizes, seed):
    """Seeded slice contents, by position modulo 4: random bytes (incompressible: raw / stored blocks, the largest frames), a short
    period (highly compressible: one long match to the slice end), text over a small vocabulary whose last third repeats its start, a
    long period (a text unit of 300 .. 4 099 bytes repeated).  -> [(bytes, period or None)]"""
    global _WORDS
    rng = np.random.default_rng(seed)
    if _WORDS is None:
        w = np.random.default_rng(77)
        _WORDS = [bytes(w.integers(97, 123, int(w.integers(2, 10)), dtype=np.uint8)) + b" " for _ in range(300)]

    def text(n):
        if n == 0:
            return b""
        k = n // 4 + 2                                    # (words are 3 bytes and more)
        idx = (rng.integers(0, len(_WORDS), k) * rng.random(k)).astype(np.int64)
        return b"".join(_WORDS[int(j)] for j in idx)[:n]

    res = []
    for i, n in enumerate(sizes):
        k = i % 4
        if k == 0:
            res.append((rng.integers(0, 256, n, dtype=np.uint8).tobytes(), None))
        elif k == 2:
            p = max(1, (2 * n) // 3)                       # text whose last third repeats its start: a period of two thirds
            res.append(((text(p) * 2)[:n], p if n >= 12 else None))
        else:
            p = int(rng.choice((1, 3, 5, 37))) if k == 1 else int(rng.choice((300, 1000, 4099)))
            p = max(1, min(p, n // 8)) if n >= 8 else max(1, n)
            unit = text(p) if k == 3 else rng.integers(0, 256, p, dtype=np.uint8).tobytes()
            res.append(((unit * (n // p + 1))[:n], p if n else None))
    return res


def content_mix(datas):
    """(incompressible, highly compressible) counts of a batch: zlib level 1 saves nothing / leaves less than a quarter"""
    inc = comp = 0
    for d in datas:
        z = len(zlib.compress(d, 1)) - 6
        if z >= len(d):
            inc += 1
        elif z * 4 < len(d):
            comp += 1
    return inc, comp


def check_content_mix(datas):
    inc, comp = content_mix(datas)
    assert inc * 4 >= len(datas), f"{inc} of {len(datas)} entries are incompressible, a quarter wanted"
    assert comp * 4 >= len(datas), f"{comp} of {len(datas)} entries are highly compressible, a quarter wanted"


# ---- what the emulator tests and the device tests share ----------------------------------------------------------------
# 64 sizes: the edges up to 16 KiB + 1 and what fills a batch at little cost
SIZES = SMALL_SIZES + (1, 7, 8, 9, 16, 17, 4095, 4096, 4097, 16384, 16385) + (4, 11, 12, 20, 40, 50, 80, 150, 400, 600, 800, 1200, 1800, 2200,
                                                                               2700, 3500, 5000, 6000, 7000, 8000, 9000, 10000, 12000)
BODIES = (9, 64, 300, 1000, 4097, 16385, 3000, 20, 700, 40000)          # aliased: 7 entries over each, and 64 more
assert len(SIZES) == 64
# ... with every edge above 16 KiB + 1 as well (EDGE_SIZES complete)
EDGES = tuple(SIZES[:-5]) + tuple(x for x in EDGE_SIZES if x > 16385)
assert len(EDGES) == 64 and set(EDGE_SIZES) <= set(EDGES)
NONEMPTY = tuple(x or 13 for x in EDGES)                                # for paths that have no empty entry


def with_large(sizes, *large):
    """the batch with its last sizes replaced by large ones; the positions keep the content kinds in turn (random, short period, text,
    long period)"""
    s = list(sizes)
    for k, x in enumerate(large):
        s[len(s) - 1 - k] = x
    return tuple(s)


def families(slot_of, seed, sizes=SIZES, tempting_sizes=None, bodies=BODIES):
    """-> {family: make(filler) -> Layout}; slot_of(length) = the documented room"""
    ex = contents(sizes, seed)
    te = contents(tempting_sizes or sizes, seed + 1)
    bo = [d for d, _ in contents(bodies, seed + 2)]
    return {
        "exact": lambda f: exact([d for d, _ in ex], [slot_of(len(d)) for d, _ in ex], seed, f),
        "tempting": lambda f: tempting([d for d, _ in te], [p for _, p in te], [slot_of(len(d)) for d, _ in te], seed + 1, f),
        "aliased": lambda f: aliased(bo, slot_of, seed + 2, f),
    }


def n_entries(family, sizes=SIZES, bodies=BODIES):
    return len(sizes) if family != "aliased" else sum(7 if b >= 4 else 3 for b in bodies) + 64


def empty_frame(dict_id=0):
    """the zstd frame of an empty input (RFC 8878: magic, a descriptor with the single-segment flag and the size code of the
    dictionary ID, the ID, a content size of 0, one empty raw last block)"""
    code = 0 if not dict_id else 1 if dict_id < 256 else 2 if dict_id < 65536 else 3
    return b"\x28\xb5\x2f\xfd" + bytes([code + 0x20]) + dict_id.to_bytes((0, 1, 2, 4)[code], "little") + b"\x00\x01\x00\x00"


def zlib_ref(level, fmt, wb=15, ml=8):
    """zlib's stream: fmt 0 raw, 1 zlib, 2 gzip"""
    def ref(d):
        c = zlib.compressobj(level, zlib.DEFLATED, (-wb, wb, wb + 16)[fmt], ml, 0)
        return c.compress(d) + c.flush()
    return ref


def decode_layout(entries, behind, caps, seed, filler):
    """entries: what d_in_len covers; `behind` stands right behind each (a VALID frame / stream of other content: a decoder that ran
    past d_in_len would append it or run out of room); in front of each lies filler.  caps: d_out_cap, the slots."""
    return build([Region(e, b"", behind) for e in entries], [(i, 0, len(e)) for i, e in enumerate(entries)], caps, seed, filler)


def twins(make):
    """make(filler) -> Layout; -> the two twins, which share every offset and differ in every filler byte"""
    a, b = make("random"), make("complement")
    assert np.array_equal(a.in_off, b.in_off) and np.array_equal(a.out_off, b.out_off) and a.dst_size == b.dst_size
    assert np.array_equal(a.canary, ~b.canary)
    return a, b
