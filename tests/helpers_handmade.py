"""A zstd frame composer (RFC 8878) and the hand-made cases of tests/golden/zstd_handmade_golden.json: legal zstd that no libzstd encoder
writes -- size fields wider than needed, RLE-mode sequence tables with any code, an FSE table one symbol owns, "Repeat" after
"Predefined", 4-stream literals of 6 bytes, empty blocks -- and the illegal neighbours of each.  Plain Python: nothing here knows the
product (the dictionary cases borrow tests/helpers.py's dictionaries, one case of several frames a libzstd frame of its foreign_frames()).  The yardstick is libzstd 1.5.7 alone: the fixture
(tests/golden/make_golden_handmade.py) records what the library answers for every entry; it stores no frame bytes, the cases are rebuilt
here from code and seeds.

A case is (family, name, entry, capacity, dictionary or None, intent).  intent: "ok" -- the library must accept it; "reject" -- it must
refuse it; "lenient" -- a Huffman literal stream composed to be under- or over-consumed: libzstd's fast loop lets it through, a decoder
that checks the stream's end may refuse it (tests/fuzz_decoders.py).  The generator fails where the library contradicts an intent: that
is the composer's own test.

Run as a program (the emulator's helpers are imported then), every entry is placed so that it ends at a PROT_NONE page and every output
so that its capacity ends at one, and goes through k_zstd_decode alone, behind the pre-decoders, the sort key and kx_frame_info:

    python tests/helpers_handmade.py          # prints "OK <n>" and exits 0
"""
import hashlib
import os
import random
import sys

MAGIC = bytes.fromhex("28b52ffd")
BLOCK_MAX = 128 * 1024
SEED = 88711
EXACT_FAMILIES = ("header", "blocks", "multi")          # families whose error codes are compared for equality
EXACT_NAMES = ("4 streams of 5 literals",)              # ... and single cases
# What the library accepts and the decoder refuses, by name, with the decoder's code: a Huffman code of 12 bits is beyond RFC 8878's 11 and
# beyond the decoder's table of 2048 entries; libzstd 1.5.7 decodes it all the same.  The tests hold the decoder to exactly this.
REFUSED_THOUGH_ACCEPTED = {"tree depth 12": 20, "tree depth 12, 4 streams": 20}


# ---------------------------------------------------------------- bits ----
class BackBits:
    """A bitstream read backwards from its end mark: put() takes the fields in the order the decoder reads them."""
    def __init__(self):
        self.acc = 1                      # the end mark: the highest set bit of the last byte

    def put(self, v, n):
        assert 0 <= v < (1 << n) or (n == 0 and v == 0), (v, n)
        self.acc = (self.acc << n) | v

    def bytes(self):
        return self.acc.to_bytes((self.acc.bit_length() + 7) // 8, "little")


class FwdBits:
    """LSB-first bits, for table descriptions"""
    def __init__(self):
        self.acc = 0; self.n = 0

    def put(self, v, n):
        self.acc |= (v & ((1 << n) - 1)) << self.n; self.n += n

    def bytes(self):
        return self.acc.to_bytes((self.n + 7) // 8, "little")


def ncount(norm, log, first_bits=None):
    """The FSE normalized-count description of norm (counts, -1 for "less than 1") at table log `log`: the 4-bit log, values whose width
    shrinks with what remains, 2-bit zero-run flags behind every count of 0.  Counts that do not sum to the table size are written
    as they come (the field is masked): a hostile description."""
    w = FwdBits()
    w.put(log - 5 if first_bits is None else first_bits, 4)
    remaining, threshold, nb = (1 << log) + 1, 1 << log, log + 1
    sym, prev0 = 0, False
    while remaining > 1 and sym < len(norm):
        if prev0:
            run = 0
            while sym + run < len(norm) and norm[sym + run] == 0:
                run += 1
            sym += run
            while run >= 3:
                w.put(3, 2); run -= 3
            w.put(run, 2)
            if sym >= len(norm):
                break
        c = norm[sym]; sym += 1
        mx = 2 * threshold - 1 - remaining
        v = c + 1
        remaining -= abs(c)
        if v < mx:
            w.put(v, nb - 1)
        else:
            w.put(v + mx if v >= threshold else v, nb)
        prev0 = c == 0
        while remaining < threshold and threshold > 1:
            nb -= 1; threshold >>= 1
    return w.bytes()


def fse_table(norm, log):
    """The decoding table of FSE_buildDTable: [(symbol, nbBits, newStateBase)] per state"""
    size = 1 << log
    sym_of = [0] * size
    high = size - 1
    nxt = {}
    for s, c in enumerate(norm):
        if c == -1:
            sym_of[high] = s; high -= 1; nxt[s] = 1
        else:
            nxt[s] = c
    step, pos = (size >> 1) + (size >> 3) + 3, 0
    for s, c in enumerate(norm):
        for _ in range(max(c, 0)):
            sym_of[pos] = s
            pos = (pos + step) & (size - 1)
            while pos > high:
                pos = (pos + step) & (size - 1)
    out = []
    for u in range(size):
        s = sym_of[u]; x = nxt[s]; nxt[s] += 1
        nbits = log - (x.bit_length() - 1)
        out.append((s, nbits, (x << nbits) - size))
    return out


def fse_chain(table, syms, pick=0):
    """States that make the decoder emit syms: -> (the first state, per symbol (bits, nbBits) read behind it, None behind the last)"""
    states = {}
    for u, (s, _, _) in enumerate(table):
        states.setdefault(s, []).append(u)
    st = states[syms[-1]][pick % len(states[syms[-1]])]
    trans = [None] * len(syms)
    for i in range(len(syms) - 2, -1, -1):
        for cand in states[syms[i]]:
            _, nbits, base = table[cand]
            if base <= st < base + (1 << nbits):
                trans[i] = (st - base, nbits); st = cand
                break
        else:
            raise AssertionError("no state of the symbol reaches the next one")
    return st, trans


# ---------------------------------------------------------------- sequence tables ----
LL_BASE = [0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11, 12, 13, 14, 15, 16, 18, 20, 22, 24, 28, 32, 40, 48, 64, 0x80, 0x100, 0x200, 0x400, 0x800, 0x1000,
           0x2000, 0x4000, 0x8000, 0x10000]
LL_BITS = [0] * 16 + [1, 1, 1, 1, 2, 2, 3, 3, 4, 6, 7, 8, 9, 10, 11, 12, 13, 14, 15, 16]
ML_BASE = list(range(3, 35)) + [35, 37, 39, 41, 43, 47, 51, 59, 67, 83, 99, 0x83, 0x103, 0x203, 0x403, 0x803, 0x1003, 0x2003, 0x4003, 0x8003, 0x10003]
ML_BITS = [0] * 32 + [1, 1, 1, 1, 2, 2, 3, 3, 4, 4, 5, 7, 8, 9, 10, 11, 12, 13, 14, 15, 16]
DEFAULT = {"ll": ([4, 3, 2, 2, 2, 2, 2, 2, 2, 2, 2, 2, 2, 1, 1, 1, 2, 2, 2, 2, 2, 2, 2, 2, 2, 3, 2, 1, 1, 1, 1, 1, -1, -1, -1, -1], 6),
           "of": ([1, 1, 1, 1, 1, 1, 2, 2, 2, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, -1, -1, -1, -1, -1], 5),
           "ml": ([1, 4, 3, 2, 2, 2, 2, 2, 2] + [1] * 37 + [-1] * 7, 6)}
MAX_LOG = {"ll": 9, "of": 8, "ml": 9}
MAX_SYM = {"ll": 35, "of": 31, "ml": 52}


class Tab:
    """One symbol type's table in one of the four modes: what goes into the section (mode, desc) and what the decoder makes of it"""
    def __init__(self, mode, desc, table, log):
        self.mode, self.desc, self.table, self.log = mode, desc, table, log

    @staticmethod
    def predefined(kind):
        norm, log = DEFAULT[kind]
        return Tab(0, b"", fse_table(norm, log), log)

    @staticmethod
    def rle(sym):
        return Tab(1, bytes([sym]), [(sym, 0, 0)], 0)

    @staticmethod
    def fse(norm, log):
        return Tab(2, ncount(norm, log), fse_table(norm, log), log)

    def repeat(self):
        return Tab(3, b"", self.table, self.log)


def code_of(bases, v):
    c = max(i for i, b in enumerate(bases) if b <= v)
    return c, v - bases[c]


def seq(ll, ml, ofv):
    """(literal length, match length, offset VALUE: 1 .. 3 the repeat codes, offset + 3 beyond) -> codes and extra bits"""
    lc, lx = code_of(LL_BASE, ll); mc, mx = code_of(ML_BASE, ml)
    oc = ofv.bit_length() - 1
    return (lc, lx, oc, ofv - (1 << oc), mc, mx)


def count_bytes(n, form=None):
    form = form or (1 if n < 128 else 2 if n < 0x7F00 else 3)
    if form == 1:
        assert n < 128
        return bytes([n])
    if form == 2:
        assert n < 0x7F00
        return bytes([128 + (n >> 8), n & 255])
    return b"\xff" + ((n - 0x7F00) & 0xFFFF).to_bytes(2, "little")


def sequences(seqs, ll, of, ml, form=None, reserved=0, picks=(0, 0, 0), count=None):
    """The sequences section: count, modes byte, the three descriptions, the bitstream.  seqs: [(ll code, extra, of code, extra, ml code, extra)]"""
    n = len(seqs) if count is None else count
    head = count_bytes(n, form)
    if not seqs:
        return head
    head += bytes([(ll.mode << 6) | (of.mode << 4) | (ml.mode << 2) | reserved]) + ll.desc + of.desc + ml.desc
    sl, tl = fse_chain(ll.table, [s[0] for s in seqs], picks[0])
    so, to = fse_chain(of.table, [s[2] for s in seqs], picks[1])
    sm, tm = fse_chain(ml.table, [s[4] for s in seqs], picks[2])
    b = BackBits()
    b.put(sl, ll.log); b.put(so, of.log); b.put(sm, ml.log)
    for i, (lc, lx, oc, ox, mc, mx) in enumerate(seqs):
        b.put(ox, oc); b.put(mx, ML_BITS[mc]); b.put(lx, LL_BITS[lc])
        if i + 1 < len(seqs):
            b.put(*tl[i]); b.put(*tm[i]); b.put(*to[i])
    return head + b.bytes()


# ---------------------------------------------------------------- literals ----
def lit_plain(ltype, data, sf, regen=None):
    """Raw (0) / RLE (1) literals: sf 0 -- 1 byte, 5 bits (the format is one bit there); 1 -- 2 bytes, 12 bits; 3 -- 3 bytes, 20 bits"""
    n = len(data) if regen is None else regen
    body = data if ltype == 0 else data[:1]
    if sf == 0:
        assert n < 32
        return bytes([ltype | (n << 3)]) + body
    if sf == 1:
        assert n < 4096
        return (ltype | (1 << 2) | (n << 4)).to_bytes(2, "little") + body
    return (ltype | (3 << 2) | (n << 4)).to_bytes(3, "little") + body


class Huf:
    """A Huffman code from weights (the last one included): code lengths and values as the decoder's table has them"""
    def __init__(self, weights):
        self.weights = list(weights)
        total = sum(1 << (w - 1) for w in weights if w)
        self.log = total.bit_length() - 1
        assert total == 1 << self.log, "the weights do not complete a power of two"
        self.code = {}
        pos = 0
        for w in range(1, self.log + 1):
            for s, x in enumerate(weights):
                if x == w:
                    self.code[s] = (pos >> (w - 1), self.log + 1 - w)
                    pos += 1 << (w - 1)

    def direct(self, listed=None):
        """the tree description with the weights written as nibbles (the last weight is implied)"""
        ws = self.weights[:-1] if listed is None else listed
        assert 1 <= len(ws) <= 128
        p = ws + [0] * (len(ws) & 1)
        return bytes([127 + len(ws)]) + bytes((p[i] << 4) | p[i + 1] for i in range(0, len(p), 2))

    def compressed(self, norm, log):
        """the tree description with the weights FSE-compressed: two interleaved states, as FSE_compress has it"""
        ws = self.weights[:-1]
        table = fse_table(norm, log)
        s1, t1 = fse_chain(table, ws[0::2]); s2, t2 = fse_chain(table, ws[1::2])
        b = BackBits()
        b.put(s1, log); b.put(s2, log)
        for i in range(len(ws)):
            t = (t1 if i % 2 == 0 else t2)[i // 2]
            if t:
                b.put(*t)
        body = ncount(norm, log) + b.bytes()
        assert len(body) < 128
        return bytes([len(body)]) + body

    def stream(self, data, pad=None):
        b = BackBits()
        if pad:
            b.put(0, pad)                     # bits between the end mark and the first code: an under-consumed stream
        for x in data:
            b.put(*self.code[x])
        return b.bytes()


def lit_huf(huf, data, sf, tree=None, ltype=2, regen=None, jump=None, streams=None, comp=None):
    """Huffman-coded literals (ltype 2 with a tree description, 3 without).  sf 0: 1 stream, 10-bit sizes; 1, 2, 3: 4 streams with 10-,
    14- and 18-bit sizes."""
    n = len(data) if regen is None else regen
    tree = (huf.direct() if tree is None else tree) if ltype == 2 else b""
    if sf == 0:
        body = streams[0] if streams else huf.stream(data)
    else:
        seg = (len(data) + 3) // 4
        st = streams or [huf.stream(data[i * seg:(i + 1) * seg]) for i in range(4)]
        j = jump or [len(x) for x in st[:3]]
        body = b"".join(x.to_bytes(2, "little") for x in j) + b"".join(st)
    c = len(tree) + len(body) if comp is None else comp
    bits, hsize = ((10, 3), (10, 3), (14, 4), (18, 5))[sf]
    assert n < (1 << bits) and c < (1 << bits), (n, c)
    return (ltype | (sf << 2) | (n << 4) | (c << (4 + bits))).to_bytes(hsize, "little") + tree + body


# ---------------------------------------------------------------- blocks and frames ----
def block(body, btype=2, last=0, size=None):
    return (((len(body) if size is None else size) << 3) | (btype << 1) | last).to_bytes(3, "little") + body


def raw(data, last=0):
    return block(data, 0, last)


def rle(byte, n, last=0):
    return block(bytes([byte]), 1, last, size=n)


def xxh64(data):
    P1, P2, P3, P4, P5, M = 11400714785074694791, 14029467366897019727, 1609587929392839161, 9650029242287828579, 2870177450012600261, (1 << 64) - 1
    rotl = lambda x, r: ((x << r) | (x >> (64 - r))) & M                  # noqa: E731
    rnd = lambda a, x: (rotl((a + x * P2) & M, 31) * P1) & M              # noqa: E731
    i, n = 0, len(data)
    if n >= 32:
        v = [(P1 + P2) & M, P2, 0, (-P1) & M]
        while i + 32 <= n:
            for k in range(4):
                v[k] = rnd(v[k], int.from_bytes(data[i + 8 * k:i + 8 * k + 8], "little"))
            i += 32
        h = (rotl(v[0], 1) + rotl(v[1], 7) + rotl(v[2], 12) + rotl(v[3], 18)) & M
        for k in range(4):
            h = ((h ^ rnd(0, v[k])) * P1 + P4) & M
    else:
        h = P5
    h = (h + n) & M
    while i + 8 <= n:
        h = (rotl(h ^ rnd(0, int.from_bytes(data[i:i + 8], "little")), 27) * P1 + P4) & M; i += 8
    if i + 4 <= n:
        h = (rotl(h ^ (int.from_bytes(data[i:i + 4], "little") * P1) & M, 23) * P2 + P3) & M; i += 4
    while i < n:
        h = (rotl(h ^ (data[i] * P5) & M, 11) * P1) & M; i += 1
    h ^= h >> 33; h = (h * P2) & M; h ^= h >> 29; h = (h * P3) & M; h ^= h >> 32
    return h


W17 = (17 - 10) << 3            # a window of 128 KiB: every block size is allowed


def frame(blocks, window=W17, single=None, fcs=None, did_code=0, did=0, fcs_code=0, checksum=None, reserved=0, unused=0):
    """A frame header in front of the blocks.  single: the declared content size of a single-segment frame; else a window descriptor
    byte and, with fcs, a content size field.  fcs_code 1, 2, 3: the field has 2, 4, 8 bytes (0: 1 byte, single-segment frames only).
    checksum: None, or the content the XXH64 word is computed over, or an int (the word itself)"""
    fhd = (fcs_code << 6) | ((single is not None) << 5) | (unused << 4) | (reserved << 3) | ((checksum is not None) << 2) | did_code
    out = MAGIC + bytes([fhd])
    if single is None:
        out += bytes([window])
    out += did.to_bytes((0, 1, 2, 4)[did_code], "little")
    size = single if single is not None else fcs
    assert (size is not None) == (single is not None or fcs_code != 0)
    if size is not None:
        out += (size - 256 if fcs_code == 1 else size).to_bytes((1, 2, 4, 8)[fcs_code], "little")
    out += blocks
    if checksum is not None:
        out += ((xxh64(checksum) if isinstance(checksum, (bytes, bytearray)) else checksum) & 0xFFFFFFFF).to_bytes(4, "little")
    return out


def _block_heads(f):
    """where the block headers of a well-formed single frame lie"""
    fhd = f[4]
    pos = 5 + (0 if fhd & 0x20 else 1) + (0, 1, 2, 4)[fhd & 3] + ((1 if fhd & 0x20 else 0), 2, 4, 8)[fhd >> 6]
    out = []
    while pos + 3 <= len(f):
        bh = int.from_bytes(f[pos:pos + 3], "little")
        out.append(pos)
        pos += 3 + (1 if (bh >> 1) & 3 == 1 else bh >> 3)
        if bh & 1:
            break
    return out


def skippable(k, payload=b""):
    return (0x184D2A50 + k).to_bytes(4, "little") + len(payload).to_bytes(4, "little") + payload


# ---------------------------------------------------------------- a model of the sequence execution (sizes and intents only) ----
def execute(history, lits, seqs, rep=(1, 4, 8), dict_size=0):
    """What a block regenerates behind `history` (the frame's output so far; dict_size more bytes of unknown content lie before it), or
    None where a sequence is invalid.  seqs: [(ll, ml, offset value)].  -> (block bytes with '?' for dictionary bytes, repeat offsets)"""
    out = bytearray(history); rep = list(rep); lp = 0
    for ll, ml, ofv in seqs:
        if lp + ll > len(lits):
            return None
        out += lits[lp:lp + ll]; lp += ll
        if ofv > 3:
            off = ofv - 3; rep = [off, rep[0], rep[1]]
        else:
            idx = ofv - 1 + (ll == 0)
            if idx == 0:
                off = rep[0]
            else:
                off = rep[idx] if idx < 3 else rep[0] - 1
                if off == 0:
                    return None
                rep = [off, rep[0], rep[1]] if idx != 1 else [off, rep[0], rep[2]]
        if off > len(out) + dict_size:
            return None
        for _ in range(ml):
            out.append(out[-off] if off <= len(out) else 0x3F)
    out += lits[lp:]
    if len(out) - len(history) > BLOCK_MAX:
        return None
    return bytes(out[len(history):]), tuple(rep)


def seq_block(lits, seqs, tabs=None, last=1, lit_sf=None, **kw):
    """A compressed block: raw literals, the sequences (ll, ml, offset value) through RLE-free tables given, or predefined ones"""
    ll, of, ml = tabs or (Tab.predefined("ll"), Tab.predefined("of"), Tab.predefined("ml"))
    sf = lit_sf if lit_sf is not None else (0 if len(lits) < 32 else 1 if len(lits) < 4096 else 3)
    return block(lit_plain(0, lits, sf) + sequences([seq(*s) for s in seqs], ll, of, ml, **kw), 2, last)


def one_seq_block(lits, ll, ml, ofv, last=1, lc=None, mc=None, oc=None, lx=None, mx=None, ox=None):
    """A block of one sequence through three RLE-mode tables: any code, any extra bits"""
    s = list(seq(ll, ml, ofv))
    for i, v in enumerate((lc, lx, oc, ox, mc, mx)):
        if v is not None:
            s[i] = v
    sf = 0 if len(lits) < 32 else 1 if len(lits) < 4096 else 3
    return block(lit_plain(0, lits, sf) + sequences([tuple(s)], Tab.rle(s[0]), Tab.rle(s[2]), Tab.rle(s[4])), 2, last)


def seeded(n, seed):
    return random.Random(seed).randbytes(n)


def text(n, seed):
    """n bytes over a small alphabet with repeats (compressible history)"""
    r = random.Random(seed)
    words = [bytes(r.choice(b"abcdefghij klmnop") for _ in range(r.randrange(2, 9))) for _ in range(40)]
    out = bytearray()
    while len(out) < n:
        out += r.choice(words)
    return bytes(out[:n])


# ---------------------------------------------------------------- the families ----
def _header(add):
    abc = b"abc"; big = text(300, 1)
    for fhd in range(256):
        if fhd & 0x18:                                     # reserved bit (below), unused bit (two of them below)
            continue
        fcs_code, single, did_code, chk = fhd >> 6, (fhd >> 5) & 1, fhd & 3, (fhd >> 2) & 1
        data = big if fcs_code == 1 else abc
        if single:
            f = frame(raw(data, 1), single=len(data), fcs_code=fcs_code, did_code=did_code, checksum=data if chk else None)
        else:
            f = frame(raw(data, 1), window=0, fcs=len(data) if fcs_code else None, fcs_code=fcs_code, did_code=did_code, checksum=data if chk else None)
        assert f[4] == fhd, (f[4], fhd)
        add("header", f"descriptor {fhd:#04x}", f, len(data) + 8, None, "ok")
    add("header", "unused bit set", frame(raw(abc, 1), unused=1), 8, None, "ok")
    add("header", "unused bit set, single segment", frame(raw(abc, 1), single=3, unused=1), 8, None, "ok")
    add("header", "reserved bit set", frame(raw(abc, 1), reserved=1), 8, None, "reject")
    for did_code in (1, 2, 3):
        add("header", f"dictionary ID 5 in code {did_code}, none loaded", frame(raw(abc, 1), did_code=did_code, did=5), 8, None, "reject")
    for log in (10, 17, 31, 32):
        for mant in (0, 7):
            add("header", f"window log {log} mantissa {mant}", frame(raw(abc, 1), window=((log - 10) << 3) | mant), 8, None, "ok" if log < 32 else "reject")
    add("header", "declares 4, holds 3", frame(raw(abc, 1), single=4), 8, None, "reject")
    add("header", "declares 2, holds 3", frame(raw(abc, 1), single=2), 8, None, "reject")
    add("header", "window frame declares 2, holds 3", frame(raw(abc, 1), fcs=2, fcs_code=2), 8, None, "reject")
    for code, width in ((2, 4), (3, 8)):
        add("header", f"content size 3 in {width} bytes", frame(raw(abc, 1), fcs=3, fcs_code=code), 8, None, "ok")
        add("header", f"content size 3 in {width} bytes, single segment", frame(raw(abc, 1), single=3, fcs_code=code), 8, None, "ok")
    add("header", "content size 256 in 2 bytes", frame(raw(big[:256], 1), fcs=256, fcs_code=1), 256, None, "ok")
    add("header", "capacity below the content", frame(raw(abc, 1)), 2, None, "reject")
    add("header", "capacity below the declared size", frame(raw(abc, 1), single=3), 2, None, "reject")
    for n in (0, 1, 31, 32, 33):
        data = seeded(n, 40 + n)
        add("header", f"checksum right over {n}", frame(raw(data, 1), checksum=data), n, None, "ok")
        add("header", f"checksum wrong over {n}", frame(raw(data, 1), checksum=xxh64(data) ^ 0x10000), n, None, "reject")
        add("header", f"checksum missing over {n}", frame(raw(data, 1), checksum=data)[:-4], n, None, "reject")
        add("header", f"checksum cut over {n}", frame(raw(data, 1), checksum=data)[:-1], n, None, "reject")


def _lit_block(lits, last=1):
    return block(lits + b"\x00", 2, last)                 # a literals section and a sequence count of 0


def _blocks(add):
    abc = b"abc"
    add("blocks", "empty raw blocks before data", frame(raw(b"") + raw(b"") + raw(abc, 1)), 8, None, "ok")
    add("blocks", "empty raw last block", frame(raw(abc) + raw(b"", 1)), 8, None, "ok")
    add("blocks", "RLE block of size 0", frame(rle(0x41, 0) + raw(abc, 1)), 8, None, "ok")
    add("blocks", "RLE block of size 0, last", frame(raw(abc) + rle(0x41, 0, 1)), 8, None, "ok")
    add("blocks", "empty compressed non-last block", frame(_lit_block(b"\x00", 0) + raw(abc, 1)), 8, None, "ok")
    add("blocks", "block type 3", frame(block(abc, 3, 1)), 8, None, "reject")
    add("blocks", "block type 3 behind data", frame(raw(abc) + block(abc, 3, 1)), 8, None, "reject")
    big = seeded(BLOCK_MAX + 1, 7)
    for extra in (0, 1):
        n = BLOCK_MAX + extra
        # (the one-shot call checks neither the raw nor the RLE block's size, nor what a block's sequences regenerate)
        add("blocks", f"raw block of 128 KiB + {extra}", frame(raw(big[:n], 1), window=W17), n, None, "ok")
        add("blocks", f"RLE block of 128 KiB + {extra}", frame(rle(0x5A, n, 1), window=W17), n, None, "ok")
        add("blocks", f"RLE literals of 128 KiB + {extra}", frame(_lit_block(lit_plain(1, b"\x5a", 3, regen=n)), window=W17), n, None, "ok" if not extra else "reject")
        # 70 000 bytes of history, then 7 literals and one match that fills the block to 128 KiB (+ 1)
        hist = big[:70000]
        add("blocks", f"sequences regenerating 128 KiB + {extra}", frame(raw(hist) + one_seq_block(b"literal", 7, n - 7, 70000 + 3), window=W17), 70000 + n, None, "ok")
    add("blocks", "compressed block of 6 in a single segment of 4", frame(_lit_block(lit_plain(0, b"abcd", 0)), single=4), 8, None, "reject")
    add("blocks", "compressed block of 4 in a single segment of 4", frame(block(lit_plain(1, b"x", 0, regen=4) + b"\x80\x00", 2, 1), single=4), 8, None, "ok")
    add("blocks", "compressed block of 3 in a single segment of 4", frame(_lit_block(lit_plain(1, b"x", 0, regen=4)), single=4), 8, None, "ok")
    add("blocks", "compressed block in a single segment of 0", frame(_lit_block(b"\x00"), single=0), 8, None, "reject")
    k1 = seeded(1100, 9)
    add("blocks", "compressed block above a 1 KiB window", frame(block(lit_plain(0, k1[:1030], 1) + b"\x00", 2, 1), window=0), 2000, None, "reject")
    add("blocks", "compressed block of a 1 KiB window", frame(block(lit_plain(0, k1[:1021], 1) + b"\x00", 2, 1), window=0), 2000, None, "ok")
    add("blocks", "raw block above a 1 KiB window", frame(raw(k1, 1), window=0), 2000, None, "ok")
    add("blocks", "RLE block above a 1 KiB window", frame(rle(7, 5000, 1), window=0), 5000, None, "ok")
    add("blocks", "RLE literals above a 1 KiB window", frame(_lit_block(lit_plain(1, b"x", 1, regen=1025)), window=0), 2000, None, "reject")
    add("blocks", "RLE literals of a 1 KiB window", frame(_lit_block(lit_plain(1, b"x", 1, regen=1024)), window=0), 2000, None, "ok")
    # (sequences regenerating more than the window's 1 KiB: the library's answer depends on where it keeps the literals, which depends on
    # the capacity -- DESIGN.md; no case here)
    add("blocks", "no last block", frame(raw(abc) + raw(abc)), 8, None, "reject")
    add("blocks", "no block", frame(b""), 8, None, "reject")
    add("blocks", "bytes after the last block", frame(raw(abc, 1)) + b"\x00", 8, None, "reject")
    add("blocks", "raw block cut", frame(raw(abc, 1))[:-1], 8, None, "reject")
    add("blocks", "RLE block without its byte", frame(rle(1, 3, 1))[:-1], 8, None, "reject")
    add("blocks", "compressed block of 1 byte", frame(block(b"\x00", 2, 1)), 8, None, "reject")
    add("blocks", "compressed block of 0 bytes", frame(block(b"", 2, 1)), 8, None, "reject")


def _depth_weights(d):
    """weights whose longest code has d bits: 1, 1, 2, 3, .. d"""
    return [1, 1] + list(range(2, d + 1))


def _literals(add):
    for ltype, tname in ((0, "raw"), (1, "RLE")):
        for n in (0, 1, 31, 32, 4095, 4096):
            data = seeded(n, 100 + n) if ltype == 0 else bytes([0x61]) * max(n, 1)
            for sf in (0, 1, 3):
                if (sf == 0 and n >= 32) or (sf == 1 and n >= 4096):
                    continue
                add("literals", f"{tname} literals of {n}, format {sf}", frame(_lit_block(lit_plain(ltype, data, sf, regen=n))), n, None, "ok")
    abc = Huf([3, 2, 1, 1])                               # symbols 0 .. 3
    d1 = bytes(random.Random(5).choices([0, 1, 2, 3], [4, 2, 1, 1], k=200))
    for sf in range(4):
        add("literals", f"Huffman literals, format {sf}", frame(_lit_block(lit_huf(abc, d1, sf))), 200, None, "ok")
    for n in (5, 6, 8):
        d = bytes([0, 1, 2, 3, 0, 0, 1, 0][:n])
        streams = None
        if n == 5:                                        # segments of 2, 2, 2 and -1: the streams of 6 literals, the header says 5
            streams = [abc.stream(x) for x in (d[0:2], d[2:4], d[4:5] + b"\x00", b"\x00")]
        add("literals", f"4 streams of {n} literals", frame(_lit_block(lit_huf(abc, d, 1, regen=n, streams=streams))), 8, None, "ok" if n >= 6 else "reject")
    add("literals", "4 streams of 4 literals", frame(_lit_block(lit_huf(abc, b"\x00\x01\x02\x03", 1))), 8, None, "reject")
    # direct weights, 1, 2, 127 and 128 listed
    add("literals", "1 listed weight", frame(_lit_block(lit_huf(Huf([1, 1]), b"\x00\x01\x01\x00\x00", 0))), 8, None, "ok")
    add("literals", "2 listed weights", frame(_lit_block(lit_huf(Huf([2, 1, 1]), b"\x00\x01\x02\x00\x00", 0))), 8, None, "ok")
    for listed in (127, 128):
        w = [0] * (listed + 1); w[0] = 2; w[listed - 1] = 1; w[listed] = 1
        d = bytes([0, listed - 1, listed, 0, 0, listed])
        add("literals", f"{listed} listed weights", frame(_lit_block(lit_huf(Huf(w), d, 0))), 8, None, "ok")
    for d in range(1, 13):
        w = _depth_weights(d)
        data = bytes(range(len(w))) * 2
        add("literals", f"tree depth {d}", frame(_lit_block(lit_huf(Huf(w), data, 0))), 64, None, "ok")
        add("literals", f"tree depth {d}, 4 streams", frame(_lit_block(lit_huf(Huf(w), data * 2, 1))), 64, None, "ok")
        # (depth 12 is beyond RFC 8878's 11 and libzstd 1.5.7 decodes it all the same: REFUSED_THOUGH_ACCEPTED)
    h = Huf([2, 1, 1])
    add("literals", "weights that complete no power of two", frame(_lit_block(lit_huf(h, b"\x00\x01", 0, tree=h.direct([2, 1, 2])))), 8, None, "reject")
    add("literals", "no symbol of weight 1", frame(_lit_block(lit_huf(Huf([1, 1]), b"\x00\x00", 0, tree=bytes([129, 0x22])))), 8, None, "reject")
    add("literals", "three symbols of weight 1", frame(_lit_block(lit_huf(Huf([1, 1]), b"\x00\x00", 0, tree=bytes([131, 0x11, 0x12])))), 8, None, "reject")
    add("literals", "a weight of 13", frame(_lit_block(lit_huf(Huf([1, 1]), b"\x00\x00", 0, tree=bytes([129, 0x1D])))), 8, None, "reject")
    add("literals", "all weights zero", frame(_lit_block(lit_huf(Huf([1, 1]), b"\x00\x00", 0, tree=bytes([129, 0x00])))), 8, None, "reject")
    # FSE-compressed weights at logs 5 and 6: 30 symbols of weights 1 .. 4; no weight takes more than half the table, so every state
    # reads a bit at least and the weights' stream ends where the decoder runs out of bits
    for log, norm in ((5, [0, 16, 9, 5, 2]), (6, [0, 32, 18, 9, 5])):
        r = random.Random(log)
        w = [4, 4, 3, 3, 3, 3] + [2] * 8 + [1] * 16
        r.shuffle(w)
        hw = Huf(w)
        data = bytes(r.randrange(len(w)) for _ in range(100))
        add("literals", f"FSE-compressed weights, log {log}", frame(_lit_block(lit_huf(hw, data, 0, tree=hw.compressed(norm, log)))), 100, None, "ok")
        add("literals", f"FSE-compressed weights, log {log}, 4 streams", frame(_lit_block(lit_huf(hw, data, 2, tree=hw.compressed(norm, log)))), 100, None, "ok")
    add("literals", "FSE-compressed weights, log 7", frame(_lit_block(lit_huf(abc, d1, 0, tree=bytes([3]) + ncount([0, 64, 64], 7, first_bits=2) + b"\x01"))), 200, None, "reject")
    # the jump table, the sizes
    st = [abc.stream(d1[i * 50:(i + 1) * 50]) for i in range(4)]
    add("literals", "jump table past the section", frame(_lit_block(lit_huf(abc, d1, 1, streams=st, jump=[len(st[0]), len(st[1]), 900]))), 200, None, "reject")
    add("literals", "jump table with an empty stream", frame(_lit_block(lit_huf(abc, d1, 1, streams=st, jump=[len(st[0]), 0, len(st[2])]))), 200, None, "reject")
    d8 = bytes([0, 1, 2, 3, 0, 0, 1, 0])
    add("literals", "compressed size above the regenerated size", frame(_lit_block(lit_huf(abc, d8, 0))), 8, None, "ok")
    add("literals", "compressed size beyond the block", frame(_lit_block(lit_huf(abc, d1, 0, comp=500))), 200, None, "reject")
    add("literals", "compressed size 0", frame(_lit_block(lit_huf(abc, d1, 0, comp=0, tree=b"", streams=[b""]) + b"\x00\x00")), 200, None, "reject")
    # tree-less literals
    b1 = _lit_block(lit_huf(abc, d1, 0), 0)
    tl = lambda last=1, sf=0: _lit_block(lit_huf(abc, d1[::-1], sf, ltype=3), last)          # noqa: E731
    add("literals", "tree-less after a tree", frame(b1 + tl()), 400, None, "ok")
    add("literals", "tree-less with 4 streams after a tree", frame(b1 + tl(sf=1)), 400, None, "ok")
    add("literals", "tree-less twice", frame(b1 + tl(0) + tl()), 600, None, "ok")
    add("literals", "tree-less across a raw block", frame(b1 + raw(b"xyz") + tl()), 403, None, "ok")
    add("literals", "tree-less across an RLE block", frame(b1 + rle(9, 3) + tl()), 403, None, "ok")
    add("literals", "tree-less across raw literals", frame(b1 + _lit_block(lit_plain(0, b"xyz", 0), 0) + tl()), 403, None, "ok")
    add("literals", "tree-less across RLE literals", frame(b1 + _lit_block(lit_plain(1, b"x", 0, regen=3), 0) + tl()), 403, None, "ok")
    add("literals", "tree-less as the first block", frame(tl()), 400, None, "reject")
    add("literals", "tree-less in a second frame", frame(b1 + raw(b"", 1)) + frame(tl()), 400, None, "reject")
    # a stream composed to be under-consumed (bits between the end mark and the first code) and over-consumed (a code cut short)
    dl = bytes(random.Random(6).choices([0, 1, 2, 3], [4, 2, 1, 1], k=4000))
    sl = [abc.stream(dl[i * 1000:(i + 1) * 1000]) for i in range(4)]
    add("literals", "Huffman stream under-consumed", frame(_lit_block(lit_huf(abc, dl, 2, streams=[abc.stream(dl[:1000], pad=3)] + sl[1:]))), 4000, None, "lenient")
    add("literals", "Huffman stream over-consumed", frame(_lit_block(lit_huf(abc, dl, 2, streams=[abc.stream(dl[:999])] + sl[1:]))), 4000, None, "lenient")
    add("literals", "short Huffman stream under-consumed", frame(_lit_block(lit_huf(abc, d1, 0, streams=[abc.stream(d1, pad=3)]))), 200, None, "reject")
    add("literals", "short Huffman stream over-consumed", frame(_lit_block(lit_huf(abc, d1 + b"\x02", 0, streams=[abc.stream(d1)]))), 201, None, "reject")


def _rle_tabs(lc, oc, mc):
    return Tab.rle(lc), Tab.rle(oc), Tab.rle(mc)


def _seqhdr(add):
    lits = b"abcdefgh"
    P = (Tab.predefined("ll"), Tab.predefined("of"), Tab.predefined("ml"))
    # the count in its three forms
    for form in (1, 2, 3):
        for n in (0, 1, 127, 128):
            if form == 1 and n > 127:
                continue
            name = f"count {n} in {form} byte{'s' if form > 1 else ''}"
            if form == 3:
                # the 3-byte form counts from 0x7F00: the four values there
                n3 = 0x7F00 + n
                seqs = [(0, 3, 1)] * n3
                body = lit_plain(0, lits, 0) + sequences([seq(*s) for s in seqs], *_rle_tabs(0, 0, 0), form=3)
                add("seqhdr", f"count 0x7F00 + {n} in 3 bytes", frame(raw(b"zyxwvuts") + block(body, 2, 1)), 8 + 8 + 3 * n3, None, "ok")
                continue
            seqs = [(0, 3, 1)] * n
            body = lit_plain(0, lits, 0) + sequences([seq(*s) for s in seqs], *_rle_tabs(0, 0, 0), form=form)
            add("seqhdr", name, frame(raw(b"zyxwvuts") + block(body, 2, 1)), 8 + 8 + 3 * n, None, "ok")
    add("seqhdr", "count 0 followed by a byte", frame(block(lit_plain(0, b"abcd", 0) + b"\x00\x00", 2, 1)), 8, None, "reject")
    add("seqhdr", "count 0 in 2 bytes followed by a byte", frame(block(lit_plain(0, b"abcd", 0) + b"\x80\x00\x00", 2, 1)), 8, None, "reject")
    add("seqhdr", "count 1 and nothing else", frame(block(lit_plain(0, b"abcd", 0) + b"\x01", 2, 1)), 8, None, "reject")
    add("seqhdr", "count 1 and modes only", frame(block(lit_plain(0, b"abcd", 0) + b"\x01\x00", 2, 1)), 8, None, "reject")
    add("seqhdr", "no count", frame(block(lit_plain(0, b"abcd", 0), 2, 1)), 8, None, "reject")
    for r in (1, 2, 3):
        add("seqhdr", f"reserved mode bits {r}", frame(raw(b"z") + seq_block(lits, [(2, 3, 1)], reserved=r)), 32, None, "reject")
    # the 4 x 3 mode combinations, one type at a time (the others predefined), two sequences each
    flat = {"ll": ([2] * 16 + [0] * 20, 5), "of": ([4] * 8, 5), "ml": ([1] * 32 + [0] * 21, 5)}
    seqs = [(2, 4, 1 + 3), (1, 3, 1)]
    for ti, kind in enumerate(("ll", "of", "ml")):
        first = [Tab.predefined(k) for k in ("ll", "of", "ml")]
        variants = {"Predefined": Tab.predefined(kind), "RLE": None, "FSE": Tab.fse(*flat[kind])}
        for mname, tab in variants.items():
            if tab is None:
                # RLE: both sequences carry the same code of this type
                s2 = [(2, 4, 4), (2, 4, 4)]
                c = seq(*s2[0])[2 * ti]
                tabs = list(first); tabs[ti] = Tab.rle(c)
                add("seqhdr", f"{kind} table RLE", frame(raw(b"zyxwvutsrqponmlk") + seq_block(lits, s2, tabs)), 64, None, "ok")
                prev, ps = tabs, s2
            else:
                tabs = list(first); tabs[ti] = tab
                add("seqhdr", f"{kind} table {mname}", frame(raw(b"zyxwvutsrqponmlk") + seq_block(lits, seqs, tabs)), 64, None, "ok")
                prev, ps = tabs, seqs
            # ... and Repeat behind it: in the next block, across a raw block
            rep = list(first); rep[ti] = prev[ti].repeat()
            b1 = seq_block(lits, ps, prev, last=0)
            add("seqhdr", f"{kind} table Repeat after {mname}", frame(raw(b"zyxwvutsrqponmlk") + b1 + seq_block(lits, ps, rep)), 64, None, "ok")
            add("seqhdr", f"{kind} table Repeat after {mname} across a raw block", frame(raw(b"zyxwvutsrqponmlk") + b1 + raw(b"q") + seq_block(lits, ps, rep)), 64, None, "ok")
            add("seqhdr", f"{kind} table Repeat after {mname} across a block of no sequences", frame(raw(b"zyxwvutsrqponmlk") + b1 + _lit_block(b"\x00", 0) + seq_block(lits, ps, rep)), 64, None, "ok")
        rep = list(first); rep[ti] = first[ti].repeat()
        add("seqhdr", f"{kind} table Repeat as the first block", frame(raw(b"zyxwvutsrqponmlk") + seq_block(lits, seqs, rep)), 64, None, "reject")
        add("seqhdr", f"{kind} table Repeat in a second frame", frame(raw(b"zyxwvutsrqponmlk") + seq_block(lits, seqs, first)) + frame(raw(b"zyxwvutsrqponmlk") + seq_block(lits, seqs, rep)), 64, None, "reject")
    allrep = [t.repeat() for t in P]
    add("seqhdr", "all tables Repeat after Predefined", frame(raw(b"zyxwvutsrqponmlk") + seq_block(lits, seqs, P, last=0) + seq_block(lits, seqs, allrep)), 64, None, "ok")
    # RLE symbols beyond the alphabets
    for kind, sym in (("ll", 36), ("ml", 53), ("of", 32)):
        tabs = list(P); ti = ("ll", "of", "ml").index(kind); tabs[ti] = Tab.rle(0); tabs[ti].desc = bytes([sym])
        add("seqhdr", f"{kind} RLE symbol {sym}", frame(raw(b"zyxwvutsrqponmlk") + seq_block(lits, [(0, 3, 1)], tabs)), 64, None, "reject")
    # FSE descriptions
    hist = raw(b"zyxwvutsrqponmlk")
    for kind in ("ll", "of", "ml"):
        ti = ("ll", "of", "ml").index(kind)
        nsym = {"ll": 16, "of": 8, "ml": 32}[kind]        # (codes without extra bits, small offsets)
        for log in range(5, MAX_LOG[kind] + 2):
            size = 1 << log
            norm = [size // nsym] * nsym
            tabs = list(P); tabs[ti] = Tab.fse(norm, log) if log <= 9 else Tab(2, ncount(norm, log, first_bits=log - 5), fse_table(norm, log), log)
            add("seqhdr", f"{kind} FSE log {log}", frame(hist + seq_block(lits, [(2, 4, 1), (1, 5, 1), (0, 3, 1)], tabs)), 64, None, "ok" if log <= MAX_LOG[kind] else "reject")
        for log in (5, MAX_LOG[kind]):
            tabs = list(P); tabs[ti] = Tab.fse([1 << log], log)      # code 0 owns the table: every state 0 bits
            s = {"ll": [(0, 3, 1)] * 3, "of": [(1, 3, 1)] * 3, "ml": [(1, 3, 1)] * 3}[kind]
            add("seqhdr", f"{kind} FSE one symbol owns the table, log {log}", frame(hist + seq_block(lits, s, tabs)), 64, None, "ok")
        norm = [-1] * 8 + [24]                               # eight "less than 1" counts and one symbol with the rest (log 5)
        tabs = list(P); tabs[ti] = Tab.fse(norm, 5)
        s = {"ll": [(8, 3, 1), (1, 3, 1), (8, 4, 1)], "of": [(0, 3, 1 << 8), (1, 3, 2), (1, 3, 1)], "ml": [(1, 11, 1), (1, 4, 1), (1, 11, 1)]}[kind]
        add("seqhdr", f"{kind} FSE counts of -1", frame(raw(seeded(300, 3)) + seq_block(lits * 3, s, tabs)), 400, None, "ok")
        top = MAX_SYM[kind] if kind != "of" else 20
        norm = [16] + [0] * (top - 1) + [16]                 # a zero run that chains the 3-flag
        tabs = list(P); tabs[ti] = Tab.fse(norm, 5)
        if kind == "of":
            add("seqhdr", "of FSE zero runs chained", frame(hist + seq_block(lits, [(1, 3, 1), (1, 3, 1)], tabs)), 64, None, "ok")
        else:
            s = [(0, 3, 1), (0, 3, 1)] if kind == "ll" else [(1, 3, 1), (1, 3, 1)]
            add("seqhdr", f"{kind} FSE zero runs chained", frame(hist + seq_block(lits, s, tabs)), 64, None, "ok")
        norm = [16] + [0] * MAX_SYM[kind] + [16]             # the second symbol lies beyond the alphabet
        tabs = list(P); tabs[ti] = Tab(2, ncount(norm, 5), fse_table([32], 5), 5)
        add("seqhdr", f"{kind} FSE symbol beyond the alphabet", frame(hist + seq_block(lits, [(0, 3, 1)], tabs)), 64, None, "reject")
        tabs = list(P); tabs[ti] = Tab(2, ncount([20, 20], 5), fse_table([32], 5), 5)
        add("seqhdr", f"{kind} FSE counts that overshoot", frame(hist + seq_block(lits, [(0, 3, 1)], tabs)), 64, None, "reject")
        tabs = list(P); tabs[ti] = Tab(2, ncount([20, 5], 5), fse_table([32], 5), 5)
        add("seqhdr", f"{kind} FSE counts that fall short", frame(hist + seq_block(lits, [(0, 3, 1)], tabs)), 64, None, "reject")
    body = lit_plain(0, lits, 0) + b"\x01" + bytes([2 << 6]) + ncount([2] * 16, 5)[:3]
    add("seqhdr", "FSE description cut off by the block end", frame(hist + block(body, 2, 1)), 64, None, "reject")
    body = lit_plain(0, lits, 0) + b"\x01" + bytes([2 << 6]) + ncount([2] * 16, 5)
    add("seqhdr", "FSE description and no bitstream", frame(hist + block(body, 2, 1)), 64, None, "reject")


def _seqval(add):
    H = seeded(70000, 11)
    hist = raw(H)
    lit = seeded(BLOCK_MAX, 12)
    W18 = (18 - 10) << 3
    for lc in range(36):
        for ones in (0, 1):
            x = ((1 << LL_BITS[lc]) - 1) * ones
            ll = LL_BASE[lc] + x
            if not ones or LL_BITS[lc]:
                add("seqval", f"literal length code {lc} extra bits {'ones' if ones else 'zero'}",
                    frame(hist + one_seq_block(lit[:ll], ll, 3, 4, lc=lc, lx=x), window=W18), 70000 + ll + 3, None, "ok" if ll + 8 <= BLOCK_MAX else "reject")
    for mc in range(53):
        for ones in (0, 1):
            x = ((1 << ML_BITS[mc]) - 1) * ones
            ml = ML_BASE[mc] + x
            if not ones or ML_BITS[mc]:
                add("seqval", f"match length code {mc} extra bits {'ones' if ones else 'zero'}",
                    frame(hist + one_seq_block(b"ab", 2, ml, 5, mc=mc, mx=x), window=W18), 70000 + ml + 2, None, "ok")
    for oc in range(32):
        for ones in (0, 1):
            if ones and not oc:
                continue
            ofv = (1 << oc) + ((1 << oc) - 1) * ones
            good = ofv <= 3 or ofv - 3 <= 70002
            if oc >= 17:
                good = False
            add("seqval", f"offset code {oc} extra bits {'ones' if ones else 'zero'}",
                frame(hist + one_seq_block(b"ab", 2, 4, ofv, oc=oc, ox=ofv - (1 << oc)), window=W18), 70000 + 6, None, "ok" if good else "reject")
    # the repeat-offset rules: chains of four sequences over offset values 1 .. 3 and literal lengths 0 / 1
    short = raw(text(40, 2))
    chains = []
    for a in (1, 2, 3):
        for la in (0, 1):
            for b in (1, 2, 3):
                for lb in (0, 1):
                    chains.append([(1, 3, 9 + 3), (la, 3, a), (lb, 4, b), (1 - la, 3, 3)])
    chains += [[(0, 3, 3), (0, 3, 1), (1, 3, 1), (0, 3, 2)], [(1, 3, 1 + 3), (0, 3, 3), (1, 3, 1), (0, 3, 1)],
               [(1, 3, 2 + 3), (0, 3, 3), (0, 3, 3), (0, 3, 3)], [(0, 3, 3), (0, 3, 3), (0, 3, 3), (0, 3, 3)]]
    for k, ch in enumerate(chains):
        lits = b"LMNOPQRS"[:sum(s[0] for s in ch) + 1]
        ok = execute(text(40, 2), lits, ch) is not None
        add("seqval", f"repeat offsets chain {k}: " + " ".join(f"{ll}/{ofv}" for ll, _, ofv in ch), frame(short + seq_block(lits, ch)), 128, None, "ok" if ok else "reject")
    add("seqval", "rep1 - 1 = 0", frame(raw(b"xy") + one_seq_block(b"", 0, 3, 3), window=0), 64, None, "reject")
    add("seqval", "rep1 - 1 = 0 in the second sequence", frame(raw(b"xy") + seq_block(b"a", [(1, 4, 1 + 3), (0, 3, 3)])), 64, None, "reject")
    add("seqval", "rep1 - 1 = 1", frame(raw(b"xy") + seq_block(b"a", [(1, 4, 2 + 3), (0, 3, 3)])), 64, None, "ok")
    # offsets at the position
    for extra, verdict in ((0, "ok"), (1, "reject")):
        add("seqval", f"offset equal to the position + {extra}", frame(raw(b"0123456789") + seq_block(b"ab", [(2, 4, 12 + extra + 3)])), 64, None, verdict)
        add("seqval", f"offset equal to the position + {extra} in the first block", frame(seq_block(b"ab", [(2, 4, 2 + extra + 3)])), 64, None, verdict)
        add("seqval", f"offset equal to the position + {extra} in a second frame", frame(raw(b"0123456789", 1)) + frame(seq_block(b"ab", [(2, 4, 2 + extra + 3)])), 64, None, verdict)
    # overlapping matches
    for off in (1, 2, 3, 7, 8, 63, 64, 65):
        for ml in (3, 64, 65, 65539, 70001):
            add("seqval", f"overlapping match offset {off} length {ml}", frame(raw(H[:100]) + one_seq_block(b"ab", 2, ml, off + 3), window=W18), 102 + ml, None, "ok")
    # sequences per block
    r = random.Random(77)
    for n in (1, 63, 64, 65, 127, 128, 2000):
        seqs = [(r.randrange(0, 4), r.randrange(3, 12), r.choice((1, 2, 3, r.randrange(4, 60)))) for _ in range(n)]
        lits = text(sum(s[0] for s in seqs) + 5, n)
        got = execute(H[:100], lits, seqs)
        add("seqval", f"{n} sequences in a block", frame(raw(H[:100]) + seq_block(lits, seqs)), 100 + (len(got[0]) if got else 0), None, "ok" if got else "reject")
    add("seqval", "literals left over after the last sequence", frame(hist + seq_block(b"abcdefgh", [(2, 4, 5)])), 70000 + 12, None, "ok")
    add("seqval", "literal lengths that exceed the literals", frame(hist + seq_block(b"ab", [(3, 4, 5)])), 70000 + 12, None, "reject")
    add("seqval", "literal lengths that exceed the literals in the second sequence", frame(hist + seq_block(b"ab", [(1, 4, 5), (2, 3, 1)])), 70000 + 12, None, "reject")
    good = seq_block(b"abcdefgh", [(2, 4, 5), (1, 3, 1)])
    add("seqval", "bitstream with a zero last byte", frame(hist + block(good[3:] + b"\x00", 2, 1)), 70000 + 20, None, "reject")
    add("seqval", "bitstream with a byte too many", frame(hist + block(good[3:-1] + b"\x00" + good[-1:], 2, 1)), 70000 + 20, None, "reject")
    add("seqval", "bitstream a byte short", frame(hist + block(good[3:-2] + good[-1:], 2, 1)), 70000 + 20, None, "reject")
    # repeat offsets carried across raw and RLE blocks
    for name, mid in (("a raw block", raw(b"0123456789")), ("an RLE block", rle(0x2E, 10)), ("a block of no sequences", _lit_block(lit_plain(0, b"0123456789", 0), 0))):
        add("seqval", f"repeat offsets across {name}", frame(raw(H[:50]) + seq_block(b"ab", [(1, 4, 17 + 3), (1, 3, 30 + 3)], last=0) + mid + seq_block(b"cd", [(1, 5, 1), (0, 3, 1), (1, 3, 3)])),
            256, None, "ok")
    add("seqval", "capacity one below the sequences' output", frame(raw(H[:50]) + seq_block(b"ab", [(2, 40, 17 + 3)])), 50 + 41, None, "reject")
    add("seqval", "capacity one below the leftover literals", frame(raw(H[:50]) + seq_block(b"abcdef", [(2, 4, 17 + 3)])), 50 + 9, None, "reject")


def _helpers():
    here = os.path.dirname(os.path.abspath(__file__))
    sys.path[:0] = [here, os.path.dirname(here)]
    import helpers
    return helpers


def _multi(add):
    abc = frame(raw(b"abc", 1))
    # the smallest of libzstd's own frames in tests/golden/foreign_frames.bin that holds a compressed block
    enc, plain = min(((f, p) for _, f, p in _helpers().foreign_frames() if 0 < len(p) <= 20000 and any((int.from_bytes(f[h:h + 3], "little") >> 1) & 3 == 2 for h in _block_heads(f))),
                     key=lambda fp: (len(fp[0]), fp[0]))
    for k in range(16):
        add("multi", f"skippable magic {k} with size 0", skippable(k) + abc, 8, None, "ok")
    add("multi", "skippable frame alone", skippable(3, b"hello"), 8, None, "ok")
    add("multi", "skippable frame behind a frame", abc + skippable(0, b"xy"), 8, None, "ok")
    add("multi", "skippable frame cut", abc + skippable(0, b"xy")[:-1], 8, None, "reject")
    add("multi", "skippable header cut", abc + skippable(0)[:7], 8, None, "reject")
    for n in (1, 2, 3, 4):
        add("multi", f"a frame followed by {n} zero bytes", abc + bytes(n), 8, None, "reject")
        add("multi", f"a frame followed by {n} bytes of a magic", abc + MAGIC[:n], 8, None, "reject")
    add("multi", "two hand-made frames", abc + frame(seq_block(b"ab", [(2, 4, 2 + 3)])), 16, None, "ok")
    add("multi", "three frames, the second empty", abc + frame(raw(b"", 1)) + abc, 16, None, "ok")
    add("multi", "a hand-made frame followed by an encoder's frame", frame(raw(b"abc") + seq_block(b"de", [(2, 5, 5 + 3)])) + enc, 10 + len(plain), None, "ok")
    add("multi", "an encoder's frame followed by a hand-made frame", enc + frame(raw(b"abc") + seq_block(b"de", [(2, 5, 5 + 3)])), 10 + len(plain), None, "ok")
    add("multi", "capacity for the first frame only", abc + abc, 5, None, "reject")


def _found(add):
    """The three entries the two seeded generators found: accepted by the decoder then, refused by the library"""
    a = frame(block(lit_plain(0, b"abcd", 0) + b"\x00\x00", 2, 1), window=0)
    b = frame(_lit_block(lit_plain(0, b"abcd", 0)), single=4)
    c = frame(raw(b"xy") + one_seq_block(b"", 0, 3, 3), window=0)
    assert (a.hex(), b.hex(), c.hex()) == ("28b52ffd00003d000020616263640000", "28b52ffd2004350000206162636400", "28b52ffd000010000078793d000000015400010003")
    add("blocks", "found: a sequence count of 0 followed by a byte", a, 8, None, "reject")
    add("blocks", "found: a single segment of 4 with a compressed block of 6", b, 8, None, "reject")
    add("seqval", "found: literal length 0, offset value 3, first repeat offset 1", c, 8, None, "reject")


def read_ncount(b, max_sym):
    """ncount() backwards, as FSE_readNCount reads: -> (norm, log, bytes taken)"""
    v, pos = int.from_bytes(b, "little"), 4
    log = (v & 15) + 5
    remaining, threshold, nb = (1 << log) + 1, 1 << log, log + 1
    norm, prev0 = [], False
    while remaining > 1 and len(norm) <= max_sym:
        if prev0:
            while True:
                run = (v >> pos) & 3; pos += 2
                norm += [0] * run
                if run < 3:
                    break
        mx = 2 * threshold - 1 - remaining
        if ((v >> pos) & (threshold - 1)) < mx:
            c = (v >> pos) & (threshold - 1); pos += nb - 1
        else:
            c = (v >> pos) & (2 * threshold - 1); pos += nb
            if c >= threshold:
                c -= mx
        c -= 1
        remaining -= abs(c)
        norm.append(c); prev0 = c == 0
        while remaining < threshold and threshold > 1:
            nb -= 1; threshold >>= 1
    assert remaining == 1 and len(norm) <= max_sym + 1
    return norm, log, (pos + 7) // 8


def read_huf_weights(b):
    """A tree description (Huf.direct or Huf.compressed) -> (the weights, the implied last one included; bytes taken)"""
    if b[0] >= 128:
        n = b[0] - 127
        ws, used = [(b[1 + i // 2] >> (4 * (1 - i % 2))) & 15 for i in range(n)], 1 + (n + 1) // 2
    else:
        body = b[1:1 + b[0]]
        norm, log, k = read_ncount(body, 12)
        table = fse_table(norm, log)
        v = int.from_bytes(body[k:], "little")
        pos = v.bit_length() - 1                      # below the end mark

        def take(n):
            nonlocal pos
            pos -= n
            return ((v >> pos) if pos >= 0 else (v << -pos)) & ((1 << n) - 1)
        s, ws, k = [take(log), take(log)], [], 0
        while True:                                   # two states take turns; the one whose turn comes behind the stream's end gives its symbol and ends
            sym, nbits, base = table[s[k]]
            ws.append(sym); s[k] = base + take(nbits); k ^= 1
            if pos < 0:
                ws.append(table[s[k]][0])
                break
        used = 1 + b[0]
    total = sum(1 << (w - 1) for w in ws if w)
    rest = (1 << total.bit_length()) - total
    assert rest == 1 << (rest.bit_length() - 1)
    return ws + [rest.bit_length()], used


def dict_entropy(d):
    """What a formatted dictionary brings into a frame's first block: -> (Huf of its literals tree, [ll, of, ml] tables in Repeat mode,
    its three repeat offsets, the size of its content)"""
    ws, pos = read_huf_weights(d[8:])
    pos += 8
    tabs = {}
    for kind in ("of", "ml", "ll"):
        norm, log, k = read_ncount(d[pos:pos + 128], MAX_SYM[kind])
        tabs[kind] = Tab(3, b"", fse_table(norm, log), log)
        pos += k
    reps = tuple(int.from_bytes(d[pos + 4 * i:pos + 4 * i + 4], "little") for i in range(3))
    return Huf(ws), [tabs["ll"], tabs["of"], tabs["ml"]], reps, len(d) - pos - 12


def _dict_first_blocks(add, name, d, kw):
    """First blocks that lean on a formatted dictionary's tables: sequence tables in Repeat mode, tree-less literals, its repeat offsets"""
    huf, tabs, reps, content = dict_entropy(d)
    assert content >= 200 and all(1 <= r <= content for r in reps)
    avail = [sorted({s for s, _, _ in t.table}) for t in tabs]
    lc, mc = avail[0][min(2, len(avail[0]) - 1)], avail[2][min(3, len(avail[2]) - 1)]
    lits = bytes(s for s in sorted(huf.code) for _ in range(3))[:120]            # every coded symbol the tree has (the first 40), three times each
    assert LL_BASE[lc] <= 20 <= len(lits)
    ocs = [c for c in avail[1] if c >= 2 and (1 << c) - 3 <= content]            # a real offset, within the dictionary's content
    one = lambda oc: [(lc, 0, oc, 0, mc, 0)]                                     # noqa: E731
    sf = lambda n: 0 if n < 32 else 1                                            # noqa: E731
    plain_l = lit_plain(0, lits, sf(len(lits)))
    for what, oc in (("its smallest offset code", ocs[0]), ("its largest offset code within the content", ocs[-1])):
        add("dict", f"{name}: first block in Repeat mode, {what}", frame(block(plain_l + sequences(one(oc), *tabs), 2, 1), **kw), 400, d, "ok")
    if 0 in avail[1] and LL_BASE[lc] > 0:
        add("dict", f"{name}: first block in Repeat mode, the dictionary's first repeat offset", frame(block(plain_l + sequences(one(0), *tabs), 2, 1), **kw), 400, d, "ok")
    add("dict", f"{name}: first block in Repeat mode behind a raw block", frame(raw(b"0123456789") + block(plain_l + sequences(one(ocs[0]), *tabs), 2, 1), **kw), 400, d, "ok")
    add("dict", f"{name}: first block in Repeat mode, no ID in the header", frame(block(plain_l + sequences(one(ocs[0]), *tabs), 2, 1)), 400, d, "ok")
    for s, sname in ((0, "1 stream"), (1, "4 streams")):
        add("dict", f"{name}: tree-less literals as the first block, {sname}", frame(_lit_block(lit_huf(huf, lits, s, ltype=3)), **kw), 400, d, "ok")
    add("dict", f"{name}: tree-less literals behind a raw block", frame(raw(b"0123456789") + _lit_block(lit_huf(huf, lits, 0, ltype=3)), **kw), 400, d, "ok")
    add("dict", f"{name}: tree-less literals and Repeat mode as the first block", frame(block(lit_huf(huf, lits, 0, ltype=3) + sequences(one(ocs[0]), *tabs), 2, 1), **kw), 400, d, "ok")
    add("dict", f"{name}: tree-less literals in a second frame", frame(raw(b"abc", 1), **kw) + frame(_lit_block(lit_huf(huf, lits, 0, ltype=3)), **kw), 400, d, "ok")


def _dict(add):
    """Offsets that end in, start in and straddle a dictionary's content: raw-content dictionaries, and formatted ones whose ID the header names;
    with the formatted ones, first blocks that use the dictionary's tables"""
    helpers = _helpers()
    cases = [(name, d, len(d), 0) for name, d, _ in helpers.dict_cases()[:2]]
    for name, d, _, row in helpers.formatted_dict_cases()[:2]:
        did = int.from_bytes(d[4:8], "little")
        cases.append((name, d, None, did))
    for name, d, content, did in cases:
        if content is None:
            # (a formatted dictionary: the content's size is the library's business; offsets stay within the last 200 bytes, which every one has)
            content = 200
        kw = {} if not did else {"did_code": 3, "did": did}
        for what, ll, ml, off in (("ends in the dictionary", 2, 5, 2 + 50), ("starts in the dictionary and ends in the frame", 2, 40, 2 + 10), ("straddles with a long match", 2, 300, 2 + 100),
                                  ("reaches the dictionary's first byte", 2, 4, 2 + content), ("reaches one before the dictionary", 2, 4, 2 + content + 1)):
            if did and "first byte" in what or did and "one before" in what:
                continue
            verdict = "reject" if "one before" in what else "ok"
            add("dict", f"{name}: match {what}", frame(seq_block(b"ab", [(ll, ml, off + 3)]), **kw), 400, d, verdict)
            add("dict", f"{name}: match {what}, behind a raw block", frame(raw(b"0123456789") + seq_block(b"ab", [(ll, ml, off + 10 + 3)]), **kw), 400, d, verdict)
        add("dict", f"{name}: another dictionary's ID", frame(raw(b"abc", 1), did_code=3, did=(did or 1) + 1), 8, d, "reject")
        add("dict", f"{name}: no ID in the header", frame(seq_block(b"ab", [(2, 5, 30 + 3)])), 64, d, "ok")
        if did:
            _dict_first_blocks(add, name, d, kw)


def _random_norm(r, nsym, log):
    """counts for nsym used symbols that sum to the table size, some of them -1"""
    size = 1 << log
    cuts = sorted(r.sample(range(1, size), nsym - 1)) if nsym > 1 else []
    parts = [b - a for a, b in zip([0] + cuts, cuts + [size])]
    return [-1 if p == 1 and r.random() < 0.5 else p for p in parts]


def _random(add):
    r = random.Random(SEED)
    H = text(3000, 8)
    # blocks of 1 .. 4 chained compressed blocks with random FSE descriptions and Repeat
    for case in range(300):
        nblocks = r.randrange(1, 5)
        prev = [None, None, None]
        out = bytearray(H); rep = (1, 4, 8); body = raw(H); ok = True
        for bi in range(nblocks):
            n = r.choice((1, 2, 3, 8, 30, 70, 200))
            codes = {"ll": r.sample(range(0, 20), r.randrange(1, 8)), "of": r.sample(range(0, 12), r.randrange(1, 6)), "ml": r.sample(range(0, 36), r.randrange(1, 8))}
            tabs = []
            for ti, kind in enumerate(("ll", "of", "ml")):
                mode = r.choice((0, 2, 2, 2, 3)) if prev[ti] else r.choice((0, 2, 2))
                if mode == 3:
                    tabs.append(prev[ti].repeat())
                elif mode == 0:
                    tabs.append(Tab.predefined(kind))
                else:
                    log = r.randrange(5, MAX_LOG[kind] + 1)
                    used = sorted(codes[kind])
                    cnt = _random_norm(r, len(used), log)
                    norm = [0] * (used[-1] + 1)
                    for s, c in zip(used, cnt):
                        norm[s] = c
                    tabs.append(Tab.fse(norm, log))
            avail = [sorted({s for s, _, _ in t.table}) for t in tabs]
            seqs = []
            for _ in range(n):
                lc, oc, mc = r.choice(avail[0]), r.choice(avail[1]), r.choice(avail[2])
                lc = min(lc, 24); mc = min(mc, 42); oc = min(oc, 11)
                if lc not in avail[0] or oc not in avail[1] or mc not in avail[2]:
                    lc, oc, mc = avail[0][0], avail[1][0], avail[2][0]
                seqs.append((lc, r.getrandbits(LL_BITS[lc]), oc, r.getrandbits(oc), mc, r.getrandbits(ML_BITS[mc])))
            plain = [(LL_BASE[a] + ax, ML_BASE[c] + cx, (1 << b) + bx) for a, ax, b, bx, c, cx in seqs]
            lits = text(sum(s[0] for s in plain) + r.randrange(0, 4), case * 8 + bi)
            got = execute(bytes(out), lits, plain, rep)
            picks = (r.randrange(8), r.randrange(8), r.randrange(8))
            body += block(lit_plain(0, lits, 0 if len(lits) < 32 else 1 if len(lits) < 4096 else 3) + sequences(seqs, *tabs, picks=picks), 2, bi == nblocks - 1)
            if got is None:
                ok = False
                break
            out += got[0]; rep = got[1]
            prev = tabs
        add("random", f"FSE blocks {case}", frame(bytes(body), window=(17 - 10) << 3), len(out) + r.choice((0, 0, 16)), None, "ok" if ok else "reject")
    # RLE-table blocks with random codes and counts
    for case in range(110):
        lc, oc, mc = r.randrange(0, 30), r.randrange(0, 13), r.randrange(0, 46)
        n = r.choice((1, 2, 5, 64, 65, 300))
        seqs = [(lc, r.getrandbits(LL_BITS[lc]), oc, r.getrandbits(oc), mc, r.getrandbits(ML_BITS[mc])) for _ in range(n)]
        plain = [(LL_BASE[a] + ax, ML_BASE[c] + cx, (1 << b) + bx) for a, ax, b, bx, c, cx in seqs]
        total = sum(s[0] for s in plain)
        lits = text(min(total, BLOCK_MAX) + r.randrange(0, 4), 5000 + case)
        got = execute(H, lits, plain) if total <= len(lits) else None
        sf = 0 if len(lits) < 32 else 1 if len(lits) < 4096 else 3
        body = raw(H) + block(lit_plain(0, lits, sf) + sequences(seqs, *_rle_tabs(lc, oc, mc)), 2, 1)
        if len(body) > 3 + len(H) + 3 + BLOCK_MAX:
            continue
        add("random", f"RLE tables {case}: codes {lc} {oc} {mc} x {n}", frame(bytes(body), window=(18 - 10) << 3), len(H) + (len(got[0]) if got else 64), None, "ok" if got else "reject")


_CASES = None


def cases():
    """[(family, name, entry, capacity, dictionary or None, intent)], the same list at every call"""
    global _CASES
    if _CASES is None:
        out = []
        seen = set()

        def add(family, name, entry, cap, dictionary, intent):
            assert name not in seen, name
            seen.add(name)
            out.append((family, name, bytes(entry), cap, dictionary, intent))
        for fam in (_header, _blocks, _literals, _seqhdr, _seqval, _multi, _found, _dict, _random):
            fam(add)
        _CASES = out
    return _CASES


def sha256(b):
    return hashlib.sha256(b).hexdigest()


# ---------------------------------------------------------------- the library's answers and the fixture ----
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "zstd_handmade_golden.json")
INFO_FIELDS = ("content", "bound", "status", "frames", "dict_id", "flags")        # kmp_zstd_frame_info, as helpers_frame_info.expected has it


def library_rows(lib, cs):
    """What libzstd 1.5.7 (lib: helpers_frame_info.live_lib()) answers for the cases: per case {"status": ZSTD_getErrorCode of
    ZSTD_decompress (ZSTD_decompress_usingDict with a dictionary) at the case's capacity, "out_len", "out_sha256" of what it wrote,
    "info": what the three frame-size calls come to as a kmp_zstd_frame_info}"""
    import ctypes
    import helpers_frame_info as hf
    lib.ZSTD_decompress.restype = ctypes.c_size_t
    lib.ZSTD_decompress.argtypes = [ctypes.c_void_p, ctypes.c_size_t, ctypes.c_void_p, ctypes.c_size_t]
    lib.ZSTD_createDCtx.restype = ctypes.c_void_p
    lib.ZSTD_freeDCtx.argtypes = [ctypes.c_void_p]
    lib.ZSTD_decompress_usingDict.restype = ctypes.c_size_t
    lib.ZSTD_decompress_usingDict.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_void_p, ctypes.c_size_t]
    lib.ZSTD_getErrorCode.restype = ctypes.c_int
    lib.ZSTD_getErrorCode.argtypes = [ctypes.c_size_t]
    lib.ZSTD_isError.restype = ctypes.c_uint
    lib.ZSTD_isError.argtypes = [ctypes.c_size_t]
    rows = []
    for _, _, e, cap, d, _ in cs:
        out = ctypes.create_string_buffer(cap + 1)
        src = ctypes.create_string_buffer(e, len(e) + 1)
        if d is None:
            n = lib.ZSTD_decompress(out, cap, src, len(e))
        else:
            dctx = lib.ZSTD_createDCtx()
            n = lib.ZSTD_decompress_usingDict(dctx, out, cap, src, len(e), d, len(d))
            lib.ZSTD_freeDCtx(dctx)
        err = lib.ZSTD_isError(n)
        row = {"status": int(lib.ZSTD_getErrorCode(n)) if err else 0, "out_len": 0 if err else int(n), "out_sha256": "" if err else sha256(out.raw[:n]),
               "info": [int(x) for x in hf.expected(hf.live_answers(lib, e))]}
        assert not err or row["status"] != 0
        rows.append(row)
    return rows


def check_intents(cs, rows):
    """The composer's own test: -> findings (empty: the library accepts every "ok" case, refuses every "reject" case, accepts 60 % of all,
    and at most 2 % are "lenient")"""
    bad = [f"{fam} / {name}: intent {intent}, the library answers {r['status']}" for (fam, name, _, _, _, intent), r in zip(cs, rows)
           if (intent == "ok" and r["status"] != 0) or (intent == "reject" and r["status"] == 0) or intent not in ("ok", "reject", "lenient")]
    accepted = sum(1 for r in rows if r["status"] == 0)
    if accepted * 100 < 60 * len(rows):
        bad.append(f"the library accepts {accepted} of {len(rows)} cases: below 60 %")
    lenient = sum(1 for c in cs if c[5] == "lenient")
    if lenient * 100 > 2 * len(rows):
        bad.append(f"{lenient} of {len(rows)} cases are lenient: above 2 %")
    return bad


def write_golden(cs, rows):
    """Column by column, a line each: per case the head of the entry's sha256 (one sha256 over all of them in full), the capacity, the
    library's status, and for what it accepts the length and sha256 of the output; the six frame info fields"""
    import json
    shas = [sha256(c[2]) for c in cs]
    doc = {"libzstd": 10507, "seed": SEED, "cases": len(cs), "sha256_of_all": sha256("".join(shas).encode()),
           "sha256_head": [s[:8] for s in shas], "cap": [c[3] for c in cs], "status": [r["status"] for r in rows],
           "out_len": {str(i): r["out_len"] for i, r in enumerate(rows) if r["out_len"]},
           "out_sha256": {str(i): r["out_sha256"] for i, r in enumerate(rows) if r["status"] == 0}}
    for k, f in enumerate(INFO_FIELDS):
        doc["info_" + f] = [r["info"][k] for r in rows]
    with open(GOLDEN, "w") as f:
        f.write("{\n" + ",\n".join(f' "{k}": {json.dumps(v, separators=(",", ":"))}' for k, v in doc.items()) + "\n}\n")


def golden():
    """-> (cases, rows): the cases rebuilt and checked against the fixture's hashes, the library's recorded answers in library_rows' form"""
    import json
    with open(GOLDEN) as f:
        d = json.load(f)
    assert d["libzstd"] == 10507
    cs = cases()
    assert len(cs) == d["cases"], (len(cs), d["cases"])
    shas = [sha256(c[2]) for c in cs]
    for c, s, head, cap in zip(cs, shas, d["sha256_head"], d["cap"]):
        assert s[:8] == head and c[3] == cap, f"the composer no longer makes the fixture's entry: {c[0]} / {c[1]}"
    assert sha256("".join(shas).encode()) == d["sha256_of_all"], "the composer no longer makes the fixture's entries"
    rows = [{"status": d["status"][i], "out_len": d["out_len"].get(str(i), 0), "out_sha256": d["out_sha256"].get(str(i), ""),
             "info": [d["info_" + f][i] for f in INFO_FIELDS]} for i in range(len(cs))]
    return cs, rows


# ---------------------------------------------------------------- the emulator ----
KNOWN_CODES = (1, 10, 14, 16, 20, 22, 24, 32, 66, 70, 72)       # include/kompressor_hip.h


def emu_decode(cs, pre):
    """k_zstd_decode's body over the cases without a dictionary in one batch (alone, or behind the sort and both pre-decoders), each case
    with a dictionary through emu_zstd_decompress_dict -> per case (status, out_len, sha256 of the output or "")"""
    import ctypes
    import numpy as np
    import helpers
    import helpers_decode_status as hd
    import helpers_frame_info as hf
    res = [None] * len(cs)
    plain = [i for i, c in enumerate(cs) if c[4] is None]
    fn = hd._decode_fn()
    src, so, sl = hf.pack([cs[i][2] for i in plain])
    hd._no_pre(not pre)
    try:
        for b in range(0, len(plain), 64):
            idx = plain[b:b + 64]
            caps = np.array([cs[i][3] for i in idx], dtype=np.uint32)
            ooff = (np.cumsum(caps.astype(np.uint64) + 16) - (caps.astype(np.uint64) + 16)).astype(np.uint64)
            out = np.full(int(caps.astype(np.uint64).sum()) + 16 * len(idx) + 64, 0xC3, dtype=np.uint8)
            olen = np.zeros(len(idx), dtype=np.uint32); st = np.zeros(len(idx), dtype=np.uint32)
            io = np.ascontiguousarray(so[b:b + 64]); il = np.ascontiguousarray(sl[b:b + 64])
            r = fn(helpers._vp(src), helpers._vp(io), helpers._vp(il), len(idx), 2, helpers._vp(out), helpers._vp(ooff), helpers._vp(caps), helpers._vp(olen), helpers._vp(st), hd.LIT_CAP)
            assert r == 0, f"emulator reported {r}"
            for k, i in enumerate(idx):
                o, n = int(ooff[k]), int(olen[k])
                assert (out[o + int(caps[k]):o + int(caps[k]) + 16] == 0xC3).all(), f"{cs[i][1]}: written behind the capacity"
                res[i] = (int(st[k]), n, sha256(out[o:o + n].tobytes()) if int(st[k]) == 0 else "")
        for i, c in enumerate(cs):
            if c[4] is not None:
                got, st = helpers.emu_decompress([c[2]], [c[3]], dictionary=c[4])
                res[i] = (st[0], len(got[0]), sha256(got[0]) if st[0] == 0 else "")
    finally:
        hd._no_pre(False)
    return res


def emu_info(cs):
    import helpers_frame_info as hf
    src, offs, lens = hf.pack([c[2] for c in cs])
    info = hf.emu_frame_info(src, offs, lens)
    return [[int(info[i][f]) for f in INFO_FIELDS] for i in range(len(cs))]


def compare(cs, rows, got):
    """The decoder's answers (status, out_len, sha256) against the library's -> findings"""
    bad = []
    for (fam, name, _, _, _, intent), r, g in zip(cs, rows, got):
        what = f"{fam} / {name}: ({g[0]}, {g[1]}), the library ({r['status']}, {r['out_len']})"
        if r["status"] == 0:
            if g[0] != 0 and intent == "lenient" and g[0] in KNOWN_CODES:
                continue
            if name in REFUSED_THOUGH_ACCEPTED:
                if (g[0], g[1]) != (REFUSED_THOUGH_ACCEPTED[name], 0):
                    bad.append(what + f" (the named exception is code {REFUSED_THOUGH_ACCEPTED[name]})")
                continue
            if g[0] != 0 or g[1] != r["out_len"] or g[2] != r["out_sha256"]:
                bad.append(what + (" other bytes" if g[0] == 0 and g[1] == r["out_len"] else ""))
        elif g[0] == 0 or g[0] not in KNOWN_CODES or g[1] != 0:
            bad.append(what)
        elif (fam in EXACT_FAMILIES or name in EXACT_NAMES) and g[0] != r["status"]:
            bad.append(what + " (the code is compared in this family)")
    return bad


# ---------------------------------------------------------------- every entry and every output at a guard page ----
def main():
    import numpy as np
    sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
    import helpers
    import helpers_decode_status as hd
    import helpers_frame_info as hf
    import fuzz_decoders
    cs, rows = golden()
    fn = hd._decode_fn()
    n = 0
    for (fam, name, e, cap, d, intent), r in zip(cs, rows):
        if d is not None:
            continue                                  # (the dictionary call has its guard pages in tests/fuzz_decoders.py --dict)
        gin = fuzz_decoders.Guarded(len(e), 0); gout = fuzz_decoders.Guarded(cap, 0)
        gin.write(e)
        off = np.array([gin.off], dtype=np.uint64); ln = np.array([len(e)], dtype=np.uint32)
        ooff = np.array([gout.off], dtype=np.uint64); caps = np.array([cap], dtype=np.uint32)
        print(fam, "/", name, flush=True)
        for pre in (False, True):
            hd._no_pre(not pre)
            olen = np.zeros(1, dtype=np.uint32); st = np.zeros(1, dtype=np.uint32)
            rc = fn(gin.base, helpers._vp(off), helpers._vp(ln), 1, 1, gout.base, helpers._vp(ooff), helpers._vp(caps), helpers._vp(olen), helpers._vp(st), hd.LIT_CAP)
            hd._no_pre(False)
            assert rc == 0, f"emulator reported {rc}"
            got = (int(st[0]), int(olen[0]), sha256(gout.read(int(olen[0]))) if int(st[0]) == 0 else "")
            bad = compare([(fam, name, e, cap, d, intent)], [r], [got])
            assert not bad, bad[0]
        hd.emu_sort_keys(gin.base, off, ln)
        hf.emu_frame_info(gin.base, off, ln)
        gin.close(); gout.close()
        n += 1
    print(f"OK {n}")
    return 0


if __name__ == "__main__":
    sys.exit(main())
