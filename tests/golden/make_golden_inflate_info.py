"""Writes tests/golden/inflate_info_golden.json: DEFLATE streams (base64) written by zlib.compressobj and by hand (a bit writer below),
each with the format it is read in and the kmp_inflate_info it answers.  Acceptance and size are zlib's (tests/helpers_inflate_info.py
verdict); blocks, flags and window_bits of the accepted streams come from a walk in plain Python (walk() below), which also has to
agree with zlib on the size.  A rejected entry answers its status alone: -5 when zlib still waits for input (and for every entry too
short to hold its wrapper), -3 otherwise.  A stream zlib refuses for its data check alone is answered as if the check had passed: the
sizing pass has no output to sum (kind "checksum").
Run from the repository root: python tests/golden/make_golden_inflate_info.py"""
import base64
import json
import os
import random
import struct
import sys
import zlib

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.join(ROOT, "tests"))

import helpers_inflate_info as hi                      # noqa: E402

ORDER = (16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15)
LBASE = (3, 4, 5, 6, 7, 8, 9, 10, 11, 13, 15, 17, 19, 23, 27, 31, 35, 43, 51, 59, 67, 83, 99, 115, 131, 163, 195, 227, 258)
LEXT = (0, 0, 0, 0, 0, 0, 0, 0, 1, 1, 1, 1, 2, 2, 2, 2, 3, 3, 3, 3, 4, 4, 4, 4, 5, 5, 5, 5, 0)
DBASE = (1, 2, 3, 4, 5, 7, 9, 13, 17, 25, 33, 49, 65, 97, 129, 193, 257, 385, 513, 769, 1025, 1537, 2049, 3073, 4097, 6145, 8193, 12289, 16385, 24577)
DEXT = (0, 0, 0, 0, 1, 1, 2, 2, 3, 3, 4, 4, 5, 5, 6, 6, 7, 7, 8, 8, 9, 9, 10, 10, 11, 11, 12, 12, 13, 13)
FIXED_L = [8] * 144 + [9] * 112 + [7] * 24 + [8] * 8
FIXED_D = [5] * 32


def text(seed, n):
    r = random.Random(seed)
    words = [bytes(r.choice(b"abcdefghijklmnopqrstuvwxyz") for _ in range(r.randrange(2, 9))) for _ in range(200)]
    out = bytearray()
    while len(out) < n:
        out += r.choice(words) + b" "
    return bytes(out[:n])


def noise(seed, n):
    return random.Random(seed).randbytes(n)


# ---------------------------------------------------------------- writing streams by hand ----
class Bits:
    def __init__(self):
        self.acc = 0; self.n = 0

    def put(self, v, k):                   # k bits of v, least significant first
        self.acc |= (v & ((1 << k) - 1)) << self.n; self.n += k

    def code(self, c, k):                  # a Huffman code: most significant bit first
        for i in range(k - 1, -1, -1):
            self.put((c >> i) & 1, 1)

    def align(self):
        self.n = (self.n + 7) & ~7

    def bytes(self):
        return self.acc.to_bytes((self.n + 7) // 8, "little")


def canonical(lens):
    """{symbol: (code, length)} of a list of code lengths"""
    count = [0] * 17
    for l in lens:
        count[l] += 1
    count[0] = 0
    nxt, c = [0] * 17, 0
    for l in range(1, 16):
        c = (c + count[l - 1]) << 1
        nxt[l] = c
    out = {}
    for s, l in enumerate(lens):
        if l:
            out[s] = (nxt[l], l); nxt[l] += 1
    return out


def balanced(k):
    """k code lengths that fill the code space exactly (k >= 2)"""
    b = k.bit_length() - 1
    short = (1 << (b + 1)) - k
    return [b] * short + [b + 1] * (k - short)


def dynamic_header(w, final, llens, dlens, cl_ops=None, hlit=None, hdist=None):
    """block header of a dynamic block.  llens / dlens: code lengths by symbol.  cl_ops: the code-length symbols to write, as
    (symbol, extra value) -- by default the lengths one by one with runs of zeros as 17 / 18."""
    hlit = len(llens) if hlit is None else hlit
    hdist = len(dlens) if hdist is None else hdist
    if cl_ops is None:
        cl_ops, seq, i = [], list(llens) + list(dlens), 0
        while i < len(seq):
            if seq[i] == 0:
                j = i
                while j < len(seq) and seq[j] == 0 and j - i < 138:
                    j += 1
                if j - i >= 11:
                    cl_ops.append((18, j - i - 11)); i = j; continue
                if j - i >= 3:
                    cl_ops.append((17, j - i - 3)); i = j; continue
            cl_ops.append((seq[i], 0)); i += 1
    used = sorted({s for s, _ in cl_ops} | {0, 18})
    cl = [0] * 19
    for s, l in zip(used, balanced(len(used))):
        cl[s] = l
    codes = canonical(cl)
    hclen = max(i for i, s in enumerate(ORDER) if cl[s]) + 1
    w.put(1 if final else 0, 1); w.put(2, 2)
    w.put(hlit - 257, 5); w.put(hdist - 1, 5); w.put(max(hclen, 4) - 4, 4)
    for s in ORDER[:max(hclen, 4)]:
        w.put(cl[s], 3)
    for s, x in cl_ops:
        w.code(*codes[s])
        if s >= 16:
            w.put(x, (2, 3, 7)[s - 16])


def put_syms(w, lcodes, dcodes, syms):
    """syms: a literal byte, 256, or (length, distance)"""
    for s in syms:
        if isinstance(s, int):
            w.code(*lcodes[s]); continue
        length, dist = s
        lc = max(i for i in range(29) if LBASE[i] <= length)
        w.code(*lcodes[257 + lc]); w.put(length - LBASE[lc], LEXT[lc])
        dc = max(i for i in range(30) if DBASE[i] <= dist)
        w.code(*dcodes[dc]); w.put(dist - DBASE[dc], DEXT[dc])


def lens_of(pairs, n):
    out = [0] * n
    for s, l in pairs.items():
        out[s] = l
    return out


def dynamic(llens_by_sym, dlens_by_sym, syms, **kw):
    hl = max(max(llens_by_sym) + 1, 257)
    llens = lens_of(llens_by_sym, hl)
    dlens = lens_of(dlens_by_sym, max(max(dlens_by_sym, default=0) + 1, 1))
    w = Bits()
    dynamic_header(w, True, llens, dlens, **kw)
    put_syms(w, canonical(llens), canonical(dlens), syms)
    return w.bytes()


def fixed(syms, final=True):
    w = Bits()
    w.put(1 if final else 0, 1); w.put(1, 2)
    put_syms(w, canonical(FIXED_L), canonical(FIXED_D), syms)
    return w.bytes()


def fixed_raw_codes(codes):
    """a final fixed block of literal/length codes given as (code, bits) (symbols no encoder writes)"""
    w = Bits()
    w.put(1, 1); w.put(1, 2)
    for c, k in codes:
        w.code(c, k)
    return w.bytes()


def comb(symbols):
    """lengths 1, 2, 3, .. k - 1, k - 1 for the k symbols in this order: the last two carry the longest codes"""
    k = len(symbols)
    return {s: min(i + 1, k - 1) for i, s in enumerate(symbols)}


# ---------------------------------------------------------------- the walk in plain Python ----
class Reader:
    def __init__(self, data):
        self.v = int.from_bytes(data, "little"); self.pos = 0; self.nbits = 8 * len(data)

    def take(self, k):
        assert self.pos + k <= self.nbits, "ran out"
        r = (self.v >> self.pos) & ((1 << k) - 1); self.pos += k
        return r

    def sym(self, table):
        c, k = 0, 0
        while True:
            c = (c << 1) | self.take(1); k += 1
            if (c, k) in table:
                return table[(c, k)]
            assert k < 15, "no such code"


def walk(deflate):
    """-> (size, blocks, flags, bytes used) of a raw DEFLATE stream zlib accepts"""
    r = Reader(deflate)
    op = blocks = flags = 0
    while True:
        last = r.take(1); bt = r.take(2); blocks += 1
        assert bt != 3
        if bt == 0:
            r.pos = (r.pos + 7) & ~7
            ln, nl = r.take(16), r.take(16)
            assert ln ^ 0xFFFF == nl
            r.pos += 8 * ln; op += ln; flags |= 1
            assert r.pos <= r.nbits, "ran out"
        else:
            flags |= 2 if bt == 1 else 4
            if bt == 1:
                ll, dl = FIXED_L, FIXED_D
            else:
                hlit, hdist, hclen = r.take(5) + 257, r.take(5) + 1, r.take(4) + 4
                cl = [0] * 19
                for s in ORDER[:hclen]:
                    cl[s] = r.take(3)
                ct = {v: s for s, v in canonical(cl).items()}
                seq = []
                while len(seq) < hlit + hdist:
                    s = r.sym(ct)
                    if s < 16:
                        seq.append(s)
                    elif s == 16:
                        seq += [seq[-1]] * (3 + r.take(2))
                    elif s == 17:
                        seq += [0] * (3 + r.take(3))
                    else:
                        seq += [0] * (11 + r.take(7))
                assert len(seq) == hlit + hdist
                ll, dl = seq[:hlit], seq[hlit:]
            lt = {v: s for s, v in canonical(ll).items()}
            dt = {v: s for s, v in canonical(dl).items()}
            while True:
                s = r.sym(lt)
                if s < 256:
                    op += 1
                elif s == 256:
                    break
                else:
                    assert s <= 285
                    length = LBASE[s - 257] + r.take(LEXT[s - 257])
                    d = r.sym(dt)
                    assert d <= 29
                    dist = DBASE[d] + r.take(DEXT[d])
                    assert dist <= op
                    op += length
        if last:
            return op, blocks, flags, (r.pos + 7) // 8


# ---------------------------------------------------------------- wrappers ----
def deflate_raw(data, level=6, wbits=15, mem=8):
    c = zlib.compressobj(level, zlib.DEFLATED, -wbits, mem)
    return c.compress(data) + c.flush()


def zlib_wrap(body, content, cinfo=7, flevel=2, fdict=0):
    cmf = 8 | (cinfo << 4); flg = (flevel << 6) | (fdict << 5)
    flg |= 31 - ((cmf << 8) | flg) % 31 if ((cmf << 8) | flg) % 31 else 0
    return bytes((cmf, flg)) + body + struct.pack(">I", zlib.adler32(content))


def gzip_wrap(body, content, extra=None, name=None, comment=None, hcrc=False, flg_or=0, isize_add=0):
    flg = (4 if extra is not None else 0) | (8 if name is not None else 0) | (16 if comment is not None else 0) | (2 if hcrc else 0) | flg_or
    h = bytes((0x1F, 0x8B, 8, flg, 0, 0, 0, 0, 0, 3))
    if extra is not None:
        h += struct.pack("<H", len(extra)) + extra
    if name is not None:
        h += name + b"\0"
    if comment is not None:
        h += comment + b"\0"
    if hcrc:
        h += struct.pack("<H", zlib.crc32(h) & 0xFFFF)
    return h + body + struct.pack("<II", zlib.crc32(content), (len(content) + isize_add) & 0xFFFFFFFF)


def content_of(body):
    """what a raw body decodes to, b"" when zlib does not get through it"""
    o = zlib.decompressobj(-15)
    try:
        return o.decompress(body)
    except zlib.error:
        return b""


# ---------------------------------------------------------------- rows ----
ROWS = []
NAMES = set()


def add(name, entry, fmt, stored=None):
    """stored: (seed, block sizes) of an entry made of stored blocks of seeded random bytes alone: the recipe is kept, not the bytes"""
    assert (name, fmt) not in NAMES, name
    NAMES.add((name, fmt))
    kind, val = hi.verdict(entry, fmt)
    row = {"name": name, "fmt": fmt, "kind": kind, "status": 0, "content": 0, "blocks": 0, "flags": 0, "window_bits": 0}
    if stored is None:
        row["b64"] = base64.b64encode(entry).decode()
    else:
        assert fmt == 0 and hi.stored_stream(*stored) == entry, name
        row["stored"] = {"seed": stored[0], "blocks": stored[1]}
    f = fmt
    if f == 3:
        f = 2 if entry[:2] == b"\x1f\x8b" else 1
    if len(entry) < hi.WRAPPER_MIN[f]:
        assert kind == "reject" or len(entry) >= 2, (name, kind)
        row["kind"] = "reject"; row["status"] = -5
    elif kind == "reject":
        row["status"] = val
    else:
        hdr = 0
        if f == 1:
            hdr, tail = 2, 4
            row["window_bits"] = (entry[0] >> 4) + 8
        elif f == 2:
            flg, hdr, tail = entry[3], 10, 8
            if flg & 4:
                hdr += 2 + struct.unpack("<H", entry[10:12])[0]
            for bit in (8, 16):
                if flg & bit:
                    hdr = entry.index(b"\0", hdr) + 1
            if flg & 2:
                hdr += 2
            row["flags"] = 8 | (16 if flg & 0x1E else 0)
        else:
            tail = 0
        region = entry[hdr:len(entry) - tail]
        try:
            size, blocks, flags, used = walk(region)
            assert used == len(region), name
            assert f != 2 or struct.unpack("<I", entry[-4:])[0] == size & 0xFFFFFFFF
        except AssertionError as e:
            # only where zlib objects to the data check: it read the stream another way than "the entry minus wrapper and trailer"
            assert kind == "checksum", (name, kind, e)
            row["status"] = -5 if "ran out" in str(e) else -3
            row["flags"] = row["window_bits"] = 0
            ROWS.append(row)
            return
        if kind == "ok":
            assert size == len(val), (name, size, len(val))
        row["content"] = size; row["blocks"] = blocks; row["flags"] |= flags
    ROWS.append(row)


def add_body(name, body, fmts=(0, 1, 2), content=None):
    """a raw DEFLATE body in the formats it applies to (wrappers made here, with the sums of what the body decodes to)"""
    c = content_of(body) if content is None else content
    for fmt in fmts:
        add(name, body if fmt == 0 else zlib_wrap(body, c) if fmt == 1 else gzip_wrap(body, c), fmt)


def main():
    # ---- block types
    add_body("empty input", deflate_raw(b""))
    add_body("1 byte", deflate_raw(b"x"))
    for n in (0, 1, 65535, 65536):
        body = deflate_raw(noise(n, n), level=0)
        if n < 4096:
            add_body(f"level 0, {n} bytes", body)
        else:
            add(f"level 0, {n} bytes", body, 0, stored=(n, stored_sizes(body)))
    c = zlib.compressobj(6, zlib.DEFLATED, -15)
    sync = c.flush(zlib.Z_SYNC_FLUSH) + c.compress(b"after the flush") + c.flush()
    assert sync[:5] == b"\x00\x00\x00\xff\xff"
    add_body("empty stored block of Z_SYNC_FLUSH in front of a final block", sync)
    c = zlib.compressobj(0, zlib.DEFLATED, -15)
    mixed = c.compress(noise(3, 300)) + c.flush(zlib.Z_FULL_FLUSH)
    c2 = zlib.compressobj(6, zlib.DEFLATED, -15)
    mixed += c2.compress(b"abcabcabcabd") + c2.flush(zlib.Z_FULL_FLUSH)                    # a fixed block
    c3 = zlib.compressobj(6, zlib.DEFLATED, -15)
    mixed += c3.compress(text(5, 3000)) + c3.flush()                                      # a dynamic block
    assert walk(mixed)[2] == 7
    add_body("stored + fixed + dynamic blocks", mixed)
    add_body("dynamic block, distance set of one code of length 1", dynamic({97: 1, 256: 2, 257: 2}, {0: 1}, [97, (3, 1), 256]))
    add_body("dynamic block, no distance code, literals only", dynamic({97: 1, 98: 2, 256: 2}, {}, [97, 98, 97, 98, 256]))
    add_body("dynamic block, literal/length set of the end-of-block code alone", dynamic({256: 1}, {}, [256]))
    # ---- sizes and shapes
    add_body("100 000 zero bytes", deflate_raw(bytes(100000)))
    body = deflate_raw(noise(7, 70000))                     # (zlib stores what does not compress: blocks of 16 383 bytes)
    add("70 000 random bytes at level 6", body, 0, stored=(7, stored_sizes(body)))
    r = random.Random(7)
    add_body("70 000 random bytes of 200 values at level 6 (more than 65 535 literals without a match)", deflate_raw(bytes(r.randrange(200) for _ in range(70000))), fmts=(0,))
    add_body("300 000 bytes of text", deflate_raw(text(9, 300000)), fmts=(0,))
    lsyms = [97, 98, 99, 100, 101, 102, 103, 104, 105, 106, 107, 108, 256, 257, 258, 285]          # comb: 1 .. 15, 15 bits
    dsyms = [0, 1, 2, 3, 4, 5, 6, 7, 20, 29]                                                        # comb: 1 .. 9, 9 bits
    add_body("codes of 15 bits (literal/length) and 9 bits (distance)",
             dynamic(comb(lsyms), comb(dsyms), [97, 98, 108, 107, (3, 1), (4, 4), (258, 2), 106, (4, 3), (258, 16)] + [(258, 1)] * 100 +
                     [(3, 1029), (4, 24580), (258, 5), 105, 256]))
    # ---- wrappers
    t = text(11, 400)
    for wb in (9, 15):
        c = zlib.compressobj(6, zlib.DEFLATED, wb)
        s = c.compress(t) + c.flush()
        assert (s[0] >> 4) + 8 == wb
        add(f"zlib, windowBits {wb}", s, 1)
    body = deflate_raw(t)
    add("zlib, FDICT set", zlib_wrap(body, t, fdict=1), 1)
    bad = bytearray(zlib_wrap(body, t)); bad[1] ^= 1
    add("zlib, header fails the mod-31 check", bytes(bad), 1)
    bad = bytearray(zlib_wrap(body, t)); bad[0] = 0x79; bad[1] = 0
    bad[1] = 31 - (bad[0] << 8) % 31
    add("zlib, compression method 9", bytes(bad), 1)
    bad = bytearray(zlib_wrap(body, t)); bad[-1] ^= 1
    add("zlib, wrong Adler-32", bytes(bad), 1)
    c = zlib.compressobj(6, zlib.DEFLATED, 31)
    add("gzip plain", c.compress(t) + c.flush(), 2)
    add("gzip, FEXTRA", gzip_wrap(body, t, extra=b"AB\x03\x00xyz"), 2)
    add("gzip, FNAME", gzip_wrap(body, t, name=b"file.txt"), 2)
    add("gzip, FCOMMENT", gzip_wrap(body, t, comment=b"a comment"), 2)
    add("gzip, FHCRC", gzip_wrap(body, t, hcrc=True), 2)
    add("gzip, FEXTRA + FNAME + FCOMMENT + FHCRC", gzip_wrap(body, t, extra=b"", name=b"n", comment=b"", hcrc=True), 2)
    add("gzip, reserved FLG bit", gzip_wrap(body, t, flg_or=0x20), 2)
    add("gzip, ISIZE off by one", gzip_wrap(body, t, isize_add=1), 2)
    bad = bytearray(gzip_wrap(body, t)); bad[-8] ^= 1
    add("gzip, wrong CRC-32", bytes(bad), 2)
    add("gzip, FNAME without its zero byte", gzip_wrap(body, t, name=b"x" * 30)[:30] + b"\x01" * 10, 2)
    add("format 3 over zlib", zlib_wrap(body, t), 3)
    add("format 3 over gzip", gzip_wrap(body, t, name=b"auto"), 3)
    add("format 3 over neither", b"\x1f\x8c" + body + bytes(8), 3)
    add("format 3 over zlib, wrong Adler-32", zlib_wrap(body, t)[:-1] + b"\xff", 3)
    # ---- damage
    for fmt, want in ((0, 60), (1, 60), (2, 60)):
        s = None
        for n in range(20, 400):
            for seed in range(40):
                d = text(100 + seed, n)
                e = add_wrap(deflate_raw(d), d, fmt)
                if len(e) == want:
                    s = e; break
            if s:
                break
        assert s is not None
        add(f"60-byte {hi.FMT_NAMES[fmt]} stream", s, fmt)
        for k in range(60):
            add(f"60-byte {hi.FMT_NAMES[fmt]} stream, first {k} bytes", s[:k], fmt)
            if k >= hi.WRAPPER_MIN[fmt]:
                assert ROWS[-1]["status"] == -5, ROWS[-1]
        add(f"60-byte {hi.FMT_NAMES[fmt]} stream, one byte appended", s + b"\0", fmt)
        assert ROWS[-1]["status"] == -3
    add_body("block type 3", b"\x07")
    add_body("stored block, LEN / NLEN mismatch", b"\x01\x05\x00\x00\x00hello")
    add_body("stored block longer than the entry", b"\x01\x05\x00\xfa\xffhel")
    add_body("over-subscribed literal/length set", dynamic({97: 1, 98: 1, 256: 1}, {0: 1}, []))
    add_body("incomplete literal/length set", dynamic({97: 2, 256: 2}, {0: 1}, []))
    add_body("incomplete distance set of two codes", dynamic({97: 1, 256: 2, 257: 2}, {0: 2, 1: 2}, []))
    add_body("over-subscribed distance set", dynamic({97: 1, 256: 2, 257: 2}, {0: 1, 1: 1, 2: 1}, []))
    add_body("no end-of-block code", dynamic({97: 1, 98: 1}, {0: 1}, []))
    add_body("distance beyond the output so far", fixed([97, 98, (3, 3), 256]))
    add_body("match as the first symbol", fixed([(3, 1), 256]))
    add_body("fixed block, literal/length symbol 286", fixed_raw_codes([(0b11000110, 8)]) + b"\0")
    add_body("fixed block, distance symbol 30", fixed_raw_codes([(0b00110000 + 97, 8), (0b0000001, 7), (30, 5)]) + b"\0")
    add_body("single distance code, the other code used", dynamic({97: 1, 256: 2, 257: 2}, {0: 1}, [97])[:-1] + b"\xff\xff")
    add_body("no distance code, a match", dynamic({97: 1, 256: 2, 257: 2}, {}, [97]) [:-1] + b"\xff\xff")
    w = Bits(); w.put(1, 1); w.put(2, 2); w.put(30, 5); w.put(0, 5); w.put(0, 4); w.put(0, 12)
    add_body("HLIT 287", w.bytes() + bytes(8))
    w = Bits(); w.put(1, 1); w.put(2, 2); w.put(0, 5); w.put(30, 5); w.put(0, 4); w.put(0, 12)
    add_body("HDIST 31", w.bytes() + bytes(8))
    ll = lens_of({97: 1, 256: 2, 257: 2}, 258)
    w = Bits(); dynamic_header(w, True, ll, [1], cl_ops=[(16, 0), (0, 0), (18, 127)])
    add_body("repeat with nothing before it", w.bytes() + bytes(4))
    w = Bits(); dynamic_header(w, True, ll, [1], cl_ops=[(1, 0), (18, 127), (18, 127)])
    add_body("repeat past the end", w.bytes() + bytes(4))
    w = Bits(); w.put(1, 1); w.put(2, 2); w.put(0, 5); w.put(0, 5); w.put(0, 4); w.put(0, 12)
    add_body("code-length code without codes", w.bytes() + bytes(40))
    add_body("code-length code without codes, entry ends inside the lengths", w.bytes() + bytes(8))
    add_body("final bit never set", fixed([97, 256], final=False), fmts=(0,))
    add("empty entry", b"", 0)
    add("zlib, 5 bytes", zlib_wrap(body, t)[:5], 1)
    add("gzip, 17 bytes", gzip_wrap(body, t)[:17], 2)
    out = os.path.join(ROOT, "tests", "golden", "inflate_info_golden.json")
    with open(out, "w") as f:
        json.dump({"zlib": zlib.ZLIB_RUNTIME_VERSION, "rows": ROWS}, f, indent=0)
    kinds = {k: sum(1 for r in ROWS if r["kind"] == k) for k in ("ok", "reject", "checksum")}
    print(f"{len(ROWS)} rows, {kinds}, {os.path.getsize(out)} bytes")


def stored_sizes(body):
    """the block sizes of a stream of stored blocks"""
    out, p = [], 0
    while True:
        assert body[p] in (0, 1)
        n = struct.unpack("<H", body[p + 1:p + 3])[0]
        out.append(n); p += 5 + n
        if body[p - 5 - n]:
            assert p == len(body)
            return out


def add_wrap(body, content, fmt):
    return body if fmt == 0 else zlib_wrap(body, content) if fmt == 1 else gzip_wrap(body, content)


if __name__ == "__main__":
    main()
