"""Helpers for the tests of the BGZF container (kompressor_amd/csrc/bgzf.h, kmp_bgzf.hip: kmp_bgzf_*).  The yardstick is
tests/golden/bgzf_golden.json (make_golden_bgzf.py): the payloads are zlib 1.2.11's raw DEFLATE streams block by block, the wrappers
are struct's, the checksums zlib.crc32's.  The tests read the fixture; the head test and the walk are restated here in Python for the
mutants the fixture does not hold."""
import base64
import ctypes
import json
import os
import random
import struct
import subprocess
import zlib

import numpy as np

import helpers

EOF = bytes.fromhex("1f8b08040000000000ff0600424302001b0003000000000000000000")
BLOCK_MAX = 65280
NO_EOF = 1
END_CANDIDATES = 1 << 20
STAT = np.dtype([("content", "<u8"), ("blocks", "<u4"), ("max_block", "<u4"), ("max_compressed", "<u4"), ("flags", "<u4"), ("status", "<i4"),
                 ("reserved", "<u4")])
assert STAT.itemsize == 32
STAT_FIELDS = ("content", "blocks", "max_block", "max_compressed", "flags", "status")
_GOLDEN = None
_EMU = None


# ---------------------------------------------------------------- cases ----
def cases():
    """(name, corpus class, seed, size, block_bytes, level, source offset): what compress is asked for.  Sizes around the block size;
    300 blocks of 64 bytes (more members than a workgroup has threads); htslib's block size; one block of 65 280 incompressible bytes
    (the largest member: stored); levels 1, 4, 9; a source at an odd address."""
    B = 4096
    out = []
    for size in (0, 1, B - 1, B, B + 1, 3 * B + 17):
        out.append((f"size{size}", "T", 95000 + size, size, B, 6, 0))
    out.append(("blocks300", "X", 95100, 300 * 64, 64, 6, 0))
    out.append(("b65280", "T", 95101, 3 * BLOCK_MAX + 17, BLOCK_MAX, 6, 0))
    out.append(("stored65280", "R", 95102, BLOCK_MAX, BLOCK_MAX, 6, 0))
    out.append(("level1", "T", 95103, 3 * B + 17, B, 1, 0))
    out.append(("level4", "S", 95104, 3 * B + 17, B, 4, 0))
    out.append(("level9", "T", 95105, 3 * B + 17, B, 9, 0))
    out.append(("odd_source", "T", 95106, 2 * B + 33, B, 6, 1))
    return out


def case_input(cls, seed, size):
    from kompressor_amd import corpus
    return corpus.make(seed, 1, size, mix=ord(cls)).tobytes() if size else b""


def blocks_of(data, block_bytes):
    return [data[i:i + block_bytes] for i in range(0, len(data), block_bytes)]


def member(payload, data, before=b"", after=b"", crc=None, isize=None, bsize=None, bc=None):
    """one BGZF member around a raw DEFLATE payload; before / after: other subfields around BC; the keyword arguments damage it"""
    extra_len = len(before) + 6 + len(after)
    total = 12 + extra_len + len(payload) + 8
    bc = struct.pack("<2sHH", b"BC", 2, (total - 1 if bsize is None else bsize) & 0xFFFF) if bc is None else bc
    extra = before + bc + after
    return (bytes.fromhex("1f8b08040000000000ff") + struct.pack("<H", len(extra)) + extra + payload
            + struct.pack("<II", zlib.crc32(data) if crc is None else crc, len(data) if isize is None else isize))


def golden():
    global _GOLDEN
    if _GOLDEN is None:
        with open(os.path.join(helpers.ROOT, "tests", "golden", "bgzf_golden.json")) as f:
            _GOLDEN = json.load(f)
        assert _GOLDEN["zlib"] == "1.2.11"
        for r in _GOLDEN["blobs"]:
            r["blob"] = base64.b64decode(r["b64"])
            if "content_b64" in r:
                r["content"] = base64.b64decode(r["content_b64"])
    return _GOLDEN


def golden_case(name):
    return next(r for r in golden()["cases"] if r["name"] == name)


def blobs(kind=None):
    """the foreign, damaged and wrong blobs: rows with name, kind ("foreign" / "damaged" / "wrong"), blob, stat (the expected kmp_bgzf_stat
    fields) and, for the readable ones, content"""
    return [r for r in golden()["blobs"] if kind is None or r["kind"] == kind]


def expected_stat(row):
    out = np.zeros(1, dtype=STAT)
    for f in STAT_FIELDS:
        out[0][f] = row["stat"][f]
    return out[0]


# ---------------------------------------------------------------- the restatement ----
def head_reference(blob, p):
    """the member head test at p, in the order of its checks -> (status, total, xlen, isize, extra)"""
    r = len(blob) - p
    b = blob[p:]
    if b[:min(r, 4)] != b"\x1f\x8b\x08\x04"[:min(r, 4)]:
        return (-3, 0, 0, 0, 0)
    if r < 12:
        return (-5, 0, 0, 0, 0)
    xlen, = struct.unpack("<H", b[10:12])
    if xlen < 6:
        return (-3, 0, 0, 0, 0)
    if r < 12 + xlen:
        return (-5, 0, 0, 0, 0)
    q, bsize, extra = 0, None, 0
    while q < xlen:
        if xlen - q < 4:
            return (-3, 0, 0, 0, 0)
        si, slen = b[12 + q:14 + q], struct.unpack("<H", b[14 + q:16 + q])[0]
        if slen > xlen - q - 4:
            return (-3, 0, 0, 0, 0)
        if si == b"BC":
            if slen != 2 or bsize is not None:
                return (-3, 0, 0, 0, 0)
            bsize, = struct.unpack("<H", b[16 + q:18 + q])
        else:
            extra = 1
        q += 4 + slen
    if bsize is None:
        return (-3, 0, 0, 0, 0)
    total = bsize + 1
    if total < 12 + xlen + 2 + 8:
        return (-3, 0, 0, 0, 0)
    if r < total:
        return (-5, 0, 0, 0, 0)
    isize, = struct.unpack("<I", b[total - 4:total])
    if isize > 65536:
        return (-3, 0, 0, 0, 0)
    return (0, total, xlen, isize, extra)


def walk_reference(blob):
    """the serial walk -> (STAT record, member_off, content_off, in_off, in_len, out_cap); the lists are empty with a status"""
    out = np.zeros(1, dtype=STAT)[0]
    p = content = 0
    mo, co, io, il, oc = [], [], [], [], []
    mb = mc = flags = 0
    status = 0 if len(blob) else -5
    while not status and p < len(blob):
        status, total, xlen, isize, extra = head_reference(blob, p)
        if status:
            break
        mo.append(p); co.append(content); io.append(p + 12 + xlen); il.append(total - 20 - xlen); oc.append(isize)
        mb, mc = max(mb, isize), max(mc, total)
        flags = (flags & 2) | (2 if extra else 0) | (1 if blob[p:p + total] == EOF else 0)
        p += total; content += isize
    if status:
        out["status"] = status
        return out, [], [], [], [], []
    out["content"], out["blocks"], out["max_block"], out["max_compressed"], out["flags"] = content, len(mo), mb, mc, flags
    return out, mo + [p], co + [content], io, il, oc


def mutants(count, seed, good):
    """seeded damage to good blobs: a byte changed, a cut at the back or the front, bytes appended, a member doubled or dropped"""
    rng = random.Random(seed)
    out = []
    while len(out) < count:
        b = bytearray(rng.choice(good))
        k = rng.randrange(7)
        if k == 0 and b:
            i = rng.randrange(len(b))
            b[i] = rng.choice((b[i] ^ (1 << rng.randrange(8)), rng.randrange(256)))
        elif k == 1 and b:                                   # a byte of some member's head
            _, mo, _, _, _, _ = walk_reference(bytes(b))
            if mo:
                i = min(rng.choice(mo) + rng.randrange(18), len(b) - 1)
                b[i] = rng.choice((b[i] ^ (1 << rng.randrange(8)), rng.randrange(256)))
        elif k == 2:
            b = b[:rng.randrange(len(b) + 1)]
        elif k == 3:
            b = b[rng.randrange(len(b) + 1):]
        elif k == 4:
            b += bytes(rng.randrange(256) for _ in range(rng.choice((1, 3, 4, 11, 12, 28, 30))))
        elif k == 5:
            b += rng.choice((EOF, EOF[:rng.randrange(28)], b"\x1f\x8b\x08\x04"))
        else:                                                # the magic planted somewhere
            if len(b) > 4:
                i = rng.randrange(len(b) - 4)
                b[i:i + 4] = b"\x1f\x8b\x08\x04"
        out.append(bytes(b))
    return out


def many_members(count, seed=7):
    """a blob of `count` members of a few bytes each (the marker among them), built without zlib's deflate: stored blocks"""
    rng = random.Random(seed)
    parts, content = [], []
    for i in range(count):
        k = rng.randrange(4)
        if k == 0:
            parts.append(EOF)
            continue
        data = bytes(rng.randrange(256) for _ in range(k))
        payload = b"\x01" + struct.pack("<HH", len(data), len(data) ^ 0xFFFF) + data
        parts.append(member(payload, data))
        content.append(data)
    return b"".join(parts), b"".join(content)


# ---------------------------------------------------------------- emulator ----
def build_emu_bgzf():
    """tests/emu/emu_bgzf.cpp, a library of its own (helpers.build_emu compiles a fixed file list)."""
    emu_dir = os.path.join(helpers.ROOT, "tests", "emu")
    csrc = os.path.join(helpers.ROOT, "kompressor_amd", "csrc")
    lib = os.path.join(emu_dir, "libkxemu_bgzf.so")
    srcs = [os.path.join(emu_dir, f) for f in ("emu_core.cpp", "emu_core.h", "kx_wave.h", "emu_bgzf.cpp")]
    srcs += [os.path.join(csrc, f) for f in os.listdir(csrc) if f.endswith(".h")] + [os.path.join(helpers.ROOT, "include", "kompressor_hip.h")]
    if helpers._newer(lib, srcs):
        subprocess.run(["g++", "-O1", "-std=c++17", "-shared", "-fPIC", "-I" + emu_dir, "-I" + csrc, "-o", lib,
                        os.path.join(emu_dir, "emu_core.cpp"), os.path.join(emu_dir, "emu_bgzf.cpp")], check=True)
    return lib


def emu():
    global _EMU
    if _EMU is None:
        _EMU = ctypes.CDLL(build_emu_bgzf())
        P, U32, U64, I = ctypes.c_void_p, ctypes.c_uint32, ctypes.c_uint64, ctypes.c_int
        _EMU.emu_bgzf_plan.argtypes = [U64, U32, U32, U64, P, P, P, U32]
        _EMU.emu_bgzf_wrap.argtypes = [P, P, P, P, P, P, U32, U32]
        _EMU.emu_bgzf_finish.argtypes = [P, P, P, U32, U32, P, P, I]
        _EMU.emu_bgzf_verify.argtypes = [P, P, P, P, P, P, P, P, U32, U32, U32]
        _EMU.emu_bgzf_walk.argtypes = [P, U64, P, P, P, U64, P, P, P]
        _EMU.emu_bgzf_head.argtypes = [P, U64, U64, P]
        _EMU.emu_bgzf_count.argtypes = [P, U64, U32, I]; _EMU.emu_bgzf_count.restype = ctypes.c_int64
        _EMU.emu_bgzf_open.argtypes = [P, U64, U32, P, P, P, P, P, P, U64, P, U32, I]
    return _EMU


def member_bound(n):
    return n + (n >> 12) + (n >> 14) + (n >> 25) + 7 + 18 + 8


def emu_container(data, block_bytes, level, flags=0, src_offset=0, status_word=0, drop=None):
    """The container as kmp_bgzf_compress makes it, on the emulator: the plan body, the DEFLATE kernels of the level (format 0), the
    wrap body over the payloads where they lie 18 bytes into their stride slots, the packing (numpy), the finish body.  drop: a block
    whose stream is taken away (the batch refused it).  -> (container bytes, result[2])"""
    vp = helpers._vp
    n = (len(data) + block_bytes - 1) // block_bytes
    src = np.zeros(src_offset + len(data) + 8, dtype=np.uint8)
    src[src_offset:src_offset + len(data)] = np.frombuffer(data, dtype=np.uint8)
    base = src.ctypes.data + src_offset
    stride = (18 + member_bound(block_bytes) + 63) & ~63
    in_off = np.full(n + 1, 0x1111111111111111, dtype=np.uint64); out_off = in_off.copy(); in_len = np.full(n + 1, 0x22222222, dtype=np.uint32)
    if n:
        assert emu().emu_bgzf_plan(len(data), block_bytes, n, stride, vp(in_off), vp(in_len), vp(out_off), 3) == 0
    assert in_off[n] == 0x1111111111111111 and out_off[n] == 0x1111111111111111 and in_len[n] == 0x22222222, "the plan wrote behind its arrays"
    chunks = [data[int(in_off[i]):int(in_off[i]) + int(in_len[i])] for i in range(n)]
    assert b"".join(chunks) == data
    streams = helpers.emu_deflate(chunks, fmt=0, level=level) if n else []
    CANARY = 0xC7
    frames = np.full(64 + n * stride + 64, CANARY, dtype=np.uint8)
    out_len = np.full(n + 1, 0x33333333, dtype=np.uint32)
    for i, s in enumerate(streams):
        if i == drop:
            s = b""
        frames[64 + i * stride + 18:64 + i * stride + 18 + len(s)] = np.frombuffer(s, dtype=np.uint8)
        out_len[i] = len(s)
    if n:
        assert emu().emu_bgzf_wrap(base, vp(in_off), vp(in_len), frames.ctypes.data + 64, vp(out_off), vp(out_len), n, 3) == 0
    assert out_len[n] == 0x33333333 and (frames[:64] == CANARY).all() and (frames[64 + n * stride:] == CANARY).all(), "the wrap wrote outside the slots"
    for i in range(n):
        assert (frames[64 + i * stride + int(out_len[i]):64 + (i + 1) * stride] == CANARY).all() or out_len[i] == 0, "the wrap wrote behind a member"
    members = [frames[64 + i * stride:64 + i * stride + int(out_len[i])].tobytes() for i in range(n)]
    dense = np.zeros(n + 1, dtype=np.uint64); dense[1:] = np.cumsum(out_len[:n], dtype=np.uint64)
    total = int(dense[n]) + (0 if flags & NO_EOF else 28)
    dst = np.full(64 + total + 64, CANARY, dtype=np.uint8)
    dst[64:64 + int(dense[n])] = np.frombuffer(b"".join(members), dtype=np.uint8)
    result = np.full(2, 7, dtype=np.uint64); word = np.array([status_word], dtype=np.uint32)
    assert emu().emu_bgzf_finish(dst.ctypes.data + 64, vp(dense), vp(out_len), n, flags, vp(word), vp(result), 4) == 0
    assert (dst[:64] == CANARY).all() and (dst[64 + total:] == CANARY).all(), "the finish kernel wrote outside the container"
    return dst[64:64 + total].tobytes(), [int(result[0]), int(result[1])]


def _exact(blob):
    """a copy of exactly the blob's length between canaries -> (keeper, address)"""
    buf = np.full(64 + len(blob) + 64, 0xEE, dtype=np.uint8)
    buf[64:64 + len(blob)] = np.frombuffer(blob, dtype=np.uint8)
    return buf, buf.ctypes.data + 64


class Opened:
    """what an open gives: stat (STAT record) and, for a good blob, the lists member_off / content_off (blocks + 1) and in_off / in_len /
    out_cap (blocks); path: 1 the parallel open, 2 the serial walk; candidates, levels"""


def _arrays(room):
    C8, C4 = 0x5A5A5A5A5A5A5A5A, 0x5A5A5A5A
    return ([np.full(room + 1 + 16, C8, dtype=np.uint64) for _ in range(3)], [np.full(room + 1 + 16, C4, dtype=np.uint32) for _ in range(2)], C8, C4)


def _collect(o, stat, a8, a4, C8, C4, room):
    o.stat = stat[0]
    n = int(stat[0]["blocks"]) if int(stat[0]["status"]) == 0 else -1
    for a, used in ((a8[0], n + 1), (a8[1], n + 1), (a8[2], n), (a4[0], n), (a4[1], n)):
        c = C8 if a.dtype == np.uint64 else C4
        assert (a[:8] == c).all() and (a[8 + room + 1:] == c).all(), "an open wrote outside an output array"
        # (with a status the arrays are never handed out: the gather may have filled them as far as the chain went)
        assert n < 0 or (a[8 + used:8 + room + 1] == c).all(), "an open wrote entries no member stands for"
    o.member_off, o.content_off = [int(x) for x in a8[0][8:8 + n + 1]], [int(x) for x in a8[1][8:8 + n + 1]]
    o.in_off, o.in_len, o.out_cap = [int(x) for x in a8[2][8:8 + max(n, 0)]], [int(x) for x in a4[0][8:8 + max(n, 0)]], [int(x) for x in a4[1][8:8 + max(n, 0)]]
    return o


def emu_open(blob, max_candidates=END_CANDIDATES, nblocks=3, waves=4):
    """the open as kmp_bgzf_open runs it, emulated, every output array between canaries -> Opened"""
    keep, at = _exact(blob)
    e = emu()
    room = e.emu_bgzf_count(at, len(blob), nblocks, waves)
    assert room >= 0
    ref = walk_reference(blob)
    room = max(room, int(ref[0]["blocks"])) if max_candidates < room else room        # (the walk's path is sized by the members)
    a8, a4, C8, C4 = _arrays(room)
    stat = np.zeros(1, dtype=STAT); info = np.zeros(3, dtype=np.uint32)
    p8 = [ctypes.c_void_p(a.ctypes.data + 64) for a in a8]; p4 = [ctypes.c_void_p(a.ctypes.data + 32) for a in a4]
    rc = e.emu_bgzf_open(at, len(blob), max_candidates, helpers._vp(stat), p8[0], p8[1], p8[2], p4[0], p4[1], room, helpers._vp(info), nblocks, waves)
    assert rc == 0, f"emu_bgzf_open: {rc}"
    assert (keep[:64] == 0xEE).all() and (keep[64 + len(blob):] == 0xEE).all()
    o = Opened()
    o.path, o.candidates, o.levels = int(info[0]), int(info[1]), int(info[2])
    return _collect(o, stat, a8, a4, C8, C4, room)


def emu_walk(blob):
    """k_bgzf_walk as the library's serial open runs it (once for the stat, once into arrays of that size) -> Opened"""
    keep, at = _exact(blob)
    stat = np.zeros(1, dtype=STAT)
    assert emu().emu_bgzf_walk(at, len(blob), helpers._vp(stat), None, None, 0, None, None, None) == 0
    room = int(stat[0]["blocks"])
    a8, a4, C8, C4 = _arrays(room)
    p8 = [ctypes.c_void_p(a.ctypes.data + 64) for a in a8]; p4 = [ctypes.c_void_p(a.ctypes.data + 32) for a in a4]
    if int(stat[0]["status"]) == 0:
        assert emu().emu_bgzf_walk(at, len(blob), helpers._vp(stat), p8[0], p8[1], room + 1, p8[2], p4[0], p4[1]) == 0
    o = Opened()
    o.path, o.candidates, o.levels = 2, 0, 0
    return _collect(o, stat, a8, a4, C8, C4, room)


def same_open(a, want_stat, ref):
    """an Opened against the restatement's answer"""
    assert a.stat.tobytes() == want_stat.tobytes(), f"{a.stat} != {want_stat}"
    _, mo, co, io, il, oc = ref
    assert (a.member_off, a.content_off, a.in_off, a.in_len, a.out_cap) == (mo, co, io, il, oc)


def emu_verify(blob, content_parts, opened, status, verify=1):
    """the verify body over decoded members (content_parts: what each decoded to, back to back) -> the statuses afterwards"""
    vp = helpers._vp
    dst = np.frombuffer(b"".join(content_parts) + b"\0" * 8, dtype=np.uint8)
    n = len(content_parts)
    out_len = np.array([len(c) for c in content_parts], dtype=np.uint32)
    out_off = np.zeros(n, dtype=np.uint64); out_off[1:] = np.cumsum(out_len[:-1], dtype=np.uint64)
    st = np.array(status, dtype=np.int32)
    keep, at = _exact(blob)
    assert emu().emu_bgzf_verify(at, vp(np.array(opened.in_off, dtype=np.uint64)), vp(np.array(opened.in_len, dtype=np.uint32)), vp(dst), vp(out_off),
                                 vp(out_len), vp(np.array(opened.out_cap, dtype=np.uint32)), vp(st), n, verify, 2) == 0
    return [int(x) for x in st]


# ---------------------------------------------------------------- the sanitizer program ----
def build_asan_program(out_dir):
    """tests/emu/bgzf_asan_main.cpp: a program of its own (g++ -fsanitize=address,undefined) around kx_bgzf_head and kx_bgzf_walk"""
    emu_dir = os.path.join(helpers.ROOT, "tests", "emu")
    csrc = os.path.join(helpers.ROOT, "kompressor_amd", "csrc")
    exe = os.path.join(out_dir, "bgzf_asan")
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-I" + csrc, "-o", exe,
                    os.path.join(emu_dir, "bgzf_asan_main.cpp")], check=True)
    return exe


def write_cases(path, entries, want):
    """the program's input: u32 count, then per blob u32 length, the bytes, the 32 bytes of the expected kmp_bgzf_stat"""
    with open(path, "wb") as f:
        f.write(np.uint32(len(entries)).tobytes())
        for e, w in zip(entries, want):
            f.write(np.uint32(len(e)).tobytes()); f.write(e); f.write(w.tobytes())
