"""Helpers for the tests of zstd's seekable container (kompressor_amd/csrc/zstd_seekable.h, kmp_seekable.hip: kmp_zstd_seekable_*).
The yardstick is tests/golden/zstd_seekable_golden.json (make_golden_seekable.py): the frames are the binary libzstd 1.5.7's, chunk by
chunk, the table is struct's, the checksums are the xxhash module's -- each also asserted there against the checksum libzstd itself
appends to the chunk's frame.  The tests need neither module: they read the fixture."""
import base64
import ctypes
import json
import os
import struct
import subprocess

import numpy as np

import helpers

SEEKABLE_MAGIC = 0x8F92EAB1
SKIP_MAGIC = 0x184D2A5E
STAT = np.dtype([("content", "<u8"), ("table_off", "<u8"), ("frames", "<u4"), ("max_frame", "<u4"), ("max_compressed", "<u4"),
                 ("flags", "<u4"), ("status", "<u4"), ("reserved", "<u4")])
assert STAT.itemsize == 40
STAT_FIELDS = ("content", "table_off", "frames", "max_frame", "max_compressed", "flags", "status")
_GOLDEN = None
_EMU = None


# ---------------------------------------------------------------- cases ----
def cases():
    """(name, corpus class, seed, size, frame_bytes, level, checksums, source offset): what compress is asked for.  Sizes around the
    frame size; 300 chunks of 64 bytes (more chunks than one workgroup of the table kernel has threads); the frame sizes 64, 4 096,
    65 536 and 131 072; levels 3, 1, -5, 7; checksums on and off; last chunks of 1 .. 33 bytes and frame sizes 32 k + {0, 1, 4, 8, 31}:
    every branch of XXH64 (no stripe, one stripe, the 8-, 4- and 1-byte tails); a source at an odd address."""
    F = 4096
    out = []
    for size in (0, 1, F - 1, F, F + 1, 3 * F + 17):
        out.append((f"size{size}", "T", 91000 + size, size, F, 3, 1, 0))
    out.append(("chunks300", "X", 91100, 300 * 64, 64, 3, 1, 0))
    out.append(("f65536", "T", 91101, 3 * 65536 + 17, 65536, 3, 1, 0))
    out.append(("f131072", "B", 91102, 131072 + 1, 131072, 3, 1, 0))
    out.append(("level1", "T", 91103, 3 * F + 17, F, 1, 1, 0))
    out.append(("level-5", "S", 91104, 3 * F + 17, F, -5, 1, 0))
    out.append(("level7", "T", 91105, 3 * F + 17, F, 7, 1, 0))
    out.append(("level1_f65536", "D", 91106, 65536 + 4097, 65536, 1, 0, 0))
    out.append(("nosum", "T", 91107, 3 * F + 17, F, 3, 0, 0))
    out.append(("nosum_chunks300", "B", 91108, 300 * 64 - 5, 64, 3, 0, 0))
    for tail in range(1, 34):
        out.append((f"tail{tail}", "T", 91200 + tail, 64 + tail, 64, 3, 1, 0))
    for fb in (96, 97, 100, 104, 127):
        out.append((f"f{fb}", "X", 91300 + fb, 3 * fb + 5, fb, 3, 1, 0))
    out.append(("odd_source", "T", 91400, 2 * F + 33, F, 3, 1, 1))
    return out


def case_input(cls, seed, size):
    from kompressor_amd import corpus
    return corpus.make(seed, 1, size, mix=ord(cls)).tobytes() if size else b""


def chunks_of(data, frame_bytes):
    return [data[i:i + frame_bytes] for i in range(0, len(data), frame_bytes)]


def seek_table(entries, checksums, descriptor=None, frame_size=None, magic=SEEKABLE_MAGIC, skip_magic=SKIP_MAGIC, frames=None):
    """entries: [(compressed size, decompressed size, checksum)] -> the table's bytes; the keyword arguments damage it"""
    body = b"".join(struct.pack("<III", c, d, x) if checksums else struct.pack("<II", c, d) for c, d, x in entries)
    desc = (0x80 if checksums else 0) if descriptor is None else descriptor
    size = len(body) + 9 if frame_size is None else frame_size
    n = len(entries) if frames is None else frames
    return struct.pack("<II", skip_magic, size) + body + struct.pack("<IB", n, desc) + struct.pack("<I", magic)


def golden():
    global _GOLDEN
    if _GOLDEN is None:
        with open(os.path.join(helpers.ROOT, "tests", "golden", "zstd_seekable_golden.json")) as f:
            _GOLDEN = json.load(f)
        assert _GOLDEN["libzstd"] == 10507
        for r in _GOLDEN["blobs"]:
            r["blob"] = base64.b64decode(r["b64"])
    return _GOLDEN


def golden_case(name):
    return next(r for r in golden()["cases"] if r["name"] == name)


def blobs(kind=None):
    """the foreign and damaged containers: rows with name, kind ("foreign" / "damaged" / "flipped"), blob, stat (the expected
    kmp_seekable_stat fields) and, for the readable ones, cls / seed / size of the content"""
    return [r for r in golden()["blobs"] if kind is None or r["kind"] == kind]


def expected_stat(row):
    out = np.zeros(1, dtype=STAT)
    for f in STAT_FIELDS:
        out[0][f] = row["stat"][f]
    return out[0]


def edge_ranges(content_size, frame_starts):
    """Ranges that start or end on, one before and one after frame edges, a one-byte range in the last frame, the full range, an empty
    one and one that reaches past the end: [(lo, hi)] with lo < hi <= content_size except the last two."""
    pts = sorted({p for s in frame_starts for p in (s - 1, s, s + 1) if 0 <= p <= content_size} | {0, content_size})
    out = [(0, content_size)]
    for i, a in enumerate(pts):
        for b in pts[i + 1:i + 4]:
            out.append((a, b))
    if len(pts) > 2:
        out.append((pts[1], pts[-2]))
    if content_size:
        out.append((content_size - 1, content_size))
    out += [(content_size // 2, content_size // 2), (max(content_size - 3, 0), content_size + 1000)]
    return [r for r in dict.fromkeys(out)]


# ---------------------------------------------------------------- emulator ----
def build_emu_seekable():
    """tests/emu/emu_zstd_seekable.cpp, a library of its own (helpers.build_emu compiles a fixed file list)."""
    emu = os.path.join(helpers.ROOT, "tests", "emu")
    csrc = os.path.join(helpers.ROOT, "kompressor_amd", "csrc")
    lib = os.path.join(emu, "libkxemu_seekable.so")
    srcs = [os.path.join(emu, f) for f in ("emu_core.cpp", "emu_core.h", "kx_wave.h", "emu_zstd_seekable.cpp")]
    srcs += [os.path.join(csrc, f) for f in os.listdir(csrc) if f.endswith(".h")] + [os.path.join(helpers.ROOT, "include", "kompressor_hip.h")]
    if helpers._newer(lib, srcs):
        subprocess.run(["g++", "-O1", "-std=c++17", "-shared", "-fPIC", "-I" + emu, "-I" + csrc, "-o", lib,
                        os.path.join(emu, "emu_core.cpp"), os.path.join(emu, "emu_zstd_seekable.cpp")], check=True)
    return lib


def emu():
    global _EMU
    if _EMU is None:
        _EMU = ctypes.CDLL(build_emu_seekable())
        P, U32, U64 = ctypes.c_void_p, ctypes.c_uint32, ctypes.c_uint64
        _EMU.emu_seekable_plan.argtypes = [U64, U32, U32, U64, P, P, P, U32]
        _EMU.emu_seekable_xxh64.argtypes = [P, P, P, U32, P, P, P, U32, ctypes.c_int]
        _EMU.emu_seekable_table.argtypes = [P, P, P, P, P, U32, U32, P, P, ctypes.c_int]
        _EMU.emu_seekable_index.argtypes = [P, U64, P]
    return _EMU


def emu_frames(chunks, level):
    """the chunks' frames from the emulated compress kernels of the level (tests/helpers.py)"""
    if not chunks:
        return []
    if level in (0, 3):
        return helpers.emu_compress(chunks)
    if level in (1, 2) or level < 0:
        return helpers.emu_compress_level(chunks, level)
    return helpers.emu_compress_lazy(chunks, level)


def emu_container(data, frame_bytes, level, checksums, src_offset=0, status_word=0):
    """The container as kmp_zstd_seekable_compress makes it, on the emulator: the plan body, the XXH64 body over the chunks, the level's
    compress kernels, the packing (numpy), the table body.  -> (container bytes, result[2])"""
    vp = helpers._vp
    n = (len(data) + frame_bytes - 1) // frame_bytes
    src = np.zeros(src_offset + len(data) + 8, dtype=np.uint8)
    src[src_offset:src_offset + len(data)] = np.frombuffer(data, dtype=np.uint8)
    base = src.ctypes.data + src_offset
    stride = (helpers.compress_bound(frame_bytes) + 8 + 63) & ~63
    in_off = np.full(n + 1, 0x1111111111111111, dtype=np.uint64); out_off = in_off.copy(); in_len = np.full(n + 1, 0x22222222, dtype=np.uint32)
    if n:
        assert emu().emu_seekable_plan(len(data), frame_bytes, n, stride, vp(in_off), vp(in_len), vp(out_off), 3) == 0
    assert in_off[n] == 0x1111111111111111 and out_off[n] == 0x1111111111111111 and in_len[n] == 0x22222222, "the plan wrote behind its arrays"
    assert [int(x) for x in in_off[:n]] == [i * frame_bytes for i in range(n)] and [int(x) for x in out_off[:n]] == [i * stride for i in range(n)]
    chunks = [data[int(in_off[i]):int(in_off[i]) + int(in_len[i])] for i in range(n)]
    assert b"".join(chunks) == data
    cks = np.full(n + 1, 0x33333333, dtype=np.uint32)
    if checksums and n:
        assert emu().emu_seekable_xxh64(base, vp(in_off), vp(in_len), n, vp(cks), None, None, 3, 2) == 0
        assert cks[n] == 0x33333333
    frames = emu_frames(chunks, level)
    clen = np.array([len(f) for f in frames] + [0], dtype=np.uint32)
    dense = np.zeros(n + 1, dtype=np.uint64); dense[1:] = np.cumsum(clen[:n], dtype=np.uint64)
    table = 17 + n * (12 if checksums else 8)
    total = int(dense[n]) + table
    CANARY = 0xC7
    dst = np.full(64 + total + 64, CANARY, dtype=np.uint8)
    dst[64:64 + int(dense[n])] = np.frombuffer(b"".join(frames), dtype=np.uint8)
    result = np.zeros(2, dtype=np.uint64); word = np.array([status_word], dtype=np.uint32)
    assert emu().emu_seekable_table(dst.ctypes.data + 64, vp(dense), vp(clen), vp(in_len), vp(cks), n, 1 if checksums else 0, vp(word), vp(result), 4) == 0
    assert (dst[:64] == CANARY).all() and (dst[64 + total:] == CANARY).all(), "the table kernel wrote outside the container"
    return dst[64:64 + total].tobytes(), [int(result[0]), int(result[1])]


def emu_index(blob):
    """kx_seekable_index as the kernel runs it, over a copy of exactly the blob's length between canaries -> STAT record"""
    buf = np.full(64 + len(blob) + 64, 0xEE, dtype=np.uint8)
    buf[64:64 + len(blob)] = np.frombuffer(blob, dtype=np.uint8)
    out = np.zeros(1, dtype=STAT)
    assert emu().emu_seekable_index(buf.ctypes.data + 64, len(blob), helpers._vp(out)) == 0
    return out[0]


def emu_verify(content, frame_starts, frame_lens, entries12, status):
    """the XXH64 body in its verifying form over decoded frames -> the statuses afterwards"""
    vp = helpers._vp
    src = np.frombuffer(content + b"\0" * 8, dtype=np.uint8)
    off = np.array(frame_starts, dtype=np.uint64); ln = np.array(frame_lens, dtype=np.uint32)
    st = np.array(status, dtype=np.uint32); ent = np.frombuffer(entries12 + b"\0", dtype=np.uint8)
    assert emu().emu_seekable_xxh64(vp(src), vp(off), vp(ln), len(frame_lens), None, vp(ent), vp(st), 2, 2) == 0
    return [int(x) for x in st]


def parse_table(blob):
    """(entries [(c, d, checksum or None)], frame starts, content starts) of a container the fixture calls good"""
    n, desc = struct.unpack("<IB", blob[-9:-4])
    eb = 12 if desc & 0x80 else 8
    at = len(blob) - 17 - n * eb
    ents, fo, co, c0, d0 = [], [], [], 0, 0
    for i in range(n):
        e = blob[at + 8 + i * eb:at + 8 + (i + 1) * eb]
        c, d = struct.unpack("<II", e[:8])
        ents.append((c, d, struct.unpack("<I", e[8:])[0] if eb == 12 else None))
        fo.append(c0); co.append(d0); c0 += c; d0 += d
    return ents, fo + [c0], co + [d0]


# ---------------------------------------------------------------- the sanitizer program ----
def build_asan_program(out_dir):
    """tests/emu/seekable_asan_main.cpp: a program of its own (g++ -fsanitize=address,undefined) around kx_seekable_index"""
    emu_dir = os.path.join(helpers.ROOT, "tests", "emu")
    csrc = os.path.join(helpers.ROOT, "kompressor_amd", "csrc")
    exe = os.path.join(out_dir, "seekable_asan")
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-I" + csrc, "-o", exe,
                    os.path.join(emu_dir, "seekable_asan_main.cpp")], check=True)
    return exe


def write_cases(path, entries, want):
    """the program's input: u32 count, then per blob u32 length, the bytes, the 40 bytes of the expected kmp_seekable_stat"""
    with open(path, "wb") as f:
        f.write(np.uint32(len(entries)).tobytes())
        for e, w in zip(entries, want):
            f.write(np.uint32(len(e)).tobytes()); f.write(e); f.write(w.tobytes())


def index_reference(blob):
    """The validation restated in Python (the order of the issue's checks), for mutants the fixture does not hold -> STAT record"""
    out = np.zeros(1, dtype=STAT)[0]

    def bad(code):
        out["status"] = code
        return out
    size = len(blob)
    if size < 17 or struct.unpack("<I", blob[-4:])[0] != SEEKABLE_MAGIC:
        return bad(10)
    n, desc = struct.unpack("<IB", blob[-9:-4])
    if desc & 0x7C:
        return bad(20)
    eb = 12 if desc & 0x80 else 8
    if n > (1 << 27) or n * eb + 17 > size:
        return bad(20)
    at = size - (n * eb + 17)
    if struct.unpack("<I", blob[at:at + 4])[0] != SKIP_MAGIC:
        return bad(10)
    if struct.unpack("<I", blob[at + 4:at + 8])[0] != n * eb + 9:
        return bad(20)
    cs = ds = mc = md = 0
    for i in range(n):
        c, d = struct.unpack("<II", blob[at + 8 + i * eb:at + 16 + i * eb])
        if d > (1 << 30):
            return bad(20)
        cs += c; ds += d; mc = max(mc, c); md = max(md, d)
    if cs != at:
        return bad(20)
    out["content"], out["table_off"], out["frames"], out["max_frame"], out["max_compressed"], out["flags"] = ds, at, n, md, mc, desc >> 7
    return out
