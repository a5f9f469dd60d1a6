"""Helpers for the tests of the frame inspection calls (kompressor_amd/csrc/zstd_frame_info.h: kmp_zstd_frame_info_batch,
kmp_zstd_frame_info_host, kmp_batch_layout).  The yardstick is the binary libzstd 1.5.7: tests/golden/zstd_frame_info_golden.json
(make_golden_frame_info.py) holds what ZSTD_findDecompressedSize, ZSTD_decompressBound and a walk with ZSTD_findFrameCompressedSize
(+ ZSTD_getFrameHeader for the frames it accepts) answer for each entry, and the live library answers for mutants where it is present."""
import base64
import ctypes
import json
import os
import random
import subprocess

import numpy as np

import helpers

# kmp_zstd_frame_info (include/kompressor_hip.h), 32 bytes
INFO = np.dtype([("content", "<u8"), ("bound", "<u8"), ("status", "<u4"), ("frames", "<u4"), ("dict_id", "<u4"), ("flags", "<u4")])
assert INFO.itemsize == 32
FIELDS = INFO.names
UNKNOWN = (1 << 64) - 1          # ZSTD_CONTENTSIZE_UNKNOWN
ERROR = (1 << 64) - 2            # ZSTD_CONTENTSIZE_ERROR
MAGIC = b"\x28\xb5\x2f\xfd"
_EMU = None
_GOLDEN = None


# ---------------------------------------------------------------- the live library ----
class _FrameHeader(ctypes.Structure):          # ZSTD_frameHeader of 1.5.7
    _fields_ = [("frameContentSize", ctypes.c_ulonglong), ("windowSize", ctypes.c_ulonglong), ("blockSizeMax", ctypes.c_uint),
                ("frameType", ctypes.c_int), ("headerSize", ctypes.c_uint), ("dictID", ctypes.c_uint), ("checksumFlag", ctypes.c_uint),
                ("_reserved1", ctypes.c_uint), ("_reserved2", ctypes.c_uint)]


def live_lib():
    """ctypes handle of the machine's libzstd 1.5.7 with the four functions typed, or None."""
    import sys
    sys.path.insert(0, os.path.join(helpers.ROOT, "oracle"))
    from libzstd_ref import find_libzstd_157
    lib = find_libzstd_157()
    if lib is None:
        return None
    for name in ("ZSTD_findDecompressedSize", "ZSTD_decompressBound"):
        fn = getattr(lib, name); fn.restype = ctypes.c_ulonglong; fn.argtypes = [ctypes.c_void_p, ctypes.c_size_t]
    lib.ZSTD_findFrameCompressedSize.restype = ctypes.c_size_t
    lib.ZSTD_findFrameCompressedSize.argtypes = [ctypes.c_void_p, ctypes.c_size_t]
    lib.ZSTD_getFrameHeader.restype = ctypes.c_size_t
    lib.ZSTD_getFrameHeader.argtypes = [ctypes.POINTER(_FrameHeader), ctypes.c_void_p, ctypes.c_size_t]
    return lib


def live_answers(lib, entry):
    """The library's answers for one entry: {"content": ZSTD_findDecompressedSize, "bound": ZSTD_decompressBound, "walk": the sizes
    ZSTD_findFrameCompressedSize returns frame by frame, "status": 0 or the error code of the frame it rejects (-(ssize_t) of the return
    value), and of the frames it accepts, by ZSTD_getFrameHeader: "frames", "dict_id", "flags"}."""
    n = len(entry)
    buf = ctypes.create_string_buffer(bytes(entry), n + 1)
    base = ctypes.addressof(buf)
    out = {"content": int(lib.ZSTD_findDecompressedSize(base, n)), "bound": int(lib.ZSTD_decompressBound(base, n)),
           "walk": [], "status": 0, "frames": 0, "dict_id": 0, "flags": 0}
    pos = 0
    while pos < n:
        r = int(lib.ZSTD_findFrameCompressedSize(base + pos, n - pos))
        if r > (1 << 63):
            out["status"] = (1 << 64) - r
            break
        h = _FrameHeader()
        assert 0 < r <= n - pos
        if lib.ZSTD_getFrameHeader(ctypes.byref(h), base + pos, n - pos) != 0:
            # a frame the library sizes and ZSTD_getFrameHeader does not know: the formats of zstd 0.5 .. 0.7 (the library's legacy support)
            assert entry[pos + 1:pos + 4] == MAGIC[1:] and entry[pos] in (0x25, 0x26, 0x27), entry[pos:pos + 8].hex()
            out["frames"] += 1
            out["flags"] |= 4
        elif h.frameType == 1:
            out["flags"] |= 2
        else:
            if out["frames"] == 0:
                out["dict_id"] = int(h.dictID)
            out["frames"] += 1
            out["flags"] |= 1 if h.checksumFlag else 0
        out["walk"].append(r)
        pos += r
    return out


def expected(ans):
    """kmp_zstd_frame_info of an entry, from the library's answers (the fixture's rows or live_answers): a tuple in FIELDS order.
    A rejected entry has content 0 and bound 0 (the library says ZSTD_CONTENTSIZE_ERROR for the bound, and ERROR or -- when a frame
    without a size stands in front of the damage -- UNKNOWN for the content); an accepted one has the library's two numbers."""
    if ans["status"]:
        assert ans["bound"] == ERROR and ans["content"] in (ERROR, UNKNOWN), ans
        return (0, 0, ans["status"], ans["frames"], ans["dict_id"], ans["flags"])
    return (ans["content"], ans["bound"], 0, ans["frames"], ans["dict_id"], ans["flags"])


# ---------------------------------------------------------------- the fixture ----
def golden():
    """[(name, entry bytes, the library's answers)]"""
    global _GOLDEN
    if _GOLDEN is None:
        with open(os.path.join(helpers.ROOT, "tests", "golden", "zstd_frame_info_golden.json")) as f:
            g = json.load(f)
        assert g["libzstd"] == 10507
        _GOLDEN = [(r["name"], base64.b64decode(r["b64"]), r) for r in g["rows"]]
    return _GOLDEN


def expected_array(rows):
    out = np.zeros(len(rows), dtype=INFO)
    for i, r in enumerate(rows):
        out[i] = expected(r)
    return out


def diff(got, want, names):
    """-> findings (empty: equal in every field)"""
    bad = []
    for i in range(len(want)):
        for f in FIELDS:
            if int(got[i][f]) != int(want[i][f]):
                bad.append(f"entry {i} ({names[i]}): {f} {int(got[i][f])}, the library says {int(want[i][f])}")
    return bad


def pack(entries, gap=0):
    """entries back to back (gap bytes of 0xA5 between them) -> (src uint8, in_off uint64, in_len uint32)"""
    lens = np.array([len(e) for e in entries], dtype=np.uint32)
    offs = np.zeros(len(entries), dtype=np.uint64)
    pos = 0
    for i, e in enumerate(entries):
        offs[i] = pos
        pos += len(e) + gap
    src = np.full(pos + 1, 0xA5, dtype=np.uint8)
    for i, e in enumerate(entries):
        src[int(offs[i]):int(offs[i]) + len(e)] = np.frombuffer(e, dtype=np.uint8)
    return src, offs, lens


def block_bounds(entry):
    """Where the frame headers end and the blocks begin and end, for choosing mutation points (accepts what it can follow, stops where
    it cannot): -> (positions of block headers, positions right behind blocks and frames)"""
    heads, ends = [], []
    pos, n = 0, len(entry)
    while pos + 5 <= n:
        m = int.from_bytes(entry[pos:pos + 4], "little")
        if m & 0xFFFFFFF0 == 0x184D2A50:
            if pos + 8 > n:
                break
            pos += 8 + int.from_bytes(entry[pos + 4:pos + 8], "little")
            ends.append(pos)
            continue
        if m != 0xFD2FB528:
            break
        fhd = entry[pos + 4]
        single = (fhd >> 5) & 1
        p = pos + 5 + (1 - single) + (0, 1, 2, 4)[fhd & 3] + ((1 << (fhd >> 6)) if fhd >> 6 else single)
        ends.append(p)
        while p + 3 <= n:
            bh = int.from_bytes(entry[p:p + 3], "little")
            heads.append(p)
            p += 3 + (1 if (bh >> 1) & 3 == 1 else bh >> 3)
            ends.append(p)
            if bh & 1:
                break
        else:
            break
        if fhd & 4:
            p += 4
            ends.append(p)
        pos = p
    return heads, [e for e in ends if e <= n]


def mutants(count, seed):
    """Seeded mutants of the fixture entries: truncations at every block boundary +- 1, single-byte changes within the first 24 bytes and
    in block headers, concatenations of two entries.  -> [(name, bytes)]"""
    rng = random.Random(seed)
    rows = [(n, e) for n, e, _ in golden()]
    out = []
    for name, e in rows:                                   # every boundary of every entry, +- 1
        if len(e) > 4096:
            continue
        _, ends = block_bounds(e)
        for p in ends:
            for q in (p - 1, p, p + 1):
                if 0 <= q < len(e):
                    out.append((f"{name}[:{q}]", e[:q]))
    rng.shuffle(out)
    out = out[:count // 3]
    nonempty = [(n, e) for n, e in rows if e]
    while len(out) < count:
        name, e = rng.choice(nonempty)
        k = rng.randrange(3)
        if k == 0:
            i = rng.randrange(min(len(e), 24))
            m = bytearray(e); m[i] = rng.choice((m[i] ^ (1 << rng.randrange(8)), rng.randrange(256)))
            out.append((f"{name} byte {i}", bytes(m)))
        elif k == 1:
            heads, _ = block_bounds(e)
            if not heads:
                continue
            i = rng.choice(heads) + rng.randrange(3)
            if i >= len(e):
                continue
            m = bytearray(e); m[i] = rng.choice((m[i] ^ (1 << rng.randrange(8)), rng.randrange(256)))
            out.append((f"{name} block header byte {i}", bytes(m)))
        else:
            n2, e2 = rng.choice(rows)
            if len(e) + len(e2) > 8192:
                continue
            out.append((f"{name} + {n2}", e + e2))
    return out


# ---------------------------------------------------------------- the product's host call ----
def host_info(entries, lib=None):
    """kmp_zstd_frame_info_host over the entries -> INFO array"""
    if lib is None:
        from kompressor_amd import _lib
        lib = _lib.load()
    src, offs, lens = pack(entries)
    info = np.zeros(len(entries), dtype=INFO)
    rc = lib.kmp_zstd_frame_info_host(helpers._vp(src), helpers._vp(offs), helpers._vp(lens), len(entries), helpers._vp(info))
    assert rc == 0, rc
    return info


# ---------------------------------------------------------------- emulator ----
def build_emu_frame_info():
    """The emulator entry points of the two kernels, a library of its own (helpers.build_emu compiles a fixed file list)."""
    emu = os.path.join(helpers.ROOT, "tests", "emu")
    csrc = os.path.join(helpers.ROOT, "kompressor_amd", "csrc")
    lib = os.path.join(emu, "libkxemu_frame_info.so")
    srcs = [os.path.join(emu, f) for f in ("emu_core.cpp", "emu_core.h", "kx_wave.h", "emu_zstd_frame_info.cpp")]
    srcs += [os.path.join(csrc, "zstd_frame_info.h"), os.path.join(helpers.ROOT, "include", "kompressor_hip.h")]
    if helpers._newer(lib, srcs):
        subprocess.run(["g++", "-O1", "-std=c++17", "-shared", "-fPIC", "-I" + emu, "-I" + csrc, "-o", lib,
                        os.path.join(emu, "emu_core.cpp"), os.path.join(emu, "emu_zstd_frame_info.cpp")], check=True)
    return lib


def emu():
    global _EMU
    if _EMU is None:
        _EMU = ctypes.CDLL(build_emu_frame_info())
        _EMU.emu_zstd_frame_info.argtypes = [ctypes.c_void_p] * 3 + [ctypes.c_uint32, ctypes.c_uint32, ctypes.c_int, ctypes.c_void_p]
        _EMU.emu_batch_layout.argtypes = [ctypes.c_void_p, ctypes.c_uint32, ctypes.c_uint32] + [ctypes.c_void_p] * 3
    return _EMU


def emu_frame_info(src_base, in_off, in_len, nblocks=2, waves=2):
    """src_base: an address or a uint8 array; in_off / in_len as the C ABI takes them -> INFO array"""
    n = len(in_len)
    in_off = np.ascontiguousarray(in_off, dtype=np.uint64); in_len = np.ascontiguousarray(in_len, dtype=np.uint32)
    info = np.zeros(n, dtype=INFO)
    base = src_base if isinstance(src_base, int) else helpers._vp(src_base)
    r = emu().emu_zstd_frame_info(base, helpers._vp(in_off), helpers._vp(in_len), n, nblocks, waves, helpers._vp(info))
    assert r == 0, f"emulated kernel failed: {r}"
    return info


def emu_layout(info, align):
    """-> (out_off uint64, out_cap uint32, total uint64[2])"""
    n = len(info)
    info = np.ascontiguousarray(info)
    off = np.full(n + 1, 0x1111111111111111, dtype=np.uint64); cap = np.full(n + 1, 0x22222222, dtype=np.uint32)
    total = np.zeros(2, dtype=np.uint64)
    r = emu().emu_batch_layout(helpers._vp(info), n, align, helpers._vp(off), helpers._vp(cap), helpers._vp(total))
    assert r == 0, f"emulated kernel failed: {r}"
    assert off[n] == 0x1111111111111111 and cap[n] == 0x22222222, "the layout kernel wrote behind its outputs"
    return off[:n], cap[:n], total


def layout_reference(info, align):
    """numpy's cumsum in 64 bits"""
    bad = (info["status"] != 0) | (info["bound"] >= (1 << 32))
    cap = np.where(bad, 0, info["bound"]).astype(np.uint64)
    step = (cap + np.uint64(align - 1)) & ~np.uint64(align - 1)
    run = np.cumsum(step, dtype=np.uint64)
    off = run - step
    return off, cap.astype(np.uint32), np.array([int(run[-1]) if len(run) else 0, int(bad.sum())], dtype=np.uint64)


# ---------------------------------------------------------------- the sanitizer program ----
def build_asan_program(out_dir):
    """tests/emu/frame_info_asan_main.cpp: a program of its own (g++ -fsanitize=address,undefined) around the parse body"""
    emu_dir = os.path.join(helpers.ROOT, "tests", "emu")
    csrc = os.path.join(helpers.ROOT, "kompressor_amd", "csrc")
    exe = os.path.join(out_dir, "frame_info_asan")
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-I" + csrc, "-o", exe,
                    os.path.join(emu_dir, "frame_info_asan_main.cpp")], check=True)
    return exe


def write_cases(path, entries, want):
    """the program's input: u32 count, then per entry u32 length, the bytes, the 32 bytes of the expected kmp_zstd_frame_info"""
    with open(path, "wb") as f:
        f.write(np.uint32(len(entries)).tobytes())
        for e, w in zip(entries, want):
            f.write(np.uint32(len(e)).tobytes()); f.write(e); f.write(w.tobytes())
