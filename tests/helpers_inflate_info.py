"""Helpers for the tests of the inflate sizing pass (kompressor_amd/csrc/deflate_info.h: kmp_inflate_info_batch).  The authority is this
machine's zlib through Python's zlib module: verdict() is the rule every comparison uses.  tests/golden/inflate_info_golden.json
(make_golden_inflate_info.py) holds streams written by zlib.compressobj and by hand with the 32 bytes each one answers."""
import base64
import ctypes
import json
import os
import random
import subprocess
import zlib

import numpy as np

import helpers

# kmp_inflate_info (include/kompressor_hip.h), 32 bytes
INFO = np.dtype([("content", "<u8"), ("bound", "<u8"), ("status", "<i4"), ("blocks", "<u4"), ("flags", "<u4"), ("window_bits", "<u4")])
assert INFO.itemsize == 32
FIELDS = INFO.names
WBITS = {0: -15, 1: 15, 2: 31, 3: 47}
FMT_NAMES = {0: "raw", 1: "zlib", 2: "gzip", 3: "auto"}
WRAPPER_MIN = {0: 0, 1: 6, 2: 18}
_EMU = None
_GOLDEN = None


# ---------------------------------------------------------------- the rule ----
def verdict(entry, fmt):
    """zlib's word on one entry read in one format (0 raw, 1 zlib, 2 gzip, 3 zlib or gzip):
    ("ok", content bytes)   no exception, the stream ended, nothing behind it
    ("checksum", None)      refused with "incorrect data check" alone: the sizing pass may answer either way
    ("reject", -3 | -5)     everything else; -5: zlib raised nothing and still waits for input, -3: it raised, or bytes are left over"""
    o = zlib.decompressobj(WBITS[fmt])
    try:
        ref = o.decompress(bytes(entry))
    except zlib.error as e:
        return ("checksum", None) if "incorrect data check" in str(e) else ("reject", -3)
    if not o.eof:
        return ("reject", -5)
    if o.unused_data:
        return ("reject", -3)
    return ("ok", ref)


def check_against_zlib(cases, got):
    """cases: [(name, entry, fmt)], got: INFO array -> (findings, counts of ok / reject / checksum by zlib alone)"""
    bad = []
    counts = {"ok": 0, "reject": 0, "checksum": 0}
    for (name, e, fmt), g in zip(cases, got):
        kind, val = verdict(e, fmt)
        counts[kind] += 1
        st, content, bound = int(g["status"]), int(g["content"]), int(g["bound"])
        what = None
        if st not in (0, -3, -5) or content != bound or (st != 0 and content != 0):
            what = "malformed answer"
        elif kind == "ok" and (st != 0 or content != len(val)):
            what = f"zlib decodes it to {len(val)} bytes"
        elif kind == "reject" and st == 0:
            what = "zlib rejects it"
        if what:
            bad.append(f"{name} ({FMT_NAMES[fmt]}, {len(e)} bytes, {bytes(e[:48]).hex()}): status {st} content {content} bound {bound}; {what}")
    return bad, counts


def assert_not_hollow(counts):
    """the three conditions that keep a comparison with zlib from going hollow"""
    n = sum(counts.values())
    assert counts["ok"] >= 0.10 * n, counts
    assert counts["reject"] >= 0.30 * n, counts
    assert counts["checksum"] <= 0.10 * n, counts


# ---------------------------------------------------------------- the fixture ----
def stored_stream(seed, blocks):
    """a raw stream of stored blocks of these sizes over seeded random bytes (the fixture keeps such entries as this recipe)"""
    data = random.Random(seed).randbytes(sum(blocks))
    out, p = bytearray(), 0
    for k, n in enumerate(blocks):
        out += bytes((1 if k == len(blocks) - 1 else 0,)) + n.to_bytes(2, "little") + (n ^ 0xFFFF).to_bytes(2, "little") + data[p:p + n]
        p += n
    return bytes(out)


def golden():
    """[(name, entry bytes, fmt, row)]; row: status, content, blocks, flags, window_bits, kind ("ok" / "reject" / "checksum")"""
    global _GOLDEN
    if _GOLDEN is None:
        with open(os.path.join(helpers.ROOT, "tests", "golden", "inflate_info_golden.json")) as f:
            g = json.load(f)
        _GOLDEN = [(r["name"], base64.b64decode(r["b64"]) if "b64" in r else stored_stream(r["stored"]["seed"], r["stored"]["blocks"]), r["fmt"], r)
                   for r in g["rows"]]
    return _GOLDEN


def expected(row):
    return (row["content"], row["content"], row["status"], row["blocks"], row["flags"], row["window_bits"])


def expected_array(rows):
    out = np.zeros(len(rows), dtype=INFO)
    for i, r in enumerate(rows):
        out[i] = expected(r)
    return out


def diff(got, want, names):
    bad = []
    for i in range(len(want)):
        for f in FIELDS:
            if int(got[i][f]) != int(want[i][f]):
                bad.append(f"entry {i} ({names[i]}): {f} {int(got[i][f])}, expected {int(want[i][f])}")
    return bad


def by_format(rows):
    """{fmt: [index into rows]}"""
    out = {}
    for i, r in enumerate(rows):
        out.setdefault(r[2], []).append(i)
    return out


def pack(entries, seed=0):
    """every entry at an unaligned offset (the starts walk through the residues modulo 16), 1 .. 15 canary bytes (0xA5) between them
    -> (src uint8, in_off uint64, in_len uint32)"""
    rng = random.Random(seed)
    lens = np.array([len(e) for e in entries], dtype=np.uint32)
    offs = np.zeros(len(entries), dtype=np.uint64)
    pos = 1
    for i, e in enumerate(entries):
        pos += rng.randrange(1, 16)
        if i % 3 == 0 and pos % 16 == 0:
            pos += 1
        offs[i] = pos
        pos += len(e)
    src = np.full(pos + 16, 0xA5, dtype=np.uint8)
    for i, e in enumerate(entries):
        src[int(offs[i]):int(offs[i]) + len(e)] = np.frombuffer(e, dtype=np.uint8)
    return src, offs, lens


# ---------------------------------------------------------------- mutants ----
def mutants(count, seed, max_len=1500):
    """Seeded cases for the comparison with the live zlib: accepted fixture streams of up to max_len bytes (two in three raw), one in six intact (some
    zlib / gzip ones read through format 3), the others through the mutation kinds of tests/fuzz_decoders.py.  -> [(name, bytes, fmt)]"""
    from fuzz_decoders import mutate
    rng = random.Random(seed)
    base = [(n, e, f) for n, e, f, r in golden() if r["kind"] == "ok" and len(e) <= max_len]
    only = [e for _, e, _ in base]
    raw, wrapped = [b for b in base if b[2] == 0], [b for b in base if b[2] != 0]
    out = []
    while len(out) < count:
        # (two in three are raw streams: a damaged literal in a wrapped one is the class zlib refuses for its data check alone, which
        #  says nothing about the walk and must stay a small share)
        name, e, fmt = rng.choice(raw if rng.randrange(3) else wrapped)
        if fmt in (1, 2) and rng.random() < 0.3:
            fmt = 3
        if rng.randrange(6) == 0:
            out.append((f"{name} intact", e, fmt))
        else:
            m, what = mutate(rng, e, only)
            out.append((f"{name} {what}", m, fmt))
    return out


def by_fmt_cases(cases):
    out = {}
    for i, c in enumerate(cases):
        out.setdefault(c[2], []).append(i)
    return out


# ---------------------------------------------------------------- emulator ----
def build_emu_inflate_info():
    """The emulator entry point of k_inflate_size, a library of its own (helpers.build_emu compiles a fixed file list)."""
    emu = os.path.join(helpers.ROOT, "tests", "emu")
    csrc = os.path.join(helpers.ROOT, "kompressor_amd", "csrc")
    lib = os.path.join(emu, "libkxemu_inflate_info.so")
    srcs = [os.path.join(emu, f) for f in ("emu_core.cpp", "emu_core.h", "kx_wave.h", "emu_inflate_info.cpp")]
    srcs += [os.path.join(csrc, f) for f in os.listdir(csrc) if f.endswith(".h")] + [os.path.join(helpers.ROOT, "include", "kompressor_hip.h")]
    if helpers._newer(lib, srcs):
        subprocess.run(["g++", "-O1", "-std=c++17", "-shared", "-fPIC", "-I" + emu, "-I" + csrc, "-o", lib,
                        os.path.join(emu, "emu_core.cpp"), os.path.join(emu, "emu_inflate_info.cpp")], check=True)
    return lib


def emu():
    global _EMU
    if _EMU is None:
        _EMU = ctypes.CDLL(build_emu_inflate_info())
        _EMU.emu_inflate_info.argtypes = [ctypes.c_void_p] * 3 + [ctypes.c_uint32, ctypes.c_uint32, ctypes.c_void_p]
    return _EMU


def emu_inflate_info(src_base, in_off, in_len, fmt):
    """src_base: an address or a uint8 array; in_off / in_len as the C ABI takes them -> INFO array (prefilled with 0xEE bytes)"""
    n = len(in_len)
    in_off = np.ascontiguousarray(in_off, dtype=np.uint64); in_len = np.ascontiguousarray(in_len, dtype=np.uint32)
    info = np.frombuffer(bytearray(b"\xEE" * (32 * (n + 1))), dtype=INFO)
    base = src_base if isinstance(src_base, int) else helpers._vp(src_base)
    r = emu().emu_inflate_info(base, helpers._vp(in_off), helpers._vp(in_len), n, fmt, helpers._vp(info))
    assert r == 0, f"emulated kernel failed: {r}"
    assert info[n:].tobytes() == b"\xEE" * 32, "the kernel wrote behind its output"
    return info[:n].copy()


def emu_cases(cases, seed=0):
    """[(name, bytes, fmt)] -> INFO array in the cases' order: one emulated batch per format, hostile packing"""
    got = np.zeros(len(cases), dtype=INFO)
    for fmt, idx in by_fmt_cases(cases).items():
        src, offs, lens = pack([cases[i][1] for i in idx], seed + fmt)
        got[idx] = emu_inflate_info(src, offs, lens, fmt)
    return got


# ---------------------------------------------------------------- the sanitizer program ----
def build_asan_program(out_dir):
    """tests/emu/inflate_info_asan_main.cpp + the emulator core: a program of its own (g++ -fsanitize=address,undefined)"""
    emu_dir = os.path.join(helpers.ROOT, "tests", "emu")
    csrc = os.path.join(helpers.ROOT, "kompressor_amd", "csrc")
    exe = os.path.join(out_dir, "inflate_info_asan")
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-I" + emu_dir, "-I" + csrc,
                    "-o", exe, os.path.join(emu_dir, "inflate_info_asan_main.cpp"), os.path.join(emu_dir, "emu_core.cpp")], check=True)
    return exe


def write_cases(path, cases, want):
    """the program's input: u32 count, then per entry u32 length, u32 format, the bytes, the 32 bytes of the expected kmp_inflate_info"""
    with open(path, "wb") as f:
        f.write(np.uint32(len(cases)).tobytes())
        for (_, e, fmt), w in zip(cases, want):
            f.write(np.uint32(len(e)).tobytes()); f.write(np.uint32(fmt).tobytes()); f.write(bytes(e)); f.write(w.tobytes())
