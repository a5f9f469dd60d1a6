"""Helpers for the tests of zstd levels 1, 2 and the negative ones with a dictionary (kompressor_amd/csrc/zstd_match_fast_dict.h,
kmp_zstd_compress_batch_dict_level).  The oracle has no restatement of this parser: the yardstick is the binary libzstd 1.5.7 --
tests/golden/zstd_dict_levels_golden.json (make_golden_dict_levels.py) and the live library where it is present."""
import ctypes
import json
import os
import random
import subprocess

import numpy as np

import helpers

LEVELS = (1, 2, -1, -5)
FEW_ROWS_LEVEL = -131072                        # the lowest level: on one dictionary's rows
# raw dictionaries: the smallest, odd sizes, around the CDict's row change (the binary library changes rows between 15 885 and 15 886:
# unknown source size + dictionary + 500 wraps to size + 499 <= 16 384), the two sides of a sixth of 128 KiB, a size at which a level-1
# CDict indexes only the dictionary's end, the largest
DICT_SIZES = (8, 33, 255, 4096, 15884, 15885, 15886, 21845, 21846, 65536, 130560)
# 6 / 7 / 8: no parse, the first parse; 8 192: the attach cut-off of strategy "fast"; 16 384: level 3's; 131 072: one block (5 000: what the
# test of the streaming entry point feeds)
SLICE_SIZES = (0, 1, 5, 6, 7, 8, 9, 63, 64, 65, 1024, 5000, 8191, 8192, 8193, 16384, 16385, 65536, 131071, 131072)
ALL_KINDS_AT = (1024, 8193, 65536)
KINDS = ("shared", "other", "substr")
_EMU = None
_GOLDEN = None
_CASES = None
_TEXT = {}


def word_text(seed, n, vocab):
    """n bytes of synthetic word text: words drawn (seeded) from a vocabulary of 400 made-up words that `vocab` seeds."""
    key = (seed, n, vocab)
    if key not in _TEXT:
        vr = random.Random(1000 + vocab)
        words = [bytes(vr.choice(b"abcdefghijklmnopqrstuvwxyz") for _ in range(vr.randrange(2, 10))) for _ in range(400)]
        r = random.Random(seed)
        out = bytearray()
        while len(out) < n:
            out += b" ".join(r.choices(words, k=256)) + (b". " if r.random() < 0.5 else b"\n")
        _TEXT[key] = bytes(out[:n])
    return _TEXT[key]


def _slice(kind, n, d, salt):
    if kind == "shared":
        return word_text(500 + salt, n, 1)
    if kind == "other":
        return word_text(600 + salt, n, 2)
    a = (salt * 977) % (len(d) - n + 1)                        # a substring of the dictionary
    return d[a:a + n]


def cases():
    """[(name, dictionary, [(slice name, bytes)])]: the raw dictionaries of DICT_SIZES (word text) with slices of SLICE_SIZES -- text that
    shares the dictionary's vocabulary, text that does not, substrings of the dictionary, the kinds in turn and all three at ALL_KINDS_AT --,
    raw dictionaries of three corpus classes with slices that mix pieces of the dictionary with fresh material, and the formatted
    dictionaries of helpers.formatted_dict_built with helpers.formatted_dict_inputs of their class."""
    global _CASES
    if _CASES is not None:
        return _CASES
    from kompressor_amd import corpus
    out = []
    for di, dsz in enumerate(DICT_SIZES):
        d = word_text(40 + di, dsz, 1)
        sl = []
        for i, n in enumerate(SLICE_SIZES):
            kinds = KINDS if n in ALL_KINDS_AT else (KINDS[(i + di) % 3],)
            for kind in kinds:
                if kind == "substr" and n > dsz:                 # (no such substring: the kind's turn goes to the shared text)
                    if len(kinds) > 1:
                        continue
                    kind = "shared"
                sl.append((f"{kind}_{n}", _slice(kind, n, d, di * 31 + i)))
        out.append((f"raw_{dsz}", d, sl))
    for k, (cls, dsz) in enumerate((("X", 8192), ("S", 32768), ("B", 2048))):
        d = corpus.make(33000 + k, 1, dsz, mix=ord(cls)).tobytes()
        sl = []
        for j, psz in enumerate((3000, 8192, 8193, 40000)):
            fresh = corpus.make(34000 + 10 * k + j, 1, psz, mix=ord(cls)).tobytes()
            third = psz // 3
            plain = (d[-200:] + fresh[:third] + d[:300] + fresh[third:2 * third] + d[dsz // 2:dsz // 2 + 500] + fresh[2 * third:])[:psz]
            sl.append((f"mixed_{psz}", plain))
        out.append((f"raw_{cls}_{dsz}", d, sl))
    for name, d, cls in helpers.formatted_dict_built()[:5]:
        ins = helpers.formatted_dict_inputs(cls, salt=7)
        out.append((name, d, [(f"{cls}_{len(p)}", p) for p in ins]))
    _CASES = out
    return out


def levels_of(name):
    return LEVELS + ((FEW_ROWS_LEVEL,) if name == "raw_4096" else ())


def golden():
    """{(dictionary name, level): [[frame length, sha256], ...]} in the order of cases()."""
    global _GOLDEN
    if _GOLDEN is None:
        with open(os.path.join(helpers.ROOT, "tests", "golden", "zstd_dict_levels_golden.json")) as f:
            g = json.load(f)
        _GOLDEN = {(r["dict"], r["level"]): r for r in g["rows"]}
    return _GOLDEN


def check_frames(name, d, slices, level, frames):
    """frames against the golden row of (name, level)."""
    import hashlib
    row = golden()[(name, level)]
    assert row["dict_sha256"] == hashlib.sha256(d).hexdigest(), name
    assert len(row["frames"]) == len(slices), name
    for (sname, p), f, (flen, sha) in zip(slices, frames, row["frames"]):
        assert len(f) == flen and hashlib.sha256(f).hexdigest() == sha, (name, level, sname, len(f), flen)


def build_emu_dict_level():
    """The emulator entry point of this parser, a library of its own (helpers.build_emu compiles a fixed file list)."""
    emu = os.path.join(helpers.ROOT, "tests", "emu")
    csrc = os.path.join(helpers.ROOT, "kompressor_amd", "csrc")
    lib = os.path.join(emu, "libkxemu_dict_level.so")
    srcs = [os.path.join(emu, f) for f in os.listdir(emu) if f.endswith((".cpp", ".h"))]
    srcs += [os.path.join(csrc, f) for f in os.listdir(csrc) if f.endswith(".h")]
    if helpers._newer(lib, srcs):
        subprocess.run(["g++", "-O1", "-std=c++17", "-shared", "-fPIC", "-I" + emu, "-I" + csrc, "-o", lib,
                        os.path.join(emu, "emu_core.cpp"), os.path.join(emu, "emu_zstd_dict_level.cpp")], check=True)
    return lib


def emu_dict_level():
    global _EMU
    if _EMU is None:
        _EMU = ctypes.CDLL(build_emu_dict_level())
    return _EMU


def emu_params(dict_size, level):
    """The host's CDict parameters: (windowLog, chainLog, hashLog, minMatch)."""
    out = (ctypes.c_uint32 * 4)()
    emu_dict_level().emu_dict_level_params(dict_size, level, out)
    return tuple(out)


def emu_compress(datas, dictionary, level, G=4, nblocks=2):
    """The host's CDict, the parser's body and the entropy body on the emulator: frames of ZstdCompressor(level, dictionary)."""
    n = len(datas)
    lens = np.array([len(d) for d in datas], dtype=np.uint32)
    offs = np.zeros(n, dtype=np.uint64)
    pos = 3                                         # (input offsets that are no multiple of 4)
    for i, d in enumerate(datas):
        offs[i] = pos
        pos += len(d) + 1
    buf = np.zeros(pos + 64, dtype=np.uint8)
    for i, d in enumerate(datas):
        buf[int(offs[i]):int(offs[i]) + len(d)] = np.frombuffer(d, dtype=np.uint8)
    cap = max([len(d) for d in datas] + [64])
    stride = (helpers.compress_bound(cap) + 64 + 15) & ~15
    out = np.zeros(n * stride, dtype=np.uint8); ooff = np.arange(n, dtype=np.uint64) * stride; olen = np.zeros(n, dtype=np.uint32)
    dbuf = np.frombuffer(dictionary, dtype=np.uint8).copy()
    status = ctypes.c_uint32(0)
    vp = helpers._vp
    r = emu_dict_level().emu_zstd_compress_dict_level(vp(buf), vp(offs), vp(lens), n, G, nblocks, vp(out), vp(ooff), vp(olen), cap,
                                                      vp(dbuf), len(dictionary), level, ctypes.byref(status))
    assert r == 0 and status.value == 0, f"emulated kernels failed: {r}, status {status.value}"
    return [out[i * stride:i * stride + int(olen[i])].tobytes() for i in range(n)]
