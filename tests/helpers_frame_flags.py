"""Helpers for the tests of the frame flags (kmp_batch_set_frame_flags, ZSTD_c_contentSizeFlag / checksumFlag / dictIDFlag of
kmp_zstd_cctx_set_parameter): the cases, the golden file of the binary libzstd 1.5.7 (tests/golden/zstd_frame_flags_golden.json,
make_golden_frame_flags.py), the live library driven with the same parameters, and the emulator entry point."""
import ctypes
import hashlib
import json
import os
import random
import subprocess

import numpy as np

import helpers
import helpers_dict_levels as hd

CHECKSUM, NO_CONTENT_SIZE, NO_DICT_ID = 1, 2, 4                 # KMP_FRAME_*
FLAG_SETS = (CHECKSUM, NO_CONTENT_SIZE, CHECKSUM | NO_CONTENT_SIZE)
FLAG_SETS_FORMATTED = FLAG_SETS + (NO_DICT_ID, CHECKSUM | NO_CONTENT_SIZE | NO_DICT_ID)
# 0 .. 33: XXH64's short path and its stripe of 32 bytes; 255 / 256 and 65 791 / 65 792: the Frame_Content_Size codes; 131 072 / 131 073:
# one block against two; 5 000, 20 000 and 65 536: what the tests of the streaming entry points feed
SIZES = (0, 1, 31, 32, 33, 255, 256, 5000, 20000, 65536, 65791, 65792, 131072, 131073)
BIG_SIZE = 300000
LEVELS = (3, 1, -5, 4, 7)
BIG_LEVELS = (3, 6)                                             # at BIG_SIZE (6: the lazy several-block path)
DICT_LEVELS = (3, 1)
DICT_SLICE_SIZES = (1024, 20000)
_GOLDEN = None
_EMU = None


def text(n):
    return hd.word_text(900 + n % 997, n, 1)


def slices_of(level, big=None):
    """[(name, bytes)] of a level's row without a dictionary: the word text of SIZES, 4 096 equal bytes (an RLE block), 4 096 random bytes
    (a raw block); big: True only BIG_SIZE, False without it, None both where the level has it."""
    small = [(f"text_{n}", text(n)) for n in SIZES] + [("rle_4096", b"\x5a" * 4096), ("rand_4096", random.Random(4096).randbytes(4096))]
    large = [(f"text_{BIG_SIZE}", text(BIG_SIZE))] if level in BIG_LEVELS else []
    if level not in LEVELS:
        small = []
    return large if big is True else small if big is False else small + large


def dictionaries():
    """[(name, bytes, formatted)]: a raw dictionary of 4 096 bytes of the slices' vocabulary, the first two built formatted dictionaries (the
    first one's ID is 0, which no header names: the second shows what KMP_FRAME_NO_DICT_ID leaves out)"""
    built = helpers.formatted_dict_built()
    return [("raw_4096", hd.word_text(40, 4096, 1), False)] + [(name, d, True) for name, d, _ in built[:2]]


def dict_slices():
    return [(f"text_{n}", text(n)) for n in DICT_SLICE_SIZES]


def rows():
    """[(level, dictionary name or None, dictionary bytes or None, flags, [(slice name, bytes)])] in the golden file's order"""
    out = []
    for level in LEVELS + tuple(v for v in BIG_LEVELS if v not in LEVELS):
        for fl in FLAG_SETS + ((0,) if level == 3 else ()):               # (level 3 also without flags: what a fresh context writes)
            out.append((level, None, None, fl, slices_of(level)))
    for name, d, formatted in dictionaries():
        for level in DICT_LEVELS:
            for fl in (FLAG_SETS_FORMATTED if formatted else FLAG_SETS):
                out.append((level, name, d, fl, dict_slices()))
    return out


def golden():
    global _GOLDEN
    if _GOLDEN is None:
        with open(os.path.join(helpers.ROOT, "tests", "golden", "zstd_frame_flags_golden.json")) as f:
            g = json.load(f)
        g["by_key"] = {(r["level"], r["dict"], r["flags"]): r for r in g["rows"]}
        _GOLDEN = g
    return _GOLDEN


def golden_frames(level, dict_name, flags):
    """{slice name: (length, sha256)} of one row"""
    r = golden()["by_key"][(level, dict_name, flags)]
    return {s: (f[0], f[1]) for s, f in zip(r["slices"], r["frames"])}


def check_frame(frame, want, what):
    assert (len(frame), hashlib.sha256(frame).hexdigest()) == tuple(want), (what, len(frame), want[0], frame[:12].hex())


def params_of(flags):
    """the ZSTD_cParameter settings of a flag set: [(id, value)]"""
    return ([(201, 1)] if flags & CHECKSUM else []) + ([(200, 0)] if flags & NO_CONTENT_SIZE else []) + ([(202, 0)] if flags & NO_DICT_ID else [])


# ---- the binary library with these parameters ---------------------------------------------------------------------------------------
def _cctx(z, level, params, dictionary=None):
    lib = z.lib
    lib.ZSTD_CCtx_loadDictionary.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_size_t]
    lib.ZSTD_CCtx_loadDictionary.restype = ctypes.c_size_t
    cctx = lib.ZSTD_createCCtx()
    lib.ZSTD_CCtx_setParameter(cctx, 100, level)
    for pid, value in params:
        r = lib.ZSTD_CCtx_setParameter(cctx, pid, value)
        assert not lib.ZSTD_isError(r), (pid, value)
    if dictionary is not None:
        r = lib.ZSTD_CCtx_loadDictionary(cctx, dictionary, len(dictionary))
        assert not lib.ZSTD_isError(r)
    return cctx


def lib_set_parameter(z, pid, value):
    """what ZSTD_CCtx_setParameter returns on a fresh context (an error: its negated code, as a negative number)"""
    lib = z.lib
    cctx = lib.ZSTD_createCCtx()
    try:
        r = lib.ZSTD_CCtx_setParameter(cctx, pid, value)
        return -int((1 << 64) - r) if lib.ZSTD_isError(r) else int(r)
    finally:
        lib.ZSTD_freeCCtx(cctx)


def lib_compress2(z, data, level, flags, dictionary=None):
    """ZSTD_CCtx_setParameter(level, the flag set's parameters) [+ ZSTD_CCtx_loadDictionary] + ZSTD_compress2 into a bound-sized buffer"""
    lib = z.lib
    cctx = _cctx(z, level, params_of(flags), dictionary)
    try:
        cap = lib.ZSTD_compressBound(len(data))
        out = ctypes.create_string_buffer(cap)
        n = lib.ZSTD_compress2(cctx, out, cap, data, len(data))
        assert not lib.ZSTD_isError(n), lib.ZSTD_getErrorName(n)
        return out.raw[:n]
    finally:
        lib.ZSTD_freeCCtx(cctx)


def lib_stream(z, data, cuts, level, flags, out_chunk, end_from_first=False):
    """ZSTD_compressStream2 over data[cuts[i]:cuts[i + 1]]: e_continue for every piece but the last, e_end for that (end_from_first: e_end
    from the first call, the reference's one-shot loop, SliceTransform.kt:33-45); output drained through slices of out_chunk bytes"""
    lib = z.lib
    _ZBuf = lib.ZSTD_compressStream2.argtypes[1]._type_          # (the loader's ZSTD_inBuffer / ZSTD_outBuffer: one prototype for all callers)
    cctx = _cctx(z, level, params_of(flags))
    src = ctypes.create_string_buffer(data, len(data) + 1)
    out = ctypes.create_string_buffer(out_chunk)
    res = bytearray()
    pieces = list(zip(cuts[:-1], cuts[1:]))
    try:
        for j, (a, b) in enumerate(pieces):
            end = end_from_first or j == len(pieces) - 1
            ib = _ZBuf(ctypes.cast(src, ctypes.c_void_p).value, b, a)
            while True:
                ob = _ZBuf(ctypes.cast(out, ctypes.c_void_p).value, out_chunk, 0)
                r = lib.ZSTD_compressStream2(cctx, ctypes.byref(ob), ctypes.byref(ib), 2 if end else 0)
                assert not lib.ZSTD_isError(r), lib.ZSTD_getErrorName(r)
                res += out.raw[:ob.pos]
                if (end and r == 0) or (not end and ib.pos == ib.size and ob.pos < out_chunk):
                    break
    finally:
        lib.ZSTD_freeCCtx(cctx)
    return bytes(res)


# ---- the emulator entry point -------------------------------------------------------------------------------------------------------
def build_emu_frame_flags():
    """A library of its own (helpers.build_emu compiles a fixed file list), as helpers_dict_levels.build_emu_dict_level"""
    emu = os.path.join(helpers.ROOT, "tests", "emu")
    csrc = os.path.join(helpers.ROOT, "kompressor_amd", "csrc")
    lib = os.path.join(emu, "libkxemu_frame_flags.so")
    srcs = [os.path.join(emu, f) for f in os.listdir(emu) if f.endswith((".cpp", ".h"))]
    srcs += [os.path.join(csrc, f) for f in os.listdir(csrc) if f.endswith(".h")]
    if helpers._newer(lib, srcs):
        subprocess.run(["g++", "-O1", "-std=c++17", "-shared", "-fPIC", "-I" + emu, "-I" + csrc, "-o", lib,
                        os.path.join(emu, "emu_core.cpp"), os.path.join(emu, "emu_zstd_frame_flags.cpp")], check=True)
    return lib


def emu_frame_flags():
    global _EMU
    if _EMU is None:
        _EMU = ctypes.CDLL(build_emu_frame_flags())
    return _EMU


def emu_compress(datas, level, flags, dictionary=None, G=4, nblocks=2, stream=0):
    """The XXH64 pass, the level's parse and the frame writers on the emulator, their arguments built by zstd_launch.h with the flags:
    slices up to 128 KiB through the one-block bodies, longer ones through the block chain's / zstd_lazy_big.h's."""
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
    dbuf = np.frombuffer(dictionary, dtype=np.uint8).copy() if dictionary else np.zeros(8, dtype=np.uint8)
    vp = helpers._vp
    r = emu_frame_flags().emu_zstd_compress_flags(vp(buf), vp(offs), vp(lens), n, G, nblocks, vp(out), vp(ooff), vp(olen), cap,
                                                  vp(dbuf), len(dictionary) if dictionary else 0, level, flags, stream)
    assert r == 0, f"emulated kernels failed: {r}"
    return [out[i * stride:i * stride + int(olen[i])].tobytes() for i in range(n)]
