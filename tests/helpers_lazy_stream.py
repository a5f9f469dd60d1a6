"""Helpers for the tests of zstd levels 5 .. 10 as streams and as the reference driver's staged frames, 0 .. 2 MiB
(kompressor_amd/csrc/zstd_lazy_big.h with a KFrameArgs.stream mode).  The oracle has no such mode at these levels: the yardstick is the
binary libzstd 1.5.7 -- tests/golden/zstd_lazy_stream_golden.json (make_golden_lazy_stream.py) and the live library where it is present."""
import ctypes
import json
import os
import random
import subprocess

import numpy as np

import helpers

LEVELS = (5, 6, 7, 8, 9, 10)
MODES = {"stream": 1, "stream_empty_end": 2, "staged": 3}      # KFrameArgs.stream
STREAM_SIZES = (0, 1, 6, 7, 5000, 16384, 131071, 131072, 131073, 200000, 262144, 262145, 400000, (1 << 20) + 1, 2 << 20)
STAGED_FROM = 131073
_EMU = None
_GOLDEN = None
_INPUTS = None


def inputs():
    """The golden file's inputs by name, in its order: one per stream size, classes of kompressor_amd.corpus in turn, and three whose
    statistics change inside a chunk and across chunks (the pre-splitter cuts there, and the staged frame leaves the one-shot one)."""
    global _INPUTS
    if _INPUTS is None:
        from kompressor_amd import corpus
        mk = lambda seed, n, mix: corpus.make(seed, 1, n, mix=ord(mix)).tobytes() if n else b""
        out = []
        for t, n in enumerate(STREAM_SIZES):               # (the two largest of a class the emulator parses quickly)
            out.append((f"{'TXSBDIZTXSBDDZD'[t]}{n}", mk(71000 + t, n, "TXSBDIZTXSBDDZD"[t])))
        # text, then binary records 70 000 bytes into the second chunk; three classes with changes at 100 000 and 300 000; text that turns
        # into a short period inside the fourth chunk
        out.append(("change_200000+200000", mk(71100, 200000, "T") + mk(71101, 200000, "B")))
        out.append(("change_100000+200000+300000", mk(71102, 100000, "X") + mk(71103, 200000, "T") + mk(71104, 300000, "S")))
        out.append(("change_450000+periodic", mk(71105, 450000, "T") + (mk(71106, 97, "T") * 3000)[:250000]))
        out.append(("change_100000+100000+100000", mk(71107, 100000, "D") + mk(71108, 100000, "T") + mk(71109, 100000, "I")))
        _INPUTS = out
    return _INPUTS


def cuts_for(name, n):
    """Where a stream is cut into pieces (the last one closes it): seeded by the input's name.  A piece of no bytes comes first where the
    stream has fewer than two: bytes must have arrived (or a call been made) before the closing one, or libzstd knows the size."""
    if n < 2:
        return [0, 0, n]
    rng = random.Random(name)
    return sorted({0, n} | {rng.randrange(1, n) for _ in range(3)})


def golden():
    global _GOLDEN
    if _GOLDEN is None:
        with open(os.path.join(helpers.ROOT, "tests", "golden", "zstd_lazy_stream_golden.json")) as f:
            _GOLDEN = json.load(f)
    return _GOLDEN


def live_frame(z, d, level, framing, name=""):
    """The live library's frame of d in one of the three framings."""
    n = len(d)
    if framing == "staged":
        return z.compress_streaming(d, [0, n], out_chunk=max(8192, n // 10), level=level)
    cuts = cuts_for(name or str(n), n)
    if framing == "stream_empty_end":
        cuts = cuts + [n]
    return z.compress_streaming(d, cuts, out_chunk=8192, level=level)


def build_emu_lazy_stream():
    """The emulator entry point with a mode argument, a library of its own (helpers.build_emu compiles a fixed file list)."""
    emu = os.path.join(helpers.ROOT, "tests", "emu")
    csrc = os.path.join(helpers.ROOT, "kompressor_amd", "csrc")
    lib = os.path.join(emu, "libkxemu_lazy_stream.so")
    srcs = [os.path.join(emu, f) for f in os.listdir(emu) if f.endswith((".cpp", ".h"))]
    srcs += [os.path.join(csrc, f) for f in os.listdir(csrc) if f.endswith(".h")]
    if helpers._newer(lib, srcs):
        subprocess.run(["g++", "-O1", "-std=c++17", "-shared", "-fPIC", "-I" + emu, "-I" + csrc, "-o", lib,
                        os.path.join(emu, "emu_core.cpp"), os.path.join(emu, "emu_zstd_lazy_stream.cpp")], check=True)
    return lib


def emu_lazy_stream():
    global _EMU
    if _EMU is None:
        _EMU = ctypes.CDLL(build_emu_lazy_stream())
    return _EMU


def emu_compress(datas, level, framing, slice_cap=None, piece=0, nblocks=2, out_chunk=0):
    """A batch at level 5 .. 10 in one of the framings of MODES as a context for slices of up to slice_cap bytes runs it, on the emulator,
    `piece` table slots (0: one per slice).  -> (frames, status bits, bytes of a table slot); a refused slice comes back as b''."""
    n = len(datas)
    cap = max(max((len(d) for d in datas), default=1), (128 << 10) + 1)
    slice_cap = slice_cap or cap
    lens = np.array([len(d) for d in datas], dtype=np.uint32)
    offs = np.zeros(n, dtype=np.uint64)
    pos = 3                                         # (input offsets that are no multiple of 4)
    for i, d in enumerate(datas):
        offs[i] = pos
        pos += len(d) + 1
    buf = np.zeros(pos + 64, dtype=np.uint8)
    for i, d in enumerate(datas):
        buf[int(offs[i]):int(offs[i]) + len(d)] = np.frombuffer(d, dtype=np.uint8)
    ostride = (helpers.compress_bound(cap) + 16 + 63) & ~63
    out = np.zeros(n * ostride + 64, dtype=np.uint8); ooff = np.arange(n, dtype=np.uint64) * ostride; olen = np.zeros(n, dtype=np.uint32)
    status = ctypes.c_uint32(0); slot = ctypes.c_uint64(0)
    vp = helpers._vp
    r = emu_lazy_stream().emu_zstd_compress_lazy_stream(vp(buf), vp(offs), vp(lens), n, nblocks, vp(out), vp(ooff), vp(olen), slice_cap, level,
                                                        MODES[framing], out_chunk, piece, ctypes.byref(status), ctypes.byref(slot))
    assert r == 0, f"emulated kernels of levels 5 .. 10 ({framing}) failed: {r}"
    return [out[int(ooff[i]):int(ooff[i]) + int(olen[i])].tobytes() for i in range(n)], status.value, slot.value
