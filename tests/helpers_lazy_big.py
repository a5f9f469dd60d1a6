"""Helpers for the tests of zstd levels 5 .. 10 above 128 KiB (frames of several blocks; kompressor_amd/csrc/zstd_lazy_big.h).

A correction to tests/helpers.py: the docstring of Oracle.compress_lazy_big says "No product path yet".  There is one now --
kmp_zstd_compress_batch_level at levels 5 .. 10 on a context created for slices above 128 KiB serves 128 KiB + 1 .. 2 MiB -- and that oracle
is its yardstick (test_emu_lazy_big.py, test_gpu_lazy_big.py)."""
import ctypes
import os
import subprocess

import numpy as np

import helpers

_EMU = None


def build_emu_lazy_big():
    """The emulator entry point of the new kernel bodies, a library of its own (helpers.build_emu compiles a fixed file list)."""
    emu = os.path.join(helpers.ROOT, "tests", "emu")
    csrc = os.path.join(helpers.ROOT, "kompressor_amd", "csrc")
    lib = os.path.join(emu, "libkxemu_lazy_big.so")
    srcs = [os.path.join(emu, f) for f in os.listdir(emu) if f.endswith((".cpp", ".h"))]
    srcs += [os.path.join(csrc, f) for f in os.listdir(csrc) if f.endswith(".h")]
    if helpers._newer(lib, srcs):
        subprocess.run(["g++", "-O1", "-std=c++17", "-shared", "-fPIC", "-I" + emu, "-I" + csrc, "-o", lib,
                        os.path.join(emu, "emu_core.cpp"), os.path.join(emu, "emu_zstd_lazy_big.cpp")], check=True)
    return lib


def emu_lazy_big():
    global _EMU
    if _EMU is None:
        _EMU = ctypes.CDLL(build_emu_lazy_big())
    return _EMU


def emu_compress_lazy_big(datas, level, slice_cap=None, piece=0, nblocks=2):
    """A batch at level 5 .. 10 as a context for slices of up to slice_cap bytes (default: the largest slice, at least 128 KiB + 1) runs
    it, on the emulator: the one-block kernels for the slices up to 128 KiB, k_zstd_lazy_big's body for the others, `piece` table slots
    (0: one per slice).  -> (frames, status bits); a refused slice comes back as b''."""
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
    ostride = (helpers.compress_bound(cap) + 8 + 63) & ~63
    out = np.zeros(n * ostride + 64, dtype=np.uint8); ooff = np.arange(n, dtype=np.uint64) * ostride; olen = np.zeros(n, dtype=np.uint32)
    status = ctypes.c_uint32(0)
    vp = helpers._vp
    r = emu_lazy_big().emu_zstd_compress_lazy_big(vp(buf), vp(offs), vp(lens), n, nblocks, vp(out), vp(ooff), vp(olen), slice_cap, level, piece,
                                                  ctypes.byref(status))
    assert r == 0, f"emulated kernels of levels 5 .. 10 above 128 KiB failed: {r}"
    return [out[int(ooff[i]):int(ooff[i]) + int(olen[i])].tobytes() for i in range(n)], status.value


def oracle_frame(d, level):
    """The oracle's frame of a slice at levels 5 .. 10 on such a context: one block up to 128 KiB, several up to 2 MiB; None = refused."""
    o = helpers.oracle()
    if len(d) == 0:
        import layouts
        return layouts.empty_frame()                # (the oracle has no row for it: a header and an empty raw block, at every level)
    if len(d) <= (128 << 10):
        return o.compress_lazy(d, level)
    if len(d) > (2 << 20):
        return None
    r = o.compress_lazy_big(d, level)
    return None if r is None else r[0]


class OddLayout:
    """A hostile layout for a handful of large entries (numpy only): slices and slots in a seeded permutation of the entry order, every
    slice start at 1, 2 or 3 modulo 4, output slots of exactly kmp_zstd_compress_bound(len) + 8 with 1 .. 63 canary bytes behind each,
    the buffers full of seeded bytes.  check() compares every destination byte outside the slots with the canary."""

    def __init__(self, datas, seed):
        rng = np.random.default_rng(seed)
        n = len(datas)
        self.datas = datas
        self.in_len = np.array([len(d) for d in datas], dtype=np.int32)
        self.in_off = np.zeros(n, dtype=np.int64); self.out_off = np.zeros(n, dtype=np.int64)
        self.slot = np.array([helpers.compress_bound(len(d)) + 8 for d in datas], dtype=np.int64)
        pos = 4096
        for i in rng.permutation(n):
            pos += int(rng.integers(1, 64))
            pos += (1 + int(rng.integers(0, 3)) - pos) % 4                 # 1, 2 or 3 modulo 4
            self.in_off[i] = pos
            pos += len(datas[i])
        self.src = rng.integers(0, 256, pos + 4096, dtype=np.uint8)
        for i, d in enumerate(datas):
            self.src[int(self.in_off[i]):int(self.in_off[i]) + len(d)] = np.frombuffer(d, dtype=np.uint8)
        pos = 4096
        for i in rng.permutation(n):
            pos += int(rng.integers(1, 64))
            self.out_off[i] = pos
            pos += int(self.slot[i])
        self.canary = rng.integers(0, 256, pos + 4096, dtype=np.uint8)
        assert all(int(o) % 4 != 0 for o in self.in_off)

    def frames(self, dst, out_len):
        return [dst[int(o):int(o) + int(l)].tobytes() for o, l in zip(self.out_off, out_len)]

    def check(self, dst, out_len):
        """-> findings (empty: every out_len fits its slot, no byte outside the slots changed)"""
        bad = [f"entry {i}: out_len {int(l)} above its slot of {int(s)}" for i, (l, s) in enumerate(zip(out_len, self.slot)) if int(l) > int(s)]
        keep = np.ones(len(self.canary), dtype=bool)
        for o, s in zip(self.out_off, self.slot):
            keep[int(o):int(o) + int(s)] = False
        hit = np.flatnonzero((np.asarray(dst) != self.canary) & keep)
        if hit.size:
            bad.append(f"{hit.size} bytes outside the slots changed, first at {int(hit[0])}")
        return bad
