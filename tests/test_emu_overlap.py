"""The entropy sweeps beside the level-3 parse (kmp_batch.hip zstd_compress_dfast) on the CPU wave emulator
(tests/emu/emu_overlap.cpp): the parse's completion records -- the host's stream waits rely on the count reaching n in every
batch -- and the sweeps' result, which must not depend on which slices were finished when a sweep ran."""
import ctypes
import os
import random
import subprocess

import numpy as np
import pytest

import helpers
from kompressor_amd import corpus

LENGTHS = (0, 1, 7, 8, 9, 4096, 65536)
_EMU = None


def emu():
    global _EMU
    if _EMU is None:
        d = os.path.join(helpers.ROOT, "tests", "emu")
        csrc = os.path.join(helpers.ROOT, "kompressor_amd", "csrc")
        lib = os.path.join(d, "libkxemu_overlap.so")
        srcs = [os.path.join(d, f) for f in ("emu_core.cpp", "emu_core.h", "kx_wave.h", "emu_overlap.cpp")]
        srcs += [os.path.join(csrc, f) for f in os.listdir(csrc) if f.endswith(".h")]
        if helpers._newer(lib, srcs):
            subprocess.run(["g++", "-O1", "-std=c++17", "-shared", "-fPIC", "-I" + d, "-I" + csrc, "-o", lib,
                            os.path.join(d, "emu_core.cpp"), os.path.join(d, "emu_overlap.cpp")], check=True)
        _EMU = ctypes.CDLL(lib)
        _EMU.emu_overlap_thresholds.restype = ctypes.c_uint32
    return _EMU


@pytest.fixture(scope="module")
def batch():
    """[(name, bytes, golden row or None)]: every length of LENGTHS as zeros, noise and text, in a shuffled order.  The golden rows
    are the existing ones that cover such a slice (tests/golden/zstd_l3_golden.json: empty, one byte, 64 KiB of zeros, a 64 KiB
    text slice of the bench's corpus)."""
    G = helpers.golden()
    special = {r["name"]: (r["len"], r["sha256"]) for r in G["special"]}
    row = next(r for r in G["config1"] if r[1] == "T")
    text = corpus.make(row[0], 1, 65536).tobytes()
    noise = random.Random(4242).randbytes(65536)
    out = []
    for n in LENGTHS:
        out.append((f"zeros_{n}", bytes(n), special.get({0: "empty", 65536: "zeros_64k"}.get(n))))
        out.append((f"noise_{n}", noise[:n], None))
        out.append((f"text_{n}", text[:n], (row[2], row[3]) if n == 65536 else None))
    out.append(("one_byte", b"a", special["one_byte"]))
    random.Random(7).shuffle(out)
    return out


def run(datas, order=None, cuts=(), level4=False, frames=True, nblocks=2):
    """-> (done, done_count, status, frames or None, slices coded per sweep)"""
    n = len(datas)
    lens = np.array([len(d) for d in datas], dtype=np.uint32)
    offs = np.zeros(n, dtype=np.uint64)
    pos = 0
    for i, d in enumerate(datas):
        offs[i] = pos
        pos += len(d)
    buf = np.zeros(pos + 64, dtype=np.uint8)
    for i, d in enumerate(datas):
        buf[int(offs[i]):int(offs[i]) + len(d)] = np.frombuffer(d, dtype=np.uint8)
    cap = max(int(lens.max()), 64)
    stride = (helpers.compress_bound(cap) + 64 + 15) & ~15
    out = np.zeros(n * stride, dtype=np.uint8)
    ooff = np.arange(n, dtype=np.uint64) * stride
    olen = np.zeros(n, dtype=np.uint32)
    done = np.full(n, 0xEEEEEEEE, dtype=np.uint32)
    count = np.full(1, 0xEEEEEEEE, dtype=np.uint32)
    status = np.zeros(n, dtype=np.uint32)
    order = np.array(order if order is not None else range(n), dtype=np.uint32)
    cuts = np.array(list(cuts) + [0], dtype=np.uint32)
    swept = np.zeros(len(cuts), dtype=np.uint32)
    vp = helpers._vp
    r = emu().emu_overlap_compress(vp(buf), vp(offs), vp(lens), n, nblocks, cap, 1 if level4 else 0, vp(done), vp(count), vp(status),
                                   vp(out) if frames else None, vp(ooff), vp(olen), vp(order), vp(cuts), len(cuts) - 1, vp(swept))
    assert r == 0, f"emulator reported {r}"
    fr = [out[i * stride:i * stride + int(olen[i])].tobytes() for i in range(n)] if frames else None
    return done, int(count[0]), status, fr, [int(x) for x in swept]


@pytest.fixture(scope="module")
def plain(batch):
    """the frames of the plain path (one parse launch, one entropy launch)"""
    return helpers.emu_compress([d for _, d, _ in batch], G=4)


def test_plain_path_matches_the_goldens(batch, plain):
    o = helpers.oracle()
    seen = 0
    for (name, d, want), f in zip(batch, plain):
        if want is not None:
            assert (len(f), helpers.sha256(f)) == tuple(want), name
            seen += 1
        assert f == o.compress(d), name
    assert seen == 4


def test_every_slice_is_recorded_once(batch):
    datas = [d for _, d, _ in batch]
    done, count, status, _, _ = run(datas, frames=False, nblocks=1)       # one wave: its sixteen teams claim slices again and again
    assert done.tolist() == [1] * len(datas) and count == len(datas)
    assert not status.any()


def test_refused_slices_are_recorded_too(batch):
    # level 4's double-fast row serves slices above 16 KiB only: the others leave the parse with status 3, straight from the claim
    datas = [d for _, d, _ in batch]
    done, count, status, _, _ = run(datas, level4=True, frames=False)
    assert done.tolist() == [1] * len(datas) and count == len(datas)
    assert [int(s) for s in status] == [3 if len(d) <= 16384 else 0 for d in datas]


@pytest.mark.parametrize("seed", [1, 2, 3])
def test_sweeps_in_any_order_give_the_plain_frames(batch, plain, seed):
    datas = [d for _, d, _ in batch]
    n = len(datas)
    order = list(range(n))
    random.Random(seed).shuffle(order)
    cuts = sorted(random.Random(100 + seed).sample(range(1, n), 3))
    done, count, _, frames, swept = run(datas, order=order, cuts=cuts)
    assert count == n and done.tolist() == [1] * n
    assert swept == [cuts[0], cuts[1] - cuts[0], cuts[2] - cuts[1], n - cuts[2]]        # every slice coded by exactly one sweep
    assert frames == plain


def test_thresholds():
    T = (ctypes.c_uint32 * 16)()
    for n in (1, 2, 3, 63, 64, 65, 257, 16384, 65536):
        for K in (0, 1, 2, 3, 4, 8, 16, 17, 1000):
            k = emu().emu_overlap_thresholds(n, K, T)
            got = [int(T[i]) for i in range(k)]
            want = sorted({j * n // min(K, 16) for j in range(1, min(K, 16))} - {0})
            assert got == want and all(0 < t <= n for t in got), (n, K, got)
