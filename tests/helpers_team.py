"""Helpers for the tests of the parsers' shared team pieces (kompressor_amd/csrc/zstd_team.h): the emulator library of
tests/emu/emu_team.cpp, and the "ladder" -- a batch of small slices whose sequence counts step through the sizes at which the sequence
sink changes what it does (nothing to store, one entry, a line short of one, a full line, one more).  Expected frames are the binary
libzstd 1.5.7's: tests/golden/zstd_team_ladder_golden.json (make_golden_team_ladder.py)."""
import ctypes
import json
import os
import random
import subprocess

import numpy as np

import helpers

META = np.dtype([("nbSeq", "<u4"), ("litSize", "<u4"), ("lastLL", "<u4"), ("longType", "<u4"), ("longPos", "<u4"), ("status", "<u4"),
                 ("pad", "<u4", (2,))])          # KSliceMeta (zstd_common.h)
assert META.itemsize == 32
SEQ = np.dtype([("offBase", "<u4"), ("litLength", "<u2"), ("mlBase", "<u2")])                  # KSeq
TEAMS = (4, 8)
MAX_REPEATS = 3 * max(TEAMS) + 2
DICT_BYTES = 16384
# (name, level, with the dictionary)
CONFIGS = (("l3", 3, False), ("l1", 1, False), ("dict_l3", 3, True), ("dict_l1", 1, True))
_EMU = None
_LADDER = None
_GOLDEN = None


def ladder():
    """-> (dictionary, [slice bytes]): seeded noise with r planted repeats, r = 0 .. 3 G + 2 for the widest team: 96 bytes of noise, then r
    times 40 bytes of fresh noise and a copy of 32 bytes from those first 96 (non-adjacent: every repeat is one sequence).  Each r
    twice: as it is, and behind 24 bytes of the dictionary, which a parse with the dictionary finds (one sequence more) and one
    without does not.  At most 4 KiB each."""
    global _LADDER
    if _LADDER is None:
        rng = random.Random(20261)
        d = rng.randbytes(DICT_BYTES)
        out = []
        for with_chunk in (False, True):
            for r in range(MAX_REPEATS + 1):
                head = rng.randbytes(96)
                s = bytearray(d[5000 + 64 * r:5024 + 64 * r] if with_chunk else b"") + head
                for _ in range(r):
                    a = rng.randrange(0, 64)
                    s += rng.randbytes(40) + head[a:a + 32]
                s += rng.randbytes(16)
                assert len(s) <= 4096
                out.append(bytes(s))
        _LADDER = (d, out)
    return _LADDER


def wanted_counts(G):
    return {0, 1, 2 * G - 1, 2 * G, 2 * G + 1}


def golden():
    """{config name: [[frame length, sha256], ...]} in the ladder's order"""
    global _GOLDEN
    if _GOLDEN is None:
        with open(os.path.join(helpers.ROOT, "tests", "golden", "zstd_team_ladder_golden.json")) as f:
            g = json.load(f)
        assert g["libzstd"] == 10507
        d, slices = ladder()
        assert g["dict_sha256"] == helpers.sha256(d) and g["slices_sha256"] == [helpers.sha256(s) for s in slices]
        _GOLDEN = g["frames"]
    return _GOLDEN


def check_frames(name, frames):
    want = golden()[name]
    bad = [(i, len(f), w[0]) for i, (f, w) in enumerate(zip(frames, want)) if [len(f), helpers.sha256(f)] != w]
    assert len(frames) == len(want) and not bad, f"{name}: (slice, frame, libzstd's frame) {bad}"


def build_emu_team():
    """tests/emu/emu_team.cpp, a library of its own (helpers.build_emu compiles a fixed file list)."""
    emu = os.path.join(helpers.ROOT, "tests", "emu")
    csrc = os.path.join(helpers.ROOT, "kompressor_amd", "csrc")
    lib = os.path.join(emu, "libkxemu_team.so")
    srcs = [os.path.join(emu, f) for f in ("emu_core.cpp", "emu_core.h", "kx_wave.h", "emu_team.cpp")]
    srcs += [os.path.join(csrc, f) for f in os.listdir(csrc) if f.endswith(".h")]
    if helpers._newer(lib, srcs):
        subprocess.run(["g++", "-O1", "-std=c++17", "-shared", "-fPIC", "-I" + emu, "-I" + csrc, "-o", lib,
                        os.path.join(emu, "emu_core.cpp"), os.path.join(emu, "emu_team.cpp")], check=True)
    return lib


def emu():
    global _EMU
    if _EMU is None:
        _EMU = ctypes.CDLL(build_emu_team())
    return _EMU


def emu_sink(G, triples, guard=0xA5A5A5A5):
    """KSeqSink over the (offBase, ll, mlBase) triples, one emulated wave of 64 / G teams, every team into a region of its own ->
    ([a team's seqs region: N entries and at least 2 G + 8 guard entries behind them], the record of meta(77, 5))"""
    n = len(triples)
    per = (n + 2 * G + 8 + 1) & ~1
    teams = 64 // G
    raw = np.full(teams * per * 2 + 4, guard, dtype=np.uint32)
    seqs = raw[(-raw.ctypes.data // 4) % 4:][:teams * per * 2]           # 16-byte aligned
    assert seqs.ctypes.data % 16 == 0
    tin = np.array(triples, dtype=np.uint32).reshape(-1)
    meta = np.zeros(1, dtype=META)
    vp = helpers._vp
    r = emu().emu_team_sink(G, vp(seqs), vp(tin) if n else None, n, vp(meta))
    assert r == 0, f"emulated sink failed: {r}"
    return [seqs[t * per * 2:(t + 1) * per * 2].view(SEQ) for t in range(teams)], meta[0]


def emu_parse_meta(datas, G, level, dictionary=None, nblocks=2):
    """The parse body alone on the emulator -> the slices' records (META array)"""
    n = len(datas)
    lens = np.array([len(d) for d in datas], dtype=np.uint32)
    offs = np.zeros(n, dtype=np.uint64)
    pos = 3
    for i, d in enumerate(datas):
        offs[i] = pos
        pos += len(d) + 1
    buf = np.zeros(pos + 64, dtype=np.uint8)
    for i, d in enumerate(datas):
        buf[int(offs[i]):int(offs[i]) + len(d)] = np.frombuffer(d, dtype=np.uint8)
    meta = np.zeros(n, dtype=META)
    dbuf = np.frombuffer(dictionary, dtype=np.uint8).copy() if dictionary else None
    vp = helpers._vp
    r = emu().emu_team_parse_meta(vp(buf), vp(offs), vp(lens), n, G, nblocks, max(int(lens.max()), 64),
                                  vp(dbuf) if dictionary else None, len(dictionary) if dictionary else 0, level, vp(meta))
    assert r == 0, f"emulated parser failed: {r}"
    assert not meta["status"].any(), meta["status"]
    return meta
