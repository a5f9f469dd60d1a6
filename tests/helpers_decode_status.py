"""Helpers for the decode status snapshot (tests/golden/decode_status_golden.json, made by tests/golden/make_golden_decode_status.py):
which status, length and bytes every damaged entry gets from k_zstd_decode alone and with the two pre-decoders, which sort key and
which kx_frame_info answer -- what a change to the framing readers (kompressor_amd/csrc/zstd_format.h) can alter without any
accept / reject test noticing.  The cases are rebuilt from seeds (the fixture stores their sha256, not their bytes): seeded mutants of
the C restatement's frames and of the foreign frames, then the framing edges.

Run as a program it places every framing edge against a PROT_NONE page (fuzz_decoders.Guarded, slack 0) and sends it through the
decoder alone, the decoder with the pre-decoders, the sort key and kx_frame_info: a read behind the entry kills the process.

    python tests/helpers_decode_status.py          # prints "EDGES OK <n>" and exits 0
"""
import ctypes
import json
import os
import random
import sys
import zlib

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import helpers                    # noqa: E402
import helpers_frame_info as hf   # noqa: E402
import fuzz_decoders              # noqa: E402

SEED = 20261
N_MUTANTS = 1200
LIT_CAP = 128 * 1024 + 64
GOLDEN = os.path.join(helpers.ROOT, "tests", "golden", "decode_status_golden.json")
MAGIC = bytes.fromhex("28b52ffd")
HEAD = MAGIC + b"\x20\x00"        # a single-segment frame that declares 0 bytes: the 6-byte header in front of the block edges
DECODE_FIELDS = ("status", "out_len", "crc")


def _block(body, btype=2, last=1):
    return ((len(body) << 3) | (btype << 1) | last).to_bytes(3, "little") + body


def edges():
    """[(name, entry)]: framing cut short in every way the readers distinguish.  Every one is rejected by the decoder;
    kx_frame_info rejects those whose name starts with "header" or "block header" (the others are whole at the level it walks)."""
    out = [("raw literals, 3-byte size, block of 2", HEAD + _block(b"\x0c\x00")),
           ("RLE literals, 3-byte size, block of 2", HEAD + _block(b"\x0d\x00"))]
    for size in (2, 3, 4):
        for ltype in (2, 3):
            for sf in range(4):
                out.append((f"literals type {ltype} format {sf}, block of {size}", HEAD + _block(bytes([ltype | (sf << 2)]) + bytes(size - 1))))
    for cut in (1, 2):
        out.append((f"block header cut after {cut}", HEAD + _block(b"\x00\x00")[:cut]))
    for fhd in range(256):
        if fhd & 0x14:                                          # (the checksum bit and the unused bit change no length)
            continue
        single, did, fcs = (fhd >> 5) & 1, (0, 1, 2, 4)[fhd & 3], (1 << (fhd >> 6)) if fhd >> 6 else (fhd >> 5) & 1
        size = 5 + (1 - single) + did + fcs
        full = MAGIC + bytes([fhd]) + bytes(size - 5)
        for n in range(5, size):
            out.append((f"header {fhd:#04x} cut at {n} of {size}", full[:n]))
    # the sequence count's three forms (a raw literals section of no bytes in front), cut at each byte; then no count at all
    for name, count in (("1-byte", b"\x05"), ("2-byte", b"\x80\x05"), ("3-byte", b"\xff\x01\x00")):
        for n in range(1, len(count) + 1):
            out.append((f"{name} sequence count cut after {n} (no modes byte)" if n == len(count) else f"{name} sequence count cut after {n}",
                        HEAD + _block(b"\x00" + count[:n])))
    out.append(("no sequence count", HEAD + _block(b"\x08\xaa")))
    return out


def base_frames():
    """[(frame, content length)]: the C restatement's level-3 frames of the fuzzer's sources and the foreign frames, content <= 64 KiB"""
    rng = random.Random(SEED)
    o = helpers.oracle()
    out = [(o.compress(d), len(d)) for d in fuzz_decoders.sources(rng, 24) if len(d) <= 65536]
    out += [(f, len(plain)) for _, f, plain in helpers.foreign_frames() if len(plain) <= 65536]
    return out


def cases():
    """[(name, entry, capacity)]: N_MUTANTS seeded mutants (every 32nd intact), then the framing edges"""
    base = base_frames()
    only = [f for f, _ in base]
    rng = random.Random(SEED + 1)
    out = []
    for i in range(N_MUTANTS):
        k = rng.randrange(len(base))
        f0, n = base[k]
        f, what = (f0, "intact") if i % 32 == 0 else fuzz_decoders.mutate(rng, f0, only)
        cap = n + rng.choice((0, 0, 0, 1, 64, 5000)) if rng.random() < 0.85 else rng.randrange(0, n + 1)
        out.append((f"case {i}: base {k} {what}", f, cap))
    return out + [(name, e, 64) for name, e in edges()]


# ---------------------------------------------------------------- the emulator ----
def _decode_fn():
    fn = helpers.emu().emu_zstd_decompress
    fn.argtypes = [ctypes.c_void_p] * 3 + [ctypes.c_uint32, ctypes.c_uint32] + [ctypes.c_void_p] * 5 + [ctypes.c_uint32]
    return fn


def _no_pre(on):
    if on:
        os.environ["KXEMU_NO_PRE"] = "1"
    else:
        os.environ.pop("KXEMU_NO_PRE", None)


def emu_decode(src_base, in_off, in_len, caps, pre):
    """k_zstd_decode's body over the entries at src_base + in_off, alone (pre=False) or behind the sort and the two pre-decoders
    -> [(status, out_len, crc32 of the output)]"""
    n = len(in_len)
    fn = _decode_fn()
    caps = np.asarray(caps, dtype=np.uint32)
    ooff = (np.cumsum(caps.astype(np.uint64) + 16) - (caps.astype(np.uint64) + 16)).astype(np.uint64)
    out = np.zeros(int(caps.astype(np.uint64).sum()) + 16 * n + 64, dtype=np.uint8)
    res = []
    _no_pre(not pre)
    try:
        for b in range(0, n, 64):                              # (a chunk at a time: the emulator's staging is per entry and large)
            e = min(n, b + 64)
            olen = np.zeros(e - b, dtype=np.uint32); st = np.zeros(e - b, dtype=np.uint32)
            io = np.ascontiguousarray(in_off[b:e], dtype=np.uint64); il = np.ascontiguousarray(in_len[b:e], dtype=np.uint32)
            oo = np.ascontiguousarray(ooff[b:e]); oc = np.ascontiguousarray(caps[b:e])
            base = src_base if isinstance(src_base, int) else helpers._vp(src_base)
            r = fn(base, helpers._vp(io), helpers._vp(il), e - b, 2, helpers._vp(out), helpers._vp(oo), helpers._vp(oc), helpers._vp(olen), helpers._vp(st), LIT_CAP)
            assert r == 0, f"emulator reported {r}"
            for i in range(e - b):
                o = int(oo[i])
                res.append((int(st[i]), int(olen[i]), zlib.crc32(out[o:o + int(olen[i])].tobytes())))
    finally:
        _no_pre(False)
    return res


def emu_sort_keys(src_base, in_off, in_len):
    n = len(in_len)
    io = np.ascontiguousarray(in_off, dtype=np.uint64); il = np.ascontiguousarray(in_len, dtype=np.uint32)
    key = np.zeros(n, dtype=np.uint32); perm = np.zeros(n, dtype=np.uint32)
    base = src_base if isinstance(src_base, int) else helpers._vp(src_base)
    fn = helpers.emu().emu_seq_sort
    fn.argtypes = [ctypes.c_void_p] * 3 + [ctypes.c_uint32] + [ctypes.c_void_p] * 2
    r = fn(base, helpers._vp(io), helpers._vp(il), n, helpers._vp(key), helpers._vp(perm))
    assert r == 0, f"emulator reported {r}"
    assert sorted(int(x) for x in perm) == list(range(n)), "the slot order is no permutation"
    return [int(k) for k in key]


def emu_rows(cs):
    """What the emulator answers for the cases, in the fixture's form: every entry with 16 zero bytes behind it"""
    lens = np.array([len(e) for _, e, _ in cs], dtype=np.uint32)
    offs = (np.cumsum(lens.astype(np.uint64) + 16) - (lens.astype(np.uint64) + 16)).astype(np.uint64)
    src = np.zeros(int(offs[-1]) + int(lens[-1]) + 16, dtype=np.uint8)
    for (_, e, _), o in zip(cs, offs):
        src[int(o):int(o) + len(e)] = np.frombuffer(e, dtype=np.uint8)
    caps = [c for _, _, c in cs]
    alone = emu_decode(src, offs, lens, caps, pre=False)
    ahead = emu_decode(src, offs, lens, caps, pre=True)
    keys = emu_sort_keys(src, offs, lens)
    info = hf.emu_frame_info(src, offs, lens)
    rows = []
    for i, (name, e, cap) in enumerate(cs):
        rows.append({"name": name, "sha256": helpers.sha256(e), "len": len(e), "cap": cap,
                     "alone": list(alone[i]), "pre": list(ahead[i]), "key": keys[i], "info": [int(info[i][f]) for f in hf.FIELDS]})
    return rows


def write_golden(commit, rows):
    """The fixture, column by column (a line each): per case the head of the entry's sha256 (one sha256 over all of them in full),
    the capacity, the two decode statuses, the sort key and the six frame info fields; out_len and crc32 only where they are not 0"""
    def outputs(col):
        return {str(i): r[col][1:] for i, r in enumerate(rows) if r[col][1] or r[col][2]}
    doc = {"commit": commit, "seed": SEED, "lit_cap": LIT_CAP, "cases": len(rows),
           "sha256_of_all": helpers.sha256("".join(r["sha256"] for r in rows).encode()),
           "sha256_head": [r["sha256"][:8] for r in rows], "cap": [r["cap"] for r in rows], "key": [r["key"] for r in rows],
           "alone_status": [r["alone"][0] for r in rows], "alone_out_len_crc": outputs("alone"),
           "pre_status": [r["pre"][0] for r in rows], "pre_out_len_crc": outputs("pre")}
    for k, f in enumerate(hf.FIELDS):
        doc["info_" + f] = [r["info"][k] for r in rows]
    with open(GOLDEN, "w") as f:
        f.write("{\n" + ",\n".join(f' "{k}": {json.dumps(v, separators=(",", ":"))}' for k, v in doc.items()) + "\n}\n")


def golden():
    """-> {"commit", "lit_cap", "sha256_of_all", "rows": [{"sha256_head", "cap", "alone", "pre", "key", "info"}]}"""
    with open(GOLDEN) as f:
        d = json.load(f)
    rows = []
    for i in range(d["cases"]):
        r = {"sha256_head": d["sha256_head"][i], "cap": d["cap"][i], "key": d["key"][i], "info": [d["info_" + f][i] for f in hf.FIELDS]}
        for col in ("alone", "pre"):
            r[col] = [d[col + "_status"][i]] + d[col + "_out_len_crc"].get(str(i), [0, 0])
        rows.append(r)
    return {"commit": d["commit"], "lit_cap": d["lit_cap"], "sha256_of_all": d["sha256_of_all"], "rows": rows}


def checked_cases(g):
    """cases(), after checking that the generator still makes the fixture's entries; the rows get the cases' names"""
    cs = cases()
    assert len(cs) == len(g["rows"]), (len(cs), len(g["rows"]))
    shas = [helpers.sha256(e) for _, e, _ in cs]
    for (name, e, cap), sha, r in zip(cs, shas, g["rows"]):
        assert sha[:8] == r["sha256_head"] and cap == r["cap"], f"the generator no longer makes the fixture's entry: {name}"
        r["name"] = name
    assert helpers.sha256("".join(shas).encode()) == g["sha256_of_all"], "the generator no longer makes the fixture's entries"
    return cs


# ---------------------------------------------------------------- the edges at a guard page ----
def main():
    n = 0
    for name, e in edges():
        g = fuzz_decoders.Guarded(len(e), 0)
        g.write(e)
        off = np.array([g.off], dtype=np.uint64); ln = np.array([len(e)], dtype=np.uint32)
        print(name, flush=True)
        for pre in (False, True):
            st, olen, _ = emu_decode(g.base, off, ln, [64], pre)[0]
            assert st != 0 and olen == 0, f"{name}: status {st}, out_len {olen} ({'with' if pre else 'without'} the pre-decoders)"
        emu_sort_keys(g.base, off, ln)
        info = hf.emu_frame_info(g.base, off, ln)
        if name.startswith(("header", "block header")):
            assert int(info[0]["status"]) != 0, f"{name}: kx_frame_info accepts it"
        g.close()
        n += 1
    print(f"EDGES OK {n}")
    return 0


if __name__ == "__main__":
    sys.exit(main())
