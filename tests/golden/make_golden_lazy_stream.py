#!/usr/bin/env python3
"""Generates tests/golden/zstd_lazy_stream_golden.json with a binary libzstd 1.5.7: length + sha256 of the frames it writes at levels
5 .. 10 for the seeded inputs of tests/helpers_lazy_stream.py inputs() in three framings --

  stream            fed in pieces with ZSTD_e_continue (finish = false: SliceTransformRawSource.kt:32-55), the closing call brings the last;
  stream_empty_end  the same pieces, closed by a call without data;
  staged            one ZSTD_e_end call over [0, n] with output slices of max(8192, n // 10) bytes (SliceTransform.kt:33-56), 128 KiB + 1 up

-- and the parameter row of a stream (size unknown): ZSTD_getCParams(level, 0, 0), whose window every streaming frame's header must name.
Run where that library is present:

    python tests/golden/make_golden_lazy_stream.py
"""
import ctypes, json, os, sys
HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "..")); sys.path.insert(0, os.path.join(HERE, "..", "..")); sys.path.insert(0, os.path.join(HERE, "..", "..", "oracle"))
import helpers
import helpers_lazy_stream as hs
from libzstd_ref import LibZstd, find_libzstd_157


class CP(ctypes.Structure):
    _fields_ = [(n, ctypes.c_uint) for n in ("windowLog", "chainLog", "hashLog", "searchLog", "minMatch", "targetLength", "strategy")]


def main():
    lib = find_libzstd_157(); z = LibZstd()
    lib.ZSTD_getCParams.restype = CP; lib.ZSTD_getCParams.argtypes = [ctypes.c_int, ctypes.c_ulonglong, ctypes.c_size_t]
    params = {}
    for lvl in hs.LEVELS:
        c = lib.ZSTD_getCParams(lvl, 0, 0)
        params[str(lvl)] = [c.windowLog, c.chainLog, c.hashLog, c.searchLog, c.minMatch, c.strategy]
    inputs = hs.inputs()
    assert [len(d) for _, d in inputs[:len(hs.STREAM_SIZES)]] == list(hs.STREAM_SIZES)
    frames = {}
    for lvl in hs.LEVELS:
        rows = {}; differ = 0
        for name, d in inputs:
            row = {}
            for framing in hs.MODES:
                if framing == "staged" and len(d) < hs.STAGED_FROM:
                    continue
                f = hs.live_frame(z, d, lvl, framing, name)
                assert z.decompress(f, len(d)) == d
                row[framing] = [len(f), helpers.sha256(f)]
                if framing == "staged":
                    differ += f != z.compress(d, lvl)
                elif len(d):
                    assert f[:6] == bytes([0x28, 0xB5, 0x2F, 0xFD, 0x00, (params[str(lvl)][0] - 10) << 3]), (lvl, name, f[:6].hex())
            if len(d) in (131072, 2 << 20):
                assert row["stream"][0] + 3 == row["stream_empty_end"][0], (lvl, name)
            rows[name] = row
        assert differ >= 3, f"level {lvl}: only {differ} staged frames differ from ZSTD_compress2's"
        frames[str(lvl)] = rows
        print("level", lvl, "staged frames that differ from ZSTD_compress2's:", differ)
    path = os.path.join(HERE, "zstd_lazy_stream_golden.json")
    doc = {"libzstd": "1.5.7", "generator": "tests/golden/make_golden_lazy_stream.py", "params": params,
           "inputs": {name: [len(d), helpers.sha256(d)] for name, d in inputs}, "frames": frames}
    json.dump(doc, open(path, "w"), indent=0)
    print(path, len(inputs), "inputs x", len(hs.LEVELS), "levels", os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
