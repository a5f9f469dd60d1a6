"""Writes tests/golden/zstd_frame_flags_golden.json: length and sha256 of what the binary libzstd 1.5.7 makes of the rows of
tests/helpers_frame_flags.py -- ZSTD_CCtx_setParameter(level, then ZSTD_c_checksumFlag = 1 / ZSTD_c_contentSizeFlag = 0 /
ZSTD_c_dictIDFlag = 0 as the row's flag set says) [+ ZSTD_CCtx_loadDictionary] + ZSTD_compress2 -- and what ZSTD_CCtx_setParameter
returns for (200, 0), (201, 1), (202, 0) and (201, 2).  Flags are written as the KMP_FRAME_* bits.
Run from the repository root: python tests/golden/make_golden_frame_flags.py"""
import hashlib
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import helpers_frame_flags as hf                     # noqa: E402
from oracle.libzstd_ref import LibZstd               # noqa: E402


def main():
    z = LibZstd()
    rows = []
    for level, dname, d, flags, slices in hf.rows():
        frames = [hf.lib_compress2(z, p, level, flags, d) for _, p in slices]
        for (_, p), f in zip(slices, frames):
            assert (z.decompress_with_dict(f, len(p), d) if d else z.decompress(f, len(p))) == p
        rows.append({"level": level, "dict": dname, "dict_sha256": hashlib.sha256(d).hexdigest() if d else None, "flags": flags,
                     "slices": [s for s, _ in slices], "frames": [[len(f), hashlib.sha256(f).hexdigest()] for f in frames]})
    ret = {f"{pid},{value}": hf.lib_set_parameter(z, pid, value) for pid, value in ((200, 0), (201, 1), (202, 0), (201, 2))}
    out = os.path.join(ROOT, "tests", "golden", "zstd_frame_flags_golden.json")
    with open(out, "w") as f:
        json.dump({"libzstd": 10507, "set_parameter": ret, "rows": rows}, f, separators=(",", ":"))
        f.write("\n")
    print(out, len(rows), "rows", sum(len(r["frames"]) for r in rows), "frames", ret)


if __name__ == "__main__":
    main()
