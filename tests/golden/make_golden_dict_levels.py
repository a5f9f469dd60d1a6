"""Writes tests/golden/zstd_dict_levels_golden.json: length and sha256 of what the binary libzstd 1.5.7 makes of the cases of
tests/helpers_dict_levels.py -- LibZstd.compress_with_dict(slice, dictionary, level), i.e. ZSTD_CCtx_setParameter(level) +
ZSTD_CCtx_loadDictionary + ZSTD_compress2 -- at levels 1, 2, -1, -5 and, on one dictionary's rows, -131072.
Run from the repository root: python tests/golden/make_golden_dict_levels.py"""
import hashlib
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import helpers_dict_levels as hd                     # noqa: E402
from oracle.libzstd_ref import LibZstd               # noqa: E402


def main():
    z = LibZstd()
    rows = []
    for name, d, slices in hd.cases():
        for level in hd.levels_of(name):
            frames = [z.compress_with_dict(p, d, level) for _, p in slices]
            for (_, p), f in zip(slices, frames):
                assert z.decompress_with_dict(f, len(p), d) == p
            rows.append({"dict": name, "level": level, "dict_sha256": hashlib.sha256(d).hexdigest(),
                         "slices": [s for s, _ in slices], "frames": [[len(f), hashlib.sha256(f).hexdigest()] for f in frames]})
    out = os.path.join(ROOT, "tests", "golden", "zstd_dict_levels_golden.json")
    with open(out, "w") as f:
        json.dump({"libzstd": 10507, "rows": rows}, f, separators=(",", ":"))
        f.write("\n")
    print(out, len(rows), "rows", sum(len(r["frames"]) for r in rows), "frames")


if __name__ == "__main__":
    main()
