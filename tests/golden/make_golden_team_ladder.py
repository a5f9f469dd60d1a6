"""Writes tests/golden/zstd_team_ladder_golden.json: length and sha256 of what the binary libzstd 1.5.7 makes of the ladder of
tests/helpers_team.py at levels 3 and 1, without and with its raw dictionary (LibZstd.compress / compress_with_dict).
Run from the repository root: python tests/golden/make_golden_team_ladder.py"""
import hashlib
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import helpers_team as ht                            # noqa: E402
from oracle.libzstd_ref import LibZstd               # noqa: E402


def main():
    z = LibZstd()
    d, slices = ht.ladder()
    frames = {}
    for name, level, with_dict in ht.CONFIGS:
        fs = [z.compress_with_dict(p, d, level) if with_dict else z.compress(p, level) for p in slices]
        for p, f in zip(slices, fs):
            assert (z.decompress_with_dict(f, len(p), d) if with_dict else z.decompress(f, len(p))) == p
        frames[name] = [[len(f), hashlib.sha256(f).hexdigest()] for f in fs]
    out = os.path.join(ROOT, "tests", "golden", "zstd_team_ladder_golden.json")
    with open(out, "w") as f:
        json.dump({"libzstd": 10507, "dict_sha256": hashlib.sha256(d).hexdigest(),
                   "slices_sha256": [hashlib.sha256(s).hexdigest() for s in slices], "frames": frames}, f, separators=(",", ":"))
    print(out, os.path.getsize(out))


if __name__ == "__main__":
    main()
