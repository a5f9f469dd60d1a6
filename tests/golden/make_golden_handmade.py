#!/usr/bin/env python3
"""Makes tests/golden/zstd_handmade_golden.json: what the binary libzstd 1.5.7 (oracle/libzstd_ref.py) answers for every hand-made
case of tests/helpers_handmade.py -- ZSTD_decompress (ZSTD_decompress_usingDict where the case has a dictionary) at the case's capacity:
the error code, or the length and sha256 of the output; and ZSTD_findDecompressedSize, ZSTD_decompressBound and the walk with
ZSTD_findFrameCompressedSize as a kmp_zstd_frame_info.  No frame bytes are stored: the head of each entry's sha256 and one sha256 over all.

It FAILS where the library contradicts a case's intent ("ok" accepted, "reject" refused), where it accepts fewer than 60 % of the cases
or more than 2 % are "lenient": that is the composer's own test.  The decoder under test is never asked.

    python tests/golden/make_golden_handmade.py [--table]      # --table: also what the emulator answers, (library code, our code) counted
"""
import argparse
import collections
import os
import sys

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
import helpers_handmade as hh        # noqa: E402
import helpers_frame_info as hf      # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--table", action="store_true", help="print the (library code, our code) pairs of the emulator's answers, for DESIGN.md")
    args = ap.parse_args()
    lib = hf.live_lib()
    if lib is None:
        sys.exit("no binary libzstd 1.5.7 on this machine")
    cs = hh.cases()
    rows = hh.library_rows(lib, cs)
    bad = hh.check_intents(cs, rows)
    if bad:
        sys.exit(f"{len(bad)} findings, nothing written\n" + "\n".join(bad))
    hh.write_golden(cs, rows)
    fams = collections.Counter(c[0] for c in cs)
    print(f"{len(cs)} cases ({', '.join(f'{k} {v}' for k, v in fams.items())}), {sum(1 for r in rows if r['status'] == 0)} accepted, "
          f"statuses {sorted({r['status'] for r in rows})}, {sum(len(c[2]) for c in cs)} bytes of entries -> {hh.GOLDEN} ({os.path.getsize(hh.GOLDEN)} bytes)")
    if args.table:
        got = hh.emu_decode(cs, pre=False)
        pairs = collections.Counter((r["status"], g[0]) for r, g in zip(rows, got))
        for (a, b), n in sorted(pairs.items()):
            print(f"library {a:3d}  ours {b:3d}  x {n}" + ("" if a == b else "   " + "; ".join(c[1] for c, r, g in zip(cs, rows, got) if (r["status"], g[0]) == (a, b))[:300]))


if __name__ == "__main__":
    main()
