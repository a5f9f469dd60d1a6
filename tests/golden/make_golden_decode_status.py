#!/usr/bin/env python3
"""Makes tests/golden/decode_status_golden.json: what the decode side answers, on the CPU emulator, for the seeded cases of
tests/helpers_decode_status.py (mutants of the C restatement's frames and of the foreign frames, then the framing edges) -- status,
length and crc32 of the output through k_zstd_decode alone (KXEMU_NO_PRE) and behind the sort and the two pre-decoders, the sort key,
the six fields of kx_frame_info.  It is a record of ONE commit's behaviour, to hold later commits against: run it once, on the tree
of the commit named in the file, never to "refresh" a failing test.

    python tests/golden/make_golden_decode_status.py [--commit HASH]

The frames are not stored, only the head of each one's sha256 and one sha256 over all (the replaying tests rebuild them and check both).  Every entry is decoded with 16 zero bytes
behind it: the decoder of commit ce0018d read one byte behind a compressed block of 2 bytes whose raw / RLE literals header has the
3-byte size format.  The status of those two entries does not depend on that byte at the literal capacity used here (128 KiB + 64):
the byte only enters the regenerated size; a size above 128 KiB is "corrupted" at once, any other size does not fit the 2-byte block
(raw: 3 + size > 2; RLE: 3 + 1 > 2) and is "corrupted" as well, and no size up to 128 KiB exceeds the capacity, so "workspace" cannot come first.
"""
import argparse
import os
import subprocess
import sys

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
import helpers_decode_status as hd   # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--commit", help="the commit whose tree this runs on (default: git rev-parse HEAD)")
    args = ap.parse_args()
    commit = args.commit or subprocess.run(["git", "rev-parse", "HEAD"], capture_output=True, text=True, check=True,
                                           cwd=os.path.dirname(os.path.abspath(__file__))).stdout.strip()
    cs = hd.cases()
    rows = hd.emu_rows(cs)
    hd.write_golden(commit, rows)
    st = sorted({r["alone"][0] for r in rows})
    print(f"{len(rows)} cases at {commit[:7]}: statuses {st}, {sum(1 for r in rows if r['alone'][0] == 0)} accepted, "
          f"{sum(r['len'] for r in rows)} bytes of entries -> {hd.GOLDEN}")


if __name__ == "__main__":
    main()
