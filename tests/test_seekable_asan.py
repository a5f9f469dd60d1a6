"""kx_seekable_index (kompressor_amd/csrc/zstd_seekable.h) under AddressSanitizer and UBSan: a stand-alone program
(tests/emu/seekable_asan_main.cpp, g++ -fsanitize=address,undefined) validates the damaged and foreign blobs of the fixture and seeded
mutants of a good table, each in a heap block of exactly its length.  Nothing is loaded into python."""
import random
import struct
import subprocess

import numpy as np

import helpers_seekable as hs


def _mutants(count, seed):
    rng = random.Random(seed)
    good = [r["blob"] for r in hs.blobs("foreign")] + [bytes.fromhex(hs.golden_case("size0")["table"])]
    out = []
    while len(out) < count:
        b = bytearray(rng.choice(good))
        k = rng.randrange(5)
        n, = struct.unpack("<I", b[-9:-5])
        table = 17 + n * (12 if b[-5] & 0x80 else 8)
        if k == 0:                                   # a byte of the table
            i = len(b) - 1 - rng.randrange(table)
            b[i] = rng.choice((b[i] ^ (1 << rng.randrange(8)), rng.randrange(256)))
        elif k == 1:                                 # the frame count
            b[-9:-5] = struct.pack("<I", rng.choice((0, 1, n + 1, n - 1 if n else 7, 1 << 27, (1 << 27) + 1, 0xFFFFFFFF, rng.randrange(1 << 32))))
        elif k == 2:                                 # cut at the front: the table alone, or less
            b = b[rng.randrange(len(b)):]
        elif k == 3:                                 # cut at the back
            b = b[:rng.randrange(len(b))]
        else:                                        # the descriptor
            b[-5] = rng.randrange(256)
        out.append(bytes(b))
    return out


def test_index_body_under_sanitizers(tmp_path):
    exe = hs.build_asan_program(str(tmp_path))
    rows = hs.blobs()
    entries = [r["blob"] for r in rows]
    want = [hs.expected_stat(r) for r in rows]
    for m in [b"", b"\xb1", b"\xb1\xea\x92\x8f"] + _mutants(400, 20260101):
        entries.append(m); want.append(hs.index_reference(m))
    assert any(int(w["status"]) == 0 for w in want[len(rows):]) and any(int(w["status"]) == 10 for w in want) and any(int(w["status"]) == 20 for w in want)
    cases = tmp_path / "cases.bin"
    hs.write_cases(str(cases), entries, [np.array(w) for w in want])
    r = subprocess.run([exe, str(cases)], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
