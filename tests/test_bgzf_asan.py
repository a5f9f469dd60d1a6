"""kx_bgzf_head and kx_bgzf_walk (kompressor_amd/csrc/bgzf.h) under AddressSanitizer and UBSan: a stand-alone program
(tests/emu/bgzf_asan_main.cpp, g++ -fsanitize=address,undefined) runs the head test at every position and the walk over the blobs of
the fixture and seeded mutants, each in a heap block of exactly its length.  Nothing is loaded into python."""
import subprocess

import numpy as np

import helpers_bgzf as hb


def test_head_and_walk_under_sanitizers(tmp_path):
    exe = hb.build_asan_program(str(tmp_path))
    rows = hb.blobs()
    entries = [r["blob"] for r in rows]
    want = [hb.expected_stat(r) for r in rows]
    good = [r["blob"] for r in hb.blobs("foreign")]
    for m in [b"\x1f", b"\x1f\x8b\x08\x04", hb.EOF, hb.EOF[:27], hb.many_members(300)[0]] + hb.mutants(400, 20261023, good):
        entries.append(m); want.append(hb.walk_reference(m)[0])
    assert {int(w["status"]) for w in want[len(rows):]} == {0, -3, -5}
    cases = tmp_path / "cases.bin"
    hb.write_cases(str(cases), entries, [np.array(w) for w in want])
    r = subprocess.run([exe, str(cases)], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
