"""inflate_size_body (kompressor_amd/csrc/deflate_info.h) in a stand-alone program under AddressSanitizer and UBSan: the wave emulator
core and tests/emu/inflate_info_asan_main.cpp built with g++ -fsanitize=address,undefined, every fixture entry and 500 of the mutants in
a heap block of exactly the entry's length.  Nothing is loaded into python.  No GPU."""
import subprocess

import numpy as np

import helpers_inflate_info as hi
from test_emu_inflate_info import MUTANT_SEED, N_MUTANTS


def test_size_body_under_sanitizers(tmp_path):
    rows = hi.golden()
    muts = hi.mutants(N_MUTANTS, MUTANT_SEED)[:500]
    cases = [(n, e, f) for n, e, f, _ in rows] + muts
    # the fixture's answers, and for the mutants the answers of the plain emulator build (which test_emu_inflate_info holds against zlib)
    want = np.concatenate([hi.expected_array([r for *_, r in rows]), hi.emu_cases(muts)])
    exe = hi.build_asan_program(str(tmp_path))
    path = str(tmp_path / "cases.bin")
    hi.write_cases(path, cases, want)
    r = subprocess.run([exe, path], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    assert f"{len(cases)} entries, 0 differ" in r.stdout
