"""The hand-made zstd frames of tests/helpers_handmade.py (legal zstd no encoder writes, and its illegal neighbours) on the CPU emulator
against what libzstd 1.5.7 answered for them (tests/golden/zstd_handmade_golden.json): k_zstd_decode alone and behind the sort and both
pre-decoders, the dictionary call, kx_frame_info; the fixture against the live library where there is one; every entry and output at a
guard page; the decode path under the sanitizers in a program of its own."""
import os
import struct
import subprocess
import sys

import pytest

import helpers
import helpers_frame_info as hf
import helpers_handmade as hh


@pytest.fixture(scope="module")
def fixture():
    return hh.golden()


@pytest.fixture(scope="module")
def alone(fixture):
    return hh.emu_decode(fixture[0], pre=False)


@pytest.fixture(scope="module")
def ahead(fixture):
    return hh.emu_decode(fixture[0], pre=True)


def test_fixture_is_worth_replaying(fixture):
    """the composer's conditions hold for the recorded answers, and the cases reach every family and every code the library gave"""
    cs, rows = fixture
    assert not hh.check_intents(cs, rows)
    assert {c[0] for c in cs} == {"header", "blocks", "literals", "seqhdr", "seqval", "multi", "dict", "random"}
    assert {r["status"] for r in rows} >= {0, 14, 16, 20, 22, 24, 30, 32, 70, 72}
    assert sum(1 for c in cs if c[0] == "random") >= 400
    names = {c[1] for c in cs}
    assert set(hh.REFUSED_THOUGH_ACCEPTED) <= names and all(r["status"] == 0 for c, r in zip(cs, rows) if c[1] in hh.REFUSED_THOUGH_ACCEPTED)
    assert sum(1 for n in names if "first block in Repeat mode" in n) >= 6 and sum(1 for n in names if "tree-less literals as the first block" in n) >= 4


@pytest.mark.parametrize("pre", [False, True], ids=["alone", "pre-decoders"])
def test_decoder_accepts_what_the_library_accepts(fixture, alone, ahead, pre):
    """status 0 exactly where the library's is 0, with its bytes; its code where codes are compared (helpers_handmade.EXACT_FAMILIES)"""
    cs, rows = fixture
    bad = hh.compare(cs, rows, ahead if pre else alone)
    assert not bad, f"{len(bad)} differ\n" + "\n".join(bad[:30])


def test_the_two_decode_paths_agree(fixture, alone, ahead):
    bad = [f"{c[0]} / {c[1]}: alone {a[:2]}, behind the pre-decoders {b[:2]}" for c, a, b in zip(fixture[0], alone, ahead) if a != b]
    assert not bad, f"{len(bad)} differ\n" + "\n".join(bad[:30])


def test_the_found_entries_are_refused_with_the_librarys_codes(fixture, alone, ahead):
    cs = fixture[0]
    want = {"found: a sequence count of 0 followed by a byte": 20, "found: a single segment of 4 with a compressed block of 6": 72,
            "found: literal length 0, offset value 3, first repeat offset 1": 20, "4 streams of 5 literals": 24}
    got = {c[1]: (a[0], b[0]) for c, a, b in zip(cs, alone, ahead) if c[1] in want}
    assert got == {k: (v, v) for k, v in want.items()}


def test_frame_info_answers_what_the_library_answers(fixture):
    cs, rows = fixture
    got = hh.emu_info(cs)
    bad = [f"{c[0]} / {c[1]}: {g}, the library {r['info']}" for c, r, g in zip(cs, rows, got) if g != r["info"]]
    assert not bad, f"{len(bad)} differ\n" + "\n".join(bad[:30])


def test_fixture_against_the_live_library(fixture):
    """a drifting fixture is noticed where a libzstd 1.5.7 is present (elsewhere there is nothing to compare)"""
    lib = hf.live_lib()
    if lib is None:
        return
    cs, rows = fixture
    live = hh.library_rows(lib, cs)
    bad = [f"{c[0]} / {c[1]}: the fixture holds {r}, the library answers {v}" for c, r, v in zip(cs, rows, live) if r != v]
    assert not bad, f"{len(bad)} differ\n" + "\n".join(bad[:10])


def test_entries_and_outputs_end_at_guard_pages(fixture):
    """tests/helpers_handmade.py as a program: every entry ends at a PROT_NONE page, every output's capacity too"""
    n = sum(1 for c in fixture[0] if c[4] is None)
    r = subprocess.run([sys.executable, os.path.join(os.path.dirname(os.path.abspath(__file__)), "helpers_handmade.py")],
                       capture_output=True, text=True, timeout=900)
    assert r.returncode == 0 and f"OK {n}" in r.stdout.splitlines()[-1:], f"exit {r.returncode}\n" + r.stdout[-1500:] + r.stderr[-2000:]


def asan_cases(cs, rows):
    """the cases whose work is table descriptions and short streams: entries up to 4 KiB, outputs up to 8 KiB, no dictionary"""
    return [(c, r) for c, r in zip(cs, rows) if c[4] is None and len(c[2]) <= 4096 and c[3] <= 8192]


def test_decode_path_under_sanitizers(fixture, tmp_path):
    """tests/emu/handmade_asan_main.cpp (g++ -fsanitize=address,undefined with the emulator's sources): every entry in a heap block of
    exactly its length, decoded into one of exactly its capacity; nothing is loaded into python"""
    emu = os.path.join(helpers.ROOT, "tests", "emu")
    exe = str(tmp_path / "handmade_asan")
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-I" + emu,
                    "-I" + os.path.join(helpers.ROOT, "kompressor_amd", "csrc"), "-o", exe, os.path.join(emu, "emu_core.cpp"),
                    os.path.join(emu, "emu_zstd.cpp"), os.path.join(emu, "handmade_asan_main.cpp")], check=True)
    picked = asan_cases(*fixture)
    assert len(picked) >= 700 and {c[0] for c, _ in picked} >= {"header", "blocks", "literals", "seqhdr", "seqval", "multi", "random"}
    path = str(tmp_path / "cases.bin")
    with open(path, "wb") as f:
        f.write(struct.pack("<I", len(picked)))
        for c, r in picked:
            # (what the decoder must answer: the library's verdict, but for the named exceptions the refusal they are held to)
            st, n = (hh.REFUSED_THOUGH_ACCEPTED[c[1]], 0) if c[1] in hh.REFUSED_THOUGH_ACCEPTED else (r["status"], r["out_len"])
            f.write(struct.pack("<5I", len(c[2]), c[3], st, n, int(c[5] == "lenient"))); f.write(c[2])
    r = subprocess.run([exe, path], capture_output=True, text=True, timeout=900)
    assert r.returncode == 0 and f"{len(picked)} entries, 0 findings" in r.stdout, r.stdout[-1000:] + r.stderr[-4000:]
