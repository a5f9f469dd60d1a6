"""kmp_zstd_frame_info_host (kompressor_amd/csrc/zstd_frame_info.h through the compiler's host pass) against the binary libzstd 1.5.7:
the committed fixture on every entry and field, the live library on seeded mutants where it is present, and the parse body in a
stand-alone program under AddressSanitizer and UBSan with every entry in a heap block of exactly its length.  No GPU."""
import subprocess

import numpy as np
import pytest

import helpers_frame_info as hf

N_MUTANTS = 3000


@pytest.fixture(scope="module")
def rows():
    return hf.golden()


def test_fixture_holds_what_the_issue_lists(rows):
    names = [n for n, _, _ in rows]
    by = {n: (e, r) for n, e, r in rows}
    assert len(rows) >= 150
    widths = set()
    for _, e, r in rows:
        if r["status"] == 0 and r["frames"] == 1 and not r["flags"] & 2 and e[:4] == hf.MAGIC:
            fhd = e[4]
            widths.add((1 << (fhd >> 6)) if fhd >> 6 else (fhd >> 5) & 1)
    assert widths == {0, 1, 2, 4, 8}, widths
    for want in ("streaming 1 block", "streaming 2 blocks", "streaming 17 blocks", "skippable alone", "skippable payload 0", "window 2^31",
                 "window above the maximum (2^32)", "reserved bit", "block type 3", "last-block bit cleared, nothing behind", "empty frame"):
        assert want in by, want
    assert by["streaming 17 blocks"][1]["content"] == hf.UNKNOWN and by["streaming 17 blocks"][1]["bound"] == 17 * 131072
    assert {by[f"dictionary ID {w} bytes (edited)"][1]["dict_id"] for w in (1, 2, 4)} == {0xAB, 0xBEEF, 0xC0FFEE01}
    assert by["window above the maximum (2^32)"][1]["status"] == 16 and by["reserved bit"][1]["status"] == 14
    assert by["block type 3"][1]["status"] == 20 and by["last-block bit cleared, nothing behind"][1]["status"] == 72
    assert sum(1 for n in names if n.startswith("truncated at")) >= 50
    assert {r["status"] for _, _, r in rows} >= {0, 10, 14, 16, 20, 72}


def test_host_call_equals_the_fixture(rows):
    got = hf.host_info([e for _, e, _ in rows])
    bad = hf.diff(got, hf.expected_array([r for _, _, r in rows]), [n for n, _, _ in rows])
    assert not bad, "\n".join(bad[:20])


def test_host_call_arguments():
    from kompressor_amd import _lib
    lib = _lib.load()
    assert lib.kmp_zstd_frame_info_host(None, None, None, 0, None) == 0
    assert lib.kmp_zstd_frame_info_host(None, None, None, 1, None) == -2


def test_host_call_on_many_threads_equals_one(rows):
    """8 192 entries and more are spread over threads: the same answers, entry for entry"""
    entries = [e for _, e, _ in rows if len(e) <= 4096]
    one = hf.host_info(entries)
    many = hf.host_info(entries * (9000 // len(entries) + 1))
    assert len(many) >= 8192
    for k in range(0, len(many), len(entries)):
        part = many[k:k + len(entries)]
        assert part.tobytes() == one[:len(part)].tobytes()


def test_host_call_equals_the_live_library_on_mutants(rows):
    lib = hf.live_lib()
    if lib is None:
        pytest.skip("no binary libzstd 1.5.7 on this machine: the live comparison on mutants did not run (the fixture comparison did)")
    muts = hf.mutants(N_MUTANTS, seed=20261017)
    assert len(muts) >= N_MUTANTS
    got = hf.host_info([e for _, e in muts])
    want = hf.expected_array([hf.live_answers(lib, e) for _, e in muts])
    bad = hf.diff(got, want, [f"{n}: {e[:40].hex()}" for n, e in muts])
    assert not bad, "\n".join(bad[:20])
    codes = {int(s) for s in want["status"]}
    print(f"{len(muts)} mutants, statuses {sorted(codes)}, {int((want['status'] == 0).sum())} accepted")
    assert codes >= {0, 10, 14, 20, 72}                      # (the mutants reach the library's branches)


def test_parse_body_under_sanitizers(rows, tmp_path):
    """g++ -fsanitize=address,undefined, a program of its own: every fixture entry in a heap block of exactly its length"""
    exe = hf.build_asan_program(str(tmp_path))
    cases = str(tmp_path / "cases.bin")
    hf.write_cases(cases, [e for _, e, _ in rows], hf.expected_array([r for _, _, r in rows]))
    r = subprocess.run([exe, cases], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    assert f"{len(rows)} entries, 0 differ" in r.stdout


def test_host_batch_without_caps_names_the_error(rows):
    """decompress_host_batch(frames): an entry that fails the inspection raises with libzstd's name for the error, before any GPU work"""
    from kompressor_amd.batch import decompress_host_batch, frame_info_host
    by = {n: e for n, e, _ in rows}
    good = by["fcs1 single segment"]
    for name, text in (("wrong magic, 8 bytes", "Unknown frame descriptor"), ("reserved bit", "Unsupported frame parameter"),
                       ("block type 3", "Data corruption detected"), ("truncated at 20 of 49", "Src size is incorrect"),
                       ("window above the maximum (2^32)", "Frame requires too much memory for decoding")):
        with pytest.raises(RuntimeError, match=f"entry 1 of 2: {text}"):
            decompress_host_batch([good, by[name]])
    info = frame_info_host([e for _, e, _ in rows])
    assert info.tobytes() == hf.host_info([e for _, e, _ in rows]).tobytes()
