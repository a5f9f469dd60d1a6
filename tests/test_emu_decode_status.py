"""The decode side on the CPU emulator against the status snapshot taken at the commit before the framing readers moved into
kompressor_amd/csrc/zstd_format.h (tests/golden/decode_status_golden.json): the status, length and bytes of every seeded case through
k_zstd_decode alone and behind the two pre-decoders, its sort key and its kx_frame_info answer, field by field; the framing edges at
a guard page; the two section readers under the sanitizers, prefix by prefix, in a program of their own."""
import os
import subprocess
import sys

import numpy as np
import pytest

import helpers
import helpers_decode_status as hd
import helpers_frame_info as hf


@pytest.fixture(scope="module")
def snapshot():
    g = hd.golden()
    return g, hd.checked_cases(g)


@pytest.fixture(scope="module")
def replay(snapshot):
    return hd.emu_rows(snapshot[1])


@pytest.mark.parametrize("column", ["alone", "pre", "key", "info"])
def test_emulator_answers_what_the_snapshot_holds(snapshot, replay, column):
    """alone: k_zstd_decode by itself; pre: behind the sort and both pre-decoders; key: k_zstd_seq_count; info: kx_frame_info"""
    g, _ = snapshot
    assert g["lit_cap"] == hd.LIT_CAP and len(g["rows"]) >= 1200
    bad = [f"{w['name']}: {column} {r[column]}, the snapshot of {g['commit'][:7]} holds {w[column]}" for r, w in zip(replay, g["rows"]) if r[column] != w[column]]
    assert not bad, f"{len(bad)} differ\n" + "\n".join(bad[:20])


def test_snapshot_reaches_the_decoders_branches(snapshot):
    """(the cases are worth replaying: they are accepted and rejected in every way the framing can be)"""
    rows = snapshot[0]["rows"]
    assert {r["alone"][0] for r in rows} >= {0, 10, 14, 20, 70, 72}
    assert sum(1 for r in rows if r["alone"][0] == 0) >= 100 and sum(1 for r in rows if r["key"]) >= 100
    assert all(r["alone"] == r["pre"] for r in rows)


def test_framing_edges_end_at_a_guard_page():
    """tests/helpers_decode_status.py as a program: every edge ends exactly at a PROT_NONE page and is rejected with nothing written"""
    r = subprocess.run([sys.executable, os.path.join(os.path.dirname(os.path.abspath(__file__)), "helpers_decode_status.py")],
                       capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and f"EDGES OK {len(hd.edges())}" in r.stdout, f"exit {r.returncode}\n" + r.stdout[-1500:] + r.stderr[-2000:]


def block_bodies(cs, limit=300):
    """distinct bodies of compressed blocks, the first KiB of each, from the snapshot's base frames and then from its cases (damaged
    headers among them) until there are `limit`.  The readers look at the first 5 bytes of a literals section and at up to 4 bytes
    where it ends; every prefix of a body is tried, so the work grows with the square of the length."""
    out = {}
    for f in [f for f, _ in hd.base_frames()] + [e for _, e, _ in cs]:
        heads, _ = hf.block_bounds(f)
        for h in heads:
            bh = int.from_bytes(f[h:h + 3], "little")
            if (bh >> 1) & 3 == 2 and h + 3 + (bh >> 3) <= len(f) and len(out) < limit:
                out.setdefault(f[h + 3:h + 3 + min(bh >> 3, 1024)])
    assert len(out) == limit, len(out)
    return list(out)


def test_section_readers_under_sanitizers(snapshot, tmp_path):
    """tests/emu/zstd_format_asan_main.cpp (g++ -fsanitize=address,undefined): every prefix of every body in a heap block of exactly
    its length; no read outside it, and once a reader says "fits" its fields stay what they are at every larger length"""
    exe = str(tmp_path / "zstd_format_asan")
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    "-I" + os.path.join(helpers.ROOT, "kompressor_amd", "csrc"), "-o", exe,
                    os.path.join(helpers.ROOT, "tests", "emu", "zstd_format_asan_main.cpp")], check=True)
    bodies = block_bodies(snapshot[1])
    path = str(tmp_path / "bodies.bin")
    with open(path, "wb") as f:
        f.write(np.uint32(len(bodies)).tobytes())
        for b in bodies:
            f.write(np.uint32(len(b)).tobytes()); f.write(b)
    r = subprocess.run([exe, path], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-1000:] + r.stderr[-4000:]
    assert f"{len(bodies)} bodies, 0 findings" in r.stdout, r.stdout
