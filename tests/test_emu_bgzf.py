"""The BGZF container on the CPU: the kernel bodies of kompressor_amd/csrc/bgzf.h on the wave emulator (tests/emu/emu_bgzf.cpp) against
tests/golden/bgzf_golden.json -- zlib 1.2.11's raw DEFLATE payloads block by block, struct's wrappers, zlib.crc32's checksums
(tests/golden/make_golden_bgzf.py) -- and the emulated parallel open against the serial walk and its Python restatement."""
import gzip
import hashlib

import numpy as np
import pytest

import helpers
import helpers_bgzf as hb


# ------------------------------------------------------------------------------------------------------ compress ----
@pytest.mark.parametrize("case", hb.cases(), ids=lambda c: c[0])
def test_emulated_container_is_the_golden_one(case):
    """plan + the level's DEFLATE kernels (format 0) + wrap + packing + finish, emulated: the container byte for byte"""
    name, cls, seed, size, bb, level, src_off = case
    g = hb.golden_case(name)
    data = hb.case_input(cls, seed, size)
    blob, result = hb.emu_container(data, bb, level, 0, src_off)
    st, mo, *_ = hb.walk_reference(blob)
    assert int(st["status"]) == 0 and [b - a for a, b in zip(mo, mo[1:])] == g["members"] + [28], "the member sizes differ"
    assert len(blob) == g["length"] and hashlib.sha256(blob).hexdigest() == g["sha256"]
    assert result == [len(blob), 0]
    assert gzip.decompress(blob) == data, "Python's gzip does not decode the container to the input"


def test_empty_input_and_no_eof_rounds():
    assert hb.emu_container(b"", 4096, 6) == (hb.EOF, [28, 0])
    assert hb.emu_container(b"", 4096, 6, hb.NO_EOF) == (b"", [0, 0])
    g = hb.golden_case("size12305")
    data = hb.case_input(g["cls"], g["seed"], g["size"])
    first, r1 = hb.emu_container(data[:2 * 4096], 4096, 6, hb.NO_EOF)
    second, r2 = hb.emu_container(data[2 * 4096:], 4096, 6)
    assert r1 == [len(first), 0] and r2 == [len(second), 0]
    assert hashlib.sha256(first + second).hexdigest() == g["sha256"], "two rounds concatenated are the container of the whole"


def test_a_block_without_a_stream_voids_the_result_and_status_bits_pass_through():
    data = hb.case_input("T", 97000, 3 * 512)
    blob, result = hb.emu_container(data, 512, 6, status_word=5, drop=1)
    assert result == [0, 5]
    _, result = hb.emu_container(data, 512, 6, status_word=5)
    assert result[1] == 5 and result[0] > 0


# ------------------------------------------------------------------------------------------------------ open ----
def _check_open(blob, want_stat=None, **kw):
    ref = hb.walk_reference(blob)
    if want_stat is not None:
        assert ref[0].tobytes() == want_stat.tobytes(), "the restatement disagrees with the fixture"
    o = hb.emu_open(blob, **kw)
    hb.same_open(o, ref[0], ref)
    hb.same_open(hb.emu_walk(blob), ref[0], ref)
    return o


@pytest.mark.parametrize("row", hb.blobs(), ids=lambda r: r["name"])
def test_open_of_foreign_damaged_and_wrong_blobs(row):
    """the emulated parallel open and k_bgzf_walk, the blob in a buffer of exactly its length between canaries: the fixture's stat,
    the restatement's arrays"""
    o = _check_open(row["blob"], hb.expected_stat(row))
    assert o.path == (1 if row["blob"] else 2)
    if row["name"] == "bgzf_stored_inside_members":
        assert o.candidates > int(o.stat["blocks"]), "the nested file must give false candidates"
    if row["name"] == "false_chain_merges":
        assert o.candidates == int(o.stat["blocks"]) + 1


def test_open_of_every_golden_container_with_a_lowered_cap():
    """the product's own containers (emulated ones are the golden ones: test above) through the parallel path, and through the
    fallback that a candidate cap below their count forces"""
    for name in ("size0", "size12305", "blocks300"):
        g = hb.golden_case(name)
        data = hb.case_input(g["cls"], g["seed"], g["size"])
        blob, _ = hb.emu_container(data, g["block_bytes"], g["level"])
        o = _check_open(blob)
        assert o.path == 1 and int(o.stat["blocks"]) == len(g["members"]) + 1 and int(o.stat["flags"]) == 1
        low = _check_open(blob, max_candidates=o.candidates - 1)
        assert low.path == 2
        assert _check_open(blob, max_candidates=o.candidates).path == 1


def test_head_test_equals_the_restatement_at_every_position():
    e = hb.emu()
    out = np.zeros(4, dtype=np.uint32)
    for row in hb.blobs():
        blob = row["blob"]
        keep, at = hb._exact(blob)
        for p in range(len(blob) + 1):
            st = e.emu_bgzf_head(at, len(blob), p, helpers._vp(out))
            want = hb.head_reference(blob, p)
            assert (st,) + (tuple(int(x) for x in out) if st == 0 else (0, 0, 0, 0)) == want, (row["name"], p)


def test_open_of_seeded_mutants():
    good = [r["blob"] for r in hb.blobs("foreign")]
    seen = set()
    for m in hb.mutants(200, 20261021, good):
        o = _check_open(m)
        seen.add(int(o.stat["status"]))
    assert seen == {0, -3, -5}


def test_open_of_5000_members():
    """13 doubling levels, several scan tiles per wave and several prefix entries per lane; other grids and workgroup sizes"""
    blob, content = hb.many_members(5000)
    o = _check_open(blob)
    assert (o.path, o.levels, int(o.stat["blocks"]), int(o.stat["content"])) == (1, 13, 5000, len(content))
    assert len(blob) > 16 * 4096
    for nblocks, waves in ((1, 1), (7, 16)):
        hb.same_open(hb.emu_open(blob, nblocks=nblocks, waves=waves), o.stat, hb.walk_reference(blob))
    # the chain broken in the middle: the status is the head test's where it stops
    cut = bytearray(blob); cut[o.member_off[2500] + 3] = 0
    assert int(_check_open(bytes(cut)).stat["status"]) == -3
    assert gzip.decompress(blob) == content


# ------------------------------------------------------------------------------------------------------ verify ----
def test_verify_marks_exactly_the_wrong_member():
    for row in hb.blobs("wrong"):
        blob = row["blob"]
        o = hb.emu_open(blob)
        streams = [blob[a:a + n] for a, n in zip(o.in_off, o.in_len)]
        parts, st = helpers.emu_inflate(streams, o.out_cap, fmt=0)          # (the marker: a capacity of 0)
        assert not any(st), st
        assert b"".join(parts) == row["content"]
        n = len(parts)
        want = [-3 if i == row["bad_member"] else 0 for i in range(n)]
        assert hb.emu_verify(blob, parts, o, [0] * n, verify=1) == want
        assert hb.emu_verify(blob, parts, o, [0] * n, verify=0) == (want if row["name"] == "flipped_isize" else [0] * n)
        assert hb.emu_verify(blob, parts, o, [-5] + [0] * (n - 1), verify=1) == [-5] + want[1:], "a status the decoder set stays"
