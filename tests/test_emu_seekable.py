"""zstd's seekable container on the CPU: the kernel bodies of kompressor_amd/csrc/zstd_seekable.h on the wave emulator
(tests/emu/emu_zstd_seekable.cpp) against tests/golden/zstd_seekable_golden.json -- libzstd 1.5.7's frames chunk by chunk, struct's
table, xxhash's checksums (tests/golden/make_golden_seekable.py)."""
import hashlib
import struct

import pytest

import helpers
import helpers_seekable as hs


@pytest.mark.parametrize("case", hs.cases(), ids=lambda c: c[0])
def test_emulated_container_is_the_golden_one(case):
    """plan + XXH64 + the level's compress kernels + table, emulated: the container byte for byte, result[0] its size"""
    name, cls, seed, size, fb, level, sums, src_off = case
    g = hs.golden_case(name)
    data = hs.case_input(cls, seed, size)
    blob, result = hs.emu_container(data, fb, level, sums, src_off, status_word=0)
    assert blob[len(blob) - len(g["table"]) // 2:].hex() == g["table"], "the seek table differs"
    assert len(blob) == g["length"] and hashlib.sha256(blob).hexdigest() == g["sha256"]
    assert result == [len(blob), 0]
    z = helpers.live_libzstd()
    if z is not None:
        assert z.decompress(blob, len(data)) == data, "libzstd does not decode the container to the input"


def test_empty_input_is_a_table_of_seventeen_bytes():
    blob, result = hs.emu_container(b"", 4096, 3, 1)
    assert blob == struct.pack("<II", hs.SKIP_MAGIC, 9) + struct.pack("<IB", 0, 0x80) + struct.pack("<I", hs.SEEKABLE_MAGIC)
    assert result == [17, 0]


def test_a_chunk_without_a_frame_voids_the_result_and_status_bits_pass_through():
    """the table kernel alone: clen[i] = 0 is a chunk the batch refused -> result[0] = 0; result[1] = the context's status word"""
    import numpy as np
    vp = helpers._vp
    n = 300
    clen = np.full(n, 20, dtype=np.uint32); clen[257] = 0
    dlen = np.full(n, 64, dtype=np.uint32); cks = np.arange(n, dtype=np.uint32)
    dense = np.zeros(n + 1, dtype=np.uint64); dense[1:] = np.cumsum(clen, dtype=np.uint64)
    dst = np.zeros(int(dense[n]) + 17 + 12 * n, dtype=np.uint8); result = np.full(2, 7, dtype=np.uint64); word = np.array([5], dtype=np.uint32)
    assert hs.emu().emu_seekable_table(vp(dst), vp(dense), vp(clen), vp(dlen), vp(cks), n, 1, vp(word), vp(result), 4) == 0
    assert [int(x) for x in result] == [0, 5]


@pytest.mark.parametrize("row", hs.blobs(), ids=lambda r: r["name"])
def test_index_of_foreign_and_damaged_blobs(row):
    """kx_seekable_index as the kernel runs it, the blob in a buffer of exactly its length between canaries: the golden answers"""
    got, want = hs.emu_index(row["blob"]), hs.expected_stat(row)
    assert got.tobytes() == want.tobytes(), f"{row['name']}: {got} != {want}"
    if row["name"] in ("too_many_frames", "huge_frame_count"):
        assert int(got["status"]) in (10, 20)


def test_index_of_every_golden_case_table():
    """the product's own containers: a table alone is no container (its sizes do not sum to offset 0) unless it has no entries"""
    for r in hs.golden()["cases"]:
        table = bytes.fromhex(r["table"])
        got = hs.emu_index(table)
        assert int(got["status"]) == (0 if r["size"] == 0 else 20), r["name"]


def _reader(blob):
    ents, fo, co = hs.parse_table(blob)
    return ents, fo, co


@pytest.mark.parametrize("name", ["size12305", "f96", "chunks300"])
def test_emulated_reads_at_frame_edges(name):
    """A read = the covering frames (found as the host index finds them: the prefix sums) decoded whole by the emulated decoder, then
    the XXH64 body in its verifying form: the bytes asked for are dst[skip : skip + hi - lo], every status stays 0."""
    import bisect
    g = hs.golden_case(name)
    data = hs.case_input(g["cls"], g["seed"], g["size"])
    blob, _ = hs.emu_container(data, g["frame_bytes"], g["level"], g["checksums"])
    ents, fo, co = _reader(blob)
    at = len(blob) - 17 - 12 * len(ents)
    ranges = hs.edge_ranges(len(data), co[:-1])
    if name == "chunks300":
        ranges = ranges[:1] + ranges[-40:]
    for lo, hi in ranges:
        hi_c = min(hi, len(data))
        if lo >= hi_c:
            continue
        first = bisect.bisect_right(co, lo) - 1
        last = bisect.bisect_left(co, hi_c) - 1
        frames = [blob[fo[i]:fo[i + 1]] for i in range(first, last + 1)]
        out, dst_status = helpers.emu_decompress(frames, [ents[i][1] for i in range(first, last + 1)])
        assert not any(dst_status), (lo, hi, dst_status)
        dst = b"".join(out)
        skip = lo - co[first]
        assert dst[skip:skip + hi_c - lo] == data[lo:hi_c], (lo, hi)
        assert 0 <= skip < max(ents[first][1], 1)
        starts = [co[i] - co[first] for i in range(first, last + 1)]
        st = hs.emu_verify(dst, starts, [len(o) for o in out], blob[at + 8 + 12 * first:at + 8 + 12 * (last + 1)], [0] * len(frames))
        assert st == [0] * len(frames), (lo, hi, st)


def test_emulated_verify_marks_exactly_the_flipped_frame():
    row = hs.blobs("flipped")[0]
    blob = row["blob"]
    data = hs.case_input(row["cls"], row["seed"], row["size"])
    ents, fo, co = _reader(blob)
    at = len(blob) - 17 - 12 * len(ents)
    lens = [d for _, d, _ in ents]
    st = hs.emu_verify(data, co[:-1], lens, blob[at + 8:at + 8 + 12 * len(ents)], [0] * len(ents))
    assert st == [22 if i == row["bad_frame"] else 0 for i in range(len(ents))]
    # a frame the decoder rejected keeps its status; one that decoded to another size is 20
    st = hs.emu_verify(data, co[:-1], [lens[0] - 1] + lens[1:], blob[at + 8:at + 8 + 12 * len(ents)], [0, 72, 0, 0])
    assert st == [20, 72, 22, 0]
