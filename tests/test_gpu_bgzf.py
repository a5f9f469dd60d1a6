"""The BGZF container on the device (kmp_bgzf_*: k_bgzf_wrap, k_bgzf_finish, the parallel open's kernels, k_bgzf_walk, k_bgzf_verify):
the golden cases (tests/golden/bgzf_golden.json: zlib 1.2.11's payloads, struct's wrappers, zlib.crc32's checksums) through the C ABI
between canaries and through ZstdBatch.compress_bgzf; open / stat / read / tell on the product's own containers and on foreign ones at
ranges around the member edges; damaged blobs; wrong trailers; the open against the host index on many members and beyond the candidate
cap; rounds; argument errors; the context's memory."""
import bisect
import ctypes
import gzip
import hashlib

import numpy as np
import pytest

import helpers_bgzf as hb
import helpers_seekable as hs
from kompressor_amd import _lib

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

MARGIN = 4096
KMP_ERR_ARG, KMP_ERR_CAPACITY = -2, -3


def _ctx(**kw):
    from kompressor_amd.batch import ZstdBatch
    assert torch.cuda.is_available(), "these tests need the MI355X"
    return ZstdBatch(table_span_gib=0, **kw)


@pytest.fixture(scope="module")
def big():
    b = _ctx(max_slices=512, max_slice_bytes=65536)
    yield b
    b.close()


@pytest.fixture(scope="module")
def small():
    b = _ctx(max_slices=8, max_slice_bytes=4096)
    yield b
    b.close()


def _dev(data, offset=0):
    """bytes -> a uint8 device tensor whose first byte lies `offset` bytes behind a 256-byte boundary"""
    buf = torch.zeros(offset + len(data) + 8, dtype=torch.uint8, device="cuda")
    assert buf.data_ptr() % 256 == 0
    if data:
        buf[offset:offset + len(data)] = torch.from_numpy(np.frombuffer(data, dtype=np.uint8).copy()).cuda()
    return buf[offset:offset + len(data)]


def _vp(t, at=0):
    return ctypes.c_void_p(t.data_ptr() + at)


def _compress_abi(b, data, bb, level, flags, src_offset=0):
    """kmp_bgzf_compress with d_dst (at an odd address) and d_scratch between canaries -> (container bytes, result[2])"""
    lib = b.lib
    cap = lib.kmp_bgzf_bound(len(data), bb, flags); need = lib.kmp_bgzf_scratch(len(data), bb)
    assert need > 0
    rng = np.random.default_rng(11)
    dcan = rng.integers(0, 256, 2 * MARGIN + 1 + cap, dtype=np.uint8); scan = rng.integers(0, 256, 2 * MARGIN + need, dtype=np.uint8)
    dst = torch.from_numpy(dcan.copy()).cuda(); scratch = torch.from_numpy(scan.copy()).cuda()
    result = torch.full((2,), -1, dtype=torch.int64, device="cuda")
    src = _dev(data, src_offset)
    rc = lib.kmp_bgzf_compress(b._h, _vp(src) if data else None, len(data), bb, level, flags, _vp(dst, MARGIN + 1), cap, _vp(scratch, MARGIN), need,
                               _vp(result), b._stream())
    assert rc == 0, b._err()
    torch.cuda.synchronize()
    d, s, r = dst.cpu().numpy(), scratch.cpu().numpy(), [int(x) for x in result.cpu().numpy()]
    at = MARGIN + 1
    assert np.array_equal(d[:at], dcan[:at]) and np.array_equal(d[at + cap:], dcan[at + cap:]), "bytes around d_dst changed"
    assert np.array_equal(s[:MARGIN], scan[:MARGIN]) and np.array_equal(s[MARGIN + need:], scan[MARGIN + need:]), "bytes around d_scratch changed"
    assert 0 <= r[0] <= cap
    assert np.array_equal(d[at + r[0]:at + cap], dcan[at + r[0]:at + cap]), "bytes of d_dst behind the container changed"
    return d[at:at + r[0]].tobytes(), r


# ------------------------------------------------------------------------------------------------------ compress ----
@pytest.mark.parametrize("case", hb.cases(), ids=lambda c: c[0])
def test_golden_container_through_the_c_abi_and_the_python_call(big, case):
    name, cls, seed, size, bb, level, src_off = case
    g = hb.golden_case(name)
    data = hb.case_input(cls, seed, size)
    blob, result = _compress_abi(big, data, bb, level, 0, src_off)
    st, mo, *_ = hb.walk_reference(blob)
    assert int(st["status"]) == 0 and [z - a for a, z in zip(mo, mo[1:])] == g["members"] + [28], "the member sizes differ"
    assert len(blob) == g["length"] and hashlib.sha256(blob).hexdigest() == g["sha256"]
    assert result == [g["length"], 0]
    assert gzip.decompress(blob) == data
    out = big.compress_bgzf(_dev(data, src_off), block_bytes=bb, level=level)
    assert out.numel() == g["length"] and hashlib.sha256(out.cpu().numpy().tobytes()).hexdigest() == g["sha256"]
    assert big.status() == (0, 0)


def test_rounds_without_the_marker_concatenate_to_the_golden_container(big):
    g = hb.golden_case("size12305")
    data = hb.case_input(g["cls"], g["seed"], g["size"])
    first, r1 = _compress_abi(big, data[:2 * 4096], 4096, 6, hb.NO_EOF)
    second, r2 = _compress_abi(big, data[2 * 4096:], 4096, 6, 0)
    assert r1 == [len(first), 0] and r2 == [len(second), 0]
    assert hashlib.sha256(first + second).hexdigest() == g["sha256"]
    assert _compress_abi(big, b"", 4096, 6, hb.NO_EOF) == (b"", [0, 0])
    assert big.compress_bgzf(_dev(b""), eof=False).numel() == 0 and big.compress_bgzf(_dev(b"")).cpu().numpy().tobytes() == hb.EOF
    parts = [big.compress_bgzf(_dev(data[:2 * 4096]), block_bytes=4096, eof=False), big.compress_bgzf(_dev(data[2 * 4096:]), block_bytes=4096)]
    assert hashlib.sha256(torch.cat(parts).cpu().numpy().tobytes()).hexdigest() == g["sha256"]


def test_context_memory_is_unchanged(big):
    """kmp_batch_memory before and after a container is written, opened and read: equal (the context has deflated and inflated a batch
    before, so what those calls allocate on their first use is there)"""
    data = hb.case_input("T", 98000, 5 * 4096 + 1)
    src = _dev(data)
    big.compress_bgzf(src, block_bytes=4096)
    r = big.open_bgzf(big.compress_bgzf(src, block_bytes=4096))
    r.read_all(); r.close()
    torch.cuda.synchronize()
    before = big.memory()
    blob = big.compress_bgzf(src, block_bytes=4096, level=6)
    r = big.open_bgzf(blob)
    assert r.read_all().cpu().numpy().tobytes() == data
    r.close()
    assert big.memory() == before


def test_argument_errors(big, small):
    lib = big.lib
    data = hb.case_input("T", 98001, 3 * 4096)
    src = _dev(data)
    cap = lib.kmp_bgzf_bound(len(data), 4096, 0); need = lib.kmp_bgzf_scratch(len(data), 4096)
    dst = torch.zeros(cap + 64, dtype=torch.uint8, device="cuda"); scratch = torch.zeros(need // 8 + 1, dtype=torch.int64, device="cuda")
    res = torch.zeros(2, dtype=torch.int64, device="cuda")

    def call(b=big, src_p=_vp(src), n=len(data), bb=4096, level=6, flags=0, dst_p=_vp(dst), dcap=cap, scr_p=_vp(scratch), sbytes=need, res_p=_vp(res)):
        return lib.kmp_bgzf_compress(b._h, src_p, n, bb, level, flags, dst_p, dcap, scr_p, sbytes, res_p, b._stream())
    assert call() == 0 and call(level=-1) == 0
    for level in (0, 10, -2):
        assert call(level=level) == KMP_ERR_ARG
    assert call(flags=2) == KMP_ERR_ARG and b"unknown flag" in lib.kmp_last_error()
    assert call(bb=0) == KMP_ERR_ARG and call(bb=65281) == KMP_ERR_ARG
    assert b"block_bytes" in lib.kmp_last_error()
    assert call(b=small, bb=4097) == KMP_ERR_CAPACITY                       # above the context's max_slice_bytes
    assert call(b=small, bb=256) == KMP_ERR_CAPACITY                        # 48 blocks on a context of 8 slices
    assert call(dcap=cap - 1) == KMP_ERR_CAPACITY and call(sbytes=need - 1) == KMP_ERR_CAPACITY
    for null in ("src_p", "dst_p", "scr_p", "res_p"):
        assert call(**{null: None}) == KMP_ERR_ARG
    assert lib.kmp_bgzf_compress(None, _vp(src), len(data), 4096, 6, 0, _vp(dst), cap, _vp(scratch), need, _vp(res), None) == KMP_ERR_ARG
    assert call(scr_p=_vp(scratch, 4), sbytes=need) == KMP_ERR_ARG           # alignment
    h = ctypes.c_void_p()
    assert lib.kmp_bgzf_open(None, _vp(dst), 28, ctypes.byref(h), None) == KMP_ERR_ARG
    assert lib.kmp_bgzf_open(big._h, None, 28, ctypes.byref(h), None) == KMP_ERR_ARG
    assert lib.kmp_bgzf_open(big._h, _vp(dst), 28, None, None) == KMP_ERR_ARG
    assert lib.kmp_bgzf_stat_of(None, None) == KMP_ERR_ARG
    with pytest.raises(ValueError):
        big.compress_bgzf(src, block_bytes=65281)
    torch.cuda.synchronize()
    assert big.status() == (0, 0)


# ------------------------------------------------------------------------------------------------------ open and read ----
def _check_reads(b, blob_t, data, ranges, verify, co, mo):
    r = b.open_bgzf(blob_t)
    try:
        assert r.status == 0 and r.content_size == len(data)
        for lo, hi in ranges:
            got = r.read(lo, hi, verify=verify).cpu().numpy().tobytes()
            assert got == data[lo:min(hi, len(data))] if lo < len(data) else got == b"", (lo, hi)
            if lo < min(hi, len(data)):
                dst, skip, status = r.read_blocks(lo, hi, verify)
                i = bisect.bisect_right(co, lo) - 1
                assert skip == lo - co[i], (lo, hi, skip)
                first = ctypes.c_uint32(99)
                assert status.numel() == b.lib.kmp_bgzf_read_blocks(r._h, lo, hi, ctypes.byref(first)) and not status.any() and first.value == i
                assert r.tell(lo) == (mo[i] << 16) | (lo - co[i])
        assert r.tell(len(data)) == blob_t.numel() << 16
        with pytest.raises(ValueError):
            r.tell(len(data) + 1)
        return r
    finally:
        r.close()


@pytest.mark.parametrize("name", ["size12305", "b65280", "blocks300", "size1", "stored65280"])
@pytest.mark.parametrize("verify", [True, False])
def test_reads_of_own_containers_at_member_edges(big, name, verify):
    g = hb.golden_case(name)
    data = hb.case_input(g["cls"], g["seed"], g["size"])
    blob = big.compress_bgzf(_dev(data), block_bytes=g["block_bytes"], level=g["level"])
    _, mo, co, *_ = hb.walk_reference(blob.cpu().numpy().tobytes())
    starts = list(range(0, len(data), g["block_bytes"]))
    ranges = hs.edge_ranges(len(data), starts)
    if name == "blocks300":
        ranges = ranges[:1] + ranges[-40:]
    r = _check_reads(big, blob, data, ranges, verify, co, mo)
    assert (r.blocks, int(r.stat.flags), int(r.stat.max_block), int(r.stat.max_compressed)) == (len(starts) + 1, 1, min(len(data), g["block_bytes"]), max(g["members"]))


def test_read_between_canaries(big):
    """kmp_bgzf_read through the C ABI: d_dst of exactly read_bound bytes and d_status of exactly the covering members, between canaries"""
    g = hb.golden_case("size12305")
    data = hb.case_input(g["cls"], g["seed"], g["size"])
    blob = big.compress_bgzf(_dev(data), block_bytes=4096)
    lib = big.lib
    h = ctypes.c_void_p()
    assert lib.kmp_bgzf_open(big._h, _vp(blob), blob.numel(), ctypes.byref(h), big._stream()) == 0
    st = _lib.BgzfStat()
    assert lib.kmp_bgzf_stat_of(h, ctypes.byref(st)) == 0
    assert (st.status, st.blocks, st.content, st.max_block, st.flags, st.max_compressed) == (0, 5, 12305, 4096, 1, max(g["members"]))
    lo, hi = 4095, 8193
    need = lib.kmp_bgzf_read_bound(h, lo, hi); first = ctypes.c_uint32(99)
    m = lib.kmp_bgzf_read_blocks(h, lo, hi, ctypes.byref(first))
    assert (need, m, first.value) == (3 * 4096, 3, 0)
    rng = np.random.default_rng(5)
    can = rng.integers(0, 256, 2 * MARGIN + 3 + need, dtype=np.uint8); scan = rng.integers(1, 256, 64, dtype=np.uint8)
    dst = torch.from_numpy(can.copy()).cuda(); status = torch.from_numpy(scan.copy()).cuda()
    skip = ctypes.c_uint64(77)
    assert lib.kmp_bgzf_read(h, _vp(blob), lo, hi, 1, _vp(dst, MARGIN + 3), need - 1, ctypes.byref(skip), _vp(status, 16), big._stream()) == KMP_ERR_CAPACITY
    assert lib.kmp_bgzf_read(h, _vp(blob), lo, hi, 1, _vp(dst, MARGIN + 3), need, ctypes.byref(skip), _vp(status, 16), big._stream()) == 0
    torch.cuda.synchronize()
    d, s = dst.cpu().numpy(), status.cpu().numpy()
    at = MARGIN + 3
    assert np.array_equal(d[:at], can[:at]) and np.array_equal(d[at + need:], can[at + need:]), "bytes around d_dst changed"
    assert d[at:at + need].tobytes() == data[:need] and skip.value == lo
    assert np.array_equal(s[:16], scan[:16]) and np.array_equal(s[28:], scan[28:]) and not s[16:28].any()
    # an empty range and one past the end: KMP_OK, nothing written, no pointer needed
    for a, z in ((5, 5), (12305, 20000), (9, 3)):
        assert lib.kmp_bgzf_read(h, None, a, z, 1, None, 0, ctypes.byref(skip), None, big._stream()) == 0 and skip.value == 0
        assert lib.kmp_bgzf_read_bound(h, a, z) == 0
    lib.kmp_bgzf_close(h)


@pytest.mark.parametrize("row", hb.blobs("foreign"), ids=lambda r: r["name"])
def test_foreign_blobs(big, row):
    data = row["content"]
    blob = _dev(row["blob"], 1)
    _, mo, co, *_ = hb.walk_reference(row["blob"])
    for verify in (True, False):
        r = _check_reads(big, blob, data, hs.edge_ranges(len(data), co[:-1]), verify, co, mo)
        got = np.zeros(1, dtype=hb.STAT); ctypes.memmove(got.ctypes.data, ctypes.byref(r.stat), 32)
        assert got[0].tobytes() == hb.expected_stat(row).tobytes(), got


@pytest.mark.parametrize("row", hb.blobs("damaged"), ids=lambda r: r["name"])
def test_damaged_blobs_are_refused(big, row):
    """the blob in a device buffer of exactly its length (the allocator's granule apart); the status is the fixture's, reads are refused"""
    blob = _dev(row["blob"])
    r = big.open_bgzf(blob)
    assert r.status == row["stat"]["status"] and r.status in (-3, -5)
    assert (r.blocks, r.content_size, int(r.stat.max_block), int(r.stat.max_compressed), int(r.stat.flags)) == (0, 0, 0, 0, 0)
    skip = ctypes.c_uint64()
    spare = torch.zeros(64, dtype=torch.uint8, device="cuda")
    assert big.lib.kmp_bgzf_read(r._h, _vp(spare), 0, 1, 1, _vp(spare), 1, ctypes.byref(skip), _vp(spare), big._stream()) == KMP_ERR_ARG
    assert big.lib.kmp_bgzf_read_bound(r._h, 0, 1) == 0
    with pytest.raises(RuntimeError):
        r.read(0, 1)
    r.close()
    torch.cuda.synchronize()


@pytest.mark.parametrize("row", hb.blobs("wrong"), ids=lambda r: r["name"])
def test_wrong_trailers_give_minus_3_on_exactly_that_member(big, row):
    blob = _dev(row["blob"])
    r = big.open_bgzf(blob)
    assert r.status == 0
    assert r.blocks == 5
    want = [-3 if i == row["bad_member"] else 0 for i in range(4)]              # (the marker covers no content: it is not read)
    dst, skip, status = r.read_blocks(0, r.content_size, verify=True)
    assert status.tolist() == want and skip == 0
    _, _, co, *_ = hb.walk_reference(row["blob"])
    got = dst.cpu().numpy().tobytes()
    for i in range(4):
        assert got[co[i]:co[i] + 100] == row["content"][100 * i:100 * (i + 1)], "the decoded members must be intact"
    _, _, status = r.read_blocks(0, r.content_size, verify=False)
    assert status.tolist() == (want if row["name"] == "flipped_isize" else [0] * 4)
    with pytest.raises(RuntimeError, match="-3"):
        r.read_all()
    assert r.read(0, 50).cpu().numpy().tobytes() == row["content"][:50]       # a range the wrong member does not cover
    r.close()


def _same_as_host_index(b, blob_bytes, blob_t):
    """the device open against kmp_bgzf_index_host: the stat, and every member's start in the blob and in the content (tell at each
    member's first byte; read_blocks for the index)"""
    raw = np.frombuffer(blob_bytes, dtype=np.uint8)
    st = np.zeros(1, dtype=hb.STAT)
    assert b.lib.kmp_bgzf_index_host(raw.ctypes.data, len(raw), st.ctypes.data, None, None, 0) == 0
    n = int(st[0]["blocks"])
    mo = np.zeros(n + 1, dtype=np.uint64); co = np.zeros(n + 1, dtype=np.uint64)
    assert b.lib.kmp_bgzf_index_host(raw.ctypes.data, len(raw), st.ctypes.data, mo.ctypes.data, co.ctypes.data, n + 1) == 0
    r = b.open_bgzf(blob_t)
    got = np.zeros(1, dtype=hb.STAT); ctypes.memmove(got.ctypes.data, ctypes.byref(r.stat), 32)
    assert got[0].tobytes() == st[0].tobytes(), (got, st)
    return r, mo, co


def test_open_of_5000_members_equals_the_host_index(big):
    blob, content = hb.many_members(5000)
    t = _dev(blob)
    r, mo, co = _same_as_host_index(big, blob, t)
    assert r.blocks == 5000 and r.content_size == len(content)
    lib = big.lib
    first = ctypes.c_uint32()
    for i in list(range(0, 5000, 37)) + [4999]:
        if co[i + 1] > co[i]:                                   # a member with content: its first byte
            assert lib.kmp_bgzf_tell(r._h, int(co[i])) == (int(mo[i]) << 16)
            assert lib.kmp_bgzf_read_blocks(r._h, int(co[i]), int(co[i]) + 1, ctypes.byref(first)) == 1 and first.value == i
    assert r.read_all().cpu().numpy().tobytes() == content          # 5 000 members on a context of 512: ten rounds
    r.close()


def test_more_candidates_than_the_cap_take_the_serial_walk(big):
    """(1 << 20) + 1 markers, 28 MiB: one candidate more than the parallel open takes"""
    n = (1 << 20) + 1
    t = torch.from_numpy(np.frombuffer(hb.EOF, dtype=np.uint8).copy()).cuda().repeat(n)
    r = big.open_bgzf(t)
    assert (r.status, r.blocks, r.content_size, int(r.stat.flags), int(r.stat.max_compressed), int(r.stat.max_block)) == (0, n, 0, 1, 28, 0)
    assert big.lib.kmp_bgzf_tell(r._h, 0) == (28 * n) << 16 and big.lib.kmp_bgzf_read_bound(r._h, 0, 1) == 0
    r.close()
    raw = t[:28 * 1000].cpu().numpy()
    st = np.zeros(1, dtype=hb.STAT)
    assert big.lib.kmp_bgzf_index_host(raw.ctypes.data, len(raw), st.ctypes.data, None, None, 0) == 0 and int(st[0]["blocks"]) == 1000
    # one marker fewer: the parallel open, the same answer
    r = big.open_bgzf(t[:28 * (n - 1)])
    assert (r.status, r.blocks, r.content_size, int(r.stat.flags)) == (0, n - 1, 0, 1)
    r.close()


def test_more_covering_members_than_the_context_holds_go_through_in_rounds(big, small):
    g = hb.golden_case("blocks300")
    data = hb.case_input(g["cls"], g["seed"], g["size"])
    blob = big.compress_bgzf(_dev(data), block_bytes=64)
    r = small.open_bgzf(blob)                   # 8 slices: 300 members are 38 rounds
    assert r.blocks == 301
    for verify in (True, False):
        assert r.read_all(verify=verify).cpu().numpy().tobytes() == data
        assert r.read(63, 64 * 17 + 1, verify=verify).cpu().numpy().tobytes() == data[63:64 * 17 + 1]
    # a CRC damaged in the last round is found there
    bad = blob.clone(); bad[blob.numel() - 28 - 8] ^= 1
    rb = small.open_bgzf(bad)
    _, _, status = rb.read_blocks(0, len(data), verify=True)
    assert status.tolist() == [0] * 299 + [-3]
    rb.close(); r.close()
