"""zstd's seekable container on the device (kmp_zstd_seekable_*: k_seekable_plan, k_seekable_xxh64, k_seekable_table, k_seekable_index):
the golden cases (tests/golden/zstd_seekable_golden.json: libzstd 1.5.7's frames, struct's table, xxhash's checksums) through the C ABI
between canaries and through ZstdBatch.compress_seekable; open / stat / read on the product's own containers and on foreign ones at ranges
around the frame edges; damaged tables; a flipped checksum; rounds; argument errors; the context's memory."""
import ctypes
import hashlib

import numpy as np
import pytest

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
    b = _ctx(max_slices=512, max_slice_bytes=131072)
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


def _compress_abi(b, data, fb, level, flags, src_offset=0):
    """kmp_zstd_seekable_compress with d_dst (at an odd address) and d_scratch between canaries -> (container bytes, result[2])"""
    lib = b.lib
    cap = lib.kmp_zstd_seekable_bound(len(data), fb, flags); need = lib.kmp_zstd_seekable_scratch(len(data), fb)
    assert cap >= 17 and need > 0
    rng = np.random.default_rng(11)
    dcan = rng.integers(0, 256, 2 * MARGIN + 1 + cap, dtype=np.uint8); scan = rng.integers(0, 256, 2 * MARGIN + need, dtype=np.uint8)
    dst = torch.from_numpy(dcan.copy()).cuda(); scratch = torch.from_numpy(scan.copy()).cuda()
    result = torch.full((2,), -1, dtype=torch.int64, device="cuda")
    src = _dev(data, src_offset)
    rc = lib.kmp_zstd_seekable_compress(b._h, _vp(src) if data else None, len(data), fb, level, flags, _vp(dst, MARGIN + 1), cap, _vp(scratch, MARGIN), need,
                                        _vp(result), b._stream())
    assert rc == 0, b._err()
    torch.cuda.synchronize()
    d, s, r = dst.cpu().numpy(), scratch.cpu().numpy(), [int(x) for x in result.cpu().numpy()]
    at = MARGIN + 1
    assert np.array_equal(d[:at], dcan[:at]) and np.array_equal(d[at + cap:], dcan[at + cap:]), "bytes around d_dst changed"
    assert np.array_equal(s[:MARGIN], scan[:MARGIN]) and np.array_equal(s[MARGIN + need:], scan[MARGIN + need:]), "bytes around d_scratch changed"
    assert 0 < r[0] <= cap
    assert np.array_equal(d[at + r[0]:at + cap], dcan[at + r[0]:at + cap]), "bytes of d_dst behind the container changed"
    return d[at:at + r[0]].tobytes(), r


# ------------------------------------------------------------------------------------------------------ compress ----
@pytest.mark.parametrize("case", hs.cases(), ids=lambda c: c[0])
def test_golden_container_through_the_c_abi_and_the_python_call(big, case):
    name, cls, seed, size, fb, level, sums, src_off = case
    g = hs.golden_case(name)
    data = hs.case_input(cls, seed, size)
    blob, result = _compress_abi(big, data, fb, level, sums, src_off)
    assert blob[len(blob) - len(g["table"]) // 2:].hex() == g["table"], "the seek table differs"
    assert len(blob) == g["length"] and hashlib.sha256(blob).hexdigest() == g["sha256"]
    assert result == [g["length"], 0]
    out = big.compress_seekable(_dev(data, src_off), frame_bytes=fb, level=level, checksums=bool(sums))
    assert out.numel() == g["length"] and hashlib.sha256(out.cpu().numpy().tobytes()).hexdigest() == g["sha256"]
    rc, bits = big.status()
    assert (rc, bits) == (0, 0)


def test_context_memory_is_unchanged(big):
    """kmp_batch_memory before and after a container is written, opened and read: equal (the context has compressed and decoded a batch
    before, so what those calls allocate on their first use is there)"""
    data = hs.case_input("T", 93000, 5 * 4096 + 1)
    src = _dev(data)
    io = torch.tensor([0, 4096], dtype=torch.int64, device="cuda"); il = torch.tensor([4096, 4096], dtype=torch.int32, device="cuda")
    dst, oo, ol = big.compress(src, io, il)
    big.decompress(dst, oo, ol, out_cap=il)
    torch.cuda.synchronize()
    before = big.memory()
    blob = big.compress_seekable(src, frame_bytes=4096, level=3)
    r = big.open_seekable(blob)
    assert r.read_all().cpu().numpy().tobytes() == data
    r.close()
    assert big.memory() == before


def test_argument_errors(big, small):
    lib = big.lib
    data = hs.case_input("T", 93001, 3 * 4096)
    src = _dev(data)
    cap = lib.kmp_zstd_seekable_bound(len(data), 4096, 1); need = lib.kmp_zstd_seekable_scratch(len(data), 4096)
    dst = torch.zeros(cap + 64, dtype=torch.uint8, device="cuda"); scratch = torch.zeros(need // 8 + 1, dtype=torch.int64, device="cuda")
    res = torch.zeros(2, dtype=torch.int64, device="cuda")

    def call(b=big, src_p=_vp(src), n=len(data), fb=4096, level=3, flags=1, dst_p=_vp(dst), dcap=cap, scr_p=_vp(scratch), sbytes=need, res_p=_vp(res)):
        return lib.kmp_zstd_seekable_compress(b._h, src_p, n, fb, level, flags, dst_p, dcap, scr_p, sbytes, res_p, b._stream())
    assert call() == 0
    for level in (9, 10, 11, -131073):
        assert call(level=level) == KMP_ERR_ARG
    assert call(fb=0) == KMP_ERR_ARG and call(fb=131073) == KMP_ERR_ARG and call(flags=2) == KMP_ERR_ARG
    assert lib.kmp_zstd_seekable_bound(100, 0, 0) == 0 and lib.kmp_zstd_seekable_scratch(100, 131073) == 0
    assert call(b=small, fb=4097) == KMP_ERR_CAPACITY                       # above the context's max_slice_bytes
    assert call(b=small, fb=256) == KMP_ERR_CAPACITY                        # 48 chunks on a context of 8 slices
    assert call(dcap=cap - 1) == KMP_ERR_CAPACITY and call(sbytes=need - 1) == KMP_ERR_CAPACITY
    for null in ("src_p", "dst_p", "scr_p", "res_p"):
        assert call(**{null: None}) == KMP_ERR_ARG
    assert lib.kmp_zstd_seekable_compress(None, _vp(src), len(data), 4096, 3, 1, _vp(dst), cap, _vp(scratch), need, _vp(res), None) == KMP_ERR_ARG
    assert call(scr_p=_vp(scratch, 4), sbytes=need) == KMP_ERR_ARG           # alignment
    h = ctypes.c_void_p()
    assert lib.kmp_zstd_seekable_open(None, _vp(dst), 17, ctypes.byref(h), None) == KMP_ERR_ARG
    assert lib.kmp_zstd_seekable_open(big._h, None, 17, ctypes.byref(h), None) == KMP_ERR_ARG
    assert lib.kmp_zstd_seekable_stat(None, None) == KMP_ERR_ARG
    assert lib.kmp_zstd_seekable_read_bound(None, 0, 1) == 0
    torch.cuda.synchronize()
    assert big.status() == (0, 0)


# ------------------------------------------------------------------------------------------------------ read ----
def _check_reads(b, blob_t, data, ranges, verify):
    r = b.open_seekable(blob_t)
    try:
        assert r.status == 0 and r.content_size == len(data)
        _, _, co = hs.parse_table(blob_t.cpu().numpy().tobytes())
        for lo, hi in ranges:
            got = r.read(lo, hi, verify=verify).cpu().numpy().tobytes()
            assert got == data[lo:min(hi, len(data))] if lo < len(data) else got == b"", (lo, hi)
            if lo < min(hi, len(data)):
                dst, skip, status = r.read_frames(lo, hi, verify)
                assert skip == lo - max(c for c in co if c <= lo), (lo, hi, skip)
                assert status.numel() == b.lib.kmp_zstd_seekable_read_frames(r._h, lo, hi, None) and not status.any()
        return r.frames, r.checksums
    finally:
        r.close()


@pytest.mark.parametrize("name", ["size12305", "f65536", "f96", "nosum", "tail7", "size1"])
@pytest.mark.parametrize("verify", [True, False])
def test_reads_of_own_containers_at_frame_edges(big, name, verify):
    g = hs.golden_case(name)
    data = hs.case_input(g["cls"], g["seed"], g["size"])
    blob = big.compress_seekable(_dev(data), frame_bytes=g["frame_bytes"], level=g["level"], checksums=bool(g["checksums"]))
    starts = list(range(0, len(data), g["frame_bytes"]))
    frames, sums = _check_reads(big, blob, data, hs.edge_ranges(len(data), starts), verify)
    assert frames == len(starts) and sums == bool(g["checksums"])


def test_read_between_canaries_and_stat(big):
    """kmp_zstd_seekable_read through the C ABI: d_dst of exactly read_bound bytes and d_status of exactly the covering frames, between
    canaries; stat against the table."""
    g = hs.golden_case("size12305")
    data = hs.case_input(g["cls"], g["seed"], g["size"])
    blob = big.compress_seekable(_dev(data), frame_bytes=4096, level=3)
    lib = big.lib
    h = ctypes.c_void_p()
    assert lib.kmp_zstd_seekable_open(big._h, _vp(blob), blob.numel(), ctypes.byref(h), big._stream()) == 0
    st = _lib.SeekableStat()
    assert lib.kmp_zstd_seekable_stat(h, ctypes.byref(st)) == 0
    assert (st.status, st.frames, st.content, st.max_frame, st.flags, st.table_off) == (0, 4, 12305, 4096, 1, blob.numel() - 17 - 48)
    lo, hi = 4095, 8193
    need = lib.kmp_zstd_seekable_read_bound(h, lo, hi); first = ctypes.c_uint32(99)
    m = lib.kmp_zstd_seekable_read_frames(h, lo, hi, ctypes.byref(first))
    assert (need, m, first.value) == (3 * 4096, 3, 0)
    rng = np.random.default_rng(5)
    can = rng.integers(0, 256, 2 * MARGIN + 3 + need, dtype=np.uint8); scan = rng.integers(0, 256, 64, dtype=np.uint8)
    dst = torch.from_numpy(can.copy()).cuda(); status = torch.from_numpy(scan.copy()).cuda()
    skip = ctypes.c_uint64(77)
    assert lib.kmp_zstd_seekable_read(h, _vp(blob), lo, hi, 1, _vp(dst, MARGIN + 3), need - 1, ctypes.byref(skip), _vp(status, 16), big._stream()) == KMP_ERR_CAPACITY
    assert lib.kmp_zstd_seekable_read(h, _vp(blob), lo, hi, 1, _vp(dst, MARGIN + 3), need, ctypes.byref(skip), _vp(status, 16), big._stream()) == 0
    torch.cuda.synchronize()
    d, s = dst.cpu().numpy(), status.cpu().numpy()
    at = MARGIN + 3
    assert np.array_equal(d[:at], can[:at]) and np.array_equal(d[at + need:], can[at + need:]), "bytes around d_dst changed"
    assert d[at:at + need].tobytes() == data[:need] and skip.value == lo
    assert np.array_equal(s[:16], scan[:16]) and np.array_equal(s[28:], scan[28:]) and not s[16:28].any()
    # an empty range and one past the end: KMP_OK, nothing written, no pointer needed
    for a, z in ((5, 5), (12305, 20000), (9, 3)):
        assert lib.kmp_zstd_seekable_read(h, None, a, z, 1, None, 0, ctypes.byref(skip), None, big._stream()) == 0 and skip.value == 0
        assert lib.kmp_zstd_seekable_read_bound(h, a, z) == 0
    lib.kmp_zstd_seekable_close(h)


@pytest.mark.parametrize("row", hs.blobs("foreign"), ids=lambda r: r["name"])
def test_foreign_containers(big, row):
    data = hs.case_input(row["cls"], row["seed"], row["size"])
    blob = _dev(row["blob"], 1)
    _, _, co = hs.parse_table(row["blob"])
    for verify in (True, False):
        frames, sums = _check_reads(big, blob, data, hs.edge_ranges(len(data), co[:-1]), verify)
        assert frames == row["stat"]["frames"] and sums == bool(row["stat"]["flags"])
    host = np.zeros(1, dtype=hs.STAT)
    raw = np.frombuffer(row["blob"], dtype=np.uint8).copy()
    assert big.lib.kmp_zstd_seekable_index_host(raw.ctypes.data, len(raw), host.ctypes.data, None, None, 0) == 0
    assert host[0].tobytes() == hs.expected_stat(row).tobytes()


@pytest.mark.parametrize("row", hs.blobs("damaged"), ids=lambda r: r["name"])
def test_damaged_containers_are_refused(big, row):
    """the blob in a device buffer of exactly its length (the allocator's granule apart); the status is the fixture's, reads are refused"""
    blob = _dev(row["blob"])
    r = big.open_seekable(blob)
    assert r.status == row["stat"]["status"] and r.status in (10, 20) and (r.frames, r.content_size) == (0, 0)
    skip = ctypes.c_uint64()
    assert big.lib.kmp_zstd_seekable_read(r._h, _vp(blob), 0, 1, 1, _vp(blob), 1, ctypes.byref(skip), _vp(blob), big._stream()) == KMP_ERR_ARG
    with pytest.raises(RuntimeError):
        r.read(0, 1)
    r.close()
    torch.cuda.synchronize()


def test_flipped_checksum_gives_22_on_exactly_that_frame(big):
    row = hs.blobs("flipped")[0]
    data = hs.case_input(row["cls"], row["seed"], row["size"])
    blob = _dev(row["blob"])
    r = big.open_seekable(blob)
    assert r.status == 0 and r.checksums
    dst, skip, status = r.read_frames(0, len(data), verify=True)
    assert status.tolist() == [22 if i == row["bad_frame"] else 0 for i in range(r.frames)] and skip == 0
    assert dst[:len(data)].cpu().numpy().tobytes() == data, "the decoded frames must be intact"
    dst, skip, status = r.read_frames(0, len(data), verify=False)
    assert not status.any() and dst[:len(data)].cpu().numpy().tobytes() == data
    with pytest.raises(RuntimeError, match="22"):
        r.read_all()
    assert r.read(0, 1000).cpu().numpy().tobytes() == data[:1000]       # a range the damaged frame does not cover
    r.close()


def test_more_covering_frames_than_the_context_holds_go_through_in_rounds(big, small):
    g = hs.golden_case("chunks300")
    data = hs.case_input(g["cls"], g["seed"], g["size"])
    blob = big.compress_seekable(_dev(data), frame_bytes=64, level=3)
    r = small.open_seekable(blob)                   # 8 slices: 300 frames are 38 rounds
    assert r.frames == 300
    for verify in (True, False):
        assert r.read_all(verify=verify).cpu().numpy().tobytes() == data
        assert r.read(63, 64 * 17 + 1, verify=verify).cpu().numpy().tobytes() == data[63:64 * 17 + 1]
    # a checksum damaged in the last round is found there
    bad = blob.clone(); bad[blob.numel() - 9 - 2] ^= 1
    rb = small.open_seekable(bad)
    _, _, status = rb.read_frames(0, len(data), verify=True)
    assert status.tolist() == [0] * 299 + [22]
    rb.close(); r.close()
