"""zstd levels 5 .. 10 for slices of 128 KiB + 1 .. 2 MiB on the GPU (kmp_zstd_compress_batch_level on a context created for slices above
128 KiB; k_zstd_lazy_big): frames equal to libzstd 1.5.7's -- the golden files, the oracle, the machine's own library --, the classes that
stay refused, a hostile layout, tables between batches, the workspace in pieces, the streaming entry point and the new part's failure."""
import ctypes
import random

import numpy as np
import pytest

import helpers
import helpers_lazy_big as hl
from kompressor_amd import corpus

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

KMP_ERR_HIP = -1
PART_LAZY_BIG = 11          # kompressor_amd/csrc/kmp_internal.h KMP_PART_LAZY_BIG


def _compress(b, datas, level):
    """-> (frames, status bits)"""
    lens = np.array([len(d) for d in datas], dtype=np.int32)
    offs = np.concatenate([[0], np.cumsum(lens[:-1].astype(np.int64))]).astype(np.int64)
    host = np.frombuffer(b"".join(datas) + bytes(64), dtype=np.uint8).copy()
    dst, ooff, olen = b.compress(torch.from_numpy(host).cuda(), torch.from_numpy(offs).cuda(), torch.from_numpy(lens).cuda(), level=level)
    _, bits = b.status()
    dd, oo, ol = dst.cpu().numpy(), ooff.cpu().numpy(), olen.cpu().numpy()
    return [dd[oo[i]:oo[i] + ol[i]].tobytes() for i in range(len(datas))], bits


def _decompress(b, frames, caps):
    n = len(frames)
    lens = np.array([len(f) for f in frames], dtype=np.int32)
    offs = np.concatenate([[0], np.cumsum(lens[:-1].astype(np.int64))]).astype(np.int64)
    host = np.frombuffer(b"".join(frames) + bytes(64), dtype=np.uint8).copy()
    dst, ooff, olen, st = b.decompress(torch.from_numpy(host).cuda(), torch.from_numpy(offs).cuda(), torch.from_numpy(lens).cuda(),
                                       torch.tensor(caps, dtype=torch.int32).cuda())
    torch.cuda.synchronize()
    dd, oo, ol = dst.cpu().numpy(), ooff.cpu().numpy(), olen.cpu().numpy()
    return [dd[oo[i]:oo[i] + ol[i]].tobytes() for i in range(n)], [int(x) for x in st.cpu().numpy()]


@pytest.fixture(scope="module")
def inputs():
    return helpers.lazy_big_inputs()


@pytest.fixture(scope="module")
def batch():
    from kompressor_amd.batch import ZstdBatch
    b = ZstdBatch(max_slices=32, max_slice_bytes=2 << 20)
    yield b
    b.close()


@pytest.mark.parametrize("level", (5, 6, 7, 8, 9, 10))
def test_all_golden_inputs(batch, inputs, level):
    """All 23 inputs of tests/golden/zstd_lazy_big_golden.json in one batch: every frame is libzstd 1.5.7's (length and sha256), no status
    bit, and the frames decode back.  The (1 MiB + 5)-byte and the 2 MiB input are the windowLog 21 / hashLog 22 / 64-entry-row class."""
    rows = helpers.lazy_big_golden()["frames"][str(level)]
    assert len(rows) == len(inputs) == 23
    frames, bits = _compress(batch, inputs, level)
    assert bits == 0
    bad = [(i, len(d), len(f), flen) for i, (d, f, (flen, sha, _)) in enumerate(zip(inputs, frames, rows)) if [len(f), helpers.sha256(f)] != [flen, sha]]
    assert not bad, f"level {level}: (input, bytes, frame, libzstd's frame) {bad}"
    back, st = _decompress(batch, frames, [len(d) for d in inputs])
    assert st == [0] * len(inputs) and back == inputs


def test_short_tails_of_one_byte(batch):
    """helpers.rle_tail_cases(): a last block that is a short run of one byte is an RLE block whatever the parser found in it."""
    G = helpers.rle_tail_golden()["rows"]
    cases = helpers.rle_tail_cases()
    for level in (5, 7, 10):
        frames, bits = _compress(batch, [d for _, d in cases], level)
        assert bits == 0
        for (name, d), f in zip(cases, frames):
            assert [len(f), helpers.sha256(f)] == G[name][str(level)], (name, level)


@pytest.mark.parametrize("level", (5, 9))
def test_a_hostile_mixed_batch(inputs, level):
    """Every class in one batch on a context for slices of 4 MiB, in a permuted layout with odd input offsets, exact output slots and
    canaries: one-block slices, large ones, the refused classes (above 2 MiB; at level 9: 5 000 bytes)."""
    from kompressor_amd.batch import ZstdBatch
    big = corpus.make(65000, 1, (2 << 20) + 1, mix=ord("T")).tobytes()
    datas = [b"", inputs[0][:7], inputs[3][:5000], inputs[3][:16385], inputs[4][:131072], inputs[0], inputs[3], inputs[6], inputs[9], big]
    assert [len(d) for d in datas] == [0, 7, 5000, 16385, 131072, 131073, 200000, 262145, 700000, (2 << 20) + 1]
    L = hl.OddLayout(datas, seed=4100 + level)
    want = [hl.oracle_frame(d, level) for d in datas]
    refused = [i for i, w in enumerate(want) if w is None]
    assert refused == ([2, 9] if level == 9 else [9])
    b = ZstdBatch(max_slices=16, max_slice_bytes=4 << 20)
    try:
        dst = torch.from_numpy(L.canary.copy()).cuda()
        olen = torch.full((len(datas),), -1, dtype=torch.int32).cuda()
        b.compress(torch.from_numpy(L.src).cuda(), torch.from_numpy(L.in_off).cuda(), torch.from_numpy(L.in_len).cuda(),
                   dst=dst, out_off=torch.from_numpy(L.out_off).cuda(), out_len=olen, level=level)
        _, bits = b.status()
        dd, ol = dst.cpu().numpy(), olen.cpu().numpy()
    finally:
        b.close()
    assert bits & 4 and not bits & 3, bits
    assert [i for i in range(len(datas)) if ol[i] == 0] == refused
    assert not L.check(dd, ol)
    frames = L.frames(dd, ol)
    assert [i for i in range(len(datas)) if i not in refused and frames[i] != want[i]] == []


def test_one_context_several_batches(batch, inputs):
    """Level 10, then 5, then 3, then 7 over the same slices of one context: no batch sees the tables the one before left."""
    o = helpers.oracle()
    datas = [inputs[0], inputs[7], inputs[5], inputs[17]]
    for level in (10, 5, 3, 7):
        frames, bits = _compress(batch, datas, level)
        want = [o.compress_buffered(d, 2) if level == 3 else o.compress_lazy_big(d, level)[0] for d in datas]
        assert bits == 0 and frames == want, level


def test_more_slices_than_one_workspace_piece(monkeypatch, inputs):
    """KMP_LAZY_BIG_SLICES = 3 table slots for 8 slices: three pieces, the same frames as with a slot for every slice."""
    from kompressor_amd.batch import ZstdBatch
    rng = random.Random(4200)
    datas = [corpus.make(66000 + t, 1, rng.randrange(140000, 300001), mix=ord("TXSBDIZT"[t])).tobytes() for t in range(8)]
    frames = []
    for knob in (None, "3"):
        if knob:
            monkeypatch.setenv("KMP_LAZY_BIG_SLICES", knob)
        b = ZstdBatch(max_slices=8, max_slice_bytes=300000)
        try:
            f, bits = _compress(b, datas, 6)
            assert bits == 0
            frames.append(f)
            tables = b.memory()["other_tables"]
        finally:
            b.close()
            monkeypatch.delenv("KMP_LAZY_BIG_SLICES", raising=False)
        frames.append(tables)
    (whole, t_whole, pieces, t_pieces) = frames
    assert t_pieces < t_whole                                   # (fewer table slots were made)
    assert pieces == whole
    assert whole == [helpers.oracle().compress_lazy_big(d, 6)[0] for d in datas]


def test_the_streaming_entry_point(inputs):
    """kmp_zstd_compress_stream at level 6: 200 000 bytes in one closing call with room for kmp_zstd_compress_bound is compressed in place
    (ZSTD_compress2's frame); with the reference driver's 20 000-byte output slice libzstd stages the input, which stays refused."""
    from kompressor_amd import _lib
    lib = _lib.load()
    d = inputs[3]
    assert len(d) == 200000
    want = helpers.oracle().compress_lazy_big(d, 6)[0]
    for cap, served in ((lib.kmp_zstd_compress_bound(len(d)), True), (20000, False)):
        cctx = lib.kmp_zstd_create_cctx()
        try:
            assert lib.kmp_zstd_cctx_set_parameter(cctx, 100, 6) == 0
            obuf = ctypes.create_string_buffer(cap)
            dp, sp = ctypes.c_size_t(0), ctypes.c_size_t(0)
            r = lib.kmp_zstd_compress_stream(cctx, obuf, cap, ctypes.byref(dp), d, len(d), ctypes.byref(sp), 2)
            if served:
                assert r == 0 and sp.value == len(d) and obuf.raw[:dp.value] == want
            else:
                assert lib.kmp_zstd_is_error(r) and lib.kmp_zstd_get_error_name(r).decode() == "Unsupported parameter"
        finally:
            lib.kmp_zstd_free_cctx(cctx)


def test_against_the_machines_libzstd():
    """24 seeded slices of ragged sizes and mixed classes at levels 5, 8 and 10 against the binary library of this machine."""
    from kompressor_amd.batch import ZstdBatch
    z = helpers.require_live_libzstd()
    rng = random.Random(4300)
    datas = [corpus.make(67000 + t, 1, rng.randrange(131073, 600001), mix=ord("TXSBDIZR"[t % 8])).tobytes() for t in range(24)]
    b = ZstdBatch(max_slices=24, max_slice_bytes=600000)
    try:
        for level in (5, 8, 10):
            frames, bits = _compress(b, datas, level)
            assert bits == 0
            bad = [(i, len(d)) for i, (d, f) in enumerate(zip(datas, frames)) if f != z.compress(d, level)]
            assert not bad, (level, bad)
    finally:
        b.close()


def test_the_row_tables_part_fails_cleanly(monkeypatch, inputs):
    """The row tables are a part of their own (tests/test_gpu_parts.py): failing, it leaves nothing behind, and the next batch builds it."""
    from kompressor_amd.batch import ZstdBatch
    datas = [inputs[1], inputs[0][:30000], inputs[6]]
    lens = np.array([len(d) for d in datas], dtype=np.int32)
    offs = np.concatenate([[0], np.cumsum(lens[:-1].astype(np.int64))]).astype(np.int64)
    src = torch.from_numpy(np.frombuffer(b"".join(datas) + bytes(64), dtype=np.uint8).copy()).cuda()
    off, ln = torch.from_numpy(offs).cuda(), torch.from_numpy(lens).cuda()
    b = ZstdBatch(max_slices=4, max_slice_bytes=300000, ablations=True)
    try:
        before = b.memory()["other_tables"]
        monkeypatch.setenv("KMP_TEST_FAIL_PART", str(PART_LAZY_BIG))
        with pytest.raises(RuntimeError) as e:
            b.compress(src, off, ln, level=7)
        monkeypatch.delenv("KMP_TEST_FAIL_PART")
        assert f"({KMP_ERR_HIP})" in str(e.value) and "KMP_TEST_FAIL_PART" in str(e.value), str(e.value)
        assert b.memory()["other_tables"] == before, (b.memory(), before)
        frames, bits = _compress(b, datas, 7)
        assert bits == 0 and frames == [hl.oracle_frame(d, 7) for d in datas]
        assert b.memory()["other_tables"] > before
    finally:
        b.close()
