"""The parts a batch context adds on first use are absent or complete: an allocation that fails part-way leaves the part absent
(kmp_batch_memory says so) and the next call builds it from nothing.  The ablation build's KMP_TEST_FAIL_PART=<code> fails the named
part once its allocations have been made, as a failing last allocation would (codes: kompressor_amd/csrc/kmp_internal.h KMP_PART_*).
Also: the kernel timings after a batch in pieces and after batches of other levels."""
import numpy as np
import pytest

import helpers
from kompressor_amd import corpus

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

KMP_ERR_HIP = -1
PART_DEFLATE_LAZY, PART_DEFLATE_FAST, PART_LAZY_LEVELS, PART_DICT, PART_FLAT_TABLES, PART_TABLES4 = 1, 2, 3, 4, 5, 6


def _device_batch(datas):
    lens = np.array([len(d) for d in datas], dtype=np.int32)
    offs = np.concatenate([[0], np.cumsum(lens[:-1].astype(np.int64))]).astype(np.int64)
    host = np.frombuffer(b"".join(datas) + bytes(64), dtype=np.uint8).copy()
    return torch.from_numpy(host).cuda(), torch.from_numpy(offs).cuda(), torch.from_numpy(lens).cuda()


def _frames(dst, ooff, olen):
    torch.cuda.synchronize()
    dd, oo, ol = dst.cpu().numpy(), ooff.cpu().numpy(), olen.cpu().numpy()
    return [dd[oo[i]:oo[i] + ol[i]].tobytes() for i in range(len(ol))]


def _fails_cleanly(monkeypatch, b, code, run, field):
    """run() with part `code` failing: a clean KMP_ERR_HIP, and memory()[field] as before the call (the part absent)."""
    before = b.memory()[field]
    monkeypatch.setenv("KMP_TEST_FAIL_PART", str(code))
    with pytest.raises(RuntimeError) as e:
        run()
    monkeypatch.delenv("KMP_TEST_FAIL_PART")
    assert f"({KMP_ERR_HIP})" in str(e.value) and "KMP_TEST_FAIL_PART" in str(e.value), str(e.value)
    assert b.memory()[field] == before, (field, b.memory(), before)


def test_failed_parts_leave_nothing_behind(monkeypatch):
    from kompressor_amd.batch import ZstdBatch
    o = helpers.oracle()
    n, S = 64, 65536
    host = corpus.make(7, n, S)
    datas = [host[i * S:(i + 1) * S].tobytes() for i in range(n)]
    src, off, lens = _device_batch(datas)
    b = ZstdBatch(max_slices=256, max_slice_bytes=S, ablations=True)
    try:
        # level 4's tables (slices above 16 KiB: the double-fast parse)
        _fails_cleanly(monkeypatch, b, PART_TABLES4, lambda: b.compress(src, off, lens, level=4), "other_tables")
        assert _frames(*b.compress(src, off, lens, level=4)) == [o.compress_level(d, 4) for d in datas]
        # levels 5 .. 10
        b2 = ZstdBatch(max_slices=256, max_slice_bytes=S, ablations=True)
        try:
            _fails_cleanly(monkeypatch, b2, PART_LAZY_LEVELS, lambda: b2.compress(src, off, lens, level=5), "other_tables")
            assert _frames(*b2.compress(src, off, lens, level=5)) == [o.compress_lazy(d, 5) for d in datas]
        finally:
            b2.close()
        # dictionaries: A is built, building B fails and leaves no dictionary behind (A's set is gone too), A again is built afresh
        dict_a, dict_b = corpus.make(99, 1, 16384).tobytes(), corpus.make(98, 1, 8192).tobytes()
        no_dict = b.memory()["other_tables"]
        assert _frames(*b.compress(src, off, lens, dictionary=dict_a)) == [o.compress_dict(d, dict_a)[0] for d in datas]
        assert b.memory()["other_tables"] > no_dict
        monkeypatch.setenv("KMP_TEST_FAIL_PART", str(PART_DICT))
        with pytest.raises(RuntimeError, match=r"\(-1\).*KMP_TEST_FAIL_PART"):
            b.compress(src, off, lens, dictionary=dict_b)
        monkeypatch.delenv("KMP_TEST_FAIL_PART")
        assert b.memory()["other_tables"] == no_dict
        assert _frames(*b.compress(src, off, lens, dictionary=dict_a)) == [o.compress_dict(d, dict_a)[0] for d in datas]
        # the DEFLATE workspace of levels 4 .. 9
        D = helpers.deflate_oracle()
        _fails_cleanly(monkeypatch, b, PART_DEFLATE_LAZY, lambda: b.deflate(src, off, lens), "deflate_workspace")
        assert _frames(*b.deflate(src, off, lens)) == [D.compress(d) for d in datas]
    finally:
        b.close()


def test_failed_flat_tables_leave_nothing_behind(monkeypatch):
    """Levels 1 / 2 get tables of their own when the level-3 tables are spread over the arena (4 GiB of tables or more)."""
    from kompressor_amd.batch import ZstdBatch
    o = helpers.oracle()
    n, S = 64, 65536
    host = corpus.make(11, n, S)
    datas = [host[i * S:(i + 1) * S].tobytes() for i in range(n)]
    src, off, lens = _device_batch(datas)
    b = ZstdBatch(max_slices=16384, max_slice_bytes=S, ablations=True, table_span_gib=0)
    try:
        assert b.memory()["arena"] > 0
        _fails_cleanly(monkeypatch, b, PART_FLAT_TABLES, lambda: b.compress(src, off, lens, level=1), "other_tables")
        assert _frames(*b.compress(src, off, lens, level=1)) == [o.compress_level(d, 1) for d in datas]
        assert b.memory()["other_tables"] > 0
    finally:
        b.close()


def test_failed_deflate_fast_workspace_falls_back(monkeypatch):
    """The wide workspace of DEFLATE levels 1 .. 3 is optional: when it cannot be made the levels run in pieces over the workspace of
    the lazy levels, and it is not tried again."""
    from kompressor_amd.batch import ZstdBatch
    D = helpers.deflate_oracle()
    n, S = 300, 65536
    host = corpus.make(5, n, S)
    datas = [host[i * S:(i + 1) * S].tobytes() for i in range(n)]
    src, off, lens = _device_batch(datas)
    want = [D.compress(d, level=1) for d in datas]
    monkeypatch.setenv("KMP_DEFLATE_CHUNK", "64")          # (the wide workspace is made for contexts of more than two halves)
    grows, falls = ZstdBatch(max_slices=n, max_slice_bytes=S, ablations=True), ZstdBatch(max_slices=n, max_slice_bytes=S, ablations=True)
    monkeypatch.delenv("KMP_DEFLATE_CHUNK")
    try:
        for b in (grows, falls):
            assert _frames(*b.deflate(src, off, lens)) == [D.compress(d) for d in datas]
        lazy = falls.memory()["deflate_workspace"]
        assert _frames(*grows.deflate(src, off, lens, level=1)) == want
        assert grows.memory()["deflate_workspace"] > lazy
        monkeypatch.setenv("KMP_TEST_FAIL_PART", str(PART_DEFLATE_FAST))
        frames = _frames(*falls.deflate(src, off, lens, level=1))
        monkeypatch.delenv("KMP_TEST_FAIL_PART")
        assert falls.memory()["deflate_workspace"] == lazy
        assert frames == want
        assert _frames(*falls.deflate(src, off, lens, level=1)) == want
        assert falls.memory()["deflate_workspace"] == lazy
    finally:
        grows.close()
        falls.close()


def test_timing_after_a_batch_in_pieces():
    """A batch in pieces has no per-chunk kernel timings: last_kernel_ms(0 / 1) says so, last_chunks() counts the pieces."""
    from kompressor_amd.batch import ZstdBatch
    n, S = 2048, 65536
    host = corpus.make(0, n, S)
    b = ZstdBatch(max_slices=n, max_slice_bytes=S, team_lanes=4)
    try:
        src = torch.from_numpy(host).cuda()
        in_off = torch.arange(n, dtype=torch.int64, device="cuda") * S
        in_len = torch.full((n,), S, dtype=torch.int32, device="cuda")
        b.set_profiling(True)
        ref, ooff, rlen = b.compress(src, in_off, in_len)
        torch.cuda.synchronize()
        assert b.last_kernel_ms(0) > 0 and b.last_kernel_ms(1) > 0
        want = _frames(ref, ooff, rlen)
        streams = [torch.cuda.Stream() for _ in range(8)]
        torch.cuda.synchronize()
        dst, olen = torch.zeros_like(ref), torch.zeros_like(rlen)
        b.compress_pieces(src, in_off, in_len, dst, ooff, olen, streams)
        for which in (0, 1):
            with pytest.raises(RuntimeError, match="no timing recorded"):
                b.last_kernel_ms(which)
        assert b.last_chunks() == 8
        # ... and after a batch of another level, which records no per-chunk timings either
        b.compress(src, in_off, in_len)
        torch.cuda.synchronize()
        assert b.last_kernel_ms(0) > 0
        b.compress(src[: 64 * S], in_off[:64], in_len[:64], level=1)
        with pytest.raises(RuntimeError, match="no timing recorded"):
            b.last_kernel_ms(0)
        torch.cuda.synchronize()
        assert _frames(dst, ooff, olen) == want
    finally:
        b.close()
