"""Entropy sweeps beside the level-3 parse (kmp_batch.hip zstd_compress_dfast) through the public batch call: the
frames must be what the plain path writes and what libzstd 1.5.7 writes, whatever the sweeps found finished when they ran.  The
ablation build reads the two knobs from the environment when a context is created; KMP_ENTROPY_SWEEP_MIN=0 lets small batches take
the path, team width 4 is the width it is built for."""
import os
import random

import numpy as np
import pytest

import helpers
from kompressor_amd import corpus

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

LENGTHS = (0, 1, 7, 8, 9, 4096, 65536)
MAX_N = 257
_CTX = {}


@pytest.fixture(scope="module")
def pool():
    row = next(r for r in helpers.golden()["config1"] if r[1] == "T")
    text = corpus.make(row[0], 1, 65536).tobytes()
    noise = random.Random(4242).randbytes(65536)
    return [src[:n] for n in LENGTHS for src in (bytes(65536), noise, text)]          # the last one: 64 KiB of text


@pytest.fixture(scope="module")
def contexts():
    """context(K): one context of the ablation build per K, created with the knobs in the environment (0: sweeps off)"""
    from kompressor_amd.batch import ZstdBatch

    def get(K):
        if K not in _CTX:
            old = {k: os.environ.get(k) for k in ("KMP_ENTROPY_SWEEPS", "KMP_ENTROPY_SWEEP_MIN")}
            os.environ["KMP_ENTROPY_SWEEPS"] = str(K)
            os.environ["KMP_ENTROPY_SWEEP_MIN"] = "0"
            try:
                _CTX[K] = ZstdBatch(max_slices=MAX_N, max_slice_bytes=65536, team_lanes=4, ablations=True)
                _CTX[K].set_profiling(True)
            finally:
                for k, v in old.items():
                    if v is None:
                        os.environ.pop(k, None)
                    else:
                        os.environ[k] = v
        return _CTX[K]

    yield get
    for b in _CTX.values():
        b.close()
    _CTX.clear()


def slices(pool, n):
    return [pool[(i + len(pool) - 1) % len(pool)] for i in range(n)]


def upload(datas):
    lens = np.array([len(d) for d in datas], dtype=np.int32)
    offs = np.concatenate([[0], np.cumsum(lens[:-1].astype(np.int64))]).astype(np.int64)
    host = np.frombuffer(b"".join(datas) + bytes(64), dtype=np.uint8).copy()
    return torch.from_numpy(host).cuda(), torch.from_numpy(offs).cuda(), torch.from_numpy(lens).cuda()


def frames_of(res, n):
    dst, ooff, olen = (t.cpu().numpy() for t in res)
    return [dst[ooff[i]:ooff[i] + olen[i]].tobytes() for i in range(n)]


@pytest.fixture(scope="module")
def reference(pool):
    """libzstd 1.5.7's level-3 frame of every slice of the pool, computed once"""
    z = helpers.require_live_libzstd()
    return {d: z.compress(d) for d in pool}


@pytest.mark.parametrize("K", [1, 3, 8])
@pytest.mark.parametrize("n", [1, 63, 64, 65, 257])
def test_sweeps_write_the_plain_frames(pool, contexts, reference, n, K):
    datas = slices(pool, n)
    dev = upload(datas)
    got = contexts(K).compress(*dev, check=True)
    sweeps = contexts(K).last_sweeps()
    want = contexts(0).compress(*dev, check=True)
    assert contexts(0).last_sweeps() == []
    torch.cuda.synchronize()
    # K - 1 thresholds j n / K without zeros and duplicates, and the final sweep; every slice coded by exactly one of them
    assert len(sweeps) == len({j * n // K for j in range(1, K)} - {0}) + 1 and sum(sweeps) == n, sweeps
    assert torch.equal(got[2], want[2])
    f = frames_of(got, n)
    assert f == frames_of(want, n)
    assert f == [reference[d] for d in datas]


def test_three_batches_in_a_row_on_another_stream(pool, contexts, reference):
    b = contexts(3)
    st = torch.cuda.Stream()
    res = []
    with torch.cuda.stream(st):
        for n in (257, 63, 65):                   # nothing waits in between: each batch's clears must stay behind the one before
            datas = slices(pool, n)[::-1]
            dev = upload(datas)
            res.append((datas, b.compress(*dev), dev))
    st.synchronize()
    for datas, r, _ in res:
        assert frames_of(r, len(datas)) == [reference[d] for d in datas]
    assert b.status() == (0, 0)


def test_other_paths_after_an_overlapped_batch(pool, contexts, reference):
    z = helpers.require_live_libzstd(report=False)
    b = contexts(8)
    n = MAX_N
    datas = slices(pool, n)
    src, off, ln = upload(datas)
    first = b.compress(src, off, ln)
    assert len(b.last_sweeps()) == 8
    # the same batch in two pieces, each on a stream of its own
    dst = torch.empty(n * b.out_stride + 64, dtype=torch.uint8, device="cuda")
    ooff = torch.arange(n, dtype=torch.int64, device="cuda") * b.out_stride
    olen = torch.zeros(n, dtype=torch.int32, device="cuda")
    streams = [torch.cuda.Stream(), torch.cuda.Stream()]
    for s in streams:
        s.wait_stream(torch.cuda.current_stream())
    b.compress_pieces(src, off, ln, dst, ooff, olen, streams)
    for s in streams:
        s.synchronize()
    assert frames_of((dst, ooff, olen), n) == [reference[d] for d in datas]
    # level 4 (its own tables and, up to 16 KiB, another parser)
    l4 = b.compress(src, off, ln, level=4)
    torch.cuda.synchronize()
    assert b.last_sweeps() == []
    assert frames_of(l4, n) == [z.compress(d, 4) for d in datas]
    assert frames_of(first, n) == [reference[d] for d in datas]
    assert b.status() == (0, 0)
