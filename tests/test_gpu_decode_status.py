"""The decode side on the device against the status snapshot of tests/golden/decode_status_golden.json (taken on the CPU emulator at the
commit before the framing readers moved into kompressor_amd/csrc/zstd_format.h): ZstdBatch.decompress and frame_info over the seeded
cases, the entries packed back to back with no padding.  A batch of the first 255 runs k_zstd_decode alone; the batch of all cases
runs the two pre-decoders and, having 1024 entries and more, the slot sort in front of them.

(255 is below the library's KMP_PRE_MIN_BATCH of 256, but the suite's conftest sets that to 1 and the library reads it once per
process: what keeps the pre-decoders out of the first batch whatever ran before is the ablation build's KMP_DECODE_PRE = 0, as in
tests/test_gpu_layout.py.)"""
import zlib

import numpy as np
import pytest

import helpers_decode_status as hd
import helpers_frame_info as hf

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")


@pytest.fixture(scope="module")
def snapshot():
    g = hd.golden()
    return g, hd.checked_cases(g)


def _ctx(n, **kw):
    from kompressor_amd.batch import ZstdBatch
    assert torch.cuda.is_available(), "these tests need the MI355X"
    # slices of 128 KiB: the literal capacity the snapshot was taken with (128 KiB + 64), which decides between "corrupted" and "workspace"
    return ZstdBatch(max_slices=n, max_slice_bytes=128 * 1024, **kw)


@pytest.fixture(scope="module")
def ctx(snapshot):
    b = _ctx(len(snapshot[1]))
    yield b
    b.close()


def _decode(b, cs):
    src, offs, lens = hf.pack([e for _, e, _ in cs])
    caps = np.array([c for _, _, c in cs], dtype=np.int32)
    r = b.decompress(torch.from_numpy(src).cuda(), torch.from_numpy(offs.astype(np.int64)).cuda(), torch.from_numpy(lens.astype(np.int32)).cuda(),
                     out_cap=torch.from_numpy(caps).cuda())
    torch.cuda.synchronize()
    dd, oo, ol, st = (t.cpu().numpy() for t in r)
    return [[int(st[i]), int(ol[i]), zlib.crc32(dd[int(oo[i]):int(oo[i]) + int(ol[i])].tobytes())] for i in range(len(cs))]


def _differences(got, rows, column, commit):
    return [f"{w['name']}: {got[i]}, the snapshot of {commit[:7]} holds {w[column]} ({column})" for i, w in enumerate(rows) if got[i] != w[column]]


def test_decode_alone_answers_what_the_snapshot_holds(snapshot, monkeypatch):
    g, cs = snapshot
    monkeypatch.setenv("KMP_DECODE_PRE", "0")               # (a switch of the ablation build, read when the context is made)
    monkeypatch.delenv("KMP_PRE_MIN_BATCH", raising=False)
    b = _ctx(255, ablations=True)
    try:
        bad = _differences(_decode(b, cs[:255]), g["rows"][:255], "alone", g["commit"])
    finally:
        b.close()
    assert not bad, f"{len(bad)} differ\n" + "\n".join(bad[:20])


def test_decode_behind_the_predecoders_answers_what_the_snapshot_holds(ctx, snapshot):
    g, cs = snapshot
    assert len(cs) >= 1024                                  # (the slot sort is on)
    bad = _differences(_decode(ctx, cs), g["rows"], "pre", g["commit"])
    assert not bad, f"{len(bad)} differ\n" + "\n".join(bad[:20])


def test_frame_info_answers_what_the_snapshot_holds(ctx, snapshot):
    g, cs = snapshot
    src, offs, lens = hf.pack([e for _, e, _ in cs])
    info = ctx.frame_info(torch.from_numpy(src).cuda(), torch.from_numpy(offs.astype(np.int64)).cuda(), torch.from_numpy(lens.astype(np.int32)).cuda())
    torch.cuda.synchronize()
    cols = {f: info[f].cpu().numpy() for f in hf.FIELDS}
    # (the tensors are signed: ~0 reads -1)
    got = [[int(cols[f][i]) & ((1 << 64) - 1 if f in ("content", "bound") else 0xFFFFFFFF) for f in hf.FIELDS] for i in range(len(cs))]
    bad = _differences(got, g["rows"], "info", g["commit"])
    assert not bad, f"{len(bad)} differ\n" + "\n".join(bad[:20])
