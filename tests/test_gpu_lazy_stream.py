"""zstd levels 5 .. 10 as streams and as the reference driver's staged frames on the GPU (kmp_zstd_compress_batch_stream_level,
kmp_zstd_compress_batch_reference, kmp_zstd_compress_stream; k_zstd_lazy_big_modes): frames equal to libzstd 1.5.7's -- the golden file
tests/golden/zstd_lazy_stream_golden.json and the machine's own library --, a hostile layout, the streaming entry point, ZstdCompressor fed
in pieces, the table part in pieces and after a change of slot size, and the one-shot path on the same context afterwards."""
import ctypes
import random

import numpy as np
import pytest

import helpers
import helpers_lazy_big as hl
import helpers_lazy_stream as hs
from kompressor_amd import corpus

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

KW = {"stream": dict(streaming="data"), "stream_empty_end": dict(streaming="empty"), "staged": dict(reference=True)}


def _compress(b, datas, level, **kw):
    """-> (frames, status bits)"""
    lens = np.array([len(d) for d in datas], dtype=np.int32)
    offs = np.concatenate([[0], np.cumsum(lens[:-1].astype(np.int64))]).astype(np.int64)
    host = np.frombuffer(b"".join(datas) + bytes(64), dtype=np.uint8).copy()
    dst, ooff, olen = b.compress(torch.from_numpy(host).cuda(), torch.from_numpy(offs).cuda(), torch.from_numpy(lens).cuda(), level=level, **kw)
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


def _sig(frames):
    return [[len(f), helpers.sha256(f)] for f in frames]


@pytest.fixture(scope="module")
def inputs():
    return dict(hs.inputs())


@pytest.fixture(scope="module")
def batch():
    from kompressor_amd.batch import ZstdBatch
    b = ZstdBatch(max_slices=32, max_slice_bytes=2 << 20)
    yield b
    b.close()


@pytest.mark.parametrize("level", hs.LEVELS)
def test_all_golden_rows(batch, inputs, level):
    """Every row of the golden file in its three framings, one batch each: no status bit, libzstd 1.5.7's frames (length and sha256), and
    the frames decode back on the GPU (the streaming ones carry no content size)."""
    rows = hs.golden()["frames"][str(level)]
    for framing, kw in KW.items():
        names = [k for k in rows if framing in rows[k]]
        assert len(names) == (19 if framing != "staged" else 11)
        datas = [inputs[k] for k in names]
        frames, bits = _compress(batch, datas, level, **kw)
        assert bits == 0, (framing, bits)
        bad = [(k, len(f), rows[k][framing][0]) for k, f in zip(names, frames) if [len(f), helpers.sha256(f)] != rows[k][framing]]
        assert not bad, f"level {level} {framing}: (input, frame, libzstd's frame) {bad}"
        back, st = _decompress(batch, frames, [max(len(d), 1) for d in datas])
        assert st == [0] * len(datas) and back == datas, framing


def test_hostile_layouts(inputs):
    """Level 7, a permuted layout with odd input offsets, exact output slots and canaries (helpers_lazy_big.OddLayout) on a context for
    slices of 4 MiB: a batch of streams of every length class, and a staged batch with one-block slices and a refused one."""
    from kompressor_amd.batch import ZstdBatch
    G = hs.golden()["frames"]["7"]
    big = inputs["D2097152"] + b"x"
    s_names = ["T0", "X1", "B7", "D5000", "T131072", "X131073", "S200000", "change_200000+200000"]
    g_names = ["X131073", "S200000", "change_200000+200000"]
    small = [b"", inputs["B7"], inputs["D5000"], inputs["S200000"][:100000]]
    cases = (("stream", [inputs[k] for k in s_names], [G[k]["stream"] for k in s_names], []),
             ("staged", small + [inputs[k] for k in g_names] + [big], _sig(hl.oracle_frame(d, 7) for d in small) + [G[k]["staged"] for k in g_names], [7]))
    b = ZstdBatch(max_slices=16, max_slice_bytes=4 << 20)
    try:
        for framing, datas, want, refused in cases:
            L = hl.OddLayout(datas, seed=5100 + len(datas))
            dst = torch.from_numpy(L.canary.copy()).cuda()
            olen = torch.full((len(datas),), -1, dtype=torch.int32).cuda()
            b.compress(torch.from_numpy(L.src).cuda(), torch.from_numpy(L.in_off).cuda(), torch.from_numpy(L.in_len).cuda(),
                       dst=dst, out_off=torch.from_numpy(L.out_off).cuda(), out_len=olen, level=7, **KW[framing])
            _, bits = b.status()
            dd, ol = dst.cpu().numpy(), olen.cpu().numpy()
            assert bits == (4 if refused else 0), (framing, bits)
            assert [i for i in range(len(datas)) if ol[i] == 0] == refused
            assert not L.check(dd, ol), framing
            frames = L.frames(dd, ol)
            assert _sig(f for i, f in enumerate(frames) if i not in refused) == want, framing
    finally:
        b.close()


def _stream_through_abi(lib, d, level, cuts, out_chunk=8192):
    """kmp_zstd_compress_stream as the reference's streaming callers drive ZSTD_compressStream2: d[cuts[i]:cuts[i+1]] with e_continue, the
    last piece with e_end, output drained through out_chunk-byte slices.  -> (frame, error name or None)"""
    cctx = lib.kmp_zstd_create_cctx()
    assert lib.kmp_zstd_cctx_set_parameter(cctx, 100, level) == 0
    out = bytearray(); obuf = ctypes.create_string_buffer(out_chunk)
    pieces = list(zip(cuts[:-1], cuts[1:]))
    try:
        for j, (a0, a1) in enumerate(pieces):
            end = j == len(pieces) - 1
            sp = ctypes.c_size_t(a0)
            while True:
                dp = ctypes.c_size_t(0)
                r = lib.kmp_zstd_compress_stream(cctx, obuf, out_chunk, ctypes.byref(dp), d, a1, ctypes.byref(sp), 2 if end else 0)
                if lib.kmp_zstd_is_error(r):
                    return bytes(out), lib.kmp_zstd_get_error_name(r).decode()
                out += obuf.raw[:dp.value]
                if (end and r == 0) or (not end and sp.value == a1 and dp.value < out_chunk):
                    break
    finally:
        lib.kmp_zstd_free_cctx(cctx)
    return bytes(out), None


@pytest.mark.parametrize("level", (6, 10))
def test_the_streaming_entry_point(inputs, level):
    """kmp_zstd_compress_stream: 300 000 bytes in three e_continue calls and an e_end call with data, then the same closed by an e_end
    call without data, through output slices of 8 192 bytes; a stream of 3 MiB is refused when it closes."""
    from kompressor_amd import _lib
    lib = _lib.load()
    name = "change_100000+100000+100000"
    d = inputs[name]
    row = hs.golden()["frames"][str(level)][name]
    cuts = [0, 70000, 150001, 230000, 300000]
    for framing, cc in (("stream", cuts), ("stream_empty_end", cuts + [300000])):
        frame, err = _stream_through_abi(lib, d, level, cc)
        assert err is None, err
        assert [len(frame), helpers.sha256(frame)] == row[framing], (level, framing)
    if level == 6:
        big = corpus.make(75000, 1, 3 << 20, mix=ord("T")).tobytes()
        _, err = _stream_through_abi(lib, big, 6, [0, 1 << 20, 2 << 20, 3 << 20])
        assert err == "Unsupported parameter"


def _transform_pieces(t, d, cuts, out_chunk=8192):
    """A SliceTransform fed d[cuts[i]:cuts[i+1]] with finish = false, the last piece with finish = true."""
    from kompressor_amd.slice_transform import ByteArraySlice
    out = bytearray()
    pieces = list(zip(cuts[:-1], cuts[1:]))
    for j, (a0, a1) in enumerate(pieces):
        inp = ByteArraySlice(bytearray(d[a0:a1]))
        while True:
            o = ByteArraySlice(out_chunk)
            t.transform(inp, o, j == len(pieces) - 1)
            out += o.data[o.read_start:o.write_start]
            if not (inp.has_data or o.insufficient):
                break
    return bytes(out)


def test_zstd_compressor_fed_in_pieces(inputs):
    """ZstdCompressor(compression_level=8) fed finish = false pieces: the live library's streaming frame under the same calls (and the
    golden one), and ZstdDecompressor gives the input back."""
    from kompressor_amd import ZstdCompressor, ZstdDecompressor
    z = helpers.require_live_libzstd()
    d = inputs["S200000"]
    cuts = [0, 1, 65536, 131072, 199999, 200000]
    frame = _transform_pieces(ZstdCompressor(compression_level=8), d, cuts)
    assert frame == z.compress_streaming(d, cuts, out_chunk=8192, level=8)
    assert [len(frame), helpers.sha256(frame)] == hs.golden()["frames"]["8"]["S200000"]["stream"]
    assert ZstdDecompressor().transform_bytes(frame) == d


def test_against_the_machines_libzstd():
    """24 seeded slices of ragged sizes (1 .. 600 000, mixed classes) at levels 5, 8 and 10, as streams and staged, against the binary
    library of this machine.  Staged at level 10, the slices of 8 bytes .. 16 KiB are "btlazy2": refused per slice as in the one-shot call
    (status bit 4), every other frame equal."""
    from kompressor_amd.batch import ZstdBatch
    z = helpers.require_live_libzstd()
    rng = random.Random(5300)
    sizes = [1, 5000, 16384, 131072] + [rng.randrange(1, 600001) for _ in range(20)]
    datas = [corpus.make(77000 + t, 1, n, mix=ord("TXSBDIZR"[t % 8])).tobytes() for t, n in enumerate(sizes)]
    b = ZstdBatch(max_slices=24, max_slice_bytes=600000)
    try:
        for level in (5, 8, 10):
            for framing in ("stream", "staged"):
                frames, bits = _compress(b, datas, level, **KW[framing])
                refused = [i for i, n in enumerate(sizes) if framing == "staged" and level == 10 and 8 <= n <= 16384]
                assert bits == (4 if refused else 0), (level, framing, bits)
                assert [i for i, f in enumerate(frames) if not f] == refused
                bad = [(i, len(d)) for i, (d, f) in enumerate(zip(datas, frames)) if i not in refused and f != hs.live_frame(z, d, level, framing, str(i))]
                assert not bad, (level, framing, bad)
    finally:
        b.close()


def test_the_table_part_in_pieces_and_between_modes(monkeypatch, inputs):
    """A stream's table slot is 5 bytes << the level's hashLog whatever its length: 20 MiB at level 10 on a context for slices of 300 000
    bytes, whose one-shot slots are 5 MiB.  With KMP_LAZY_BIG_SLICES = 2 a batch of 5 streams goes through two slots in three pieces: the
    same frames, and the part grows by no more than two slots.  On the same context a one-shot level-7 batch
    before and after the streams equals the oracle: the part made for it is made once more for the streams, and the tables start clean."""
    from kompressor_amd.batch import ZstdBatch
    names = ["D5000", "T131072", "T0", "S200000", "X131073"]
    datas = [inputs[k] for k in names]
    want = [hs.golden()["frames"]["10"][k]["stream"] for k in names]
    one_shot = [inputs["S200000"], inputs["B262144"]]
    want7 = [helpers.oracle().compress_lazy_big(d, 7)[0] for d in one_shot]
    slot, one_shot_slot = 5 << 22, 5 << 20
    for knob, slots in ((None, 8), ("2", 2)):
        if knob:
            monkeypatch.setenv("KMP_LAZY_BIG_SLICES", knob)
        b = ZstdBatch(max_slices=8, max_slice_bytes=300000)
        try:
            f7, bits = _compress(b, one_shot, 7)
            assert bits == 0 and f7 == want7
            before = b.memory()["other_tables"]
            frames, bits = _compress(b, datas, 10, streaming="data")
            assert bits == 0 and _sig(frames) == want, knob
            after = b.memory()["other_tables"]
            grown = after - before - slots * (slot - one_shot_slot)           # (the part's other records stay as they are)
            assert 0 <= grown <= 4096, (knob, before, after)
            assert after - before <= 2 * slot or not knob
            f7, bits = _compress(b, one_shot, 7)
            assert bits == 0 and f7 == want7
            assert b.memory()["other_tables"] == after
        finally:
            b.close()
            monkeypatch.delenv("KMP_LAZY_BIG_SLICES", raising=False)
