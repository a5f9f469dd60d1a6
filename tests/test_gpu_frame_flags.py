"""The frame flags on the GPU (kmp_batch_set_frame_flags, ZSTD_c_contentSizeFlag / checksumFlag / dictIDFlag of
kmp_zstd_cctx_set_parameter): every row of tests/golden/zstd_frame_flags_golden.json (the binary libzstd 1.5.7's frames) through
ZstdBatch.compress with the keyword arguments, the frames' structure, the flags held on a context, the containers that ignore them, a
hostile layout at exact slots, the streaming entry points (raw calls, ZstdCompressor, the coalescer) and the ablation build.

The rows put 131 073 bytes at level 4: the size class (128 - 256 KiB) that libzstd parses "greedy" at that level, which the batch call serves
through zstd_lazy_big.h's chain with level 4's row; test_level_4_between_128_and_256_kib pins that path without flags against the live library."""
import ctypes
import threading

import numpy as np
import pytest

import helpers
import helpers_frame_flags as hf
import helpers_seekable as hs
import layouts as LY

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

KW = {hf.CHECKSUM: dict(checksum=True), hf.NO_CONTENT_SIZE: dict(content_size=False), hf.CHECKSUM | hf.NO_CONTENT_SIZE: dict(checksum=True, content_size=False),
      hf.NO_DICT_ID: dict(dict_id=False), hf.CHECKSUM | hf.NO_CONTENT_SIZE | hf.NO_DICT_ID: dict(checksum=True, content_size=False, dict_id=False), 0: {}}
ALL_LEVELS = hf.LEVELS + tuple(v for v in hf.BIG_LEVELS if v not in hf.LEVELS)


def _ctx(**kw):
    from kompressor_amd.batch import ZstdBatch
    assert torch.cuda.is_available(), "these tests need the MI355X"
    return ZstdBatch(table_span_gib=0, **kw)


@pytest.fixture(scope="module")
def one_block():
    b = _ctx(max_slices=32, max_slice_bytes=131072)
    yield b
    b.close()


@pytest.fixture(scope="module")
def chains():
    b = _ctx(max_slices=8, max_slice_bytes=hf.BIG_SIZE)
    yield b
    b.close()


def _pack(datas):
    lens = np.array([len(d) for d in datas], dtype=np.int32)
    offs = np.concatenate([[0], np.cumsum(lens[:-1].astype(np.int64))]).astype(np.int64)
    host = np.frombuffer(b"".join(datas) + bytes(64), dtype=np.uint8).copy()
    return torch.from_numpy(host).cuda(), torch.from_numpy(offs).cuda(), torch.from_numpy(lens).cuda()


def _compress(b, datas, level=3, **kw):
    """-> (frames, status bits)"""
    dst, ooff, olen = b.compress(*_pack(datas), level=level, **kw)
    _, bits = b.status()
    dd, oo, ol = dst.cpu().numpy(), ooff.cpu().numpy(), olen.cpu().numpy()
    return [dd[oo[i]:oo[i] + ol[i]].tobytes() for i in range(len(datas))], bits


def _decompress(b, frames, caps, dictionary=None):
    d = torch.from_numpy(np.frombuffer(dictionary, dtype=np.uint8).copy()).cuda() if dictionary else None
    dst, ooff, olen, st = b.decompress(*_pack(frames), torch.tensor(caps, dtype=torch.int32).cuda(), dictionary=d)
    torch.cuda.synchronize()
    dd, oo, ol = dst.cpu().numpy(), ooff.cpu().numpy(), olen.cpu().numpy()
    return [dd[oo[i]:oo[i] + ol[i]].tobytes() for i in range(len(frames))], [int(x) for x in st.cpu().numpy()]


def _check_row(b, slices, level, flags, dname=None, d=None):
    datas = [p for _, p in slices]
    frames, bits = _compress(b, datas, level, dictionary=d, **KW[flags])
    assert bits == 0, (level, dname, flags, bits, [s for (s, _), f in zip(slices, frames) if not f])
    want = hf.golden_frames(level, dname, flags)
    for (s, _), f in zip(slices, frames):
        hf.check_frame(f, want[s], (level, dname, flags, s))
    back, st = _decompress(b, frames, [max(len(p), 1) for p in datas], dictionary=d)
    assert st == [0] * len(datas) and back == datas, (level, dname, flags)
    return frames


# ------------------------------------------------------------------------------------------------------------ golden rows ----
@pytest.mark.parametrize("flags", hf.FLAG_SETS)
@pytest.mark.parametrize("level", hf.LEVELS)
def test_golden_rows_one_block(one_block, level, flags):
    """the slices up to 128 KiB, one batch on a context for one-block frames"""
    _check_row(one_block, [(s, p) for s, p in hf.slices_of(level, big=False) if len(p) <= 131072], level, flags)


@pytest.mark.parametrize("level", ALL_LEVELS)
def test_golden_rows_several_blocks(chains, level):
    """131 073 and 300 000 bytes, one batch per flag set on a context for frames of several blocks: the block chain (levels up to 4), the
    chain of zstd_lazy_big.h (6 and 7)"""
    for flags in hf.FLAG_SETS:
        _check_row(chains, [(s, p) for s, p in hf.slices_of(level) if len(p) > 131072], level, flags)


def test_level_4_between_128_and_256_kib(chains):
    """level 4 without flags at the edges of its "greedy" class above a block and inside it, beside slices of its double-fast classes in the
    same batch: ZSTD_compress2's frames from the live library (a slice up to 16 KiB on such a context stays refused: out_len 0, status bit 4)"""
    z = helpers.require_live_libzstd()
    datas = [hf.text(n) for n in (131072, 131073, 200001, 262144, 262145, 20000, hf.BIG_SIZE)]
    frames, bits = _compress(chains, datas, 4)
    assert bits == 0
    for p, f in zip(datas, frames):
        assert f == hf.lib_compress2(z, p, 4, 0), len(p)
    back, st = _decompress(chains, frames, [len(p) for p in datas])
    assert st == [0] * len(datas) and back == datas
    frames, bits = _compress(chains, [hf.text(5000), hf.text(200001)], 4)
    assert bits == 4 and frames[0] == b"" and frames[1] == hf.lib_compress2(z, hf.text(200001), 4, 0)


def test_short_slices_on_the_block_chain(chains):
    """slices up to 128 KiB on that context, where the chain's frame init and frame step write them: the same golden frames"""
    for flags in hf.FLAG_SETS:
        _check_row(chains, [(s, p) for s, p in hf.slices_of(3) if len(p) in (0, 1, 33, 256, 5000, 65792)], 3, flags)


@pytest.mark.parametrize("level", hf.DICT_LEVELS)
@pytest.mark.parametrize("which", range(3))
def test_golden_rows_dictionary(one_block, which, level):
    name, d, formatted = hf.dictionaries()[which]
    for flags in (hf.FLAG_SETS_FORMATTED if formatted else hf.FLAG_SETS):
        _check_row(one_block, hf.dict_slices(), level, flags, name, d)


# -------------------------------------------------------------------------------------------------- what the frames are ----
def test_damaged_trailer_is_status_22(one_block):
    p = hf.text(65791)
    (f,), bits = _compress(one_block, [p], 3, checksum=True)
    assert bits == 0
    bad = f[:-1] + bytes([f[-1] ^ 0x40])
    back, st = _decompress(one_block, [f, bad], [len(p)] * 2)
    assert st == [0, 22] and back[0] == p


def test_frame_info(one_block):
    datas = [p for _, p in hf.slices_of(3, big=False) if len(p) <= 131072]
    for flags in hf.FLAG_SETS:
        frames, _ = _compress(one_block, datas, 3, **KW[flags])
        info = one_block.frame_info(*_pack(frames))
        torch.cuda.synchronize()
        assert [int(x) for x in info["status"].cpu()] == [0] * len(datas)
        assert [int(x) & 1 for x in info["flags"].cpu()] == [flags & hf.CHECKSUM] * len(datas), flags
        content = [int(x) for x in info["content"].cpu()]
        assert content == ([-1] * len(datas) if flags & hf.NO_CONTENT_SIZE else [len(p) for p in datas]), flags


def test_structure(one_block):
    """ten slices at level 3: the {201} frame is the flag-less frame of the same context with descriptor bit 2 and four more bytes, the
    low half of the content's XXH64 (helpers_seekable's, little-endian)"""
    datas = [p for _, p in hf.slices_of(3, big=False) if len(p) <= 131072][:10]
    assert len(datas) == 10
    plain, b0 = _compress(one_block, datas, 3)
    summed, b1 = _compress(one_block, datas, 3, checksum=True)
    assert (b0, b1) == (0, 0) and one_block.frame_flags() == 0
    n = len(datas)
    lens = np.array([len(p) for p in datas], dtype=np.uint32); offs = (np.concatenate([[0], np.cumsum(lens[:-1])]) + 5).astype(np.uint64)
    src = np.frombuffer(bytes(5) + b"".join(datas) + bytes(64), dtype=np.uint8).copy(); cks = np.zeros(n, dtype=np.uint32)
    vp = helpers._vp
    assert hs.emu().emu_seekable_xxh64(vp(src), vp(offs), vp(lens), n, vp(cks), None, None, 3, 2) == 0
    for i, (a, s) in enumerate(zip(plain, summed)):
        assert s == a[:4] + bytes([a[4] | 4]) + a[5:] + int(cks[i]).to_bytes(4, "little"), (i, len(datas[i]))


def test_flags_hold_on_the_context(one_block):
    b, lib = one_block, one_block.lib
    slices = [(s, p) for s, p in hf.slices_of(1, big=False) if len(p) <= 131072]
    datas = [p for _, p in slices]
    assert lib.kmp_batch_set_frame_flags(b._h, 1) == 0 and lib.kmp_batch_frame_flags(b._h) == 1
    try:
        frames, bits = _compress(b, datas, 1)                    # kmp_zstd_compress_batch_level, no keyword arguments
        assert bits == 0 and lib.kmp_batch_frame_flags(b._h) == 1
        want = hf.golden_frames(1, None, hf.CHECKSUM)
        for (s, _), f in zip(slices, frames):
            hf.check_frame(f, want[s], s)
        assert lib.kmp_batch_set_frame_flags(b._h, 8) == -2 and lib.kmp_batch_set_frame_flags(b._h, 1 | 8) == -2          # KMP_ERR_ARG
        assert lib.kmp_batch_frame_flags(b._h) == 1
        three, _ = _compress(b, [p for _, p in hf.slices_of(3, big=False) if len(p) <= 131072], 3)                       # kmp_zstd_compress_batch
    finally:
        assert lib.kmp_batch_set_frame_flags(b._h, 0) == 0
    assert lib.kmp_batch_frame_flags(b._h) == 0
    plain, bits = _compress(b, datas, 1)
    assert bits == 0
    for a, s in zip(plain, frames):
        assert s[:-4] == a[:4] + bytes([a[4] | 4]) + a[5:]
    slices3 = [(s, p) for s, p in hf.slices_of(3, big=False) if len(p) <= 131072]
    plain3, _ = _compress(b, [p for _, p in slices3], 3)
    for (s, _), f0, f1 in zip(slices3, plain3, three):
        hf.check_frame(f0, hf.golden_frames(3, None, 0)[s], s)
        hf.check_frame(f1, hf.golden_frames(3, None, hf.CHECKSUM)[s], s)


def test_seekable_container_ignores_the_flags(one_block):
    data = hf.text(hf.BIG_SIZE)
    src = torch.from_numpy(np.frombuffer(data, dtype=np.uint8).copy()).cuda()
    fresh = _ctx(max_slices=32, max_slice_bytes=131072)
    try:
        want = fresh.compress_seekable(src, frame_bytes=16384, level=3).cpu().numpy().tobytes()
    finally:
        fresh.close()
    one_block.set_frame_flags(1)
    try:
        got = one_block.compress_seekable(src, frame_bytes=16384, level=3).cpu().numpy().tobytes()
        assert one_block.frame_flags() == 1
    finally:
        one_block.set_frame_flags(0)
    assert got == want


def test_hostile_layout_at_exact_slots(one_block):
    """slots of kmp_zstd_compress_bound(len) + 8 with canaries between them, {200=0, 201}: the trailer fits the bound the header promises
    -- incompressible slices included, whose raw block fills it --, not a byte outside the slots"""
    flags = hf.CHECKSUM | hf.NO_CONTENT_SIZE
    slices = [(s, p) for s, p in hf.slices_of(3, big=False) if len(p) <= 131072]
    rng = np.random.default_rng(7)
    noise = [("noise_%d" % n, rng.integers(0, 256, n, dtype=np.uint8).tobytes()) for n in (1, 255, 65536, 131072)]
    datas = [p for _, p in slices + noise]
    L = LY.exact(datas, [LY.zstd_slot(len(d)) for d in datas], 4100)
    L.check_inside()
    dst = torch.from_numpy(L.new_dst()).cuda()
    olen = torch.full((len(datas),), -1, dtype=torch.int32).cuda()
    one_block.compress(torch.from_numpy(L.src).cuda(), torch.from_numpy(L.in_off).cuda(), torch.from_numpy(L.in_len).cuda(),
                       dst=dst, out_off=torch.from_numpy(L.out_off).cuda(), out_len=olen, checksum=True, content_size=False)
    _, bits = one_block.status()
    assert bits == 0
    dd, ol = dst.cpu().numpy(), olen.cpu().numpy()
    bad = L.check(dd, ol, slot_tail_ok=True)
    assert not bad, "\n".join(bad)
    frames = dict(zip(L.datas, L.frames(dd, ol)))
    want = hf.golden_frames(3, None, flags)
    for s, p in slices:
        hf.check_frame(frames[p], want[s], s)
    for s, p in noise:
        assert len(frames[p]) == 6 + 3 + len(p) + 4 and len(frames[p]) <= LY.zstd_bound(len(p)) + 8, s
    back, st = _decompress(one_block, [frames[p] for _, p in noise], [len(p) for _, p in noise])
    assert st == [0] * len(noise) and back == [p for _, p in noise]


# ------------------------------------------------------------------------------------------------- streaming entry points ----
def _stream(lib, d, cuts, out_chunk, level=3, params=()):
    """kmp_zstd_compress_stream: d[cuts[i]:cuts[i+1]] with e_continue, the last piece with e_end, output drained through out_chunk-byte
    slices -> (frame, [set_parameter's return values])"""
    cctx = lib.kmp_zstd_create_cctx()
    assert lib.kmp_zstd_cctx_set_parameter(cctx, 100, level) == 0
    rets = [lib.kmp_zstd_cctx_set_parameter(cctx, pid, value) for pid, value in params]
    out = bytearray(); obuf = ctypes.create_string_buffer(out_chunk)
    pieces = list(zip(cuts[:-1], cuts[1:]))
    try:
        for j, (a0, a1) in enumerate(pieces):
            end = j == len(pieces) - 1
            sp = ctypes.c_size_t(a0)
            while True:
                dp = ctypes.c_size_t(0)
                r = lib.kmp_zstd_compress_stream(cctx, obuf, out_chunk, ctypes.byref(dp), d, a1, ctypes.byref(sp), 2 if end else 0)
                assert not lib.kmp_zstd_is_error(r), lib.kmp_zstd_get_error_name(r).decode()
                out += obuf.raw[:dp.value]
                if (end and r == 0) or (not end and sp.value == a1 and dp.value < out_chunk):
                    break
    finally:
        lib.kmp_zstd_free_cctx(cctx)
    return bytes(out), rets


def test_streaming_raw_calls():
    from kompressor_amd import _lib
    lib = _lib.load()
    d = hf.text(5000)
    frame, rets = _stream(lib, d, [0, 5000], 8192, params=[(201, 1)])
    hf.check_frame(frame, hf.golden_frames(3, None, hf.CHECKSUM)["text_5000"], "closing call")
    recorded = hf.golden()["set_parameter"]
    assert rets == [recorded["201,1"]]
    # the return values of the three parameters are the binary library's; a value other than 0 and 1 is out of bound, another id unsupported
    cctx = lib.kmp_zstd_create_cctx()
    try:
        for pid, value in ((200, 0), (201, 1), (202, 0)):
            assert lib.kmp_zstd_cctx_set_parameter(cctx, pid, value) == recorded[f"{pid},{value}"], (pid, value)
        for pid, value in ((201, 2), (200, -1), (202, 7)):
            r = lib.kmp_zstd_cctx_set_parameter(cctx, pid, value)
            assert lib.kmp_zstd_is_error(r) and lib.kmp_zstd_get_error_name(r) == b"Parameter is out of bound", (pid, value)
        for pid in (101, 203, 1000):
            assert lib.kmp_zstd_get_error_name(lib.kmp_zstd_cctx_set_parameter(cctx, pid, 1)) == b"Unsupported parameter", pid
        # the stage rule is the level's: refused once input has been fed
        sp, dp = ctypes.c_size_t(0), ctypes.c_size_t(0)
        obuf = ctypes.create_string_buffer(8192)
        assert lib.kmp_zstd_compress_stream(cctx, obuf, 8192, ctypes.byref(dp), d, 100, ctypes.byref(sp), 0) == 0
        r = lib.kmp_zstd_cctx_set_parameter(cctx, 201, 0)
        assert lib.kmp_zstd_get_error_name(r) == b"Operation not authorized at current processing stage"
    finally:
        lib.kmp_zstd_free_cctx(cctx)
    # the same bytes as a stream: what the live library's ZSTD_compressStream2 gives under the same calls
    z = helpers.require_live_libzstd()
    frame, _ = _stream(lib, d, [0, 2000, 5000], 8192, params=[(201, 1)])
    assert frame == hf.lib_stream(z, d, [0, 2000, 5000], 3, hf.CHECKSUM, 8192)


def test_zstd_compressor_64k():
    from kompressor_amd import ZstdCompressor, ZstdDecompressor
    d = hf.text(65536)
    for kw, flags in ((dict(checksum=True), hf.CHECKSUM), (dict(content_size=False), hf.NO_CONTENT_SIZE)):
        frame = ZstdCompressor(3, **kw).transform_bytes(d)
        hf.check_frame(frame, hf.golden_frames(3, None, flags)["text_65536"], kw)
        assert ZstdDecompressor().transform_bytes(frame) == d


def test_zstd_compressor_300000():
    """the reference's loop (output slices of max(8192, n / 10) bytes, e_end from the first call) is the staged path: the live library's
    frame under the same calls; one closing call with room for the bound is the in-place path: the {201} golden row"""
    from kompressor_amd import _lib, ZstdCompressor, ZstdDecompressor
    z = helpers.require_live_libzstd()
    d = hf.text(hf.BIG_SIZE); n = len(d)
    frame = ZstdCompressor(3, checksum=True).transform_bytes(d)
    assert frame == hf.lib_stream(z, d, [0, n], 3, hf.CHECKSUM, max(8192, n // 10), end_from_first=True)
    assert ZstdDecompressor().transform_bytes(frame) == d
    lib = _lib.load()
    frame, _ = _stream(lib, d, [0, n], lib.kmp_zstd_compress_bound(n), params=[(201, 1)])
    hf.check_frame(frame, hf.golden_frames(3, None, hf.CHECKSUM)[f"text_{n}"], "in place")


def test_coalescer_keeps_flag_sets_apart():
    """two contexts close 20 000 bytes at the same moment, one with the checksum, one without: each gets its own golden frame"""
    from kompressor_amd import ZstdCompressor
    d = hf.text(20000)
    ZstdCompressor(3).transform_bytes(d)                        # (the engine behind the coalescer exists before the two meet)
    gate = threading.Barrier(2)
    out = {}

    def work(flags):
        t = ZstdCompressor(3, **KW[flags])
        for k in range(4):
            gate.wait()
            out[(flags, k)] = t.transform_bytes(d)

    threads = [threading.Thread(target=work, args=(f,)) for f in (0, hf.CHECKSUM)]
    for t in threads:
        t.start()
    for t in threads:
        t.join()
    for (flags, k), frame in out.items():
        hf.check_frame(frame, hf.golden_frames(3, None, flags)["text_20000"], (flags, k))
    assert len(out) == 8


def test_ablation_build_agrees(one_block):
    datas = [p for _, p in hf.slices_of(3, big=False) if len(p) <= 131072]
    want, _ = _compress(one_block, datas, 3, checksum=True, content_size=False)
    from kompressor_amd.batch import ZstdBatch
    a = ZstdBatch(max_slices=32, max_slice_bytes=131072, table_span_gib=0, ablations=True)
    try:
        got, bits = _compress(a, datas, 3, checksum=True, content_size=False)
    finally:
        a.close()
    assert bits == 0 and got == want
