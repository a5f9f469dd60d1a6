"""zstd levels 1, 2 and the negative ones with a dictionary on the GPU (kmp_zstd_compress_batch_dict_level, k_zstd_match_fast_dict;
kmp_zstd_compress_stream; ZstdCompressor(level, dictionary)): frames equal to libzstd 1.5.7's -- the golden file
tests/golden/zstd_dict_levels_golden.json and the machine's own library --, a hostile layout, a context that alternates between levels and
dictionaries, the streaming entry point, and the ablation build."""
import ctypes

import numpy as np
import pytest

import helpers
import helpers_dict_levels as hd
import layouts as LY

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")


def _compress(b, datas, **kw):
    """-> (frames, status bits)"""
    lens = np.array([len(d) for d in datas], dtype=np.int32)
    offs = np.concatenate([[0], np.cumsum(lens[:-1].astype(np.int64))]).astype(np.int64)
    host = np.frombuffer(b"".join(datas) + bytes(64), dtype=np.uint8).copy()
    dst, ooff, olen = b.compress(torch.from_numpy(host).cuda(), torch.from_numpy(offs).cuda(), torch.from_numpy(lens).cuda(), **kw)
    _, bits = b.status()
    dd, oo, ol = dst.cpu().numpy(), ooff.cpu().numpy(), olen.cpu().numpy()
    return [dd[oo[i]:oo[i] + ol[i]].tobytes() for i in range(len(datas))], bits


def _decompress(b, frames, caps, dictionary):
    n = len(frames)
    lens = np.array([len(f) for f in frames], dtype=np.int32)
    offs = np.concatenate([[0], np.cumsum(lens[:-1].astype(np.int64))]).astype(np.int64)
    host = np.frombuffer(b"".join(frames) + bytes(64), dtype=np.uint8).copy()
    dd = torch.from_numpy(np.frombuffer(dictionary, dtype=np.uint8).copy()).cuda()
    dst, ooff, olen, st = b.decompress(torch.from_numpy(host).cuda(), torch.from_numpy(offs).cuda(), torch.from_numpy(lens).cuda(),
                                       torch.tensor(caps, dtype=torch.int32).cuda(), dictionary=dd)
    torch.cuda.synchronize()
    out, oo, ol = dst.cpu().numpy(), ooff.cpu().numpy(), olen.cpu().numpy()
    return [out[oo[i]:oo[i] + ol[i]].tobytes() for i in range(n)], [int(x) for x in st.cpu().numpy()]


def _live():
    try:
        from oracle.libzstd_ref import LibZstd
        return LibZstd()
    except (RuntimeError, OSError):
        pytest.skip("no binary libzstd 1.5.7 on this machine")


@pytest.fixture(scope="module")
def batch():
    from kompressor_amd.batch import ZstdBatch
    b = ZstdBatch(max_slices=64, max_slice_bytes=131072)
    yield b
    b.close()


@pytest.mark.parametrize("level", hd.LEVELS + (hd.FEW_ROWS_LEVEL,))
def test_all_golden_rows(batch, level):
    """Every row of the golden file, one batch per (level, dictionary): no status bit, libzstd 1.5.7's frames (length and sha256), and
    decompress(dictionary=...) on the GPU returns the inputs."""
    done = 0
    for name, d, slices in hd.cases():
        if level not in hd.levels_of(name):
            continue
        datas = [p for _, p in slices]
        frames, bits = _compress(batch, datas, dictionary=d, level=level)
        assert bits == 0, (name, level, bits)
        hd.check_frames(name, d, slices, level, frames)
        back, st = _decompress(batch, frames, [max(len(p), 1) for p in datas], d)
        assert st == [0] * len(datas) and back == datas, (name, level)
        done += 1
    assert done == (1 if level == hd.FEW_ROWS_LEVEL else len(hd.cases()))


def test_hostile_layout():
    """Level 1 with a dictionary of 16 KiB in a permuted layout with odd offsets, exact slots and canaries (layouts.exact): slices on both
    sides of the attach cut-off of 8 KiB, an empty one, sizes without a parse; libzstd's frames and not a byte outside the slots."""
    from kompressor_amd.batch import ZstdBatch
    z = _live()
    d = hd.word_text(81, 16384, 1)
    sizes = (8192, 0, 8193, 7, 8191, 1, 20000, 8, 3000, 9, 65, 12000, 64, 8200, 5, 131072)
    datas = [(hd.word_text(900 + i, n, 1 + i % 2) if i % 3 else (d * 9)[i * 37:i * 37 + n]) for i, n in enumerate(sizes)]
    L = LY.exact(datas, [LY.zstd_slot(len(p)) for p in datas], seed=7301)
    assert len({int(x) % 2 for x in L.in_off}) == 2 and sorted(L.in_off) != list(L.in_off)
    b = ZstdBatch(max_slices=32, max_slice_bytes=131072)
    try:
        dst = torch.from_numpy(L.new_dst()).cuda()
        olen = torch.full((L.n,), -1, dtype=torch.int32).cuda()
        b.compress(torch.from_numpy(L.src).cuda(), torch.from_numpy(L.in_off).cuda(), torch.from_numpy(L.in_len).cuda(),
                   dst=dst, out_off=torch.from_numpy(L.out_off).cuda(), out_len=olen, dictionary=d, level=1)
        _, bits = b.status()
        dd, ol = dst.cpu().numpy(), olen.cpu().numpy()
        assert bits == 0
        assert not L.check(dd, ol, slot_tail_ok=True)
        assert L.frames(dd, ol) == [z.compress_with_dict(p, d, 1) for p in datas]
    finally:
        b.close()


def test_alternating_levels_and_dictionaries():
    """One context: level 1 / dictionary A, level 3 / A, level 1 / B, level 1 without a dictionary, twice.  Each result equals its own
    reference, and the context's memory does not grow on the second pass (it holds the three CDicts)."""
    from kompressor_amd.batch import ZstdBatch
    z = _live()
    o = helpers.oracle()
    A, B = hd.word_text(91, 20000, 1), hd.word_text(92, 3000, 2)
    datas = [hd.word_text(950 + i, n, 1 + i % 2) for i, n in enumerate((100, 5000, 8192, 8193, 30000, 0, 7))]
    steps = ((1, A), (3, A), (1, B), (1, None))
    want = [[z.compress_with_dict(p, d, lv) if d is not None else o.compress_level(p, lv) for p in datas] for lv, d in steps]
    b = ZstdBatch(max_slices=16, max_slice_bytes=131072)
    try:
        mem = []
        for rnd in range(2):
            for (lv, d), w in zip(steps, want):
                frames, bits = _compress(b, datas, level=lv, **({"dictionary": d} if d is not None else {}))
                assert bits == 0 and frames == w, (rnd, lv, d is None)
            mem.append(b.memory()["other_tables"])
        assert mem[0] > 0 and mem[1] == mem[0], mem
    finally:
        b.close()


def test_zstd_compressor_with_level_and_dictionary():
    """ZstdCompressor(1, dictionary=d).transform_bytes(x) and ZstdCompressor(-3, dictionary=d): the live library's frames, raw and
    formatted dictionary; ZstdDecompressor(dictionary=d) inverts them."""
    from kompressor_amd.zstd import ZstdCompressor, ZstdDecompressor
    z = _live()
    raw = hd.word_text(93, 5000, 1)
    fmt = next(c[1] for c in hd.cases() if c[0].startswith("built1_"))
    for d in (raw, fmt):
        for level, n in ((1, 3000), (-3, 3000), (1, 20000), (-3, 9000)):
            x = hd.word_text(960 + n, n, 1)
            f = ZstdCompressor(level, dictionary=d).transform_bytes(x)
            assert f == z.compress_with_dict(x, d, level), (level, n, d is fmt)
            assert ZstdDecompressor(dictionary=d).transform_bytes(f) == x


def _stream(lib, d, level, dictionary, cuts, out_chunk=1 << 18):
    """kmp_zstd_compress_stream: d[cuts[i]:cuts[i+1]] with e_continue, the last piece with e_end.  -> (frame, error name or None)"""
    cctx = lib.kmp_zstd_create_cctx()
    out = bytearray(); obuf = ctypes.create_string_buffer(out_chunk)
    try:
        assert lib.kmp_zstd_cctx_set_parameter(cctx, 100, level) == 0
        assert lib.kmp_zstd_cctx_load_dictionary(cctx, dictionary, len(dictionary)) == 0
        pieces = list(zip(cuts[:-1], cuts[1:]))
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


def test_the_streaming_entry_point(batch):
    """kmp_zstd_compress_stream with set_parameter(100, 2) and load_dictionary: a closing call of 5 000 bytes gives the golden frame, with a
    raw and with a formatted dictionary (9 000 bytes there); the same data fed with e_continue first is still "Unsupported parameter", a
    damaged formatted dictionary is "Dictionary is corrupted", ZstdBatch.compress(dictionary=d, level=7) still raises and the export
    answers KMP_ERR_ARG from level 4 on."""
    from kompressor_amd import _lib
    lib = _lib.load()
    for prefix, n in (("raw_4096", 5000), ("built0_", 9000)):
        name, d, slices = next(c for c in hd.cases() if c[0].startswith(prefix))
        i = next(k for k, (_, p) in enumerate(slices) if len(p) == n)
        frame, err = _stream(lib, slices[i][1], 2, d, [0, n])
        assert err is None, err
        assert [len(frame), helpers.sha256(frame)] == hd.golden()[(name, 2)]["frames"][i], name
        _, err = _stream(lib, slices[i][1], 2, d, [0, 2000, n])
        assert err == "Unsupported parameter", err
    bad = bytearray(d); bad[9] = 0                                       # (the formatted dictionary's Huffman table description)
    _, err = _stream(lib, slices[i][1], 2, bytes(bad), [0, n])
    assert err == "Dictionary is corrupted", err
    with pytest.raises(ValueError):
        _compress(batch, [slices[i][1]], dictionary=d, level=7)
    for level in (4, 7, 11):
        assert batch.lib.kmp_zstd_compress_batch_dict_level(batch._h, None, None, None, 0, None, None, None, d, len(d), level, None) == -2      # KMP_ERR_ARG


def test_level_3_goes_the_way_it_went(batch):
    """Level 0 or 3 through the new export: kmp_zstd_compress_batch_dict's frames, bit for bit (the oracle's)."""
    o = helpers.oracle()
    _, d, slices = next(c for c in hd.cases() if c[0] == "raw_15884")
    datas = [p for _, p in slices if 0 < len(p) <= 20000]
    want = [o.compress_dict(p, d)[0] for p in datas]
    for level in (0, 3):
        frames, bits = _compress(batch, datas, dictionary=d, level=level)
        assert bits == 0 and frames == want


def test_normal_and_ablation_builds_agree(batch):
    """The kernel compiles into both libraries: one batch, the same frames (the golden ones)."""
    from kompressor_amd.batch import ZstdBatch
    name, d, slices = next(c for c in hd.cases() if c[0] == "raw_S_32768")
    datas = [p for _, p in slices]
    b = ZstdBatch(max_slices=16, max_slice_bytes=65536, ablations=True)
    try:
        for level in (1, -5):
            frames, bits = _compress(b, datas, dictionary=d, level=level)
            assert bits == 0 and (frames, 0) == _compress(batch, datas, dictionary=d, level=level)
            hd.check_frames(name, d, slices, level, frames)
    finally:
        b.close()
