"""Frame inspection on the device (kmp_zstd_frame_info_batch, kmp_batch_layout: k_zstd_frame_info, k_batch_layout) and the decode
that needs no sizes from its caller (ZstdBatch.decompress(out_cap=None), decompress_host_batch(frames)): the fixture of the binary
libzstd 1.5.7 (tests/golden/zstd_frame_info_golden.json) plain and at a hostile layout with canaries around d_info, a mixed batch of 300
entries against the decode with known capacities, alignment, a dictionary, damaged entries among good ones, a context that has never
decoded, both builds of the library."""
import ctypes

import numpy as np
import pytest

import helpers_frame_info as hf
import layouts
from kompressor_amd import corpus

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

MARGIN = 4096


def _ctx(**kw):
    from kompressor_amd.batch import ZstdBatch
    assert torch.cuda.is_available(), "these tests need the MI355X"
    return ZstdBatch(**kw)


@pytest.fixture(scope="module")
def big():
    b = _ctx(max_slices=512, max_slice_bytes=1 << 20)
    yield b
    b.close()


@pytest.fixture(scope="module")
def small():
    b = _ctx(max_slices=256, max_slice_bytes=65536)
    yield b
    b.close()


@pytest.fixture(scope="module")
def rows():
    return hf.golden()


def _up(entries):
    """entries back to back in device memory -> (src, in_off, in_len)"""
    src, offs, lens = hf.pack(entries)
    return torch.from_numpy(src).cuda(), torch.from_numpy(offs.astype(np.int64)).cuda(), torch.from_numpy(lens.astype(np.int32)).cuda()


def _compress(b, datas, **kw):
    src, io, il = _up(datas)
    dst, oo, ol = b.compress(src, io, il, **kw)
    rc, bits = b.status()
    assert rc == 0 and bits == 0, (rc, bits)
    dd, oo, ol = dst.cpu().numpy(), oo.cpu().numpy(), ol.cpu().numpy()
    frames = [dd[int(oo[i]):int(oo[i]) + int(ol[i])].tobytes() for i in range(len(datas))]
    assert all(frames)
    return frames


def _results(r, n):
    """(dst, out_off, out_len, status) of a decompress -> ([bytes], out_len list, status list, out_off list)"""
    torch.cuda.synchronize()
    dd, oo, ol, st = (t.cpu().numpy() for t in r)
    return [dd[int(oo[i]):int(oo[i]) + int(ol[i])].tobytes() for i in range(n)], [int(x) for x in ol], [int(x) for x in st], [int(x) for x in oo]


def _info_call(b, src, io, il, n, lib=None):
    """kmp_zstd_frame_info_batch through the C ABI into a buffer with canaries around d_info (which starts 8 bytes off a 16-byte boundary)
    -> INFO array"""
    lib = lib or b.lib
    can = np.random.default_rng(3).integers(0, 256, 2 * MARGIN + 8 + 32 * n, dtype=np.uint8)
    buf = torch.from_numpy(can.copy()).cuda()
    at = MARGIN + 8
    assert (buf.data_ptr() + at) % 16 == 8
    rc = lib.kmp_zstd_frame_info_batch(b._h, ctypes.c_void_p(src.data_ptr()), ctypes.c_void_p(io.data_ptr()), ctypes.c_void_p(il.data_ptr()), n,
                                       ctypes.c_void_p(buf.data_ptr() + at), b._stream())
    assert rc == 0, b._err()
    torch.cuda.synchronize()
    out = buf.cpu().numpy()
    assert np.array_equal(out[:at], can[:at]) and np.array_equal(out[at + 32 * n:], can[at + 32 * n:]), "bytes around d_info changed"
    return out[at:at + 32 * n].copy().view(hf.INFO)


# ------------------------------------------------------------------------------------------------------ inspection ----
def test_fixture_batch_equals_the_library_and_the_host_call(big, rows):
    entries = [e for _, e, _ in rows]
    want = hf.expected_array([r for _, _, r in rows])
    src, io, il = _up(entries)
    got = _info_call(big, src, io, il, len(entries))
    bad = hf.diff(got, want, [n for n, _, _ in rows])
    assert not bad, "\n".join(bad[:20])
    assert got.tobytes() == hf.host_info(entries).tobytes()
    # the Python view of the same call
    d = big.frame_info(src, io, il)
    torch.cuda.synchronize()
    for f in hf.FIELDS:
        mask = (1 << 64) - 1 if f in ("content", "bound") else (1 << 32) - 1
        assert [int(x) & mask for x in d[f].cpu().numpy()] == [int(x) for x in want[f]], f


@pytest.mark.parametrize("filler", ("random", "complement"))
def test_fixture_batch_at_a_hostile_layout(big, rows, filler):
    entries = [e for _, e, _ in rows]
    want = hf.expected_array([r for _, _, r in rows])
    L = layouts.exact(entries, [32] * len(entries), seed=41, filler=filler)
    L.check_residues()
    src, io, il = torch.from_numpy(L.src).cuda(), torch.from_numpy(L.in_off).cuda(), torch.from_numpy(L.in_len).cuda()
    got = _info_call(big, src, io, il, L.n)
    bad = hf.diff(got, want, [n for n, _, _ in rows])
    assert not bad, "\n".join(bad[:20])


def test_both_library_builds_give_the_same_bytes(big, rows):
    entries = [e for _, e, _ in rows]
    src, io, il = _up(entries)
    a = _info_call(big, src, io, il, len(entries))
    abl = _ctx(max_slices=256, max_slice_bytes=65536, ablations=True)
    try:
        assert abl.lib is not big.lib
        b = _info_call(abl, src, io, il, len(entries))
        inf = abl._frame_info_raw(src, io, il)
        off_a, cap_a, tot_a = big.layout(big._frame_info_raw(src, io, il), 16)
        off_b, cap_b, tot_b = abl.layout(inf, 16)
        torch.cuda.synchronize()
        assert torch.equal(off_a, off_b) and torch.equal(cap_a, cap_b) and torch.equal(tot_a, tot_b)
    finally:
        abl.close()
    assert a.tobytes() == b.tobytes()


def test_inspection_allocates_no_decode_staging(rows):
    """a fresh context that has never decoded: frame_info and layout leave its memory as it was"""
    b = _ctx(max_slices=256, max_slice_bytes=65536)
    try:
        before = b.memory()
        src, io, il = _up([e for _, e, _ in rows])
        b.frame_info(src, io, il)
        b.layout(b._frame_info_raw(src, io, il), 64)
        torch.cuda.synchronize()
        after = b.memory()
        assert after["decode_staging"] == 0 and after == before, (before, after)
    finally:
        b.close()


def test_layout_arguments(small, rows):
    src, io, il = _up([e for _, e, _ in rows][:8])
    info = small._frame_info_raw(src, io, il)
    for bad in (0, 3, 8192, 48):
        with pytest.raises(RuntimeError, match="align"):
            small.layout(info, bad)
    off, cap, total = small.layout(info[:0], 1)                # n == 0
    torch.cuda.synchronize()
    assert off.numel() == 0 and [int(x) for x in total.cpu()] == [0, 0]
    with pytest.raises(ValueError):
        small.decompress(src, io, il, dst=torch.empty(64, dtype=torch.uint8, device="cuda"))


# ------------------------------------------------------------------------------------------------------ decode ----
@pytest.fixture(scope="module")
def mixed(big, rows):
    """300 entries: [(entry, true size or None where only the decode knows, plain or None)]"""
    rng = np.random.default_rng(11)
    # foreign frames: what the library accepts (in today's format) and a context of 1 MiB slices holds
    foreign = [(e, None, None) for _, e, r in rows if r["status"] == 0 and not r["flags"] & 4 and r["bound"] <= 640 * 1024]
    assert len(foreign) >= 40
    fill = 300 - len(foreign) - 6 - len(layouts.SIZES) - 9 - 2
    sizes = [0, 1, 131071, 131072, 65536, 100000] + list(layouts.SIZES) + [int(x) for x in rng.integers(0, 40000, fill)]
    datas = [corpus.make(5000 + i, 1, s).tobytes() if s else b"" for i, s in enumerate(sizes)]
    own = _compress(big, datas)
    out = [(f, len(d), d) for f, d in zip(own, datas)]
    sdatas = [corpus.make(6000 + i, 1, s).tobytes() for i, s in enumerate((3000, 131072 + 5000, 4 * 131072 + 777) * 3)]
    streams = _compress(big, sdatas, streaming="data")
    for f, d in zip(streams, sdatas):
        a = hf.host_info([f])[0]
        # no declared size: the bound is blocks x 128 KiB -- one block per 128 KiB chunk of input, or more where the pre-splitter cut
        blocks = int(a["bound"]) // 131072
        assert int(a["content"]) == hf.UNKNOWN and int(a["bound"]) % 131072 == 0 and blocks >= len(d) // 131072 + 1
        out.append((f, len(d), d))
    skip = b"\x53\x2a\x4d\x18" + (11).to_bytes(4, "little") + b"between two"
    out.append((own[7] + skip + own[9], len(datas[7]) + len(datas[9]), datas[7] + datas[9]))
    out.append((streams[0] + skip + own[3], len(sdatas[0]) + len(datas[3]), sdatas[0] + datas[3]))
    out += foreign
    assert len(out) == 300, len(out)
    order = rng.permutation(len(out))
    return [out[int(k)] for k in order]


def _known_caps(b, mixed, src, io, il):
    """the capacities a caller who knows the sizes passes: the true size; for the foreign frames what a first decode with their
    declared bound gives"""
    bound = hf.host_info([e for e, _, _ in mixed])["bound"]
    caps = np.array([t if t is not None else int(bd) for (_, t, _), bd in zip(mixed, bound)], dtype=np.int32)
    first = _results(b.decompress(src, io, il, torch.from_numpy(caps).cuda()), len(mixed))
    for i, (_, t, _) in enumerate(mixed):
        if t is None and first[2][i] == 0:
            caps[i] = first[1][i]
    return caps


def test_decompress_without_sizes_equals_decompress_with_them(big, mixed):
    n = len(mixed)
    src, io, il = _up([e for e, _, _ in mixed])
    caps = _known_caps(big, mixed, src, io, il)
    ref = _results(big.decompress(src, io, il, torch.from_numpy(caps).cuda()), n)
    got = _results(big.decompress(src, io, il), n)
    assert got[1] == ref[1] and got[2] == ref[2]
    assert got[0] == ref[0]
    for i, (_, t, plain) in enumerate(mixed):
        if plain is not None:
            assert got[2][i] == 0 and got[0][i] == plain, i
    # aligned: every offset a multiple of 256, the same content
    al = _results(big.decompress(src, io, il, align=256), n)
    assert all(o % 256 == 0 for o in al[3]) and len(set(al[3])) > n // 2
    assert al[:3] == ref[:3]
    assert any(o % 256 for o in got[3])


def test_decompress_without_sizes_with_a_dictionary(small):
    d = corpus.make(4242, 1, 20000, mix=ord("T")).tobytes()
    sizes = (0, 1, 100, 5000, 16384, 16385, 40000, 65536)
    datas = [(d[1000:1000 + s // 2] + corpus.make(7000 + i, 1, s, mix=ord("T")).tobytes())[:s] for i, s in enumerate(sizes)]
    frames = _compress(small, datas, dictionary=d)
    src, io, il = _up(frames)
    dd = torch.from_numpy(np.frombuffer(d, dtype=np.uint8).copy()).cuda()
    n = len(frames)
    ref = _results(small.decompress(src, io, il, torch.tensor([len(x) for x in datas], dtype=torch.int32).cuda(), dictionary=dd), n)
    got = _results(small.decompress(src, io, il, dictionary=dd), n)
    assert got[:3] == ref[:3] and got[0] == datas and not any(got[2])


def test_damaged_entries_among_good_ones(big, rows):
    by = {n: e for n, e, _ in rows}
    datas = [corpus.make(8000 + i, 1, s).tobytes() for i, s in enumerate((10, 700, 5000, 20000, 65536, 131072, 3, 1000, 9000, 300))]
    good = _compress(big, datas)
    frame = good[3]
    first_block = hf.block_bounds(frame)[0][0]
    damaged = {2: b"\x29" + frame[1:], 5: frame[:first_block + 3 + 100], 8: frame[:4] + bytes([frame[4] | 8]) + frame[5:],
               11: by["fcs8 edited 5 GiB declared"]}       # wrong magic, cut inside its first block, reserved bit; a bound no 32-bit capacity holds
    entries, plain = [], []
    it = iter(zip(good, datas))
    for i in range(len(good) + len(damaged)):
        f, p = (damaged[i], None) if i in damaged else next(it)
        entries.append(f); plain.append(p)
    n = len(entries)
    src, io, il = _up(entries)
    info = hf.host_info(entries)
    assert [int(info["status"][i]) for i in sorted(damaged)] == [10, 72, 14, 0] and int(info["bound"][11]) == 5 << 30
    # the C ABI's steps, the destination the test's own: canary everywhere, the regions MARGIN behind its start
    off, cap, total = big.layout(big._frame_info_raw(src, io, il), 16)
    torch.cuda.synchronize()
    tot = [int(x) for x in total.cpu()]
    assert tot[1] == 4 and tot[0] == sum((len(p) + 15) & ~15 for p in plain if p is not None)
    can = np.random.default_rng(9).integers(0, 256, tot[0] + 2 * MARGIN, dtype=np.uint8)
    dst = torch.from_numpy(can.copy()).cuda()
    r = _results(big.decompress(src, io, il, cap, dst=dst, out_off=off + MARGIN), n)
    keep = np.ones(len(can), dtype=bool)
    for i in range(n):
        if i in damaged:
            assert int(cap[i]) == 0 and r[1][i] == 0 and r[2][i] != 0, (i, r[1][i], r[2][i])
        else:
            assert r[2][i] == 0 and r[0][i] == plain[i], i
            keep[r[3][i]:r[3][i] + r[1][i]] = False
    assert np.array_equal(dst.cpu().numpy()[keep], can[keep]), "bytes outside the laid-out regions changed"
    # ... and in one call
    g = _results(big.decompress(src, io, il), n)
    assert g[1] == r[1] and g[2] == r[2] and g[0] == r[0]


def test_host_batch_without_caps(big):
    from kompressor_amd.batch import decompress_host_batch
    datas = [corpus.make(9000 + i, 1, s).tobytes() if s else b"" for i, s in enumerate((0, 1, 500, 4096, 30000, 65536, 131072))]
    frames = _compress(big, datas)
    with_caps = decompress_host_batch(frames, [len(d) for d in datas])
    without = decompress_host_batch(frames)
    assert without == with_caps and without[0] == datas and not any(without[1])
