"""The inflate sizing pass on the device (kmp_inflate_info_batch: k_inflate_size) and the inflate that needs no sizes from its caller
(ZstdBatch.inflate(out_cap=None)): the fixture of tests/golden/inflate_info_golden.json in batches of several sizes at hostile layouts,
the decode made of the answers against zlib, seeded mutants against the live zlib, the memory and ordering contract, both builds of
the library."""
import ctypes
import zlib

import numpy as np
import pytest

import helpers_inflate_info as hi
import layouts

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

FORMATS = (0, 1, 2, 3)


def _ctx(**kw):
    from kompressor_amd.batch import ZstdBatch
    assert torch.cuda.is_available(), "these tests need the MI355X"
    return ZstdBatch(**kw)


@pytest.fixture(scope="module")
def ctx():
    b = _ctx(max_slices=2048, max_slice_bytes=65536)
    yield b
    b.close()


@pytest.fixture(scope="module")
def rows():
    return hi.golden()


def _dev(src, offs, lens):
    return (torch.from_numpy(np.ascontiguousarray(src)).cuda(), torch.from_numpy(np.asarray(offs).astype(np.int64)).cuda(),
            torch.from_numpy(np.asarray(lens).astype(np.int32)).cuda())


def _info(b, src, io, il, fmt):
    """inflate_info -> INFO array (the dict's views put together again)"""
    d = b.inflate_info(src, io, il, format=hi.FMT_NAMES[fmt])
    torch.cuda.synchronize()
    out = np.zeros(il.numel(), dtype=hi.INFO)
    for f in hi.FIELDS:
        out[f] = d[f].cpu().numpy().astype(hi.INFO[f])
    return out


def test_library_has_the_export(ctx):
    assert hasattr(ctx.lib, "kmp_inflate_info_batch")


@pytest.mark.parametrize("n", (1, 15, 16, 17, 64, 65, 1030))
@pytest.mark.parametrize("fmt", FORMATS)
def test_fixture_in_batches(ctx, rows, fmt, n):
    """the fixture repeated to n entries, each a region of its own at an unaligned offset, in a permuted order"""
    mine = [r for r in rows if r[2] == fmt]
    part = [mine[k % len(mine)] for k in range(n)]
    L = layouts.exact([r[1] for r in part], [32] * n, seed=100 * fmt + n)
    got = _info(ctx, *_dev(L.src, L.in_off, L.in_len), fmt)
    want = hi.expected_array([r[3] for r in part])
    bad = hi.diff(got, want, [r[0] for r in part])
    assert not bad, "\n".join(bad[:20])
    assert got.tobytes() == want.tobytes()


@pytest.mark.parametrize("fmt", (0, 1, 2))
def test_fixture_aliased(ctx, rows, fmt):
    """entries that name the same bytes, prefixes, suffixes and overlapping middles of them, empty ranges: the emulated kernel's answers
    (which the CPU tests hold against the fixture and zlib), and zlib's rule once more"""
    bodies = [r[1] for r in rows if r[2] == fmt and r[3]["kind"] == "ok" and 8 <= len(r[1]) <= 4096][:8]
    L = layouts.aliased(bodies, lambda ln: 32, seed=300 + fmt)
    got = _info(ctx, *_dev(L.src, L.in_off, L.in_len), fmt)
    cases = [(f"aliased {i}", d, fmt) for i, d in enumerate(L.datas)]
    assert got.tobytes() == hi.emu_cases(cases).tobytes()
    bad, counts = hi.check_against_zlib(cases, got)
    assert not bad and counts["ok"] >= 2 * len(bodies), (bad[:10], counts)


@pytest.mark.parametrize("align", (1, 256))
@pytest.mark.parametrize("fmt", FORMATS)
def test_inflate_without_sizes(ctx, rows, fmt, align):
    """on the parent commit this call raises (out_cap was required): the test that fails without the feature"""
    part = [r for r in rows if r[2] == fmt and r[3]["kind"] == "ok"]
    src, io, il = _dev(*hi.pack([r[1] for r in part], seed=fmt))
    dst, oo, ol, st = (t.cpu().numpy() for t in ctx.inflate(src, io, il, out_cap=None, format=hi.FMT_NAMES[fmt], align=align))
    for i, r in enumerate(part):
        ref = zlib.decompressobj(hi.WBITS[fmt]).decompress(r[1])
        assert int(st[i]) == 0 and int(oo[i]) % align == 0, r[0]
        assert dst[int(oo[i]):int(oo[i]) + int(ol[i])].tobytes() == ref, r[0]


@pytest.mark.parametrize("fmt", FORMATS)
def test_inflate_without_sizes_mixed_batch(ctx, rows, fmt):
    """rejected entries among good ones: the others decode, the rejected ones get capacity 0 and a status of the decoder's; an entry zlib
    refuses for its data check alone gets its size from the sizing pass and its status from the decoder"""
    part = [r for r in rows if r[2] == fmt and len(r[1]) <= 4096]
    src, io, il = _dev(*hi.pack([r[1] for r in part], seed=10 + fmt))
    info = ctx._inflate_info_raw(src, io, il, fmt)
    _, cap, _ = ctx.layout(info, 64)
    dst, oo, ol, st = (t.cpu().numpy() for t in ctx.inflate(src, io, il, out_cap=None, format=hi.FMT_NAMES[fmt], align=64))
    cap = cap.cpu().numpy()
    kinds = set()
    for i, r in enumerate(part):
        kind, val = hi.verdict(r[1], fmt)
        kinds.add(kind)
        if kind == "ok":
            assert int(st[i]) == 0 and dst[int(oo[i]):int(oo[i]) + int(ol[i])].tobytes() == val, r[0]
        else:
            assert int(st[i]) != 0 and int(ol[i]) == 0, r[0]
            assert kind == "checksum" or int(cap[i]) == 0, r[0]
    assert kinds >= {"ok", "reject"}
    for a in ({"dst": dst}, {"out_off": oo}):
        with pytest.raises(ValueError):
            ctx.inflate(src, io, il, out_cap=None, **a)
    with pytest.raises(ValueError):
        ctx.inflate(src, io, il, out_cap=torch.zeros(len(part), dtype=torch.int32, device="cuda"), align=64)


def test_mutants_against_the_live_zlib(ctx):
    """the mutants the emulator has walked (tests/test_emu_inflate_info.py), one batch per format"""
    from test_emu_inflate_info import MUTANT_SEED, N_MUTANTS
    muts = hi.mutants(N_MUTANTS, MUTANT_SEED)
    got = np.zeros(len(muts), dtype=hi.INFO)
    for fmt, idx in hi.by_fmt_cases(muts).items():
        assert len(idx) <= 2048
        got[idx] = _info(ctx, *_dev(*hi.pack([muts[i][1] for i in idx], seed=fmt)), fmt)
    bad, counts = hi.check_against_zlib(muts, got)
    print(f"{len(muts)} mutants: zlib alone says {counts}")
    hi.assert_not_hollow(counts)
    assert not bad, "\n".join(bad[:20])


def test_context_memory_untouched(rows):
    b = _ctx(max_slices=64, max_slice_bytes=65536)
    try:
        before = b.memory()
        part = [r for r in rows if r[2] == 0][:64]
        src, io, il = _dev(*hi.pack([r[1] for r in part]))
        got = _info(b, src, io, il, 0)
        assert got.tobytes() == hi.expected_array([r[3] for r in part]).tobytes()
        assert b.memory() == before and before["decode_staging"] == 0
    finally:
        b.close()


def test_queued_back_to_back(ctx, rows):
    """two sizing calls and a deflate on one stream without a host wait between them: the answers of separate runs"""
    raw = [r for r in rows if r[2] == 0 and len(r[1]) <= 4096][:100]
    gz = [r for r in rows if r[2] == 2][:100]
    a, b = _dev(*hi.pack([r[1] for r in raw])), _dev(*hi.pack([r[1] for r in gz]))
    datas = [bytes([i]) * 300 + bytes(range(200)) for i in range(40)]
    d = _dev(*hi.pack(datas))
    i1 = ctx._inflate_info_raw(*a, 0)
    i2 = ctx._inflate_info_raw(*b, 2)
    dst, oo, ol = ctx.deflate(*d)
    torch.cuda.synchronize()
    assert i1.cpu().numpy().tobytes() == hi.expected_array([r[3] for r in raw]).tobytes()
    assert i2.cpu().numpy().tobytes() == hi.expected_array([r[3] for r in gz]).tobytes()
    dd, oo, ol = dst.cpu().numpy(), oo.cpu().numpy(), ol.cpu().numpy()
    for k, x in enumerate(datas):
        assert zlib.decompress(dd[int(oo[k]):int(oo[k]) + int(ol[k])].tobytes(), -15) == x


def test_arguments(ctx, rows):
    lib, p = ctx.lib, ctypes.c_void_p
    src, io, il = _dev(*hi.pack([rows[0][1]]))
    info = torch.zeros(4, dtype=torch.int64, device="cuda")
    args = (p(src.data_ptr()), p(io.data_ptr()), p(il.data_ptr()))
    assert lib.kmp_inflate_info_batch(ctx._h, None, None, None, 0, None, 0, ctx._stream()) == 0
    assert lib.kmp_inflate_info_batch(ctx._h, *args, 1, None, 0, ctx._stream()) == -2
    assert lib.kmp_inflate_info_batch(ctx._h, *args, 1, p(info.data_ptr()), 4, ctx._stream()) == -2
    assert lib.kmp_inflate_info_batch(None, *args, 1, p(info.data_ptr()), 0, ctx._stream()) == -2
    assert lib.kmp_inflate_info_batch(ctx._h, *args, 2049, p(info.data_ptr()), 0, ctx._stream()) != 0
    assert lib.kmp_inflate_info_batch(ctx._h, *args, 1, p(info.data_ptr()), 0, ctx._stream()) == 0
    torch.cuda.synchronize()


def test_both_builds_agree(rows):
    b = _ctx(max_slices=512, max_slice_bytes=65536, ablations=True)
    try:
        for fmt in FORMATS:
            part = [r for r in rows if r[2] == fmt]
            got = _info(b, *_dev(*hi.pack([r[1] for r in part], seed=fmt)), fmt)
            assert got.tobytes() == hi.expected_array([r[3] for r in part]).tobytes()
    finally:
        b.close()
