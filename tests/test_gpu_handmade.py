"""The hand-made zstd frames of tests/helpers_handmade.py on the device against what libzstd 1.5.7 answered for them
(tests/golden/zstd_handmade_golden.json): the whole fixture as one batch through kmp_zstd_decompress_batch at the cases' capacities, with
the pre-decode kernels and without them (the ablation build's KMP_DECODE_PRE = 0, as tests/test_gpu_layout.py switches them), at an exact
and a tempting layout with canaries, through ZstdBatch.decompress(out_cap=None) and frame_info, the dictionary cases through the
dictionary call; the ablation build against the normal one, the device against the CPU emulator.  No case is left out on the device."""
import numpy as np
import pytest

import helpers_frame_info as hf
import helpers_handmade as hh
import layouts as LY

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

SLICE = 256 * 1024            # the largest outputs are about 200 KiB


@pytest.fixture(scope="module")
def fixture():
    return hh.golden()


def _ctx(n, **kw):
    from kompressor_amd.batch import ZstdBatch
    assert torch.cuda.is_available(), "these tests need the MI355X"
    return ZstdBatch(max_slices=n, max_slice_bytes=SLICE, **kw)


@pytest.fixture(scope="module")
def ctx(fixture):
    b = _ctx(len(fixture[0]))
    yield b
    b.close()


def _plain(cs):
    return [i for i, c in enumerate(cs) if c[4] is None]


def _answers(r, n, off=None):
    dd, oo, ol, st = (t.cpu().numpy() for t in r)
    return [(int(st[i]), int(ol[i]), hh.sha256(dd[int(oo[i]):int(oo[i]) + int(ol[i])].tobytes()) if int(st[i]) == 0 else "") for i in range(n)]


def _decode(b, cs, dictionary=None):
    """the cases packed back to back with no padding, capacities as the cases have them -> [(status, out_len, sha256)]"""
    src, offs, lens = hf.pack([c[2] for c in cs])
    caps = np.array([c[3] for c in cs], dtype=np.int32)
    dd = None if dictionary is None else torch.from_numpy(np.frombuffer(dictionary, dtype=np.uint8).copy()).cuda()
    r = b.decompress(torch.from_numpy(src).cuda(), torch.from_numpy(offs.astype(np.int64)).cuda(), torch.from_numpy(lens.astype(np.int32)).cuda(),
                     out_cap=torch.from_numpy(caps).cuda(), dictionary=dd)
    torch.cuda.synchronize()
    return _answers(r, len(cs))


@pytest.fixture(scope="module")
def device(ctx, fixture):
    """the cases without a dictionary through the normal build, the pre-decoders on (KMP_PRE_MIN_BATCH = 1, tests/conftest.py)"""
    cs = fixture[0]
    return _decode(ctx, [cs[i] for i in _plain(cs)])


def _compare(fixture, idx, got):
    cs, rows = fixture
    return hh.compare([cs[i] for i in idx], [rows[i] for i in idx], got)


def test_batch_behind_the_predecoders(fixture, device):
    idx = _plain(fixture[0])
    assert len(idx) >= 1000
    bad = _compare(fixture, idx, device)
    assert not bad, f"{len(bad)} differ\n" + "\n".join(bad[:30])


def test_batch_without_the_predecoders_and_the_ablation_build(fixture, device, monkeypatch):
    """k_zstd_decode alone (the ablation build's KMP_DECODE_PRE = 0), then the ablation build with the pre-decoders on: the library's
    answers, and the normal build's statuses, lengths and bytes, entry for entry"""
    cs = fixture[0]
    idx = _plain(cs)
    sub = [cs[i] for i in idx]
    monkeypatch.setenv("KMP_DECODE_PRE", "0")
    b = _ctx(len(sub), ablations=True)
    try:
        alone = _decode(b, sub)
    finally:
        b.close()
    monkeypatch.delenv("KMP_DECODE_PRE")
    b = _ctx(len(sub), ablations=True)
    try:
        ablation = _decode(b, sub)
    finally:
        b.close()
    bad = _compare(fixture, idx, alone)
    bad += [f"{c[0]} / {c[1]}: alone {a[:2]}, behind the pre-decoders {d[:2]}" for c, a, d in zip(sub, alone, device) if a != d]
    bad += [f"{c[0]} / {c[1]}: the ablation build {a[:2]}, the normal build {d[:2]}" for c, a, d in zip(sub, ablation, device) if a != d]
    assert not bad, f"{len(bad)} differ\n" + "\n".join(bad[:30])


@pytest.mark.parametrize("family", ["exact", "tempting"])
def test_batch_at_hostile_layouts(ctx, fixture, device, family):
    """exact: every entry a region of its own, d_out_cap the slot, canary gaps of 1 .. 63 bytes, starts on every residue modulo 64;
    tempting: right behind every entry lies a valid frame of other content.  Both twins; the answers of the packed batch, nothing
    outside [out_off, + capacity) touched, nothing outside the output of an accepted entry"""
    cs = fixture[0]
    idx = _plain(cs)
    sub = [cs[i] for i in idx]
    behind = b"" if family == "exact" else hh.frame(hh.raw(b"INTRUDER " * 30, 1))
    caps = [c[3] for c in sub]
    for L in LY.twins(lambda f: LY.decode_layout([c[2] for c in sub], behind, caps, 4100 + len(behind), f)):
        L.check_residues(64)
        dst = torch.from_numpy(L.new_dst()).cuda()
        r = ctx.decompress(torch.from_numpy(L.src).cuda(), torch.from_numpy(L.in_off).cuda(), torch.from_numpy(L.in_len).cuda(),
                           torch.tensor(caps, dtype=torch.int32).cuda(), dst=dst, out_off=torch.from_numpy(L.out_off).cuda())
        torch.cuda.synchronize()
        got = _answers(r, len(sub))
        bad = [f"{c[0]} / {c[1]}: {g[:2]} at this layout, {d[:2]} packed" for c, g, d in zip(sub, got, device) if g != d]
        bad += L.check(dst.cpu().numpy(), [g[1] for g in got], allowed=[g[1] if g[0] == 0 else c for g, c in zip(got, caps)])
        assert not bad, f"{len(bad)} findings\n" + "\n".join(bad[:30])


def test_unknown_sizes_and_frame_info(ctx, fixture):
    """ZstdBatch.decompress(out_cap=None): the device's frame info equals the library's; what the library accepts decodes to its bytes"""
    cs, rows = fixture
    idx = _plain(cs)
    src, offs, lens = hf.pack([cs[i][2] for i in idx])
    dev = (torch.from_numpy(src).cuda(), torch.from_numpy(offs.astype(np.int64)).cuda(), torch.from_numpy(lens.astype(np.int32)).cuda())
    info = ctx.frame_info(*dev)
    torch.cuda.synchronize()
    cols = {f: info[f].cpu().numpy() for f in hh.INFO_FIELDS}
    got = [[int(cols[f][k]) & ((1 << 64) - 1 if f in ("content", "bound") else 0xFFFFFFFF) for f in hh.INFO_FIELDS] for k in range(len(idx))]
    bad = [f"{cs[i][0]} / {cs[i][1]}: frame info {g}, the library {rows[i]['info']}" for i, g in zip(idx, got) if g != rows[i]["info"]]
    r = ctx.decompress(*dev, out_cap=None)
    torch.cuda.synchronize()
    ans = _answers(r, len(idx))
    small = 0
    for i, a in zip(idx, ans):
        w = rows[i]
        if w["status"] != 0 or cs[i][5] == "lenient":
            continue
        # (the capacity is the bound; a raw or RLE block above the block maximum holds more than ZSTD_decompressBound allows for it,
        # and the library itself answers 70 at that capacity)
        want = (0, w["out_len"], w["out_sha256"]) if w["out_len"] <= w["info"][1] else (70, 0, "")
        if cs[i][1] in hh.REFUSED_THOUGH_ACCEPTED:
            want = (hh.REFUSED_THOUGH_ACCEPTED[cs[i][1]], 0, "")
        small += want[0] == 70
        if a != want:
            bad.append(f"{cs[i][0]} / {cs[i][1]}: {a[:2]}, expected {want[:2]}")
    assert small == 4
    assert sum(1 for i in idx if rows[i]["status"] == 0) >= 500
    assert not bad, f"{len(bad)} differ\n" + "\n".join(bad[:30])


def test_dictionary_cases(ctx, fixture):
    cs = fixture[0]
    idx = [i for i, c in enumerate(cs) if c[4] is not None]
    assert len(idx) >= 50 and sum(1 for i in idx if "first block in Repeat mode" in cs[i][1] or "tree-less literals" in cs[i][1]) >= 16
    bad = []
    for d in sorted({cs[i][4] for i in idx}):
        sub = [i for i in idx if cs[i][4] == d]
        bad += _compare(fixture, sub, _decode(ctx, [cs[i] for i in sub], dictionary=d))
    assert not bad, f"{len(bad)} differ\n" + "\n".join(bad[:30])


def test_device_equals_the_emulator(fixture, device):
    """status and length, entry for entry"""
    cs = fixture[0]
    sub = [cs[i] for i in _plain(cs)]
    emu = hh.emu_decode(sub, pre=True)
    bad = [f"{c[0]} / {c[1]}: the device {d[:2]}, the emulator {e[:2]}" for c, d, e in zip(sub, device, emu) if d[:2] != e[:2]]
    assert not bad, f"{len(bad)} differ\n" + "\n".join(bad[:30])
