"""The bodies of k_zstd_frame_info and k_batch_layout (kompressor_amd/csrc/zstd_frame_info.h) on the CPU wave emulator: the fixture
as one batch, at the hostile layouts of tests/layouts.py, with every entry ending on the last byte in front of a PROT_NONE page; the
layout kernel against numpy's 64-bit cumsum.  No GPU."""
import numpy as np
import pytest

import helpers_frame_info as hf
import layouts

LAYOUT_NS = (1, 2, 63, 64, 65, 1023, 1024, 1025, 4097)
ALIGNS = (1, 16, 4096)


@pytest.fixture(scope="module")
def rows():
    return hf.golden()


@pytest.fixture(scope="module")
def want(rows):
    return hf.expected_array([r for _, _, r in rows])


def test_fixture_as_one_batch(rows, want):
    src, offs, lens = hf.pack([e for _, e, _ in rows])
    for nblocks, waves in ((1, 1), (2, 2), (1, 4)):            # grids smaller than the batch: the stride loop; several waves a workgroup
        got = hf.emu_frame_info(src, offs, lens, nblocks, waves)
        bad = hf.diff(got, want, [n for n, _, _ in rows])
        assert not bad, "\n".join(bad[:20])


@pytest.mark.parametrize("filler", ("random", "complement"))
def test_hostile_layout_exact(rows, want, filler):
    """unaligned permuted offsets, canary bytes of 1 .. 63 between the entries"""
    entries = [e for _, e, _ in rows]
    L = layouts.exact(entries, [32] * len(entries), seed=41, filler=filler)
    L.check_residues()
    got = hf.emu_frame_info(L.src, L.in_off.astype(np.uint64), L.in_len.astype(np.uint32))
    bad = hf.diff(got, want, [n for n, _, _ in rows])
    assert not bad, "\n".join(bad[:20])


def test_hostile_layout_flush_and_behind(rows, want):
    """entries flush against each other (what lies behind an entry is the next one's frame), and each followed by a valid frame"""
    entries = [e for _, e, _ in rows]
    src, offs, lens = hf.pack(entries, gap=0)
    got = hf.emu_frame_info(src, offs, lens)
    assert not hf.diff(got, want, [n for n, _, _ in rows])
    good = next(e for n, e, _ in rows if n == "fcs1 single segment")
    L = layouts.decode_layout(entries, good, [32] * len(entries), seed=43, filler="random")
    got = hf.emu_frame_info(L.src, L.in_off.astype(np.uint64), L.in_len.astype(np.uint32))
    bad = hf.diff(got, want, [n for n, _, _ in rows])
    assert not bad, "\n".join(bad[:20])


def test_hostile_layout_aliased(rows):
    """entries that name the same bytes, prefixes, suffixes and overlapping middles of them, empty ranges: each equals the host body's
    answer for its own bytes (and the whole bodies equal the fixture)"""
    pick = ("three frames", "skippable between", "streaming 2 blocks", "checksum", "fcs2 5000", "sized frame, then streaming frame")
    by = {n: (e, r) for n, e, r in rows}
    bodies = [by[n][0] for n in pick]
    L = layouts.aliased(bodies, lambda ln: 32, seed=47)
    got = hf.emu_frame_info(L.src, L.in_off.astype(np.uint64), L.in_len.astype(np.uint32))
    ref = hf.host_info(L.datas)
    assert got.tobytes() == ref.tobytes()
    whole = {b: hf.expected(by[n][1]) for n, b in zip(pick, bodies)}
    seen = 0
    for d, g in zip(L.datas, got):
        if d in whole:
            assert tuple(int(x) for x in g) == whole[d]
            seen += 1
    assert seen >= 2 * len(pick)


def test_entries_end_at_a_guard_page(rows, want):
    """every entry ends on the last byte in front of a PROT_NONE page (and a short one starts right behind one): a read past the end
    kills the process"""
    from fuzz_decoders import Guarded
    got = np.zeros(len(rows), dtype=hf.INFO)
    for i, (_, e, _) in enumerate(rows):
        g = Guarded(max(len(e), 1), 0)
        at = g.off + (1 if not e else 0)                       # an empty entry: the address of the guard page's first byte
        g.write(e)
        got[i] = hf.emu_frame_info(g.base, np.array([at], dtype=np.uint64), np.array([len(e)], dtype=np.uint32), 1, 1)[0]
        g.close()
    bad = hf.diff(got, want, [n for n, _, _ in rows])
    assert not bad, "\n".join(bad[:20])


def _random_info(n, rng, big=False):
    info = np.zeros(n, dtype=hf.INFO)
    info["bound"] = rng.integers(0, 1 << 17, n, dtype=np.uint64) if not big else (1 << 32) - 1 - rng.integers(0, 4096, n, dtype=np.uint64)
    info["content"] = info["bound"]
    info["frames"] = 1
    return info


@pytest.mark.parametrize("align", ALIGNS)
@pytest.mark.parametrize("n", LAYOUT_NS)
def test_layout_against_cumsum(n, align):
    rng = np.random.default_rng(1000 * n + align)
    info = _random_info(n, rng)
    info["bound"][rng.random(n) < 0.1] = 0                     # empty frames among them
    off, cap, total = hf.emu_layout(info, align)
    roff, rcap, rtotal = hf.layout_reference(info, align)
    assert np.array_equal(cap, rcap) and np.array_equal(off, roff) and np.array_equal(total, rtotal)
    assert all(int(o) % align == 0 for o in off)


@pytest.mark.parametrize("n,crosses", ((3, 1 << 32), (9, 1 << 33), (4097, 1 << 33)))
def test_layout_totals_beyond_32_bits(n, crosses):
    rng = np.random.default_rng(n)
    info = _random_info(n, rng, big=True)
    for align in (1, 4096):
        off, cap, total = hf.emu_layout(info, align)
        roff, rcap, rtotal = hf.layout_reference(info, align)
        assert np.array_equal(cap, rcap) and np.array_equal(off, roff) and np.array_equal(total, rtotal)
        assert int(total[0]) > crosses and int(total[1]) == 0 and int(off[-1]) >= (1 << 32)


def test_layout_refuses_rejected_and_oversized_entries():
    rng = np.random.default_rng(5)
    n = 300
    info = _random_info(n, rng)
    rejected = rng.random(n) < 0.2
    info["status"][rejected] = rng.choice((10, 14, 16, 20, 72), int(rejected.sum()))
    # (the parse leaves content and bound 0 with a status; a layout kernel that looked at the bound alone must still be caught)
    oversized = ~rejected & (rng.random(n) < 0.2)
    info["bound"][oversized] = rng.choice(np.array(((1 << 32), (1 << 32) + 5, 17 << 40, hf.ERROR, hf.UNKNOWN), dtype=np.uint64), int(oversized.sum()))
    info["bound"][0] = (1 << 32) - 1                           # the largest capacity the ABI holds is served
    info["status"][0] = 0
    oversized[0] = rejected[0] = False
    for align in ALIGNS:
        off, cap, total = hf.emu_layout(info, align)
        roff, rcap, rtotal = hf.layout_reference(info, align)
        assert np.array_equal(cap, rcap) and np.array_equal(off, roff) and np.array_equal(total, rtotal)
        assert int(total[1]) == int(rejected.sum() + oversized.sum()) > 0
        assert not cap[rejected].any() and not cap[oversized].any() and int(cap[0]) == (1 << 32) - 1
