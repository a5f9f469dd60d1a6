"""zstd levels 1, 2 and the negative ones with a dictionary on the CPU wave emulator: the host's CDict of strategy "fast"
(zstd_cdict_host.h), the body of k_zstd_match_fast_dict (zstd_match_fast_dict.h) and the entropy body against the frames of the binary
libzstd 1.5.7 (tests/golden/zstd_dict_levels_golden.json), and the decoder bodies with the dictionary back to the input."""
import random

import pytest

import helpers
import helpers_dict_levels as hd

EMU_LEVELS = (1, 2, -5)
# (dictionary, largest slice run here): both rows of the CDict's parameters and the sizes next to their change, a dictionary of which a
# level-1 CDict indexes only the end, a corpus class, formatted dictionaries; one dictionary with the slices of a whole block
EMU_DICTS = (("raw_8", 16385), ("raw_4096", 16385), ("raw_15885", 16385), ("raw_15886", 16385), ("raw_65536", 16385), ("raw_S_32768", 8193),
             ("built0_", 16385), ("built1_", 16385))


def _case(name):
    """the case of that name (a formatted dictionary: by the start of its name)"""
    return next(c for c in hd.cases() if c[0] == name or (name.endswith("_") and c[0].startswith(name)))


def test_cases_cover_what_the_parser_branches_on():
    """The golden file's cases: every (dictionary, level) row is there, slices on both sides of the attach cut-off and at a whole block,
    the three kinds of content, raw and formatted dictionaries."""
    G = hd.golden()
    names = [c[0] for c in hd.cases()]
    assert [f"raw_{n}" for n in hd.DICT_SIZES] == names[:len(hd.DICT_SIZES)]
    assert sum(1 for _, d, _ in hd.cases() if d[:4] == b"\x37\xA4\x30\xEC") == 5
    for name, d, slices in hd.cases():
        for level in hd.levels_of(name):
            assert len(G[(name, level)]["frames"]) == len(slices)
    sl = [s for s, _ in _case("raw_65536")[2]]
    assert {"shared_8193", "other_8193", "substr_8193"} <= set(sl)
    assert {len(p) for _, p in _case("raw_4096")[2]} == set(hd.SLICE_SIZES)
    assert (hd.FEW_ROWS_LEVEL in hd.levels_of("raw_4096")) and len(G) == len(names) * len(hd.LEVELS) + 1


def test_cdict_parameters_of_the_fast_rows():
    """windowLog, hashLog, minMatch of ZSTD_getCParams in create-CDict mode at levels 1, 2 and row 0, on both sides of the row change (the
    binary library changes rows between 15 885 and 15 886 bytes) and for the smallest and the largest dictionary."""
    want = {1: ((14, 15, 5), (17, 13, 6)), 2: ((14, 15, 4), (17, 15, 5)), -1: ((14, 13, 5), (17, 12, 5)), -7: ((14, 13, 5), (17, 12, 5))}
    for level, (small, large) in want.items():
        for dsz, row, w in ((8, small, 10), (4096, small, 13), (15885, small, 14), (15886, large, 15), (65536, large, 17), (130560, large, 17)):
            W, C, H, M = hd.emu_params(dsz, level)
            assert (W, H, M) == (w, min(row[1], w + 1), row[2]), (level, dsz, (W, C, H, M))
    assert hd.emu_params(4096, 3) == (13, 13, 14, 4) and hd.emu_params(40000, 3) == (16, 15, 16, 5)      # level 3: as before


@pytest.mark.parametrize("name,largest", EMU_DICTS)
def test_emulated_parser_equals_libzstd(name, largest):
    """Attached CDict (slices up to 8 KiB) and copied table (above), raw and formatted dictionaries, levels 1, 2 and -5: the golden
    frames; and the emulated decoder with the dictionary gives the inputs back."""
    name, d, slices = _case(name)
    keep = [i for i, (_, p) in enumerate(slices) if len(p) <= largest]
    assert any(len(slices[i][1]) <= 8192 for i in keep) and any(len(slices[i][1]) > 8192 for i in keep)
    for k, level in enumerate(EMU_LEVELS):
        row = hd.golden()[(name, level)]
        assert row["dict_sha256"] == helpers.sha256(d)
        frames = hd.emu_compress([slices[i][1] for i in keep], d, level, G=(4, 8, 2)[k])
        bad = [(slices[i][0], len(f), row["frames"][i][0]) for i, f in zip(keep, frames) if [len(f), helpers.sha256(f)] != row["frames"][i]]
        assert not bad, f"{name} level {level}: (slice, frame, libzstd's frame) {bad}"
        if level != 2:
            plain = [slices[i][1] for i in keep]
            outs, sts = helpers.emu_decompress(frames, [max(len(p), 1) for p in plain], dictionary=d)
            assert list(sts) == [0] * len(frames) and outs == plain, (name, level)


def test_emulated_parser_on_a_whole_block():
    """The slice sizes at which libzstd could leave the CDict aside (128 KiB and at least six times the dictionary): with
    ZSTD_CCtx_loadDictionary it never does -- the frames of 131 071 and 131 072 bytes with a dictionary of 4 KiB are the copied-table
    parser's, at level 1 and at the lowest level."""
    _, d, slices = _case("raw_4096")
    keep = [i for i, (_, p) in enumerate(slices) if len(p) >= 131071]
    assert len(keep) == 2
    for level in (1, hd.FEW_ROWS_LEVEL):
        row = hd.golden()[("raw_4096", level)]
        frames = hd.emu_compress([slices[i][1] for i in keep], d, level, G=16)
        assert [[len(f), helpers.sha256(f)] for f in frames] == [row["frames"][i] for i in keep], level


def test_ragged_batch_against_the_live_library():
    """One seeded ragged batch -- lengths 0 .. 12 000 on both sides of 8 KiB, dictionary pieces mixed with fresh text, more slices than
    teams -- against the machine's libzstd 1.5.7 directly."""
    try:
        from oracle.libzstd_ref import LibZstd
        z = LibZstd()
    except (RuntimeError, OSError):
        pytest.skip("no binary libzstd 1.5.7 on this machine")
    rng = random.Random(9917)
    d = hd.word_text(77, 20000, 1)
    datas = []
    for t in range(14):
        n = rng.choice([0, 7, 8, 9, rng.randrange(10, 3000), rng.randrange(7000, 8193), rng.randrange(8193, 12000)])
        fresh = hd.word_text(300 + t, n, 1 + t % 2)
        parts, have = [], 0
        while have < n:
            a = rng.randrange(len(d))
            seg = d[a:a + rng.choice([5, 30, 400])] if rng.random() < 0.4 else fresh[have:have + rng.choice([3, 50, 700])]
            parts.append(seg); have += len(seg)
        datas.append(b"".join(parts)[:n])
    for level, G in ((1, 4), (-3, 8)):
        assert hd.emu_compress(datas, d, level, G=G, nblocks=1) == [z.compress_with_dict(p, d, level) for p in datas], level
