"""The parsers' shared team pieces (kompressor_amd/csrc/zstd_team.h) on the CPU wave emulator: the sequence sink's edges, driven
directly, and a ladder of small slices through the real parse bodies whose sequence counts sit on those edges."""
import numpy as np
import pytest

import helpers
import helpers_dict_levels as hd
import helpers_team as ht


def _triples(n, ml_last):
    """n sequences with known values; one has ll = 0x10000 and one mlBase = 0x10000 (where n allows both), the latter at the end or
    the former."""
    t = [[3 + 7 * i, (5 * i + 1) & 0xFFFF, (11 * i + 2) & 0xFFFF] for i in range(n)]
    if n >= 1:
        t[n - 1 if ml_last else n // 3][2] = 0x10000
    if n >= 2:
        t[n // 3 if ml_last else n - 1][1] = 0x10000
    return t


@pytest.mark.parametrize("ml_last", (True, False))
@pytest.mark.parametrize("G", (2, 8, 64))
def test_sink_edges(G, ml_last):
    for n in (0, 1, 2 * G - 1, 2 * G, 2 * G + 1, 4 * G, 4 * G + 3):
        t = _triples(n, ml_last)
        regions, meta = ht.emu_sink(G, t)
        # a plain loop's output
        want = np.zeros(n, dtype=ht.SEQ)
        long_type = long_pos = lit = 0
        for i, (ob, ll, ml) in enumerate(t):
            want[i] = (ob, ll & 0xFFFF, ml & 0xFFFF)
            if ll > 0xFFFF:
                long_type, long_pos = 1, i
            if ml > 0xFFFF:
                long_type, long_pos = 2, i
            lit += ll
        assert len(regions) == 64 // G
        for team, seqs in enumerate(regions):
            assert seqs[:n].tobytes() == want.tobytes(), (G, n, team)
            assert (seqs[n:].view(np.uint32) == 0xA5A5A5A5).all(), f"G {G}, {n} sequences, team {team}: the sink wrote behind entry {n}"
        assert (int(meta["nbSeq"]), int(meta["litSize"]), int(meta["longType"]), int(meta["longPos"])) == (n, lit & 0xFFFFFFFF, long_type, long_pos), (G, n)
        assert (int(meta["lastLL"]), int(meta["status"]), list(meta["pad"])) == (77, 5, [0, 0]), (G, n)
        if n >= 2:
            assert (long_type, long_pos) == (2 if ml_last else 1, n - 1)          # both long kinds occurred: the later one wins


@pytest.mark.parametrize("G", ht.TEAMS)
def test_ladder_level_3_and_1(G):
    _, slices = ht.ladder()
    ht.check_frames("l3", helpers.emu_compress(slices, G=G))
    ht.check_frames("l1", helpers.emu_compress_level(slices, 1, G=G))
    for level in (3, 1):
        counts = set(int(c) for c in ht.emu_parse_meta(slices, G, level)["nbSeq"])
        assert ht.wanted_counts(G) <= counts, (G, level, sorted(counts))


def test_ladder_dictionary_bodies():
    d, slices = ht.ladder()
    G = 4
    ht.check_frames("dict_l3", helpers.emu_compress_dict(slices, d, G=G))
    ht.check_frames("dict_l1", hd.emu_compress(slices, d, 1, G=G))
    for level in (3, 1):
        counts = set(int(c) for c in ht.emu_parse_meta(slices, G, level, dictionary=d)["nbSeq"])
        assert ht.wanted_counts(G) <= counts, (level, sorted(counts))
