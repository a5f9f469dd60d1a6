"""zstd levels 5 .. 10 above 128 KiB (frames of several blocks: kompressor_amd/csrc/zstd_lazy_big.h and the frame step's additions in
zstd_entropy.h) on the CPU wave emulator, against tests/golden/zstd_lazy_big_golden.json (libzstd 1.5.7) and the oracle: the smallest
inputs that reach each thing that can go wrong, at levels 5 (greedy), 7 (lazy with minMatch 4 up to 256 KiB, 5 above) and 10 (lazy2, rows
of 64 entries).  The larger classes belong to tests/test_gpu_lazy_big.py."""
import ctypes

import pytest

import helpers
import helpers_lazy_big as hl

LEVELS = (5, 7, 10)
# helpers.lazy_big_inputs() by index: a second block of one byte; 131 080 bytes; both sides of the parameter classes' boundary (minMatch
# 4 -> 5 at levels 7 .. 10); RLE blocks; repeat offsets across blocks; raw blocks (savings stay below 3)
INDEX = {"131073": 0, "131080": 1, "262144": 5, "262145": 6, "zeros_300000": 20, "periodic": 21, "random_280000": 22}
SPLIT_INDEX, SPLIT_PREFIX = 14, 270000      # a two-part input whose statistics change 24 576 bytes into its second block


@pytest.fixture(scope="module")
def inputs():
    return helpers.lazy_big_inputs()


def test_parameters_equal_libzstds_table():
    """kx_lazy_big_params against the golden file's ZSTD_getCParams rows (windowLog, chainLog, hashLog, searchLog, minMatch, strategy)."""
    out = (ctypes.c_uint32 * 5)()
    rows = 0
    for key, (W, C, H, S, mml, strat) in helpers.lazy_big_golden()["params"].items():
        level, n = (int(x) for x in key.split(":"))
        if level < 5:
            continue
        hl.emu_lazy_big().emu_lazy_big_params(level, n, out)
        assert list(out) == [W, H, S, mml, strat], key
        rows += 1
    assert rows >= 40
    for level, n in ((5, 131072), (5, (2 << 20) + 1), (4, 200000), (11, 200000)):
        hl.emu_lazy_big().emu_lazy_big_params(level, n, out)
        assert out[4] == 0, (level, n)


@pytest.mark.parametrize("level", LEVELS)
@pytest.mark.parametrize("name", list(INDEX))
def test_frames_equal_libzstd(inputs, name, level):
    d = inputs[INDEX[name]]
    (frame,), status = hl.emu_compress_lazy_big([d], level)
    want, blocks = helpers.oracle().compress_lazy_big(d, level)
    flen, sha, gblocks = helpers.lazy_big_golden()["frames"][str(level)][INDEX[name]]
    assert status == 0
    assert [len(want), helpers.sha256(want), blocks] == [flen, sha, gblocks], "the oracle left its golden file"
    assert [len(frame), helpers.sha256(frame)] == [flen, sha], (name, level)
    assert frame == want
    if name == "random_280000":
        assert len(frame) > len(d)          # raw blocks only


@pytest.mark.parametrize("level", LEVELS)
def test_the_pre_splitter_cuts_where_the_statistics_change(inputs, level):
    """The golden's block list of this input has a block of 24 576 bytes behind the first; a prefix that still holds 128 KiB behind the
    first block is cut at the same place (sampling rate 11 / 9 bits at levels 5 .. 7, rate 5 / 10 bits above), and the tables of the block
    before are priced for the short one."""
    gblocks = helpers.lazy_big_golden()["frames"][str(level)][SPLIT_INDEX][2]
    assert any(b % 8192 == 0 and b < 131072 for b in gblocks), gblocks
    d = inputs[SPLIT_INDEX][:SPLIT_PREFIX]
    want, blocks = helpers.oracle().compress_lazy_big(d, level)
    assert blocks[:2] == gblocks[:2] and blocks[1] % 8192 == 0 and blocks[1] < 131072, blocks
    (frame,), status = hl.emu_compress_lazy_big([d], level)
    assert status == 0 and frame == want


@pytest.mark.parametrize("level", (5, 9))
def test_a_mixed_batch_in_pieces(inputs, level):
    """One-block slices, large ones and a refused one in one batch, the large ones one after the other through ONE table slot (the second
    finds the first one's entries there); at level 9 the 5 000-byte slice is another strategy: refused, the rest served."""
    datas = [inputs[1], inputs[0][:5000], inputs[0][:20000], b"", inputs[6], inputs[0][:7]]
    frames, status = hl.emu_compress_lazy_big(datas, level, slice_cap=4 << 20, piece=1)
    want = [hl.oracle_frame(d, level) for d in datas]
    assert (want[1] is None) == (level == 9)
    assert status == (4 if level == 9 else 0)
    assert frames == [w or b"" for w in want]
