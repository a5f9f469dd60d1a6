"""zstd levels 5 .. 10 as streams and as the reference driver's staged frames, 0 .. 2 MiB (kompressor_amd/csrc/zstd_lazy_big.h under a
KFrameArgs.stream mode, the frame step of zstd_entropy.h) on the CPU wave emulator, against tests/golden/zstd_lazy_stream_golden.json
(libzstd 1.5.7 driven as the reference's callers drive it) and, where it is present, the live library's decoder."""
import ctypes

import pytest

import helpers
import helpers_lazy_stream as hs

SMALL = 400000                       # rows up to here run at every level, larger ones at levels 5 and 10 (emulator time)
NAMES = [name for name, _ in hs.inputs()]
SIZE = {name: len(d) for name, d in hs.inputs()}


@pytest.fixture(scope="module")
def inputs():
    ins = dict(hs.inputs())
    G = hs.golden()["inputs"]
    assert list(G) == NAMES and all(G[k] == [len(d), helpers.sha256(d)] for k, d in ins.items()), "the inputs left their golden file"
    return ins


def test_parameters_of_streams_and_staged_frames():
    """A stream gets the unknown-size row at every length (the golden file's ZSTD_getCParams(level, 0, 0)), a staged frame the row of its
    size (zstd_lazy_big_golden.json); nothing above 2 MiB, no staged frame of one block."""
    out = (ctypes.c_uint32 * 5)()
    emu = hs.emu_lazy_stream()
    for level in hs.LEVELS:
        W, C, H, S, mml, strat = hs.golden()["params"][str(level)]
        assert mml == 5 and W == (22 if level >= 9 else 21)
        for mode in (1, 2):
            for n in (0, 1, 5000, 16384, 131072, 262144, 300000, 2 << 20):
                emu.emu_lazy_stream_params(level, n, mode, out)
                assert list(out) == [W, H, S, mml, strat], (level, n, mode)
            emu.emu_lazy_stream_params(level, (2 << 20) + 1, mode, out)
            assert out[4] == 0
    rows = 0
    for key, (W, C, H, S, mml, strat) in helpers.lazy_big_golden()["params"].items():
        level, n = (int(x) for x in key.split(":"))
        if level >= 5:
            emu.emu_lazy_stream_params(level, n, 3, out)
            assert list(out) == [W, H, S, mml, strat], key
            rows += 1
    assert rows >= 40
    emu.emu_lazy_stream_params(7, 131072, 3, out)
    assert out[4] == 0


@pytest.mark.parametrize("name,level", [(k, lv) for k in NAMES for lv in hs.LEVELS if SIZE[k] <= SMALL or lv in (5, 10)])
def test_frames_equal_libzstd(inputs, name, level):
    """Every framing of a golden row: the emulated kernels write libzstd's frame (length and sha256), and the live library decodes it.
    (The GPU tests run the rows above 400 000 bytes at every level.)"""
    d = inputs[name]
    row = hs.golden()["frames"][str(level)][name]
    assert set(row) == ({"stream", "stream_empty_end", "staged"} if len(d) >= hs.STAGED_FROM else {"stream", "stream_empty_end"})
    z = helpers.live_libzstd()
    for framing, (flen, sha) in row.items():
        (frame,), status, _ = hs.emu_compress([d], level, framing)
        assert status == 0
        assert [len(frame), helpers.sha256(frame)] == [flen, sha], (name, level, framing)
        if framing != "staged":
            assert frame[4:6] == bytes([0, 0x60 if level >= 9 else 0x58])
        if z is not None:
            assert z.decompress(frame, len(d)) == d


def test_streams_of_every_length_through_one_table_slot(inputs):
    """Level 9: an empty, a 5 000-byte, a 131 072-byte and a 300 000-byte stream one after the other through ONE table slot (the later
    ones find their predecessors' entries there).  The short ones are lazy2 under the unknown-size row: served, not refused."""
    names = ["T0", "D5000", "T131072", "change_100000+100000+100000"]
    assert [SIZE[k] for k in names] == [0, 5000, 131072, 300000]
    for framing in ("stream", "stream_empty_end"):
        frames, status, slot = hs.emu_compress([inputs[k] for k in names], 9, framing, slice_cap=300000, piece=1)
        assert status == 0
        assert slot == 5 << 21                      # (hashLog 21 whatever the length: a one-shot context of 300 000 bytes has 5 << 20)
        want = [hs.golden()["frames"]["9"][k][framing] for k in names]
        assert [[len(f), helpers.sha256(f)] for f in frames] == want, framing


def test_a_staged_batch_with_a_one_block_and_a_refused_slice(inputs):
    """Level 7 on a context for slices of 4 MiB: 100 000 bytes go through the one-block kernels (staged = in place there), 200 000 bytes are
    a staged frame, 2 MiB + 1 is refused (status bit 4, out_len 0) and the rest is served."""
    small = inputs["S200000"][:100000]
    big = inputs["D2097152"] + b"x"
    frames, status, _ = hs.emu_compress([small, inputs["S200000"], big], 7, "staged", slice_cap=4 << 20, piece=1)
    assert status == 4
    assert frames[0] == helpers.oracle().compress_lazy(small, 7)
    assert [len(frames[1]), helpers.sha256(frames[1])] == hs.golden()["frames"]["7"]["S200000"]["staged"]
    assert frames[2] == b""
