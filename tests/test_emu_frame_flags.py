"""The frame flags on the CPU wave emulator: the kernel bodies, with the flags in the launch arguments zstd_launch.h builds, reproduce
the binary libzstd 1.5.7's frames (tests/golden/zstd_frame_flags_golden.json) -- checksum, no content size, no dictionary ID, alone
and together -- at levels 3, 1 and 7: one-block frames, frames of two blocks, with a raw and with a formatted dictionary."""
import pytest

import helpers_frame_flags as hf

EMU_LEVELS = (3, 1, 7)


@pytest.mark.parametrize("flags", hf.FLAG_SETS)
@pytest.mark.parametrize("level", EMU_LEVELS)
def test_golden_rows_one_block(level, flags):
    want = hf.golden_frames(level, None, flags)
    slices = [(s, p) for s, p in hf.slices_of(level, big=False) if len(p) <= 131072]
    frames = hf.emu_compress([p for _, p in slices], level, flags)
    for (s, _), f in zip(slices, frames):
        hf.check_frame(f, want[s], (level, flags, s))


@pytest.mark.parametrize("flags", hf.FLAG_SETS)
@pytest.mark.parametrize("level", EMU_LEVELS)
def test_golden_rows_two_blocks(level, flags):
    """131 073 bytes beside short slices on the paths of a context for frames of several blocks (the block chain; level 7: zstd_lazy_big.h)"""
    want = hf.golden_frames(level, None, flags)
    slices = [(s, p) for s, p in hf.slices_of(level, big=False) if len(p) in (0, 33, 256, 131073)]
    frames = hf.emu_compress([p for _, p in slices], level, flags)
    for (s, _), f in zip(slices, frames):
        hf.check_frame(f, want[s], (level, flags, s))


@pytest.mark.parametrize("level", hf.DICT_LEVELS)
@pytest.mark.parametrize("which", range(3))
def test_golden_rows_dictionary(which, level):
    name, d, formatted = hf.dictionaries()[which]
    slices = hf.dict_slices()
    for flags in (hf.FLAG_SETS_FORMATTED if formatted else hf.FLAG_SETS):
        want = hf.golden_frames(level, name, flags)
        frames = hf.emu_compress([p for _, p in slices], level, flags, dictionary=d)
        for (s, _), f in zip(slices, frames):
            hf.check_frame(f, want[s], (name, level, flags, s))


def test_flags_zero_is_todays_frame():
    """without flags the entry point writes the frames the other emulator tests pin: the golden {201} frame is that frame with descriptor
    bit 2 and four more bytes"""
    slices = [(s, p) for s, p in hf.slices_of(3, big=False) if len(p) <= 131072]
    plain = hf.emu_compress([p for _, p in slices], 3, 0)
    summed = hf.emu_compress([p for _, p in slices], 3, hf.CHECKSUM)
    for (s, _), a, b in zip(slices, plain, summed):
        assert len(b) == len(a) + 4 and b[4] == a[4] | 4 and b[:4] == a[:4] and b[5:-4] == a[5:], s


def test_level_4_between_128_and_256_kib():
    """level 4's "greedy" row above a block on the chain of zstd_lazy_big.h (what the batch call runs 128 KiB < size <= 256 KiB with): the
    frame of 131 073 bytes, its header replaced by the form without content size, is the golden {200=0} frame"""
    import helpers_lazy_big as hl
    p = hf.text(131073)
    frames = hl.emu_compress_lazy_big([p], 4, slice_cap=262144)
    f = (frames[0] if isinstance(frames, tuple) else frames)[0]
    assert f[:9] == bytes.fromhex("28b52ffda0") + (131073).to_bytes(4, "little")
    hf.check_frame(f[:4] + bytes([0x00, (18 - 10) << 3]) + f[9:], hf.golden_frames(4, None, hf.NO_CONTENT_SIZE)["text_131073"], "level 4")


def test_streaming_frames_take_the_checksum():
    """a streaming frame (no content size anyway) with the checksum: descriptor 0x04 and the trailer; KMP_FRAME_NO_CONTENT_SIZE changes nothing"""
    datas = [hf.text(0), hf.text(5000), hf.text(131073)]
    plain = hf.emu_compress(datas, 3, 0, stream=1)
    summed = hf.emu_compress(datas, 3, hf.CHECKSUM, stream=1)
    both = hf.emu_compress(datas, 3, hf.CHECKSUM | hf.NO_CONTENT_SIZE, stream=1)
    assert both == summed
    one_shot = hf.emu_compress(datas[:2], 3, hf.CHECKSUM)
    for a, b in zip(plain, summed):
        assert len(b) == len(a) + 4 and a[4] == 0 and b[4] == 4 and b[5:-4] == a[5:]
    for b, c in zip(summed, one_shot):
        assert b[-4:] == c[-4:]
