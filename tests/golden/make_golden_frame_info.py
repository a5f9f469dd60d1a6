"""Writes tests/golden/zstd_frame_info_golden.json: entries (base64) and what the binary libzstd 1.5.7 answers for each --
ZSTD_findDecompressedSize, ZSTD_decompressBound, a frame-by-frame walk with ZSTD_findFrameCompressedSize and, for the frames it accepts,
ZSTD_getFrameHeader (tests/helpers_frame_info.py live_answers).  The entries: frames the library compresses under the settings that decide
a header's fields, and frames no compressor writes, made here by editing bytes.
Run from the repository root: python tests/golden/make_golden_frame_info.py"""
import base64
import ctypes
import json
import os
import random
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import helpers_frame_info as hf                      # noqa: E402
from oracle.libzstd_ref import LibZstd               # noqa: E402

WINDOW_LOG, CONTENT_SIZE_FLAG, CHECKSUM_FLAG = 101, 200, 201


def text(seed, n):
    r = random.Random(seed)
    words = [bytes(r.choice(b"abcdefghijklmnopqrstuvwxyz") for _ in range(r.randrange(2, 9))) for _ in range(200)]
    out = bytearray()
    while len(out) < n:
        out += r.choice(words) + b" "
    return bytes(out[:n])


def periodic(seed, n, period=1000):
    u = text(seed, period)
    return (u * (n // period + 1))[:n]


def noise(seed, n):
    return random.Random(seed).randbytes(n)


def compress(z, data, level=3, **params):
    lib = z.lib
    cctx = lib.ZSTD_createCCtx()
    try:
        lib.ZSTD_CCtx_setParameter(cctx, 100, level)
        for k, v in params.items():
            r = lib.ZSTD_CCtx_setParameter(cctx, {"window_log": WINDOW_LOG, "content_size": CONTENT_SIZE_FLAG, "checksum": CHECKSUM_FLAG}[k], v)
            assert not lib.ZSTD_isError(r), k
        cap = lib.ZSTD_compressBound(len(data))
        out = ctypes.create_string_buffer(cap)
        n = lib.ZSTD_compress2(cctx, out, cap, data, len(data))
        assert not lib.ZSTD_isError(n)
        return out.raw[:n]
    finally:
        lib.ZSTD_freeCCtx(cctx)


def skippable(payload, nibble=0):
    return (0x184D2A50 + nibble).to_bytes(4, "little") + len(payload).to_bytes(4, "little") + payload


def header_size(f):
    fhd = f[4]
    single = (fhd >> 5) & 1
    return 5 + (1 - single) + (0, 1, 2, 4)[fhd & 3] + ((1 << (fhd >> 6)) if fhd >> 6 else single)


def with_dict_id(f, did, width):
    """the frame with a dictionary-ID field of `width` bytes put into its header"""
    assert f[4] & 3 == 0
    at = 5 + (0 if f[4] & 0x20 else 1)
    return f[:4] + bytes([f[4] | {1: 1, 2: 2, 4: 3}[width]]) + f[5:at] + did.to_bytes(width, "little") + f[at:]


def with_fcs8(f, size):
    """a single-segment frame's content-size field widened to 8 bytes holding `size`"""
    assert f[4] & 0x20 and f[4] & 3 == 0
    old = header_size(f)
    return f[:4] + bytes([(f[4] & 0x3F) | 0xC0]) + size.to_bytes(8, "little") + f[old:]


def entries(z):
    e = []
    add = lambda name, b: e.append((name, bytes(b)))            # noqa: E731
    small = compress(z, text(1, 40))                            # one small frame: single segment, 1-byte size, a raw or compressed block
    add("empty entry", b"")
    add("empty frame", compress(z, b""))
    add("fcs1 single segment", small)
    add("fcs1 255", compress(z, text(2, 255)))
    add("fcs2 256", compress(z, text(3, 256)))
    add("fcs2 5000", compress(z, text(4, 5000)))
    add("fcs2 65791", compress(z, periodic(5, 65791)))
    add("fcs4 65792", compress(z, periodic(6, 65792)))
    add("fcs4 300000 three blocks", compress(z, periodic(7, 300000)))
    add("fcs8 edited", with_fcs8(compress(z, text(8, 100)), 100))
    add("fcs8 edited 5 GiB declared", with_fcs8(compress(z, text(8, 100)), 5 << 30))
    add("window descriptor + fcs2 (no single segment)", compress(z, text(9, 5000), window_log=10))
    add("window descriptor + fcs4", compress(z, periodic(10, 70000), window_log=12))
    add("no content size", compress(z, text(11, 3000), content_size=0))
    add("no content size, window 2^10", compress(z, text(12, 3000), content_size=0, window_log=10))
    add("checksum", compress(z, text(13, 700), checksum=1))
    add("checksum, no content size", compress(z, text(14, 700), checksum=1, content_size=0))
    add("checksum, empty", compress(z, b"", checksum=1))
    for w, did in ((1, 0xAB), (2, 0xBEEF), (4, 0xC0FFEE01)):
        add(f"dictionary ID {w} bytes (edited)", with_dict_id(small, did, w))
    add("dictionary ID 2 bytes, window descriptor (edited)", with_dict_id(compress(z, text(15, 3000), content_size=0), 0x1234, 2))
    add("raw block", compress(z, noise(16, 1000)))
    add("RLE block", compress(z, bytes(5000)))
    add("compressed block", compress(z, text(17, 20000)))
    add("level 19", compress(z, text(18, 9000), level=19))
    add("level -5", compress(z, text(19, 9000), level=-5))
    # streaming frames (no declared size): what finish = false callers get
    one = z.compress_streaming(text(20, 3000), [0, 1000, 3000])
    two = z.compress_streaming(periodic(21, 131072 + 5000), [0, 70000, 131072 + 5000])
    many = z.compress_streaming(periodic(22, 16 * 131072 + 777), [0, 500000, 16 * 131072 + 777])
    rle17 = z.compress_streaming(bytes(16 * 131072 + 1), [0, 131072, 16 * 131072 + 1])
    add("streaming 1 block", one)
    add("streaming 2 blocks", two)
    add("streaming 17 blocks", many)
    add("streaming 17 RLE blocks", rle17)
    add("streaming, closed without data", z.compress_streaming(text(23, 131072), [0, 131072, 131072]))
    add("two frames", small + compress(z, text(24, 300)))
    add("three frames", small + one + compress(z, text(25, 256)))
    add("sized frame, then streaming frame", compress(z, text(26, 900)) + two)
    add("streaming frame, then sized frame", one + compress(z, text(26, 900)))
    add("skippable alone", skippable(b"hello"))
    add("skippable payload 0", skippable(b""))
    add("skippable nibble 15", skippable(b"xyz", 15))
    add("skippable before", skippable(b"meta") + small)
    add("skippable between", small + skippable(b"between", 3) + compress(z, text(27, 500)))
    add("skippable after", small + skippable(b"after"))
    add("skippable payload 0 between", small + skippable(b"") + small)
    add("two skippables", skippable(b"a") + skippable(b"bc", 1))
    add("skippable size past the entry", skippable(b"0123456789")[:-1])
    add("skippable size past the entry by far", (0x184D2A50).to_bytes(4, "little") + (1 << 20).to_bytes(4, "little") + b"abc")
    add("skippable size wraps 32 bits", (0x184D2A50).to_bytes(4, "little") + (0xFFFFFFFA).to_bytes(4, "little") + b"abc")
    add("skippable size 0xFFFFFFF7", (0x184D2A50).to_bytes(4, "little") + (0xFFFFFFF7).to_bytes(4, "little") + b"abc")
    add("skippable header cut: 5 bytes", skippable(b"hello")[:5])
    add("skippable header cut: 7 bytes", skippable(b"hello")[:7])
    add("good frame, then skippable past the entry", small + skippable(b"0123456789")[:-3])
    # windows: the descriptor is byte 5 of a frame without single segment
    nosize = compress(z, text(11, 3000), content_size=0)
    assert not nosize[4] & 0x20
    add("window 2^31", nosize[:5] + bytes([21 << 3]) + nosize[6:])
    add("window 2^31 + 7/8", nosize[:5] + bytes([(21 << 3) | 7]) + nosize[6:])
    add("window above the maximum (2^32)", nosize[:5] + bytes([22 << 3]) + nosize[6:])
    add("window 2^41", nosize[:5] + bytes([0xFF]) + nosize[6:])
    add("window 2^10 + 3/8 (edited), 17 blocks", many[:5] + bytes([3]) + many[6:])
    add("reserved bit", small[:4] + bytes([small[4] | 8]) + small[5:])
    add("reserved bit, header cut short", (small[:4] + bytes([small[4] | 8]) + small[5:])[:5])
    add("reserved bit and window above the maximum", nosize[:4] + bytes([nosize[4] | 8, 22 << 3]) + nosize[6:])
    hs = header_size(small)
    add("block type 3", small[:hs] + bytes([small[hs] | 6]) + small[hs + 1:])
    add("block type 3 in the second block", two[:header_size(two)] + _second_block_type3(two))
    add("last-block bit cleared, nothing behind", small[:hs] + bytes([small[hs] & 0xFE]) + small[hs + 1:])
    add("last-block bit cleared, a frame behind", small[:hs] + bytes([small[hs] & 0xFE]) + small[hs + 1:] + small)
    add("block size past the entry", small[:hs] + bytes([small[hs], small[hs + 1], small[hs + 2] | 0x10]) + small[hs + 3:])
    ck = compress(z, text(13, 700), checksum=1)
    for k in (1, 3, 4):
        add(f"checksum cut by {k}", ck[:-k])
    for k in range(len(small) + 1):
        add(f"truncated at {k} of {len(small)}", small[:k])
    tail = compress(z, text(28, 20), checksum=1, content_size=0)          # ... and of one with a window descriptor and a checksum
    for k in range(len(tail)):
        add(f"truncated at {k} of {len(tail)}, checksum", tail[:k])
    for k in range(1, 9):
        add(f"wrong magic, {k} bytes", (b"\x29\xb5\x2f\xfd" + small[4:])[:k])
    for k in range(2, 9):
        add(f"magic wrong in its last byte present, {k} bytes", hf.MAGIC[:k - 1] + b"\x00" if k <= 4 else (hf.MAGIC[:3] + b"\xfe" + small[4:])[:k])
    for k in range(1, 5):
        add(f"skippable magic prefix, {k} bytes", b"\x5c\x2a\x4d\x18"[:k])
    add("skippable magic's upper bytes, low byte 0x60", b"\x60\x2a\x4d\x18")
    # the binary library is built with the formats of zstd 0.5 .. 0.7 and sizes their frames: handmade ones (raw, RLE and end blocks)
    blocks = b"\x40\x00\x05hello" + b"\x80\x00\x09z" + b"\xc0\x00\x00"
    add("legacy magic 0.7 over a frame of today", b"\x27\xb5\x2f\xfd" + small[4:])
    add("legacy magic 0.4 (unknown)", b"\x24\xb5\x2f\xfd" + small[4:])
    add("legacy 0.5 frame", b"\x25\xb5\x2f\xfd\x0b" + blocks)
    add("legacy 0.6 frame, 1-byte size", b"\x26\xb5\x2f\xfd\x40\x0e" + blocks)
    add("legacy 0.6 frame, no size", b"\x26\xb5\x2f\xfd\x00" + blocks)
    add("legacy 0.7 frame, 1-byte size", b"\x27\xb5\x2f\xfd\x20\x0e" + blocks)
    add("legacy 0.7 frame, window descriptor, 2-byte size", b"\x27\xb5\x2f\xfd\x40\x00\x10\x00" + blocks)
    add("legacy 0.7 frame, then a frame of today", b"\x27\xb5\x2f\xfd\x20\x0e" + blocks + small)
    add("legacy 0.7 frame cut in a block", (b"\x27\xb5\x2f\xfd\x20\x0e" + blocks)[:12])
    add("legacy magic alone, 4 bytes", b"\x25\xb5\x2f\xfd")
    for k in (1, 3, 4, 8):
        add(f"trailing garbage: {k} zero bytes", small + bytes(k))
        add(f"trailing garbage: {k} bytes of 0xFF", small + b"\xff" * k)
    for k in (1, 3, 4):
        add(f"trailing garbage: {k} bytes that start a magic", small + hf.MAGIC[:k])
    add("trailing garbage behind a streaming frame", one + b"\x00\x00\x00")
    add("trailing garbage behind a skippable frame", skippable(b"x") + b"\x01")
    return e


def _second_block_type3(f):
    """the frame's bytes from its first block on, the second block's type set to 3"""
    hs = header_size(f)
    bh = int.from_bytes(f[hs:hs + 3], "little")
    assert not bh & 1
    nxt = hs + 3 + (1 if (bh >> 1) & 3 == 1 else bh >> 3)
    return f[hs:nxt] + bytes([f[nxt] | 6]) + f[nxt + 1:]


def main():
    z = LibZstd()
    lib = hf.live_lib()
    rows = []
    for name, b in entries(z):
        a = hf.live_answers(lib, b)
        hf.expected(a)                                  # (the rule that makes a kmp_zstd_frame_info of the answers holds for it)
        rows.append({"name": name, "b64": base64.b64encode(b).decode(), **a})
    names = [r["name"] for r in rows]
    assert len(set(names)) == len(names)
    out = os.path.join(ROOT, "tests", "golden", "zstd_frame_info_golden.json")
    with open(out, "w") as f:
        json.dump({"libzstd": 10507, "rows": rows}, f, separators=(",", ":"))
        f.write("\n")
    print(out, len(rows), "entries", os.path.getsize(out), "bytes;", sum(1 for r in rows if r["status"]), "rejected")
    for r in rows:
        print(f"{r['name']:60s} len {len(base64.b64decode(r['b64'])):7d} content {r['content']:20d} bound {r['bound']:20d} status {r['status']:3d} walk {r['walk']}")


if __name__ == "__main__":
    main()
