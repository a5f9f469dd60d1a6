"""Writes tests/golden/zstd_seekable_golden.json: for each case of tests/helpers_seekable.py cases() the seekable container's length,
sha256 and seek table (hex, verbatim), and the foreign and damaged containers (base64) with the answers a reader must give.
The frames come from the binary libzstd 1.5.7 chunk by chunk (oracle/libzstd_ref.py), the table from struct, the checksums from the xxhash
module -- each asserted here against the last four bytes of the same chunk's libzstd frame made with ZSTD_c_checksumFlag (id 201), so the
tests need no xxhash.  Every container is also handed to ZSTD_decompress and ZSTD_findDecompressedSize: it is an ordinary .zst.
Run from the repository root: python tests/golden/make_golden_seekable.py"""
import base64
import ctypes
import hashlib
import json
import os
import struct
import sys

import xxhash

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import helpers_seekable as hs                        # noqa: E402
from oracle.libzstd_ref import LibZstd               # noqa: E402

CHECKSUM_FLAG = 201


def frame_with_checksum(z, data, level):
    lib = z.lib
    cctx = lib.ZSTD_createCCtx()
    try:
        lib.ZSTD_CCtx_setParameter(cctx, 100, level)
        assert not lib.ZSTD_isError(lib.ZSTD_CCtx_setParameter(cctx, CHECKSUM_FLAG, 1))
        cap = lib.ZSTD_compressBound(len(data))
        out = ctypes.create_string_buffer(cap)
        n = lib.ZSTD_compress2(cctx, out, cap, data, len(data))
        assert not lib.ZSTD_isError(n)
        return out.raw[:n]
    finally:
        lib.ZSTD_freeCCtx(cctx)


def checksum(z, chunk, level=3):
    x = xxhash.xxh64(chunk, seed=0).intdigest() & 0xFFFFFFFF
    assert struct.pack("<I", x) == frame_with_checksum(z, chunk, level)[-4:], "xxhash and libzstd's frame checksum disagree"
    return x


def container(z, chunks, level, checksums, **damage):
    frames = [z.compress(c, level) for c in chunks]
    entries = [(len(f), len(c), checksum(z, c, level) if checksums else 0) for f, c in zip(frames, chunks)]
    return b"".join(frames) + hs.seek_table(entries, checksums, **damage), entries


def check_plain_zst(z, blob, data):
    z.lib.ZSTD_findDecompressedSize.restype = ctypes.c_ulonglong
    z.lib.ZSTD_findDecompressedSize.argtypes = [ctypes.c_void_p, ctypes.c_size_t]
    assert z.lib.ZSTD_findDecompressedSize(blob, len(blob)) == len(data)
    assert z.decompress(blob, len(data)) == data


def stat_of(blob, status=0):
    if status:
        return {"content": 0, "table_off": 0, "frames": 0, "max_frame": 0, "max_compressed": 0, "flags": 0, "status": status}
    ents, fo, co = hs.parse_table(blob)
    return {"content": co[-1], "table_off": fo[-1], "frames": len(ents), "max_frame": max([d for _, d, _ in ents] + [0]),
            "max_compressed": max([c for c, _, _ in ents] + [0]), "flags": blob[-5] >> 7, "status": 0}


def main():
    z = LibZstd()
    rows = []
    for name, cls, seed, size, fb, level, sums, src_off in hs.cases():
        data = hs.case_input(cls, seed, size)
        blob, entries = container(z, hs.chunks_of(data, fb), level, sums)
        check_plain_zst(z, blob, data)
        table = blob[len(blob) - 17 - len(entries) * (12 if sums else 8):]
        rows.append({"name": name, "cls": cls, "seed": seed, "size": size, "frame_bytes": fb, "level": level, "checksums": sums, "src_offset": src_off,
                     "length": len(blob), "sha256": hashlib.sha256(blob).hexdigest(), "table": table.hex()})

    blobs = []

    def add(name, kind, blob, status=0, content=None, **extra):
        row = {"name": name, "kind": kind, "b64": base64.b64encode(blob).decode(), "stat": stat_of(blob, status)}
        if content is not None:
            row.update(cls=content[0], seed=content[1], size=content[2])
        row.update(extra)
        blobs.append(row)

    # ---- foreign containers: what another writer of the format may produce ----
    src = ("T", 92000, 26037)
    data = hs.case_input(*src)
    cuts = [0, 1000, 6000, 6037, 26037]
    uneven = [data[a:b] for a, b in zip(cuts[:-1], cuts[1:])]
    blob, _ = container(z, uneven, 5, 1)
    check_plain_zst(z, blob, data)
    add("unequal_frames", "foreign", blob, content=src)
    blob, _ = container(z, uneven, 3, 0)
    add("no_checksums", "foreign", blob, content=src)
    blob, _ = container(z, uneven, 3, 1, descriptor=0x83)
    add("unused_descriptor_bits", "foreign", blob, content=src)
    # an inner skippable frame, listed with decompressed size 0 (its checksum: XXH64 of nothing)
    frames = [z.compress(c, 3) for c in uneven]
    skip = struct.pack("<II", 0x184D2A53, 11) + b"hello world"
    entries = [(len(f), len(c), checksum(z, c)) for f, c in zip(frames, uneven)]
    entries.insert(2, (len(skip), 0, checksum(z, b"")))
    blob = b"".join(frames[:2]) + skip + b"".join(frames[2:]) + hs.seek_table(entries, 1)
    check_plain_zst(z, blob, data)
    add("inner_skippable", "foreign", blob, content=src)

    # ---- damaged containers ----
    good, gentries = container(z, uneven, 3, 1)
    add("sixteen_bytes", "damaged", good[-16:], 10)
    add("wrong_seekable_magic", "damaged", container(z, uneven, 3, 1, magic=0x8F92EAB2)[0], 10)
    add("wrong_skippable_magic", "damaged", container(z, uneven, 3, 1, skip_magic=0x184D2A5F)[0], 10)
    add("reserved_bit", "damaged", container(z, uneven, 3, 1, descriptor=0x84)[0], 20)
    add("frame_size_off_by_one", "damaged", container(z, uneven, 3, 1, frame_size=len(gentries) * 12 + 10)[0], 20)
    add("too_many_frames", "damaged", container(z, uneven, 3, 1, frames=0x07FFFFFF)[0], 20)
    add("huge_frame_count", "damaged", container(z, uneven, 3, 1, frames=0xFFFFFFFF)[0], 20)
    short = list(gentries); short[1] = (short[1][0] - 1, short[1][1], short[1][2])
    add("sizes_do_not_sum", "damaged", b"".join(z.compress(c, 3) for c in uneven) + hs.seek_table(short, 1), 20)
    big = list(gentries); big[0] = (big[0][0], (1 << 30) + 1, big[0][2])
    add("entry_above_1gib", "damaged", b"".join(z.compress(c, 3) for c in uneven) + hs.seek_table(big, 1), 20)
    # one flipped checksum: opens cleanly; a verified read answers 22 for exactly that frame
    flipped = list(gentries); flipped[2] = (flipped[2][0], flipped[2][1], flipped[2][2] ^ 0x00010000)
    add("flipped_checksum", "flipped", b"".join(z.compress(c, 3) for c in uneven) + hs.seek_table(flipped, 1), content=src, bad_frame=2)

    for r in blobs:                                   # the restated validation agrees with what was built
        got = hs.index_reference(base64.b64decode(r["b64"]))
        assert all(int(got[f]) == r["stat"][f] for f in hs.STAT_FIELDS), (r["name"], got, r["stat"])
    out = {"libzstd": 10507, "xxhash": xxhash.VERSION, "cases": rows, "blobs": blobs}
    path = os.path.join(ROOT, "tests", "golden", "zstd_seekable_golden.json")
    with open(path, "w") as f:
        json.dump(out, f, indent=0)
    print(f"wrote {path}: {len(rows)} cases, {len(blobs)} blobs, {os.path.getsize(path)} bytes")


if __name__ == "__main__":
    main()
