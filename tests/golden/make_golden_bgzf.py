"""Writes tests/golden/bgzf_golden.json: for each case of tests/helpers_bgzf.py cases() the BGZF container's length, sha256 and member
sizes, and the foreign, damaged and wrong blobs (base64) with the answers a reader must give.  The payloads come from zlib 1.2.11
(the project's pin) block by block -- zlib.compressobj(level, DEFLATED, -15, 8, 0) --, the wrappers from struct, the checksums from
zlib.crc32.  Every good blob is also handed to gzip.decompress: it is ordinary multi-member gzip.  The expected stats are the Python
restatement's of the head test and the walk (tests/helpers_bgzf.py), each damaged blob's status also asserted here by hand.
Run from the repository root: python tests/golden/make_golden_bgzf.py"""
import base64
import gzip
import hashlib
import json
import os
import struct
import sys
import zlib

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import helpers_bgzf as hb                        # noqa: E402

assert zlib.ZLIB_RUNTIME_VERSION == "1.2.11", "the fixture is zlib 1.2.11's"


def raw(data, level, flush_at=None):
    c = zlib.compressobj(level, zlib.DEFLATED, -15, 8, 0)
    if flush_at is None:
        return c.compress(data) + c.flush()
    return c.compress(data[:flush_at]) + c.flush(zlib.Z_FULL_FLUSH) + c.compress(data[flush_at:]) + c.flush()


def container(data, block_bytes, level, eof=True, **kw):
    parts = [hb.member(raw(b, level), b, **kw) for b in hb.blocks_of(data, block_bytes)]
    return b"".join(parts) + (hb.EOF if eof else b""), [len(p) for p in parts]


def stat_of(blob):
    st, *_ = hb.walk_reference(blob)
    return {f: int(st[f]) for f in hb.STAT_FIELDS}


def row(name, kind, blob, content=None, **more):
    r = {"name": name, "kind": kind, "b64": base64.b64encode(blob).decode(), "stat": stat_of(blob)}
    if content is not None:
        r["content_b64"] = base64.b64encode(content).decode()
        if kind == "foreign":
            assert gzip.decompress(blob) == content and r["stat"]["status"] == 0 and r["stat"]["content"] == len(content), name
    r.update(more)
    return r


def main():
    assert raw(b"", 6) == b"\x03\x00" and all(hb.member(raw(b"", lv), b"") == hb.EOF for lv in range(1, 10)), "the marker is zlib's empty member"
    out = {"zlib": zlib.ZLIB_RUNTIME_VERSION, "cases": [], "blobs": []}
    largest = 0
    for name, cls, seed, size, bb, level, src_off in hb.cases():
        data = hb.case_input(cls, seed, size)
        blob, sizes = container(data, bb, level)
        assert gzip.decompress(blob) == data and max(sizes + [0]) <= 65536
        largest = max([largest] + sizes)
        out["cases"].append({"name": name, "cls": cls, "seed": seed, "size": size, "block_bytes": bb, "level": level, "src_offset": src_off,
                             "length": len(blob), "sha256": hashlib.sha256(blob).hexdigest(), "members": sizes})
    assert largest == 65280 + 4 * 5 + 26, "the incompressible block: four stored blocks (zlib closes one every 16 383 symbols)"

    # ---- foreign blobs: what other writers make ----
    T = hb.case_input("T", 96000, 3000)
    f = out["blobs"]
    blob = b"".join(hb.member(raw(b, 6, flush_at=len(b) // 2), b) for b in hb.blocks_of(T, 1000)) + hb.EOF
    f.append(row("full_flush_inside", "foreign", blob, T))
    blob = b"".join(hb.member(raw(b, 0), b) for b in hb.blocks_of(T[:900], 300)) + hb.EOF
    f.append(row("stored_only", "foreign", blob, T[:900]))
    blob = b"".join(hb.member(raw(b, 6), b, before=b"XY\x03\x00abc", after=b"ZZ\x00\x00") for b in hb.blocks_of(T, 1100)) + hb.EOF
    f.append(row("extra_subfields", "foreign", blob, T))
    assert f[-1]["stat"]["flags"] == 3
    parts = [hb.member(raw(b, 6), b) for b in hb.blocks_of(T[:1500], 500)]
    blob = parts[0] + hb.EOF + hb.EOF + parts[1] + hb.member(raw(b"", 1), b"", before=b"QQ\x00\x00") + parts[2] + hb.EOF
    f.append(row("empty_members_in_the_middle", "foreign", blob, T[:1500]))
    blob, _ = container(T[:1500], 400, 6, eof=False)
    f.append(row("no_eof_marker", "foreign", blob, T[:1500]))
    assert f[-1]["stat"]["flags"] == 0
    inner, _ = container(T[:600], 150, 6)
    blob = b"".join(hb.member(raw(b, 0), b) for b in hb.blocks_of(inner, 97)) + hb.EOF
    f.append(row("bgzf_stored_inside_members", "foreign", blob, inner))
    # a false candidate inside member 1 (stored, so its bytes stand in the blob) whose size points exactly at member 2's start
    filler = bytes(range(40))
    fake = bytes.fromhex("1f8b08040000000000ff0600") + struct.pack("<2sHH", b"BC", 2, 18 + 30 + 8 - 1)
    data1 = filler + fake + bytes(30)
    parts = [hb.member(raw(T[:200], 6), T[:200]), hb.member(raw(data1, 0), data1), hb.member(raw(T[200:500], 6), T[200:500])]
    blob = b"".join(parts) + hb.EOF
    at = len(parts[0]) + 18 + 5 + 40
    assert hb.head_reference(blob, at)[:2] == (0, 56) and at + 56 == len(parts[0]) + len(parts[1]), "the false chain must merge into the true one"
    f.append(row("false_chain_merges", "foreign", blob, T[:200] + data1 + T[200:500]))

    # ---- damaged blobs ----
    blocks = hb.blocks_of(T[:400], 100)
    good = [hb.member(raw(b, 6), b) for b in blocks]
    base = b"".join(good) + hb.EOF
    mo = [sum(len(g) for g in good[:i]) for i in range(5)]

    def third(m):
        return good[0] + good[1] + m + good[3] + hb.EOF

    p2, d2 = raw(blocks[2], 6), blocks[2]
    head10 = bytes.fromhex("1f8b08040000000000ff")

    def custom(extra, total=None):
        n = 12 + len(extra) + len(p2) + 8 if total is None else total
        e = extra.replace(b"\xFE\xFE", struct.pack("<H", n - 1))
        return head10 + struct.pack("<H", len(e)) + e + p2 + struct.pack("<II", zlib.crc32(d2), len(d2))
    damaged = [
        ("cut_inside_magic", base[:mo[2] + 2], -5), ("cut_inside_header", base[:mo[2] + 7], -5), ("cut_inside_extra", base[:mo[2] + 14], -5),
        ("cut_inside_payload", base[:mo[2] + 25], -5), ("cut_inside_trailer", base[:mo[3] - 3], -5),
        ("bad_magic_third_member", third(good[2][:2] + b"\x09" + good[2][3:]), -3),
        ("no_extra_flag_third_member", third(good[2][:3] + b"\x00" + good[2][4:]), -3),
        ("bsize_too_small", third(hb.member(p2, d2, bsize=26)), -3),
        ("bsize_past_the_end", good[0] + hb.member(p2, d2, bsize=len(good[2]) + 40), -5),
        ("subfield_overruns_xlen", third(custom(b"BC\x02\x00\xFE\xFEXY\x09\x00")), -3),
        ("subfield_header_cut_by_xlen", third(custom(b"BC\x02\x00\xFE\xFEXY\x00")), -3),
        ("slen_3", third(custom(b"BC\x03\x00\xFE\xFE\x00")), -3),
        ("two_bc_subfields", third(custom(b"BC\x02\x00\xFE\xFEBC\x02\x00\xFE\xFE")), -3),
        ("no_bc_subfield", third(custom(b"XY\x02\x00\x00\x00")), -3),
        ("xlen_below_6", third(custom(b"XY\x00\x00")), -3),
        ("isize_65537", third(hb.member(p2, d2, isize=65537)), -3),
        ("trailing_byte", base + b"\x00", -3), ("trailing_byte_of_the_magic", base + b"\x1f", -5), ("trailing_30_bytes", base + bytes(range(100, 130)), -3),
        ("size_0", b"", -5), ("garbage_at_offset_0", bytes(range(64)), -3),
    ]
    for name, blob, status in damaged:
        r = row(name, "damaged", blob)
        assert r["stat"] == {"content": 0, "blocks": 0, "max_block": 0, "max_compressed": 0, "flags": 0, "status": status}, (name, r["stat"])
        f.append(r)
    assert stat_of(third(hb.member(p2, d2, isize=65536)))["status"] == 0, "an ISIZE of 65 536 is the largest a reader accepts"

    # ---- readable but wrong: the open accepts them, the read says -3 on exactly that member ----
    content = T[:400]
    blob = good[0] + hb.member(raw(blocks[1], 6), blocks[1], crc=zlib.crc32(blocks[1]) ^ 0x100) + good[2] + good[3] + hb.EOF
    f.append(row("flipped_crc", "wrong", blob, content, bad_member=1))
    blob = good[0] + hb.member(raw(blocks[1], 6), blocks[1], isize=len(blocks[1]) | 0x200) + good[2] + good[3] + hb.EOF
    f.append(row("flipped_isize", "wrong", blob, content, bad_member=1))
    assert f[-1]["stat"]["status"] == 0 and f[-1]["stat"]["content"] == 400 + 0x200

    path = os.path.join(ROOT, "tests", "golden", "bgzf_golden.json")
    with open(path, "w") as fh:
        json.dump(out, fh, indent=1)
        fh.write("\n")
    print(path, os.path.getsize(path), "bytes;", len(out["cases"]), "cases,", len(out["blobs"]), "blobs")


if __name__ == "__main__":
    main()
