"""The body of k_inflate_size (kompressor_amd/csrc/deflate_info.h) on the CPU wave emulator: the fixture in batches of several sizes at
unaligned offsets, seeded mutants against the live zlib, and the three-step recipe -- sizing, the layout kernel, the emulated inflate
kernels -- end to end.  No GPU."""
import ctypes

import numpy as np
import pytest

import helpers
import helpers_frame_info as hf
import helpers_inflate_info as hi

N_MUTANTS = 3000
MUTANT_SEED = 20261018


@pytest.fixture(scope="module")
def rows():
    return hi.golden()


def test_fixture_holds_what_the_issue_lists(rows):
    by = {(n, f): r for n, _, f, r in rows}
    for name in ("empty input", "1 byte", "level 0, 0 bytes", "level 0, 1 bytes", "level 0, 65535 bytes", "level 0, 65536 bytes",
                 "empty stored block of Z_SYNC_FLUSH in front of a final block", "stored + fixed + dynamic blocks",
                 "dynamic block, distance set of one code of length 1", "dynamic block, no distance code, literals only", "100 000 zero bytes",
                 "70 000 random bytes at level 6", "300 000 bytes of text", "codes of 15 bits (literal/length) and 9 bits (distance)"):
        assert by[(name, 0)]["status"] == 0, name
    assert by[("level 0, 65535 bytes", 0)]["blocks"] >= 1 and by[("level 0, 65536 bytes", 0)]["blocks"] >= 2          # (as this zlib cuts them)
    assert by[("stored + fixed + dynamic blocks", 0)]["flags"] == 7 and by[("300 000 bytes of text", 0)]["blocks"] >= 3
    assert by[("100 000 zero bytes", 0)]["content"] == 100000 and by[("zlib, windowBits 9", 1)]["window_bits"] == 9
    assert by[("gzip, FEXTRA + FNAME + FCOMMENT + FHCRC", 2)]["flags"] & 24 == 24 and by[("gzip plain", 2)]["flags"] & 24 == 8
    for name, fmt in (("zlib, FDICT set", 1), ("zlib, header fails the mod-31 check", 1), ("gzip, reserved FLG bit", 2), ("gzip, ISIZE off by one", 2),
                      ("block type 3", 0), ("stored block, LEN / NLEN mismatch", 0), ("over-subscribed literal/length set", 0),
                      ("incomplete literal/length set", 0), ("no end-of-block code", 0), ("distance beyond the output so far", 0),
                      ("60-byte raw stream, one byte appended", 0), ("60-byte zlib stream, one byte appended", 1), ("60-byte gzip stream, one byte appended", 2)):
        assert by[(name, fmt)]["status"] == -3, name
    assert by[("zlib, wrong Adler-32", 1)]["kind"] == "checksum" and by[("format 3 over gzip", 3)]["status"] == 0
    for fmt in (0, 1, 2):
        for k in range(60):
            r = by[(f"60-byte {hi.FMT_NAMES[fmt]} stream, first {k} bytes", fmt)]
            assert r["status"] == -5 if k >= hi.WRAPPER_MIN[fmt] else r["status"] != 0
    for _, e, f, r in rows:                                    # the answers are the rule's
        kind, val = hi.verdict(e, f)
        assert kind == r["kind"] or (r["kind"] == "reject" and len(e) < 18), r["name"]
        if kind == "ok":
            assert (r["status"], r["content"]) == (0, len(val)), r["name"]
        elif kind == "reject":
            assert r["status"] != 0 and r["content"] == 0, r["name"]


@pytest.mark.parametrize("n", (1, 15, 16, 17, 0))
def test_fixture_in_batches(rows, n):
    """every entry at an unaligned offset with canary bytes between the entries; n = 0: each format's entries as one batch"""
    want = hi.expected_array([r for *_, r in rows])
    got = np.zeros(len(rows), dtype=hi.INFO)
    for fmt, idx in hi.by_format(rows).items():
        step = n or len(idx)
        for k in range(0, len(idx), step):
            part = idx[k:k + step]
            src, offs, lens = hi.pack([rows[i][1] for i in part], seed=n + k)
            got[part] = hi.emu_inflate_info(src, offs, lens, fmt)
    bad = hi.diff(got, want, [f"{r[0]} / {hi.FMT_NAMES[r[2]]}" for r in rows])
    assert not bad, "\n".join(bad[:20])
    assert got.tobytes() == want.tobytes()                     # all 32 bytes: nothing in the unused bits


def test_entries_end_at_a_guard_page(rows):
    """every entry ends on the last byte in front of a PROT_NONE page: a read past its end kills the process"""
    from fuzz_decoders import Guarded
    small = [r for r in rows if len(r[1]) <= 4096]
    got = np.zeros(len(small), dtype=hi.INFO)
    for i, (_, e, fmt, _) in enumerate(small):
        g = Guarded(max(len(e), 1), 0)
        at = g.off + (1 if not e else 0)
        g.write(e)
        got[i] = hi.emu_inflate_info(g.base, np.array([at], dtype=np.uint64), np.array([len(e)], dtype=np.uint32), fmt)[0]
        g.close()
    assert got.tobytes() == hi.expected_array([r for *_, r in small]).tobytes()


def test_mutants_against_the_live_zlib():
    muts = hi.mutants(N_MUTANTS, MUTANT_SEED)
    got = hi.emu_cases(muts)
    bad, counts = hi.check_against_zlib(muts, got)
    print(f"{len(muts)} mutants: zlib alone says {counts}")
    hi.assert_not_hollow(counts)
    assert not bad, "\n".join(bad[:20])


@pytest.mark.parametrize("align", (1, 64))
def test_sizing_layout_inflate(rows, align):
    """kmp_inflate_info_batch -> kmp_batch_layout -> kmp_inflate_batch as emulated kernels: a mixed batch per format"""
    e = helpers.emu()
    e.emu_inflate.argtypes = [ctypes.c_void_p] * 3 + [ctypes.c_uint32] + [ctypes.c_void_p] * 5 + [ctypes.c_uint32]
    e.emu_inflate_pre.argtypes = [ctypes.c_void_p] * 3 + [ctypes.c_uint32] + [ctypes.c_void_p] * 5 + [ctypes.c_uint32, ctypes.c_uint32, ctypes.c_void_p]
    vp = helpers._vp
    for fmt, idx in hi.by_format(rows).items():
        part = [rows[i] for i in idx]
        n = len(part)
        src, offs, lens = hi.pack([r[1] for r in part], seed=align + fmt)
        info = hi.emu_inflate_info(src, offs, lens, fmt)
        out_off, out_cap, total = hf.emu_layout(info, align)
        verdicts = [hi.verdict(r[1], fmt) for r in part]
        for i, (kind, val) in enumerate(verdicts):
            assert int(out_cap[i]) == (len(val) if kind == "ok" else int(info["content"][i])), part[i][0]
            assert int(out_off[i]) % align == 0
        assert int(total[1]) == sum(1 for g in info if g["status"] != 0)
        for pre in (False, True):
            dst = np.full(int(total[0]) + 64, 0xC3, dtype=np.uint8)
            out_len = np.zeros(n, dtype=np.uint32); st = np.zeros(n, dtype=np.int32); cov = np.zeros(n, dtype=np.uint32)
            if pre:
                rc = e.emu_inflate_pre(vp(src), vp(offs), vp(lens), n, vp(dst), vp(out_off), vp(out_cap), vp(out_len), vp(st), fmt, 65536, vp(cov))
            else:
                rc = e.emu_inflate(vp(src), vp(offs), vp(lens), n, vp(dst), vp(out_off), vp(out_cap), vp(out_len), vp(st), fmt)
            assert rc == 0
            untouched = np.ones(len(dst), dtype=bool)
            for i, (kind, val) in enumerate(verdicts):
                o = int(out_off[i])
                if kind == "ok":
                    assert int(st[i]) == 0 and dst[o:o + int(out_len[i])].tobytes() == val, part[i][0]
                    untouched[o:o + len(val)] = False
                else:
                    assert int(st[i]) != 0, part[i][0]               # (rejected by the sizing pass: capacity 0; refused for its data check: its size)
                    assert kind == "checksum" or int(out_cap[i]) == 0
                    untouched[o:o + int(out_cap[i])] = False
            assert (dst[untouched] == 0xC3).all(), "bytes between the slots were written"
