"""kmp_bgzf_index_host through the C ABI, no GPU: the serial walk (kx_bgzf_walk of kompressor_amd/csrc/bgzf.h compiled for the host)
over every blob of tests/golden/bgzf_golden.json and over seeded mutants; the prefix arrays against the restatement; BGZF's virtual
offset (what kmp_bgzf_tell answers on the device side) from those arrays against the specification's formula."""
import numpy as np
import pytest

import helpers_bgzf as hb
from kompressor_amd import _lib, build


@pytest.fixture(scope="module")
def lib():
    build.build_all()
    return _lib.load()


def _index(lib, blob, cap=None):
    raw = np.frombuffer(blob, dtype=np.uint8).copy() if blob else np.zeros(1, dtype=np.uint8)
    st = np.zeros(1, dtype=hb.STAT)
    assert lib.kmp_bgzf_index_host(raw.ctypes.data, len(blob), st.ctypes.data, None, None, 0) == 0
    n = int(st[0]["blocks"])
    cap = n + 1 if cap is None else cap
    C = 0x5A5A5A5A5A5A5A5A
    mo = np.full(cap + 2, C, dtype=np.uint64); co = mo.copy()
    st2 = np.zeros(1, dtype=hb.STAT)
    assert lib.kmp_bgzf_index_host(raw.ctypes.data, len(blob), st2.ctypes.data, mo.ctypes.data + 8, co.ctypes.data + 8, cap) == 0
    assert st2.tobytes() == st.tobytes()
    assert mo[0] == C and mo[-1] == C and co[0] == C and co[-1] == C
    return st[0], mo[1:-1], co[1:-1], C


@pytest.mark.parametrize("row", hb.blobs(), ids=lambda r: r["name"])
def test_index_host_on_every_fixture_blob(lib, row):
    blob = row["blob"]
    st, mo, co, C = _index(lib, blob)
    assert st.tobytes() == hb.expected_stat(row).tobytes(), st
    ref, rmo, rco, *_ = hb.walk_reference(blob)
    if int(st["status"]) == 0:
        assert [int(x) for x in mo] == rmo and [int(x) for x in co] == rco
        # room for one entry less than blocks + 1: nothing is written
        _, mo2, co2, _ = _index(lib, blob, cap=int(st["blocks"]))
        assert (mo2 == C).all() and (co2 == C).all()
    else:
        assert (mo == C).all() and (co == C).all(), "a damaged blob writes no prefix"


def test_index_host_on_mutants_and_many_members(lib):
    good = [r["blob"] for r in hb.blobs("foreign")]
    blob, content = hb.many_members(5000)
    for m in hb.mutants(200, 20261022, good) + [blob]:
        st, mo, co, _ = _index(lib, m)
        ref, rmo, rco, *_ = hb.walk_reference(m)
        assert st.tobytes() == ref.tobytes()
        if int(st["status"]) == 0:
            assert [int(x) for x in mo] == rmo and [int(x) for x in co] == rco


def test_argument_errors(lib):
    st = np.zeros(1, dtype=hb.STAT)
    assert lib.kmp_bgzf_index_host(None, 5, st.ctypes.data, None, None, 0) == -2
    assert lib.kmp_bgzf_index_host(st.ctypes.data, 5, None, None, None, 0) == -2
    assert lib.kmp_bgzf_index_host(None, 0, st.ctypes.data, None, None, 0) == 0 and int(st[0]["status"]) == -5
    assert lib.kmp_bgzf_bound(100, 0, 0) == 0 and lib.kmp_bgzf_bound(100, 65281, 0) == 0 and lib.kmp_bgzf_scratch(100, 65281) == 0
    assert lib.kmp_bgzf_bound(0, 4096, 0) == 28 and lib.kmp_bgzf_bound(0, 4096, hb.NO_EOF) == 0
    for g in hb.golden()["cases"]:
        assert lib.kmp_bgzf_bound(g["size"], g["block_bytes"], 0) >= g["length"]
        assert lib.kmp_bgzf_bound(g["size"], g["block_bytes"], 0) - lib.kmp_bgzf_bound(g["size"], g["block_bytes"], hb.NO_EOF) == 28
    assert lib.kmp_bgzf_tell(None, 0) == (1 << 64) - 1 and lib.kmp_bgzf_read_bound(None, 0, 1) == 0 and lib.kmp_bgzf_read_blocks(None, 0, 1, None) == 0


def test_virtual_offsets_follow_the_specification():
    """SAM specification 4.1.1: coffset << 16 | uoffset, coffset the member's start in the file, uoffset the offset in its content.
    From the index arrays of a blob with empty members in the middle: the member that HOLDS position p is the last one starting at or
    before it -- never an empty one in front."""
    import bisect
    row = next(r for r in hb.blobs("foreign") if r["name"] == "empty_members_in_the_middle")
    _, mo, co, *_ = hb.walk_reference(row["blob"])
    for p in (0, 1, 499, 500, 501, 1499):
        i = bisect.bisect_right(co, p) - 1
        v = (mo[i] << 16) | (p - co[i])
        assert co[i] <= p < co[i + 1] and v >> 16 == mo[i] and v & 0xFFFF == p - co[i]
        assert hb.head_reference(row["blob"], v >> 16)[0] == 0 and hb.head_reference(row["blob"], v >> 16)[3] > (v & 0xFFFF)
