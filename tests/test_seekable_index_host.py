"""kmp_zstd_seekable_index_host: the table's validation compiled for the host (kompressor_amd/csrc/zstd_seekable.h), no GPU touched --
the fixture's foreign and damaged containers, and the prefix sums of a good one."""
import numpy as np
import pytest

import helpers_seekable as hs


def _lib():
    from kompressor_amd import _lib
    return _lib.load()


@pytest.mark.parametrize("row", hs.blobs(), ids=lambda r: r["name"])
def test_fixture_blobs(row):
    raw = np.frombuffer(row["blob"], dtype=np.uint8).copy()
    st = np.zeros(1, dtype=hs.STAT)
    n = row["stat"]["frames"]
    fo = np.full(n + 2, 7, dtype=np.uint64); co = np.full(n + 2, 7, dtype=np.uint64)
    assert _lib().kmp_zstd_seekable_index_host(raw.ctypes.data, len(raw), st.ctypes.data, fo.ctypes.data, co.ctypes.data, n + 1) == 0
    assert st[0].tobytes() == hs.expected_stat(row).tobytes()
    if row["stat"]["status"] == 0:
        _, want_fo, want_co = hs.parse_table(row["blob"])
        assert [int(x) for x in fo[:n + 1]] == want_fo and [int(x) for x in co[:n + 1]] == want_co and fo[n + 1] == 7 and co[n + 1] == 7
    else:
        assert (fo == 7).all() and (co == 7).all()


def test_arguments():
    st = np.zeros(1, dtype=hs.STAT)
    assert _lib().kmp_zstd_seekable_index_host(None, 17, st.ctypes.data, None, None, 0) == -2
    assert _lib().kmp_zstd_seekable_index_host(None, 0, None, None, None, 0) == -2
    assert _lib().kmp_zstd_seekable_index_host(None, 0, st.ctypes.data, None, None, 0) == 0 and int(st[0]["status"]) == 10
    assert _lib().kmp_zstd_seekable_bound(300001, 65536, 1) == 4 * (65536 + 256 + 32) + (37857 + 147 + 45) + 17 + 5 * 12
    assert _lib().kmp_zstd_seekable_bound(0, 65536, 0) == 17
