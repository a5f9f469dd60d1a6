"""The ladder of tests/helpers_team.py through the public batch calls: slices whose sequence counts sit on the edges of the parsers'
shared sequence sink (kompressor_amd/csrc/zstd_team.h), at team widths 4 and 8, levels 3 and 1, without and with a 16 KiB raw
dictionary.  Frames are the binary libzstd 1.5.7's; the counts are read back from the context's slice records."""
import ctypes

import numpy as np
import pytest

import helpers_team as ht

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")


@pytest.mark.parametrize("G", ht.TEAMS)
def test_ladder_through_the_batch_calls(G):
    from kompressor_amd import _lib
    from kompressor_amd.batch import ZstdBatch
    d, slices = ht.ladder()
    n = len(slices)
    lens = np.array([len(s) for s in slices], dtype=np.int32)
    offs = np.concatenate([[0], np.cumsum(lens[:-1].astype(np.int64))]).astype(np.int64)
    host = np.frombuffer(b"".join(slices) + bytes(64), dtype=np.uint8).copy()
    src, off, ln = torch.from_numpy(host).cuda(), torch.from_numpy(offs).cuda(), torch.from_numpy(lens).cuda()
    b = ZstdBatch(max_slices=n, max_slice_bytes=4096, team_lanes=G)
    try:
        for name, level, with_dict in ht.CONFIGS:
            dst, ooff, olen = b.compress(src, off, ln, dictionary=d if with_dict else None, level=level)
            torch.cuda.synchronize()
            dd, oo, ol = dst.cpu().numpy(), ooff.cpu().numpy(), olen.cpu().numpy()
            ht.check_frames(name, [dd[oo[i]:oo[i] + ol[i]].tobytes() for i in range(n)])
            meta = np.zeros(n, dtype=ht.META)
            assert _lib.load().kmp_debug_copy_meta(b._h, ctypes.c_void_p(meta.ctypes.data), n) == 0
            counts = set(int(c) for c in meta["nbSeq"])
            assert ht.wanted_counts(G) <= counts, (name, G, sorted(counts))
    finally:
        b.close()
