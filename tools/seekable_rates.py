"""Rates of the seekable container (kmp_zstd_seekable_*), measured with HIP events on one GPU: profiles/seekable_rates.txt.

  1. the container's overhead: one buffer of --chunks x --frame-kib of the bench corpus at level 3, with and without checksums, against the
     same chunks through kmp_zstd_compress_batch + kmp_compact_batch on the same context (the way without a container).  The XXH64
     pass is the difference between the first two, plan + table the difference between the last two.
  2. the motivation: --one-slice-mib of the same buffer as ONE slice through kmp_zstd_compress_batch on a context made for it.
  3. reads: the whole content with verify on and off, a 1 MiB range, against kmp_zstd_decompress_batch over the same frames with the
     sizes known.

Every figure is the median of --steps timed runs after one warm-up (the range read: of 20; the one slice: one run).  python tools/seekable_rates.py [--out FILE]"""
import argparse
import ctypes
import os
import statistics
import struct
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from kompressor_amd import corpus                    # noqa: E402
from kompressor_amd.batch import ZstdBatch           # noqa: E402


def timed(fn, steps):
    fn(); torch.cuda.synchronize()
    ms = []
    for _ in range(steps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record(); fn(); b.record(); b.synchronize()
        ms.append(a.elapsed_time(b))
    return statistics.median(ms)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--chunks", type=int, default=16384)
    ap.add_argument("--frame-kib", type=int, default=64)
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--one-slice-mib", type=int, default=64)
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    F, n = args.frame_kib * 1024, args.chunks
    size = n * F
    lines = []

    def say(s):
        print(s, flush=True); lines.append(s)
    P = lambda t, at=0: ctypes.c_void_p(t.data_ptr() + at)          # noqa: E731
    src = torch.from_numpy(corpus.make(0, n, F)).cuda()
    b = ZstdBatch(max_slices=n, max_slice_bytes=F)
    lib, st = b.lib, b._stream()
    say(f"# {torch.cuda.get_device_name(0)}; {n} chunks x {args.frame_kib} KiB = {size / 2**30:.3f} GiB of the bench corpus (mix 1), level 3, median of {args.steps}")
    GBs = lambda nbytes, ms: nbytes / ms / 1e6                        # noqa: E731

    # ---- 1. container overhead ----
    io = torch.arange(n, dtype=torch.int64, device="cuda") * F; il = torch.full((n,), F, dtype=torch.int32, device="cuda")
    sparse, oo, ol = b.compress(src, io, il)
    dense = torch.empty(lib.kmp_zstd_seekable_bound(size, F, 1) + 64, dtype=torch.uint8, device="cuda"); offs = torch.empty(n + 1, dtype=torch.int64, device="cuda")

    def batch_way():
        b.compress(src, io, il, dst=sparse, out_off=oo, out_len=ol); b.compact_into(sparse, oo, ol, dense, offs)
    ms_batch = timed(batch_way, args.steps)
    del sparse
    need = lib.kmp_zstd_seekable_scratch(size, F)
    scratch = torch.empty(need // 8 + 1, dtype=torch.int64, device="cuda"); result = torch.zeros(2, dtype=torch.int64, device="cuda")

    def container(flags):
        rc = lib.kmp_zstd_seekable_compress(b._h, P(src), size, F, 3, flags, P(dense), dense.numel() - 64, P(scratch), need, P(result), st)
        assert rc == 0, b._err()
    ms_sum = timed(lambda: container(1), args.steps)
    ms_plain = timed(lambda: container(0), args.steps)
    container(1); csize = int(result[0].item())
    assert csize > 0 and int(result[1].item()) == 0
    say(f"compress_batch + compact_batch (no container): {ms_batch:8.2f} ms  {GBs(size, ms_batch):6.2f} GB/s")
    say(f"seekable container, no checksums             : {ms_plain:8.2f} ms  {GBs(size, ms_plain):6.2f} GB/s   (plan + table: {ms_plain - ms_batch:+.2f} ms)")
    say(f"seekable container, checksums                : {ms_sum:8.2f} ms  {GBs(size, ms_sum):6.2f} GB/s   (XXH64 pass over the input: {ms_sum - ms_plain:+.2f} ms = {GBs(size, max(ms_sum - ms_plain, 1e-3)):.0f} GB/s)")
    say(f"container: {csize} bytes, ratio {size / csize:.3f}")
    blob = dense[:csize].clone()
    del scratch

    # ---- 3. reads ----
    r = b.open_seekable(blob)
    out = torch.empty(size + 64, dtype=torch.uint8, device="cuda"); status = torch.zeros(n, dtype=torch.int32, device="cuda"); skip = ctypes.c_uint64()

    def read(lo, hi, verify):
        rc = lib.kmp_zstd_seekable_read(r._h, P(blob), lo, hi, verify, P(out), size, ctypes.byref(skip), P(status), st)
        assert rc == 0, b._err()
    ms_rv = timed(lambda: read(0, size, 1), args.steps); assert not status.any()
    ms_r = timed(lambda: read(0, size, 0), args.steps); assert not status.any()
    assert torch.equal(out[:size], src)
    table = blob[csize - 17 - 12 * n:].cpu().numpy().tobytes()
    clen = np.array([struct.unpack_from("<I", table, 8 + 12 * i)[0] for i in range(n)], dtype=np.int64)
    fin = torch.from_numpy(np.concatenate(([0], np.cumsum(clen)[:-1]))).cuda(); flen = torch.from_numpy(clen.astype(np.int32)).cuda()

    def plain_decode():
        b.decompress(blob, fin, flen, out_cap=il, dst=out, out_off=io)
    ms_d = timed(plain_decode, args.steps)
    lo = (size // 2) + 12345; hi = lo + (1 << 20)
    us_rng_v = timed(lambda: read(lo, hi, 1), 20) * 1e3; us_rng = timed(lambda: read(lo, hi, 0), 20) * 1e3
    first = ctypes.c_uint32(); m = lib.kmp_zstd_seekable_read_frames(r._h, lo, hi, ctypes.byref(first)); f0 = first.value
    us_plain = timed(lambda: b.decompress(blob, fin[f0:f0 + m], flen[f0:f0 + m], out_cap=il[:m], dst=out, out_off=io[:m]), 20) * 1e3
    say(f"decompress_batch over the same frames, sizes known: {ms_d:8.2f} ms  {GBs(size, ms_d):6.2f} GB/s of content")
    say(f"read_all, verify off                              : {ms_r:8.2f} ms  {GBs(size, ms_r):6.2f} GB/s")
    say(f"read_all, verify on                               : {ms_rv:8.2f} ms  {GBs(size, ms_rv):6.2f} GB/s   (XXH64 pass over the content: {ms_rv - ms_r:+.2f} ms = {GBs(size, max(ms_rv - ms_r, 1e-3)):.0f} GB/s)")
    say(f"read of 1 MiB at an odd offset ({m} frames): {us_rng:.0f} us, verified {us_rng_v:.0f} us   (decompress_batch over these {m} frames alone: {us_plain:.0f} us)")
    r.close(); b.close()
    del out, dense, blob

    # ---- 2. the same bytes as ONE slice ----
    one = min(args.one_slice_mib << 20, size)
    b1 = ZstdBatch(max_slices=1, max_slice_bytes=one)
    io1 = torch.zeros(1, dtype=torch.int64, device="cuda"); il1 = torch.full((1,), one, dtype=torch.int32, device="cuda")
    d1, oo1, ol1 = b1.compress(src, io1, il1)
    ms_one = timed(lambda: b1.compress(src, io1, il1, dst=d1, out_off=oo1, out_len=ol1), 1)
    assert int(ol1[0].item()) > 0
    say(f"ONE slice of {one >> 20} MiB through compress_batch        : {ms_one:8.2f} ms  {GBs(one, ms_one):6.3f} GB/s   (the container: {GBs(size, ms_sum) / GBs(one, ms_one):.0f} x)")
    b1.close()
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
