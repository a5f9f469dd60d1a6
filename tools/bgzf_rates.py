"""Rates of the BGZF container (kmp_bgzf_*), measured with HIP events on one GPU: profiles/bgzf_rates.txt.

  1. the container's overhead: one buffer of --blocks x 65 280 bytes of the bench corpus at level 6 against the same blocks through
     kmp_deflate_compress_batch_level(format 0) + kmp_compact_batch on the same context (the way without a container).  The container
     adds one read of the source for CRC-32, 26 bytes per member and two small launches.
  2. the motivation: --one-slice-mib of the same buffer as ONE slice through kmp_gzip_compress_batch on a context made for it.
  3. the open: the parallel open against k_bgzf_walk (the ablation build of the library, where the candidate cap is a variable: 0 sends
     every blob down the serial walk), on the container of 65 280-byte blocks and on one of 4 096-byte blocks over the same buffer
     (compressed in rounds of the context's max_slices with KMP_BGZF_NO_EOF and concatenated).
  4. reads: the whole content with verify on and off against kmp_inflate_batch(format 0) over the same payloads; a 1 MiB range.

Every figure is the median of --steps timed runs after one warm-up (the range read: of 20; the one slice: one run).  python tools/bgzf_rates.py [--out FILE]"""
import argparse
import ctypes
import os
import statistics
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from kompressor_amd import corpus                    # noqa: E402
from kompressor_amd.batch import ZstdBatch           # noqa: E402

B = 65280


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
    ap.add_argument("--blocks", type=int, default=16448)           # x 65 280 bytes = 1.0000 GiB
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--one-slice-mib", type=int, default=16)
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    n = args.blocks
    size = n * B
    lines = []

    def say(s):
        print(s, flush=True); lines.append(s)
    P = lambda t, at=0: ctypes.c_void_p(t.data_ptr() + at)          # noqa: E731
    GBs = lambda nbytes, ms: nbytes / ms / 1e6                        # noqa: E731
    src = torch.from_numpy(corpus.make(0, n, B)).cuda()
    b = ZstdBatch(max_slices=n, max_slice_bytes=65536, table_span_gib=0)
    lib, st = b.lib, b._stream()
    say(f"# {torch.cuda.get_device_name(0)}; {n} blocks x {B} bytes = {size / 2**30:.3f} GiB of the bench corpus (mix 1), zlib level 6, median of {args.steps}")

    # ---- 1. container overhead ----
    io = torch.arange(n, dtype=torch.int64, device="cuda") * B; il = torch.full((n,), B, dtype=torch.int32, device="cuda")
    sparse, oo, ol = b.deflate(src, io, il, format="raw")
    dense = torch.empty(lib.kmp_bgzf_bound(size, B, 0) + 64, dtype=torch.uint8, device="cuda"); offs = torch.empty(n + 1, dtype=torch.int64, device="cuda")

    def batch_way():
        b.deflate(src, io, il, dst=sparse, out_off=oo, out_len=ol, format="raw"); b.compact_into(sparse, oo, ol, dense, offs)
    ms_batch = timed(batch_way, args.steps)
    del sparse
    need = lib.kmp_bgzf_scratch(size, B)
    scratch = torch.empty(need // 8 + 1, dtype=torch.int64, device="cuda"); result = torch.zeros(2, dtype=torch.int64, device="cuda")

    def container():
        rc = lib.kmp_bgzf_compress(b._h, P(src), size, B, 6, 0, P(dense), dense.numel() - 64, P(scratch), need, P(result), st)
        assert rc == 0, b._err()
    ms_c = timed(container, args.steps)
    csize = int(result[0].item())
    assert csize > 0 and int(result[1].item()) == 0
    say(f"deflate_batch(raw) + compact_batch (no container): {ms_batch:8.2f} ms  {GBs(size, ms_batch):6.2f} GB/s")
    say(f"BGZF container                                   : {ms_c:8.2f} ms  {GBs(size, ms_c):6.2f} GB/s   (plan, CRC-32 pass over the input, headers, marker: {ms_c - ms_batch:+.2f} ms)")
    say(f"container: {csize} bytes, ratio {size / csize:.3f}")
    blob = dense[:csize].clone()
    del scratch, dense

    # ---- 4. reads ----
    r = b.open_bgzf(blob)
    assert r.status == 0 and r.blocks == n + 1
    out = torch.empty(size + 64, dtype=torch.uint8, device="cuda"); status = torch.zeros(n + 1, dtype=torch.int32, device="cuda"); skip = ctypes.c_uint64()

    def read(lo, hi, verify):
        rc = lib.kmp_bgzf_read(r._h, P(blob), lo, hi, verify, P(out), size, ctypes.byref(skip), P(status), st)
        assert rc == 0, b._err()
    ms_rv = timed(lambda: read(0, size, 1), args.steps); assert not status.any()
    ms_r = timed(lambda: read(0, size, 0), args.steps); assert not status.any()
    assert torch.equal(out[:size], src)
    raw = blob.cpu().numpy()
    stt = np.zeros(4, dtype=np.uint64); mo = np.zeros(n + 2, dtype=np.uint64)
    assert lib.kmp_bgzf_index_host(raw.ctypes.data, csize, stt.ctypes.data, mo.ctypes.data, None, n + 2) == 0
    pin = torch.from_numpy((mo[:n] + 18).astype(np.int64)).cuda(); plen = torch.from_numpy((mo[1:n + 1] - mo[:n] - 26).astype(np.int32)).cuda()

    def plain_inflate():
        b.inflate(blob, pin, plen, out_cap=il, dst=out, out_off=io, format="raw")
    ms_d = timed(plain_inflate, args.steps)
    lo = (size // 2) + 12345; hi = lo + (1 << 20)
    us_rng_v = timed(lambda: read(lo, hi, 1), 20) * 1e3; us_rng = timed(lambda: read(lo, hi, 0), 20) * 1e3
    m = lib.kmp_bgzf_read_blocks(r._h, lo, hi, None)
    say(f"inflate_batch(raw) over the same payloads, sizes known: {ms_d:8.2f} ms  {GBs(size, ms_d):6.2f} GB/s of content")
    say(f"read_all, verify off                                  : {ms_r:8.2f} ms  {GBs(size, ms_r):6.2f} GB/s")
    say(f"read_all, verify on                                   : {ms_rv:8.2f} ms  {GBs(size, ms_rv):6.2f} GB/s   (CRC-32 pass over the content: {ms_rv - ms_r:+.2f} ms)")
    say(f"read of 1 MiB at an odd offset ({m} members): {us_rng:.0f} us, verified {us_rng_v:.0f} us")
    r.close()
    del out

    # ---- 3. the open ----
    # 4 096-byte blocks over the same buffer: rounds of n blocks each, no marker on any but the last
    per = n * 4096
    parts = []
    for at in range(0, size, per):
        parts.append(b.compress_bgzf(src[at:at + per], block_bytes=4096, level=6, eof=at + per >= size).clone())
    small = torch.cat(parts)
    del parts
    b.close()
    a = ZstdBatch(max_slices=8, max_slice_bytes=4096, ablations=True, table_span_gib=0)

    def open_ms(t, cap):
        if cap is None:
            os.environ.pop("KMP_BGZF_MAX_CANDIDATES", None)
        else:
            os.environ["KMP_BGZF_MAX_CANDIDATES"] = str(cap)
        seen = []

        def once():
            h = a.open_bgzf(t); seen.append((h.status, h.blocks)); h.close()
        ms = timed(once, args.steps)
        os.environ.pop("KMP_BGZF_MAX_CANDIDATES", None)
        return ms, seen[0]
    for name, t in ((f"{B}-byte blocks", blob), ("4096-byte blocks", small)):
        ms_p, seen_p = open_ms(t, None)
        ms_w, seen_w = open_ms(t, 0)
        assert seen_p == seen_w and seen_p[0] == 0
        members = seen_p[1]
        say(f"open, {name} ({members} members, {t.numel()} bytes): parallel {ms_p:8.2f} ms ({GBs(t.numel(), ms_p):6.1f} GB/s of blob), "
            f"k_bgzf_walk {ms_w:8.2f} ms = {ms_w * 1e6 / (2 * members):.0f} ns per member and pass (two passes: the count, then the arrays; "
            f"the estimate from 900 cycles per miss at 2.4 GHz: {members * 900 / 2.4e6:.2f} ms per pass)")
    a.close()
    del small, blob

    # ---- 2. the same bytes as ONE slice ----
    one = min(args.one_slice_mib << 20, size)
    b1 = ZstdBatch(max_slices=1, max_slice_bytes=one, table_span_gib=0)
    io1 = torch.zeros(1, dtype=torch.int64, device="cuda"); il1 = torch.full((1,), one, dtype=torch.int32, device="cuda")
    cap1 = (b1.lib.kmp_deflate_bound(one) + 63) & ~63
    d1 = torch.empty(cap1 + 64, dtype=torch.uint8, device="cuda"); ol1 = torch.zeros(1, dtype=torch.int32, device="cuda")

    def one_slice():
        rc = b1.lib.kmp_gzip_compress_batch(b1._h, P(src), P(io1), P(il1), 1, P(d1), P(io1), P(ol1), b1._stream())
        assert rc == 0, b1._err()
    a0, a1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a0.record(); one_slice(); a1.record(); a1.synchronize()
    ms_one = a0.elapsed_time(a1)
    assert int(ol1[0].item()) > 0
    say(f"ONE slice of {one >> 20} MiB through gzip_compress_batch (one run, no warm-up): {ms_one:8.2f} ms  {GBs(one, ms_one):6.4f} GB/s   (the container: {GBs(size, ms_c) / GBs(one, ms_one):.0f} x)")
    b1.close()
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
