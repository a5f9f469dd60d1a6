"""What the frame flags (kmp_batch_set_frame_flags) cost the plain batch, measured with HIP events on one GPU: profiles/frame_flags_rates.txt.

  --chunks x --slice-kib of the bench corpus through kmp_zstd_compress_batch at level 3 on one context, with flags 0 and with
  KMP_FRAME_CHECKSUM (the XXH64 pass over the input is the difference).  --baseline-lib PATH: the same call through another build of the
  library in the same session, on a context of its own before and after -- the yardstick for flags 0 is the build without the feature.

Every figure is the median of --steps timed runs after one warm-up.  python tools/frame_flags_rates.py [--baseline-lib PATH] [--out FILE]"""
import argparse
import ctypes
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from kompressor_amd import _lib, corpus              # noqa: E402


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
    ap.add_argument("--slice-kib", type=int, default=64)
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--baseline-lib", default="")
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    F, n = args.slice_kib * 1024, args.chunks
    size = n * F
    lines = []

    def say(s):
        print(s, flush=True); lines.append(s)
    P = lambda t: ctypes.c_void_p(t.data_ptr())                        # noqa: E731
    GBs = lambda ms: size / ms / 1e6                                   # noqa: E731
    lib = _lib.load()
    src = torch.from_numpy(corpus.make(0, n, F)).cuda()
    io = torch.arange(n, dtype=torch.int64, device="cuda") * F; il = torch.full((n,), F, dtype=torch.int32, device="cuda")
    stride = (lib.kmp_zstd_compress_bound(F) + 8 + 63) & ~63
    dst = torch.empty(n * stride + 64, dtype=torch.uint8, device="cuda"); oo = torch.arange(n, dtype=torch.int64, device="cuda") * stride
    ol = torch.zeros(n, dtype=torch.int32, device="cuda")
    st = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    say(f"# {torch.cuda.get_device_name(0)}; {n} slices x {args.slice_kib} KiB = {size / 2**30:.3f} GiB of the bench corpus (mix 1), kmp_zstd_compress_batch (level 3), median of {args.steps}")

    def batch_on(l):
        """a context of library l for this batch -> (handle, the call)"""
        h = ctypes.c_void_p()
        l.kmp_batch_create.argtypes = [ctypes.POINTER(ctypes.c_void_p), ctypes.c_int, ctypes.c_uint32, ctypes.c_uint32, ctypes.c_int]
        l.kmp_zstd_compress_batch.argtypes = [ctypes.c_void_p] * 4 + [ctypes.c_uint32] + [ctypes.c_void_p] * 4
        l.kmp_batch_destroy.argtypes = [ctypes.c_void_p]; l.kmp_batch_destroy.restype = None
        assert l.kmp_batch_create(ctypes.byref(h), 0, n, F, 0) == 0

        def call():
            assert l.kmp_zstd_compress_batch(h, P(src), P(io), P(il), n, P(dst), P(oo), P(ol), st) == 0
        return h, call

    def baseline(label):
        base = ctypes.CDLL(args.baseline_lib)
        h, call = batch_on(base)
        ms = timed(call, args.steps)
        base.kmp_batch_destroy(h)
        say(f"{label}: {ms:8.2f} ms  {GBs(ms):6.2f} GB/s")
        return ms

    before = baseline("baseline build, before           ") if args.baseline_lib else None
    h, call = batch_on(lib)
    assert lib.kmp_batch_frame_flags(h) == 0
    ms0 = timed(call, args.steps)
    plain = int(ol.to(torch.int64).sum().item())
    assert lib.kmp_batch_set_frame_flags(h, 1) == 0
    ms1 = timed(call, args.steps)
    summed = int(ol.to(torch.int64).sum().item())
    assert lib.kmp_batch_set_frame_flags(h, 0) == 0
    ms0b = timed(call, args.steps)
    lib.kmp_batch_destroy(h)
    assert summed == plain + 4 * n and plain > 0
    say(f"flags 0                           : {ms0:8.2f} ms  {GBs(ms0):6.2f} GB/s" + (f"   ({100 * (ms0 / before - 1):+.2f} % against the baseline build)" if before else ""))
    say(f"flags KMP_FRAME_CHECKSUM          : {ms1:8.2f} ms  {GBs(ms1):6.2f} GB/s   (XXH64 pass over the input: {ms1 - ms0:+.2f} ms = {ms1 / ms0 * 100 - 100:+.2f} %)")
    say(f"flags 0 again                     : {ms0b:8.2f} ms  {GBs(ms0b):6.2f} GB/s")
    if args.baseline_lib:
        baseline("baseline build, after            ")
    say(f"frames: {plain} bytes without, {summed} with the checksums (4 bytes a frame)")
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
