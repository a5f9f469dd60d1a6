#!/usr/bin/env python3
"""What frame inspection costs beside the decode it prepares (profiles/frame_info_rates.txt).

On one MI355X, over the 65 536 level-3 frames of BASELINE configs[1]'s slices (64 KiB, mixed classes):
  (a) kmp_zstd_frame_info_batch + kmp_batch_layout alone
  (b) ZstdBatch.decompress with known capacities (the path that existed before)
  (c) ZstdBatch.decompress(out_cap=None): (a), the read-back of the total, the allocation, (b)
  (d) what a caller did without (a): the frames copied to the host, kmp_zstd_frame_info_host over them
and (a) over 8 192 streaming frames of 1 MiB in 9 blocks each (no declared size: every lane walks nine block headers spread over its
frame; 64 distinct frames, repeated).

Device times are HIP events around `reps` calls after `warmup` calls, the median of `rounds` such brackets; (c) and (d) include host
work and are wall clock around a synchronize.  KMP_LIB_PATH names another build of the library (the parent commit's) for (b).

    python tools/experiments/frame_info_rates.py [--slices 65536] [--only-b]
"""
import argparse
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)

import torch                                              # noqa: E402
from kompressor_amd import corpus                         # noqa: E402
from kompressor_amd import _lib                           # noqa: E402
from kompressor_amd.batch import ZstdBatch                # noqa: E402


def device_ms(fn, warmup, reps, rounds):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    out = []
    for _ in range(rounds):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(reps):
            fn()
        e1.record()
        torch.cuda.synchronize()
        out.append(e0.elapsed_time(e1) / reps)
    return statistics.median(out), min(out), max(out)


def wall_ms(fn, warmup, rounds):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    out = []
    for _ in range(rounds):
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        out.append((time.perf_counter() - t0) * 1e3)
    return statistics.median(out), min(out), max(out)


def fmt(name, t, extra=""):
    print(f"{name:58s} median {t[0]:10.3f} ms   min {t[1]:10.3f}   max {t[2]:10.3f}   {extra}", flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--slices", type=int, default=65536)
    ap.add_argument("--only-b", action="store_true", help="(b) alone: what another build of the library (KMP_LIB_PATH) is timed with")
    args = ap.parse_args()
    n, S = args.slices, 65536
    if args.only_b:
        # (a build from before these calls existed lacks their exports: bind what it has)
        import ctypes
        probe = ctypes.CDLL(_lib.LIB_PATH)
        _lib.SIGNATURES[:] = [sig for sig in _lib.SIGNATURES if hasattr(probe, sig[0])]
    print(f"library: {os.environ.get('KMP_LIB_PATH') or 'this tree'}; device: {torch.cuda.get_device_name(0)}; {n} slices of {S} bytes", flush=True)
    b = ZstdBatch(max_slices=n, max_slice_bytes=S)
    host = corpus.make(0, n, S)
    src = torch.from_numpy(host.reshape(-1)).cuda()
    in_off = torch.arange(n, dtype=torch.int64, device="cuda") * S
    in_len = torch.full((n,), S, dtype=torch.int32, device="cuda")
    dst, out_off, out_len = b.compress(src, in_off, in_len, check=True)
    frames, offs = b.compact(dst, out_off, out_len)
    f_off = offs[:n].contiguous()
    torch.cuda.synchronize()
    frame_bytes = int(offs[n].item())
    del dst
    print(f"frames: {frame_bytes} bytes ({frame_bytes / n:.0f} per frame)", flush=True)
    back = torch.empty(n * S + 64, dtype=torch.uint8, device="cuda")

    t_b = device_ms(lambda: b.decompress(frames, f_off, out_len, in_len, dst=back, out_off=in_off), 2, 3, 7)
    ok = torch.equal(back[:n * S], src)
    fmt("(b) decompress, known capacities (device)", t_b, f"round trip {'ok' if ok else 'WRONG'}; {n * S / t_b[0] / 1e6:.1f} GB/s decoded")
    if args.only_b:
        return
    del back

    def inspect():
        return b.layout(b._frame_info_raw(frames, f_off, out_len), 1)
    t_a = device_ms(inspect, 3, 20, 7)
    off, cap, total = inspect()
    torch.cuda.synchronize()
    assert int(total[0].item()) == n * S and int(total[1].item()) == 0 and torch.equal(cap, in_len)
    fmt("(a) frame_info + layout (device)", t_a, f"{t_a[0] / t_b[0] * 100:.3f} % of (b); {n / t_a[0] / 1e3:.1f} M entries/s")
    t_i = device_ms(lambda: b._frame_info_raw(frames, f_off, out_len), 3, 20, 7)
    fmt("    frame_info alone (device)", t_i)
    info = b._frame_info_raw(frames, f_off, out_len)
    t_l = device_ms(lambda: b.layout(info, 1), 3, 20, 7)
    fmt("    layout alone (device)", t_l)

    t_bw = wall_ms(lambda: b.decompress(frames, f_off, out_len, in_len), 2, 7)
    fmt("(b') decompress, known capacities, dst allocated (wall)", t_bw)
    t_c = wall_ms(lambda: b.decompress(frames, f_off, out_len), 2, 7)
    r = b.decompress(frames, f_off, out_len)
    torch.cuda.synchronize()
    ok = bool(int(r[3].abs().sum().item()) == 0 and torch.equal(r[0][:n * S], src))
    fmt("(c) decompress(out_cap=None) (wall)", t_c, f"(c) - (b') = {t_c[0] - t_bw[0]:.3f} ms; round trip {'ok' if ok else 'WRONG'}")
    del r

    lens_h = out_len.cpu().numpy()
    offs_h = f_off.cpu().numpy()

    def on_host():
        h = frames[:frame_bytes].cpu().numpy()
        return frame_info_host_arrays(h, offs_h, lens_h)
    t_d = wall_ms(on_host, 1, 5)
    frames_h = frames[:frame_bytes].cpu().numpy()
    t_dp = wall_ms(lambda: frame_info_host_arrays(frames_h, offs_h, lens_h), 1, 5)
    fmt("(d) frames to the host + kmp_zstd_frame_info_host (wall)", t_d, f"(a) is {t_d[0] / t_a[0]:.0f} x faster")
    fmt("    kmp_zstd_frame_info_host alone (wall)", t_dp)
    want = on_host()
    assert want.tobytes() == info.cpu().numpy().tobytes()
    del src, frames

    # the divergent case: streaming frames of 1 MiB, nine blocks each, no declared size (compressed on a context for such slices,
    # inspected on the first one: inspection uses nothing of a context but its device and max_slices)
    m, reps_of = 64, 128
    sb = ZstdBatch(max_slices=m, max_slice_bytes=1 << 20)
    shost = corpus.make(1 << 20, m * 16, S).reshape(m, 1 << 20)
    ssrc = torch.from_numpy(shost.reshape(-1)).cuda()
    s_off = torch.arange(m, dtype=torch.int64, device="cuda") << 20
    s_len = torch.full((m,), 1 << 20, dtype=torch.int32, device="cuda")
    sdst, so, sl = sb.compress(ssrc, s_off, s_len, streaming="empty", check=True)
    sframes, soffs = sb.compact(sdst, so, sl)
    torch.cuda.synchronize()
    one = int(soffs[m].item())
    rep = sframes[:one].repeat(reps_of)
    r_off = (soffs[:m].repeat(reps_of) + torch.arange(reps_of, dtype=torch.int64, device="cuda").repeat_interleave(m) * one).contiguous()
    r_len = sl.repeat(reps_of).contiguous()
    ns = m * reps_of

    def inspect_s():
        return b.layout(b._frame_info_raw(rep, r_off, r_len), 1)
    t_s = device_ms(inspect_s, 3, 20, 7)
    info_s = b._frame_info_raw(rep, r_off, r_len).cpu().numpy()
    assert (info_s[:, 0] == -1).all() and (info_s[:, 1] >= 9 * 131072).all() and (info_s[:, 2] == 1 << 32).all(), info_s[:2]
    blocks = info_s[:, 1] // 131072                          # (nine, or more where the pre-splitter cut a chunk)
    fmt(f"(a) over {ns} streaming frames of 1 MiB (device)", t_s,
        f"{ns / t_s[0] / 1e3:.1f} M entries/s; {int(blocks.min())} .. {int(blocks.max())} blocks a frame, {float(blocks.mean()):.2f} on average; {one * reps_of} bytes of frames")
    sb.close()
    b.close()


def frame_info_host_arrays(h, offs, lens):
    """kmp_zstd_frame_info_host over one host buffer (no per-frame Python objects)"""
    import ctypes
    lib = _lib.load()
    n = len(lens)
    info = np.zeros((n, 4), dtype=np.int64)
    o = np.ascontiguousarray(offs, dtype=np.uint64); ln = np.ascontiguousarray(lens, dtype=np.uint32)
    rc = lib.kmp_zstd_frame_info_host(ctypes.c_void_p(h.ctypes.data), ctypes.c_void_p(o.ctypes.data), ctypes.c_void_p(ln.ctypes.data), n,
                                      ctypes.c_void_p(info.ctypes.data))
    assert rc == 0
    return info


if __name__ == "__main__":
    main()
