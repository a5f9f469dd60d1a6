"""Throughput of ZstdBatch.compress with a dictionary at several levels on the two dictionary configurations of the README:
262 144 x 8 KiB records with a 64 KiB dictionary and 65 536 x 64 KiB slices with a 16 KiB dictionary (seeded mixed corpus, the
dictionary of bench.py --dict-kib: raw content, or --trained: zstd's own format from ZDICT on other slices of the corpus).

  python tools/experiments/dict_levels_rates.py [--config records|slices|both] [--levels 3,1,-1] [--steps 5] [--warmup 2] [--trained]

One JSON line per (configuration, level): GB/s of uncompressed input over whole compress calls (device events around `steps` calls, the
levels taken in turn `--rounds` times so that a drift of the machine shows in all of them), the compression ratio, and the per-kernel
split of one profiled call (kmp_batch_last_kernel_ms: the parse and the entropy launch; null where the library records none for this
path).  Runs with any build of the package on PYTHONPATH; a level the build refuses with a dictionary is reported as such."""
import argparse
import ctypes
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
if not any(os.path.exists(os.path.join(p, "kompressor_amd")) for p in sys.path if p):
    sys.path.insert(0, ROOT)

import torch                                        # noqa: E402
from kompressor_amd import corpus                   # noqa: E402
from kompressor_amd.batch import ZstdBatch          # noqa: E402

CONFIGS = {"records": (262144, 8192, 64), "slices": (65536, 65536, 16)}


def dictionary_of(kib, slice_bytes, trained):
    d = corpus.make(123456789, 1, kib * 1024, mix=ord("T")).tobytes()
    if not trained:
        return d
    sys.path.insert(0, os.path.join(ROOT, "oracle"))
    from libzstd_ref import find_libzstd_157
    zl = find_libzstd_157()
    if zl is None:
        sys.exit("--trained: no libzstd 1.5.7 on this machine to train the dictionary with")
    ns = 2000
    samples = corpus.make(777000, ns, min(slice_bytes, 16384)).tobytes()
    sizes = (ctypes.c_size_t * ns)(*([len(samples) // ns] * ns))
    out = ctypes.create_string_buffer(kib * 1024)
    zl.ZDICT_trainFromBuffer.restype = ctypes.c_size_t
    zl.ZDICT_trainFromBuffer.argtypes = [ctypes.c_void_p, ctypes.c_size_t, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_uint]
    dn = zl.ZDICT_trainFromBuffer(out, kib * 1024, samples, sizes, ns)
    if zl.ZSTD_isError(dn):
        sys.exit("--trained: ZDICT_trainFromBuffer failed")
    return out.raw[:dn]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--config", default="both", choices=("records", "slices", "both"))
    ap.add_argument("--levels", default="3,1,-1")
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--rounds", type=int, default=2)
    ap.add_argument("--scale", type=int, default=1, help="divide the number of slices by this (rehearsals)")
    ap.add_argument("--trained", action="store_true")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("dict_levels_rates.py measures on a GPU: none here")
    levels = [int(x) for x in args.levels.split(",")]
    for cfg in (("records", "slices") if args.config == "both" else (args.config,)):
        n, S, kib = CONFIGS[cfg]
        n //= args.scale
        d = dictionary_of(kib, S, args.trained)
        src = torch.from_numpy(corpus.make(0, n, S)).cuda()
        in_off = torch.arange(n, dtype=torch.int64, device="cuda") * S
        in_len = torch.full((n,), S, dtype=torch.int32, device="cuda")
        b = ZstdBatch(max_slices=n, max_slice_bytes=S)
        dst = torch.empty(n * b.out_stride + 64, dtype=torch.uint8, device="cuda")
        out_off = torch.arange(n, dtype=torch.int64, device="cuda") * b.out_stride
        out_len = torch.zeros(n, dtype=torch.int32, device="cuda")
        rates = {lv: [] for lv in levels}; ratio = {}; refused = {}

        def call(lv):
            kw = {} if lv == 3 else {"level": lv}                  # (level 3: the call every build has)
            b.compress(src, in_off, in_len, dst, out_off, out_len, dictionary=d, **kw)

        for rnd in range(args.rounds):
            for lv in levels:
                if lv in refused:
                    continue
                try:
                    for _ in range(args.warmup):
                        call(lv)
                except ValueError as e:
                    refused[lv] = str(e)
                    continue
                torch.cuda.synchronize()
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                for _ in range(args.steps):
                    call(lv)
                e1.record()
                torch.cuda.synchronize()
                rc, bits = b.status()
                assert rc == 0 and bits == 0, (lv, rc, bits)
                rates[lv].append(n * S / (e0.elapsed_time(e1) * 1e-3 / args.steps) / 1e9)
                ratio[lv] = n * S / float(out_len.sum().item())
        for lv in levels:
            kms = None
            if lv not in refused:
                b.set_profiling(True)
                call(lv)
                torch.cuda.synchronize()
                try:
                    kms = {"match": round(b.last_kernel_ms(0), 3), "entropy": round(b.last_kernel_ms(1), 3)}
                except RuntimeError:
                    kms = None
                b.set_profiling(False)
            print(json.dumps({"config": f"{n} x {S} B, {'trained' if args.trained else 'raw'} dictionary of {len(d)} B", "level": lv,
                              "GBps": [round(r, 2) for r in rates[lv]], "ratio": round(ratio[lv], 4) if lv in ratio else None,
                              "kernels_ms": kms, "refused": refused.get(lv), "steps": args.steps, "warmup": args.warmup}), flush=True)
        b.close()
        del src, dst


if __name__ == "__main__":
    main()
