"""Token-loss cost of masked-LM pretraining: ops.fused_cross_entropy
(csrc/cross_entropy.hip) against the eager composition
F.cross_entropy(logits.float(), t), forward + backward on the same seeded
bf16 logits [N, 32768].

    N = 9,984   bench batch 128 x L 512 x 0.15 selected, padded to 256
    N = 1,280   `train` default batch 32 x seq 256 x 0.15, padded to 256

The two variants take turns in one process, --repeats windows of --iters
calls each between two device events; the line is the median window with
its min..max spread.  Peak memory is torch.cuda.max_memory_allocated over a
call, less what the inputs hold.  Bytes come from shapes:

    fused   6 B / logit   forward reads bf16; backward reads bf16, writes bf16
    eager  36 B / logit   .float() 2 + 4; log_softmax 4 + 4; nll backward
                          writes an f32 [N, V] 4; log_softmax backward
                          4 + 4 + 4; the cast's backward 4 + 2

Kernel times come from a separate profiler run, no counters:

    rocprofv3 --kernel-trace --stats -d DIR -- \\
        python scripts/bench_mlm_loss.py --n 9984 --repeats 1 --iters 20
"""
import sys, os; sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import argparse
import json
import statistics

import torch
import torch.nn.functional as F

from tosem2021_amd import ops

FUSED_BYTES, EAGER_BYTES = 6, 36


def fused(x, t):
    ops.fused_cross_entropy(x, t).backward()


def eager(x, t):
    F.cross_entropy(x.float(), t, ignore_index=-100).backward()


def window(fn, x, t, iters):
    a = torch.cuda.Event(enable_timing=True)
    b = torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(iters):
        x.grad = None
        fn(x, t)
    b.record()
    b.synchronize()
    return a.elapsed_time(b) * 1e-3 / iters


def peak_bytes(fn, x, t):
    x.grad = None
    torch.cuda.synchronize()
    base = torch.cuda.memory_allocated()
    torch.cuda.reset_peak_memory_stats()
    fn(x, t)
    torch.cuda.synchronize()
    return torch.cuda.max_memory_allocated() - base


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--n", type=int, nargs="*", default=[9984, 1280])
    ap.add_argument("--vocab", type=int, default=32768)
    ap.add_argument("--ignored", type=float, default=0.02,
                    help="share of rows with target -100 (the padding rows)")
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--repeats", type=int, default=7)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("bench_mlm_loss.py needs a GPU")
    ops.hip_ops()
    variants = (("fused", fused, FUSED_BYTES), ("eager", eager, EAGER_BYTES))
    for n in args.n:
        g = torch.Generator().manual_seed(n)
        x = (torch.randn(n, args.vocab, generator=g) * 2).to(
            torch.bfloat16).cuda().requires_grad_()
        t = torch.randint(0, args.vocab, (n,), generator=g)
        t[torch.rand(n, generator=g) < args.ignored] = -100
        t = t.cuda()
        res = {"N": n, "V": args.vocab, "logits": n * args.vocab,
               "byte_ratio": EAGER_BYTES / FUSED_BYTES}
        grads = {}
        for name, fn, _ in variants:
            for _ in range(args.warmup):
                x.grad = None
                fn(x, t)
            grads[name] = x.grad.float()
        # same gradient up to the bf16 rounding of the f32 path
        res["grad_max_abs_diff"] = float(
            (grads["fused"] - grads["eager"]).abs().max())
        del grads
        times = {name: [] for name, _, _ in variants}
        for _ in range(args.repeats):
            for name, fn, _ in variants:        # alternate the two arms
                times[name].append(window(fn, x, t, args.iters))
        for name, fn, per_logit in variants:
            med = statistics.median(times[name])
            res[name] = {
                "median_us": round(med * 1e6, 1),
                "min_us": round(min(times[name]) * 1e6, 1),
                "max_us": round(max(times[name]) * 1e6, 1),
                "peak_MiB": round(peak_bytes(fn, x, t) / 2 ** 20, 1),
                "bytes_from_shapes": per_logit * n * args.vocab,
                "GBps_from_shapes": round(
                    per_logit * n * args.vocab / med / 1e9, 1)}
        res["time_ratio"] = round(res["eager"]["median_us"] /
                                  res["fused"]["median_us"], 2)
        print(json.dumps(res))


if __name__ == "__main__":
    main()
