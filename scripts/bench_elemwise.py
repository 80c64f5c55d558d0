"""Microbench the memory-bound kernels (LN, bias+GeLU).

Defaults are the bench.py shapes; --rows/--d/--dff select others, e.g. the
mltc-large LayerNorm backward:  --rows 32768 --d 2048 --only ln_bwd

Each line is the median of --repeats timed batches of --iters launches, with
the min..max spread of those batches, and the achieved GB/s of the median
against the ~8 TB/s HBM3E roofline.
"""
import sys, os; sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import argparse
import statistics
import time

import torch

from tosem2021_amd import ops


def timeit(fn, iters, repeats):
    for _ in range(5):
        fn()
    times = []
    for _ in range(repeats):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(iters):
            fn()
        torch.cuda.synchronize()
        times.append((time.perf_counter() - t0) / iters)
    return statistics.median(times), min(times), max(times)


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--rows", type=int, default=128 * 512,
                    help="rows N of every operand (default: bench.py's)")
    ap.add_argument("--d", type=int, default=1024, help="LayerNorm width")
    ap.add_argument("--dff", type=int, default=4096, help="bias+GeLU width")
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--only", default="",
                    help="comma-separated line names to run (default: all)")
    args = ap.parse_args()
    only = set(filter(None, args.only.split(",")))
    ext = ops.hip_ops()
    N, D, Dff = args.rows, args.d, args.dff
    print(f"rows {N}  d {D}  dff {Dff}  iters {args.iters}  "
          f"repeats {args.repeats}")

    def report(name, fn, nbytes):
        if only and name not in only:
            return
        med, lo, hi = timeit(fn, args.iters, args.repeats)
        print(f"{name:16s} {med*1e6:7.1f} us  ({lo*1e6:.1f}..{hi*1e6:.1f})  "
              f"{nbytes / med / 1e9:6.0f} GB/s")

    x = torch.randn(N, D, device="cuda").to(torch.bfloat16)
    res = torch.randn_like(x)
    g = torch.randn(D, device="cuda").to(torch.bfloat16)
    b = torch.randn(D, device="cuda").to(torch.bfloat16)
    dy = torch.randn_like(x)

    report("ln_fwd", lambda: ext.layernorm_fwd(x, None, g, b, 1e-5),
           N * D * 2 * 2)
    report("ln_fwd+res", lambda: ext.layernorm_fwd(x, res, g, b, 1e-5),
           N * D * 2 * 4)
    out = ext.layernorm_fwd(x, None, g, b, 1e-5)
    mean, rstd = out[-2], out[-1]
    report("ln_bwd", lambda: ext.layernorm_bwd(dy, x, g, mean, rstd, None),
           N * D * 2 * 3)
    report("ln_bwd+dsx", lambda: ext.layernorm_bwd(dy, x, g, mean, rstd, res),
           N * D * 2 * 4)
    # the training path: bf16 column outputs plus the folded bias gradient
    report("ln_bwd+dsx+dres",
           lambda: ext.layernorm_bwd(dy, x, g, mean, rstd, res, True, True),
           N * D * 2 * 4)
    del x, res, dy, out

    xf = torch.randn(N, Dff, device="cuda").to(torch.bfloat16)
    bf = torch.randn(Dff, device="cuda").to(torch.bfloat16)
    dyf = torch.randn_like(xf)
    report("bias_gelu_fwd", lambda: ext.bias_gelu_fwd(xf, bf),
           N * Dff * 2 * 2)
    report("bias_gelu_bwd", lambda: ext.bias_gelu_bwd(dyf, xf, bf),
           N * Dff * 2 * 3)


if __name__ == "__main__":
    main()
