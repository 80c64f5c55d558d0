"""Cost of the weight EMA in the fused AdamW step: the kernels on their own.

Three cases per gradient dtype, on a copy of the --model trainer's flat
buffers: adamw_step (the yardstick), adamw_step with ema= (the fused form),
and the non-fused alternative, adamw_step followed by the same recurrence as
torch ops on ema (ema.mul_(d), then ema.add_(master * (1 - d))).  The cases
take turns in one process: --repeats rounds, in each round every case times
--iters back-to-back launches between two device events.  A line is the
median round with its min..max spread; `vs_adamw_step` is the ratio of the
medians, and `fused_vs_unfused` the fused form over the non-fused one.  The
plain step moves 30 B/elem (28 with bf16 gradients), the fused form 8 more,
the torch ops 24 more.

    python scripts/bench_adamw_ema.py            # mltc-base
"""
import sys, os; sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import argparse
import json
import statistics

import torch

from tosem2021_amd import ops
from tosem2021_amd.train import TrainConfig, Trainer


def timed(fn, iters):
    a = torch.cuda.Event(enable_timing=True)
    b = torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(iters):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) * 1e-3 / iters


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--model", default="mltc-base")
    ap.add_argument("--ema-decay", type=float, default=0.999)
    ap.add_argument("--repeats", type=int, default=9)
    ap.add_argument("--iters", type=int, default=50)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("bench_adamw_ema.py needs a GPU")
    ops.hip_ops()
    dev = torch.device("cuda", 0)

    torch.manual_seed(1234)
    tr = Trainer(TrainConfig(model=args.model, warmup_steps=0), device=dev)
    f = tr.flat
    n = f.padded
    p, m, v, mst = (t.clone() for t in (f.flat, f.m, f.v, f.master))
    ema = mst.clone()
    g16 = torch.randn(n, device=dev).mul_(1e-2).to(torch.bfloat16)
    grads = {"bf16": g16, "f32": g16.float()}
    del tr
    hp = dict(lr=1e-4, step=10)
    d = args.ema_decay

    def unfused(g):
        ops.adamw_step(p, g, m, v, mst, **hp)
        ema.mul_(d)
        ema.add_(mst * (1.0 - d))

    cases = {}
    for gname, g in grads.items():
        # g + m, v, master read; m, v, master + p written
        nbytes = n * (g.element_size() + 12 + 12 + 2)
        cases[f"adamw_step/{gname}"] = (
            lambda g=g: ops.adamw_step(p, g, m, v, mst, **hp), nbytes)
        cases[f"adamw_step+ema/{gname}"] = (
            lambda g=g: ops.adamw_step(p, g, m, v, mst, ema=ema, ema_decay=d,
                                       **hp), nbytes + 8 * n)
        # + ema read and written, master read, the product written and read
        cases[f"adamw_step,torch_ema/{gname}"] = (
            lambda g=g: unfused(g), nbytes + 24 * n)

    for fn, _ in cases.values():          # warm up every case
        for _ in range(5):
            fn()
    torch.cuda.synchronize()
    times = {name: [] for name in cases}
    for _ in range(args.repeats):
        for name, (fn, _) in cases.items():   # the cases take turns
            times[name].append(timed(fn, args.iters))

    res = {"model": args.model, "flat_elems": n, "ema_decay": d,
           "repeats": args.repeats, "iters": args.iters}
    for name, (_, nbytes) in cases.items():
        med = statistics.median(times[name])
        res[name] = {"median_us": round(med * 1e6, 2),
                     "min_us": round(min(times[name]) * 1e6, 2),
                     "max_us": round(max(times[name]) * 1e6, 2),
                     "GBps": round(nbytes / med / 1e9, 1)}
    for gname in grads:
        base = res[f"adamw_step/{gname}"]["median_us"]
        fused = res[f"adamw_step+ema/{gname}"]
        loose = res[f"adamw_step,torch_ema/{gname}"]
        fused["vs_adamw_step"] = round(fused["median_us"] / base, 4)
        loose["vs_adamw_step"] = round(loose["median_us"] / base, 4)
        fused["fused_vs_unfused"] = round(
            fused["median_us"] / loose["median_us"], 4)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
