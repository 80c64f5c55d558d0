"""Cost of gradient-norm clipping: whole step and the kernels on their own.

Two same-seed trainers (max_grad_norm 0 and --max-norm) take turns on one
batch, --repeats windows of --steps steps each, every window bracketed by a
device synchronise; the step line is the median window with its min..max
spread.  The kernel lines time --iters back-to-back launches between two
device events on a copy of the trainer's own flat buffers, so the AdamW
figure is the reference for the norm pass in the same run.

    python scripts/bench_clip.py            # mltc-base, batch 128, L 256
"""
import sys, os; sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import argparse
import json
import statistics
import time

import torch

from tosem2021_amd import ops
from tosem2021_amd.data.synthetic import synthetic_batch
from tosem2021_amd.models.classifier import CONFIGS
from tosem2021_amd.train import TrainConfig, Trainer


def window(trainer, batch, steps):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(steps):
        trainer.step(*batch)
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / steps


def event_time(fn, iters, repeats):
    """Median / min / max seconds per launch over `repeats` event pairs."""
    for _ in range(5):
        fn()
    times = []
    for _ in range(repeats):
        a = torch.cuda.Event(enable_timing=True)
        b = torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(iters):
            fn()
        b.record()
        b.synchronize()
        times.append(a.elapsed_time(b) * 1e-3 / iters)
    return statistics.median(times), min(times), max(times)


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--model", default="mltc-base")
    ap.add_argument("--batch", type=int, default=128)
    ap.add_argument("--seq", type=int, default=256)
    ap.add_argument("--max-norm", type=float, default=1.0)
    ap.add_argument("--steps", type=int, default=10, help="steps per window")
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--iters", type=int, default=50)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("bench_clip.py needs a GPU")
    ops.hip_ops()
    dev = torch.device("cuda", 0)
    cfg = CONFIGS[args.model]
    batch = synthetic_batch(cfg, args.batch, args.seq, device=dev, seed=1)

    trainers = {}
    for name, mgn in (("off", 0.0), ("on", args.max_norm)):
        torch.manual_seed(1234)
        trainers[name] = Trainer(
            TrainConfig(model=args.model, warmup_steps=0, max_grad_norm=mgn),
            device=dev)
        for _ in range(args.warmup):
            trainers[name].step(*batch)
    step_s = {"off": [], "on": []}
    for _ in range(args.repeats):
        for name in ("off", "on"):            # alternate the two arms
            step_s[name].append(window(trainers[name], batch, args.steps))

    def line(xs):
        return {"median_ms": round(statistics.median(xs) * 1e3, 3),
                "min_ms": round(min(xs) * 1e3, 3),
                "max_ms": round(max(xs) * 1e3, 3)}

    res = {"model": args.model, "batch": args.batch, "seq": args.seq,
           "max_norm": args.max_norm,
           "step_off": line(step_s["off"]), "step_on": line(step_s["on"]),
           "last_grad_norm": trainers["on"].metrics["grad_norm"],
           "skipped_steps": trainers["on"].skipped_steps}

    # the kernels alone, on copies of the trainer's buffers
    f = trainers["on"].flat
    n = f.padded
    p, g, m, v, mst = (t.clone() for t in
                       (f.flat, f.grad_flat, f.m, f.v, f.master))
    del trainers
    hp = dict(lr=1e-4, step=10)
    state = ops.grad_clip_state(g, max_norm=args.max_norm)
    kernels = {
        # one read of the gradients
        "grad_clip_state": (
            lambda: ops.grad_clip_state(g, max_norm=args.max_norm),
            n * g.element_size()),
        # g + m, v, master read; m, v, master + p written
        "adamw_step": (
            lambda: ops.adamw_step(p, g, m, v, mst, **hp),
            n * (g.element_size() + 12 + 12 + 2)),
        "adamw_step_clipped": (
            lambda: ops.adamw_step_clipped(p, g, m, v, mst, clip_state=state,
                                           **hp),
            n * (g.element_size() + 12 + 12 + 2)),
    }
    res["flat_elems"] = n
    for name, (fn, nbytes) in kernels.items():
        med, lo, hi = event_time(fn, args.iters, args.repeats)
        res[name] = {"median_us": round(med * 1e6, 2),
                     "min_us": round(lo * 1e6, 2),
                     "max_us": round(hi * 1e6, 2),
                     "GBps": round(nbytes / med / 1e9, 1)}
    res["norm_over_adamw"] = round(
        res["grad_clip_state"]["median_us"] / res["adamw_step"]["median_us"],
        4)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
