"""Cost of dropout on the attention probabilities inside the flash kernels.

Kernels: flash_fwd, flash_bwd_fused and flash_dq_recompute on one
[B, H, L, 64] problem, each timed with device events around --iters
back-to-back launches, p = 0 (the instantiations without the mask) and
p = --dropout taking turns for --repeats windows; a line is the median window
per launch with its min..max spread.

Step: two same-seed trainers (attn_dropout 0 and --dropout) take turns on one
batch, --repeats windows of --steps steps each, every window bracketed by a
device synchronise.

    python scripts/bench_attn_dropout.py    # B 128, H 16, L 512; mltc-base
"""
import sys, os; sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import argparse
import dataclasses
import json
import statistics
import time

import torch

from tosem2021_amd import ops
from tosem2021_amd.data.synthetic import synthetic_batch
from tosem2021_amd.models.classifier import CONFIGS
from tosem2021_amd.ops import reference
from tosem2021_amd.train import TrainConfig, Trainer


def event_window(fn, iters):
    """Seconds per launch of fn over iters launches, by device events."""
    start = torch.cuda.Event(enable_timing=True)
    stop = torch.cuda.Event(enable_timing=True)
    start.record()
    for _ in range(iters):
        fn()
    stop.record()
    stop.synchronize()
    return start.elapsed_time(stop) * 1e-3 / iters


def step_window(trainer, batch, steps):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(steps):
        trainer.step(*batch)
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / steps


def line(xs, unit):
    return {f"median_{unit}": round(statistics.median(xs), 3),
            f"min_{unit}": round(min(xs), 3), f"max_{unit}": round(max(xs), 3)}


def bench_kernels(args, dev):
    ext = ops.hip_ops()
    B, H, L = args.batch, args.heads, args.seq
    g = torch.Generator(device=dev).manual_seed(1)
    q, k, v, do = (torch.randn(B, H, L, 64, generator=g, device=dev)
                   .to(torch.bfloat16) for _ in range(4))
    scale = 0.125
    thr, _ = reference.attn_dropout_threshold(args.dropout)
    arms = {"p0": {}, "drop": dict(drop_seed=1234, drop_call=1,
                                   drop_site=reference.ATTN_DROPOUT_SITE0,
                                   drop_thr=thr)}
    fns = {}
    for arm, kw in arms.items():
        o, lse = ext.flash_fwd(q, k, v, None, scale, **kw)
        ddot, dead = ext.fa_dot_flags(do, o)
        fns[arm] = {
            "flash_fwd": lambda kw=kw: ext.flash_fwd(q, k, v, None, scale,
                                                     **kw),
            "flash_bwd_fused": lambda kw=kw, lse=lse, ddot=ddot, dead=dead:
                ext.flash_bwd_fused(q, k, v, do, None, lse, ddot, scale,
                                    dead=dead, **kw),
            "flash_dq_recompute": lambda kw=kw, lse=lse, ddot=ddot, dead=dead:
                ext.flash_dq_recompute(q, k, v, do, None, lse, ddot, scale,
                                       dead=dead, **kw),
        }
    res = {}
    for name in fns["p0"]:
        us = {arm: [] for arm in arms}
        for arm in arms:
            event_window(fns[arm][name], args.warmup)
        for _ in range(args.repeats):
            for arm in arms:                  # alternate the arms
                us[arm].append(event_window(fns[arm][name], args.iters) * 1e6)
        res[name] = {arm: line(us[arm], "us") for arm in arms}
        res[name]["drop_over_p0"] = round(
            statistics.median(us["drop"]) / statistics.median(us["p0"]), 3)
    return res


def bench_step(args, dev):
    base = dataclasses.replace(
        CONFIGS[args.model],
        max_seq=max(args.seq, CONFIGS[args.model].max_seq))
    batch = synthetic_batch(base, args.batch, args.seq, device=dev, seed=1)
    arms = {"none": dict(attn_dropout=0.0),
            "attn_dropout": dict(attn_dropout=args.dropout)}
    trainers = {}
    for name, kw in arms.items():
        torch.manual_seed(1234)
        trainers[name] = Trainer(
            TrainConfig(model=args.model, warmup_steps=0), device=dev,
            model_cfg=dataclasses.replace(base, **kw))
        for _ in range(args.step_warmup):
            trainers[name].step(*batch)
    ms = {name: [] for name in arms}
    for _ in range(args.repeats):
        for name in arms:                     # alternate the arms
            ms[name].append(step_window(trainers[name], batch, args.steps)
                            * 1e3)
    res = {f"step_{name}": line(ms[name], "ms") for name in arms}
    res["attn_dropout_minus_none_ms"] = round(
        statistics.median(ms["attn_dropout"]) - statistics.median(ms["none"]),
        3)
    res["spread_ms"] = round(max(max(x) - min(x) for x in ms.values()), 3)
    return res


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--model", default="mltc-base")
    ap.add_argument("--batch", type=int, default=128)
    ap.add_argument("--heads", type=int, default=16)
    ap.add_argument("--seq", type=int, default=512)
    ap.add_argument("--dropout", type=float, default=0.1)
    ap.add_argument("--iters", type=int, default=50,
                    help="kernel launches per window")
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--steps", type=int, default=10, help="steps per window")
    ap.add_argument("--step-warmup", type=int, default=5)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--skip-step", action="store_true",
                    help="kernels only")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("bench_attn_dropout.py needs a GPU")
    dev = torch.device("cuda", 0)
    res = {"batch": args.batch, "heads": args.heads, "seq": args.seq,
           "dropout": args.dropout, "launches_per_window": args.iters,
           "windows": args.repeats, "kernels": bench_kernels(args, dev)}
    if not args.skip_step:
        res.update(model=args.model, steps_per_window=args.steps,
                   **bench_step(args, dev))
    print(json.dumps(res))


if __name__ == "__main__":
    main()
