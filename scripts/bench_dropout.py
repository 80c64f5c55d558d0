"""Cost of residual dropout: unfused (F.dropout on both sublayer outputs of
every block) against fused into the add+LayerNorm kernels.

Three same-seed trainers (dropout 0; --dropout unfused; --dropout fused) take
turns on one batch, --repeats windows of --steps steps each, every window
bracketed by a device synchronise; a step line is the median window with its
min..max spread.  Peak memory is torch.cuda.max_memory_allocated over one
step of each arm with the other arms' gradients and activations released.

    python scripts/bench_dropout.py         # mltc-base, batch 128, L 512
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
from tosem2021_amd.train import TrainConfig, Trainer


def window(trainer, batch, steps):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(steps):
        trainer.step(*batch)
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / steps


def peak_step_bytes(trainer, batch):
    """Peak allocation over one step, above what is resident before it."""
    torch.cuda.synchronize()
    base = torch.cuda.memory_allocated()
    torch.cuda.reset_peak_memory_stats()
    trainer.step(*batch)
    torch.cuda.synchronize()
    return torch.cuda.max_memory_allocated() - base


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--model", default="mltc-base")
    ap.add_argument("--batch", type=int, default=128)
    ap.add_argument("--seq", type=int, default=512)
    ap.add_argument("--dropout", type=float, default=0.1)
    ap.add_argument("--steps", type=int, default=10, help="steps per window")
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--repeats", type=int, default=5)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("bench_dropout.py needs a GPU")
    ops.hip_ops()
    dev = torch.device("cuda", 0)
    base = dataclasses.replace(CONFIGS[args.model],
                               max_seq=max(args.seq, CONFIGS[args.model].max_seq))
    batch = synthetic_batch(base, args.batch, args.seq, device=dev, seed=1)

    arms = {"none": dict(dropout=0.0),
            "unfused": dict(dropout=args.dropout),
            "fused": dict(dropout=args.dropout, fused_dropout=True)}
    trainers = {}
    for name, kw in arms.items():
        torch.manual_seed(1234)
        trainers[name] = Trainer(
            TrainConfig(model=args.model, warmup_steps=0), device=dev,
            model_cfg=dataclasses.replace(base, **kw))
        for _ in range(args.warmup):
            trainers[name].step(*batch)
    step_s = {name: [] for name in arms}
    for _ in range(args.repeats):
        for name in arms:                     # alternate the arms
            step_s[name].append(window(trainers[name], batch, args.steps))
    peak = {name: peak_step_bytes(trainers[name], batch) for name in arms}

    def line(xs):
        return {"median_ms": round(statistics.median(xs) * 1e3, 3),
                "min_ms": round(min(xs) * 1e3, 3),
                "max_ms": round(max(xs) * 1e3, 3)}

    res = {"model": args.model, "batch": args.batch, "seq": args.seq,
           "dropout": args.dropout, "steps_per_window": args.steps,
           "windows": args.repeats}
    for name in arms:
        res[f"step_{name}"] = line(step_s[name])
        res[f"peak_step_MiB_{name}"] = round(peak[name] / 2 ** 20, 1)
    med = {n: statistics.median(step_s[n]) for n in arms}
    spread = max(max(step_s[n]) - min(step_s[n]) for n in ("unfused", "fused"))
    res["fused_minus_unfused_ms"] = round((med["fused"] - med["unfused"]) * 1e3,
                                          3)
    res["spread_ms"] = round(spread * 1e3, 3)
    res["fused_faster_than_spread"] = bool(
        med["unfused"] - med["fused"] > spread)
    res["peak_saved_MiB"] = round((peak["unfused"] - peak["fused"]) / 2 ** 20,
                                  1)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
