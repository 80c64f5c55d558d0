"""Cost of parameter groups in the fused AdamW step: the kernels on their own.

adamw_step (the yardstick) against adamw_step_grouped with one segment and
with the trainer's real table (no_decay_1d and layer_decay on), for bf16 and
f32 gradients, on a copy of the --model trainer's flat buffers.  The cases
take turns in one process: --repeats rounds, in each round every case times
--iters back-to-back launches between two device events.  A line is the
median round with its min..max spread; `vs_adamw_step` is the ratio of the
medians.  The step moves 48 B/elem (46 with bf16 gradients) and the lookup
touches only LDS.

    python scripts/bench_adamw_groups.py            # mltc-base
"""
import sys, os; sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import argparse
import json
import statistics

import torch

from tosem2021_amd import ops
from tosem2021_amd.train import TrainConfig, Trainer, param_group_table


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
    ap.add_argument("--layer-decay", type=float, default=0.8)
    ap.add_argument("--repeats", type=int, default=9)
    ap.add_argument("--iters", type=int, default=50)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("bench_adamw_groups.py needs a GPU")
    ops.hip_ops()
    dev = torch.device("cuda", 0)

    torch.manual_seed(1234)
    tr = Trainer(TrainConfig(model=args.model, warmup_steps=0), device=dev)
    f = tr.flat
    n = f.padded
    real = param_group_table(tr.model, tr.model.cfg.n_layers, n,
                             weight_decay=tr.cfg.weight_decay,
                             no_decay_1d=True, layer_decay=args.layer_decay)
    tables = {"1seg": ops.segment_table([n], [1.0], [tr.cfg.weight_decay], n,
                                        device=dev),
              f"{len(real[0])}seg": ops.segment_table(*real, n, device=dev)}
    p, m, v, mst = (t.clone() for t in (f.flat, f.m, f.v, f.master))
    g16 = torch.randn(n, device=dev).mul_(1e-2).to(torch.bfloat16)
    grads = {"bf16": g16, "f32": g16.float()}
    del tr
    hp = dict(lr=1e-4, step=10)

    cases = {}
    for gname, g in grads.items():
        # g + m, v, master read; m, v, master + p written
        nbytes = n * (g.element_size() + 12 + 12 + 2)
        cases[f"adamw_step/{gname}"] = (
            lambda g=g: ops.adamw_step(p, g, m, v, mst, **hp), nbytes)
        for tname, table in tables.items():
            cases[f"adamw_step_grouped/{tname}/{gname}"] = (
                lambda g=g, table=table: ops.adamw_step_grouped(
                    p, g, m, v, mst, *table, **hp), nbytes)

    for fn, _ in cases.values():          # warm up every case
        for _ in range(5):
            fn()
    torch.cuda.synchronize()
    times = {name: [] for name in cases}
    for _ in range(args.repeats):
        for name, (fn, _) in cases.items():   # the cases take turns
            times[name].append(timed(fn, args.iters))

    res = {"model": args.model, "flat_elems": n,
           "segments": {k: int(t[0].numel()) for k, t in tables.items()},
           "repeats": args.repeats, "iters": args.iters}
    for name, (_, nbytes) in cases.items():
        med = statistics.median(times[name])
        res[name] = {"median_us": round(med * 1e6, 2),
                     "min_us": round(min(times[name]) * 1e6, 2),
                     "max_us": round(max(times[name]) * 1e6, 2),
                     "GBps": round(nbytes / med / 1e9, 1)}
    for name in cases:
        if name.startswith("adamw_step_grouped/"):
            base = "adamw_step/" + name.rsplit("/", 1)[1]
            res[name]["vs_adamw_step"] = round(
                res[name]["median_us"] / res[base]["median_us"], 4)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
