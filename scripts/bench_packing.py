"""Padded vs packed throughput on real text.

Takes the first N (default 8,192) rows of artifacts/taxonomy_mined.csv with
the text apply_classifier feeds the model ("Labels | Component"), and runs
mltc-base at max_len 256 two ways:

  padded  batches of 64, each example on its own row padded to the batch
          maximum rounded up to 64 (CodeTokenizer.encode_batch, today's path)
  packed  256 examples per pack, first-fit-decreasing into 256-token rows
          (CodeTokenizer.encode_packed, segment-aware attention and pooling)

and times inference (no_grad forward) and training (Trainer.step) over the
same examples.  Batches are tokenized and moved to the GPU before the timed
window; the window has a warm-up pass in front and a device synchronise on
both sides.  Prints the token-position counts it used and one JSON line.
Labels are random: the rates do not depend on them.
"""
import sys, os; sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import argparse
import json
import time

import torch

from tosem2021_amd.analyze.taxonomy import load_taxonomy
from tosem2021_amd.models.classifier import CONFIGS, MLTCConfig
from tosem2021_amd.models.tokenizer import CodeTokenizer
from tosem2021_amd.train import TrainConfig, Trainer


def _labels(cfg, n, device, gen):
    return {
        "strategy": (torch.rand(n, cfg.heads["strategy"], generator=gen)
                     > 0.8).float().to(device),
        "property": (torch.rand(n, cfg.heads["property"], generator=gen)
                     > 0.8).float().to(device),
        "stage": torch.randint(0, cfg.heads["stage"], (n,),
                               generator=gen).to(device),
        "method": torch.randint(0, cfg.heads["method"], (n,),
                                generator=gen).to(device),
    }


def _timed(fn, batches, warmup):
    """Seconds for one pass of fn over `batches`, after `warmup` batches."""
    for b in batches[:warmup]:
        fn(b)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for b in batches:
        fn(b)
    torch.cuda.synchronize()
    return time.perf_counter() - t0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--taxonomy", default=os.path.join(
        os.path.dirname(os.path.dirname(os.path.abspath(__file__))),
        "artifacts", "taxonomy_mined.csv"))
    ap.add_argument("--model", default="mltc-base")
    ap.add_argument("--limit", type=int, default=8192)
    ap.add_argument("--max-len", type=int, default=256)
    ap.add_argument("--row-len", type=int, default=256)
    ap.add_argument("--batch", type=int, default=64, help="padded batch")
    ap.add_argument("--pack", type=int, default=256, help="examples per pack")
    ap.add_argument("--warmup", type=int, default=4, help="warm-up batches")
    ap.add_argument("--skip-train", action="store_true")
    args = ap.parse_args()

    df = load_taxonomy(args.taxonomy).iloc[:args.limit]
    texts = (df["Labels"].astype(str) + " | " +
             df["Component"].astype(str)).tolist()
    n = len(texts)
    dev = torch.device("cuda")
    base = CONFIGS[args.model]
    cfg = MLTCConfig(**{**base.__dict__, "max_seq": args.max_len})
    tok = CodeTokenizer(cfg.vocab_size)
    gen = torch.Generator().manual_seed(0)

    padded, packed = [], []
    real = 0
    for lo in range(0, n, args.batch):
        toks, mask = tok.encode_batch(texts[lo:lo + args.batch], args.max_len,
                                      device=dev)
        real += int(mask.sum())
        padded.append((toks, mask, _labels(cfg, toks.shape[0], dev, gen)))
    for lo in range(0, n, args.pack):
        pb = tok.encode_packed(texts[lo:lo + args.pack], args.max_len,
                               args.row_len, device=dev)
        packed.append((pb, None, _labels(cfg, pb.n_segments, dev, gen)))
    pos_padded = sum(b[0].numel() for b in padded)
    pos_packed = sum(b[0].n_positions for b in packed)
    print(f"examples {n}  real tokens {real}")
    print(f"padded: {len(padded)} batches, {pos_padded} token positions "
          f"(fill {real / pos_padded:.3f})")
    print(f"packed: {len(packed)} packs, {pos_packed} token positions "
          f"(fill {real / pos_packed:.3f}); "
          f"{pos_padded / pos_packed:.2f}x fewer positions")

    torch.manual_seed(0)
    trainer = Trainer(TrainConfig(model=args.model, warmup_steps=0),
                      device=dev, model_cfg=cfg)
    model = trainer.model

    def infer(b):
        if b[1] is None:
            model(b[0].tokens, packing=b[0])
        else:
            model(b[0], b[1])

    res = {"examples": n, "real_tokens": real,
           "positions_padded": pos_padded, "positions_packed": pos_packed}
    model.eval()
    with torch.no_grad():
        # the packed pass has 4x fewer, 4x larger batches: same warm-up work
        res["infer_padded_ex_per_s"] = n / _timed(infer, padded, args.warmup)
        res["infer_packed_ex_per_s"] = n / _timed(infer, packed, args.warmup)
    model.train()
    res["infer_speedup"] = (res["infer_packed_ex_per_s"] /
                            res["infer_padded_ex_per_s"])
    if not args.skip_train:
        step = lambda b: trainer.step(*b)  # noqa: E731
        res["train_padded_ex_per_s"] = n / _timed(step, padded, args.warmup)
        res["train_packed_ex_per_s"] = n / _timed(step, packed, args.warmup)
        res["train_speedup"] = (res["train_packed_ex_per_s"] /
                                res["train_padded_ex_per_s"])
    print(json.dumps({"metric": "packing_speedup", "dtype": "bf16",
                      "data": os.path.basename(args.taxonomy),
                      "config": {"model": args.model, "max_len": args.max_len,
                                 "row_len": args.row_len, "batch": args.batch,
                                 "pack": args.pack},
                      **{k: (round(v, 3) if isinstance(v, float) else v)
                         for k, v in res.items()}}))


if __name__ == "__main__":
    main()
