"""Compare two `bench.py --dump-outputs` directories across the bias fold.

    python bench.py --gpus 1 --steps 1 --warmup 0 --dump-outputs A
    TOSEM_FOLD_BIAS_GRAD=1 \
    python bench.py --gpus 1 --steps 1 --warmup 0 --dump-outputs B
    python scripts/compare_dumps.py A B

(One step only: over more steps AdamW amplifies the reordered rounding noise
of near-zero bias gradients into a different trajectory, which is why the
fold is opt-in; see docs/PERF.md.)

Folding the projection bias gradients into the kernels that produce their
inputs changes only the summation order of those bias gradients.  So after
one step from the same seeded weights and batch:

  * loss is array-equal;
  * grads is array-equal at every sampled index outside the three bias
    families (attn.qkv.bias, attn.proj.bias, ffn.down.bias) and within the
    column-sum tolerance atol = 2e-2 + 2e-3 sqrt(N), rtol = 2e-2 inside them,
    N = batch * seq rows summed per column;
  * the sample holds a positive number of bias-family elements (computed
    here, not assumed).

The sampled indices are rebuilt from bench._DUMP_SEED / _DUMP_SAMPLE and the
flat-buffer offsets from the model config on the meta device: no GPU needed.
Exits non-zero on the first violated property.
"""
import sys, os; sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import argparse
import math

import numpy as np
import torch

import bench
from tosem2021_amd.models.classifier import CONFIGS, MLTC, MLTCConfig
from tosem2021_amd.train import PAD_ELEMS

BIAS_FAMILIES = ("attn.qkv.bias", "attn.proj.bias", "ffn.down.bias")


def flat_layout(cfg):
    """(name, offset, numel) of every parameter in FlatParams order, and the
    unpadded total."""
    with torch.device("meta"):
        model = MLTC(cfg)
    out, off = [], 0
    for name, p in model.named_parameters():
        if not p.requires_grad:
            continue
        out.append((name, off, p.numel()))
        off += p.numel()
    return out, off


def sample_indices(total):
    """The indices bench.dump_outputs keeps (it samples FlatParams.numel)."""
    if total > bench._DUMP_SAMPLE:
        g = torch.Generator(device="cpu").manual_seed(bench._DUMP_SEED)
        idx = torch.randint(0, total, (bench._DUMP_SAMPLE,), generator=g)
        return idx.sort().values.numpy()
    return np.arange(total)


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("parent")
    ap.add_argument("change")
    ap.add_argument("--model", default="mltc-base")
    ap.add_argument("--batch", type=int, default=128)
    ap.add_argument("--seq", type=int, default=512)
    args = ap.parse_args()

    cfg = CONFIGS[args.model]
    if args.seq > cfg.max_seq:
        cfg = MLTCConfig(**{**cfg.__dict__, "max_seq": args.seq})
    layout, total = flat_layout(cfg)
    assert (total + PAD_ELEMS - 1) // PAD_ELEMS * PAD_ELEMS >= total
    idx = sample_indices(total)

    in_bias = np.zeros(len(idx), dtype=bool)
    per_family = {f: 0 for f in BIAS_FAMILIES}
    for name, off, n in layout:
        fam = next((f for f in BIAS_FAMILIES if name.endswith(f)), None)
        if fam is None:
            continue
        lo, hi = np.searchsorted(idx, off), np.searchsorted(idx, off + n)
        in_bias[lo:hi] = True
        per_family[fam] += int(hi - lo)
    n_bias = int(in_bias.sum())
    print(f"{len(idx)} sampled of {total} elements; {n_bias} inside the "
          f"bias families {per_family}")

    def load(d, name):
        return np.load(os.path.join(d, name + ".npy"))

    ok = True

    def check(cond, msg):
        nonlocal ok
        print(("ok    " if cond else "FAIL  ") + msg)
        ok = ok and bool(cond)

    check(n_bias > 0, "the sample reaches the bias families")
    lp, lc = load(args.parent, "loss"), load(args.change, "loss")
    check(np.array_equal(lp, lc), f"loss array-equal ({lp[0]!r} vs {lc[0]!r})")
    gp, gc = load(args.parent, "grads"), load(args.change, "grads")
    check(gp.shape == gc.shape == idx.shape,
          f"grads shapes match the rebuilt sample {idx.shape}")
    if not ok:
        sys.exit(1)
    outside = ~in_bias
    n_diff = int((gp[outside] != gc[outside]).sum())
    check(n_diff == 0, f"grads array-equal outside the bias families "
          f"({n_diff} of {int(outside.sum())} differ)")
    N = args.batch * args.seq
    atol, rtol = 2e-2 + 2e-3 * math.sqrt(N), 2e-2
    bp, bc = gp[in_bias], gc[in_bias]
    err = np.abs(bc - bp)
    check(bool(np.all(err <= atol + rtol * np.abs(bp))),
          f"bias-family grads within atol {atol:.3g} rtol {rtol:g}: "
          f"max|diff| {float(err.max()):.3e}, max|parent| "
          f"{float(np.abs(bp).max()):.3e}, {int((bp != bc).sum())} of "
          f"{n_bias} differ")
    check(bool(np.any(bc != 0)), "bias-family grads of the change are not "
          "all zero")
    sys.exit(0 if ok else 1)


if __name__ == "__main__":
    main()
