"""bf16 vs MXFP8 serving, in one process, the two alternating.

Three sections, each printed as one JSON line:

  end_to_end  examples/s of a no_grad eval forward of the model (default
              mltc-base) at seq 256, batch 64 and 512, padded (full-length
              rows) and packed (the same tokens as one PackedBatch of
              full-length segments), bf16 against quantize_mx() on the same
              weights.
  gemms       per batch size, the four projections of a block as F.linear
              in bf16 (with bias, as the model calls them) against
              ops.mx_linear on pre-quantised operands.
  quantisers  mx_quant_rows, mx_add_layernorm and mx_bias_gelu at the
              model's shapes: bytes/s against the bytes their shapes require
              (bf16 operands read, 1 + 1/32 byte per element written, plus
              the bf16 sum for add+LayerNorm).

Every timing: warm-up calls first, then `--repeats` windows of `--iters`
calls each, a device synchronise on both sides of a window; bf16 and MX
windows alternate.  Reported: the median window and the spread
(max - min) / median over the repeats.  Inputs are seeded; weights are the
model's random initialisation, which does not change the rates.
"""
import sys, os; sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import argparse
import json
import statistics
import time

import torch
import torch.nn.functional as F

from tosem2021_amd import ops
from tosem2021_amd.data.packing import pack_examples
from tosem2021_amd.models.classifier import CONFIGS, MLTCConfig, build_model


def windows(fns, iters, repeats, warmup=3):
    """{name: [seconds per call, one per repeat]} with the fns alternating."""
    for fn in fns.values():
        for _ in range(warmup):
            fn()
    out = {k: [] for k in fns}
    for _ in range(repeats):
        for k, fn in fns.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(iters):
                fn()
            torch.cuda.synchronize()
            out[k].append((time.perf_counter() - t0) / iters)
    return out


def summary(ts):
    med = statistics.median(ts)
    return med, (max(ts) - min(ts)) / med


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--model", default="mltc-base")
    ap.add_argument("--seq", type=int, default=256)
    ap.add_argument("--batches", type=int, nargs="+", default=[64, 512])
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--repeats", type=int, default=5)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_mx_serving needs a GPU: no CPU fallback")

    dev = torch.device("cuda")
    base = CONFIGS[args.model]
    cfg = MLTCConfig(**{**base.__dict__, "max_seq": args.seq})
    torch.manual_seed(0)
    model = build_model(cfg).to(dev).eval()
    D, Dff, V = cfg.d_model, cfg.d_ff, cfg.vocab_size
    backend = ops.mx_gemm_backend()
    head = {"model": args.model, "seq": args.seq, "iters": args.iters,
            "repeats": args.repeats, "mx_gemm_backend": backend,
            "mx_bias_in_gemm": ops.mx_bias_in_gemm()}
    g = torch.Generator().manual_seed(0)

    # ---- end to end ---------------------------------------------------------
    rows = []
    for Bn in args.batches:
        tokens = torch.randint(1, V, (Bn, args.seq), generator=g)
        mask = torch.ones(Bn, args.seq, dtype=torch.bool)
        pb = pack_examples(tokens.tolist(), args.seq).to(dev)
        tokens, mask = tokens.to(dev), mask.to(dev)
        for layout, call in (("padded", lambda: model(tokens, mask)),
                             ("packed", lambda: model(None, packing=pb))):
            # switching precision (re-quantising the weights) and two
            # untimed calls happen in front of every window
            ts = {"bf16": [], "mx": []}
            with torch.no_grad():
                for _ in range(args.repeats):
                    for kind in ("bf16", "mx"):
                        model.quantize_mx() if kind == "mx" else \
                            model.clear_mx()
                        for _ in range(2):
                            call()
                        torch.cuda.synchronize()
                        t0 = time.perf_counter()
                        for _ in range(args.iters):
                            call()
                        torch.cuda.synchronize()
                        ts[kind].append((time.perf_counter() - t0)
                                        / args.iters)
            mb, sb = summary(ts["bf16"])
            mm, sm = summary(ts["mx"])
            rows.append({"batch": Bn, "layout": layout,
                         "bf16_ex_per_s": round(Bn / mb, 1),
                         "mx_ex_per_s": round(Bn / mm, 1),
                         "mx_over_bf16": round(mb / mm, 3),
                         "bf16_spread": round(sb, 3),
                         "mx_spread": round(sm, 3)})
            print(rows[-1], flush=True)
    model.clear_mx()
    print(json.dumps({"metric": "mx_serving_end_to_end", **head,
                      "rows": rows}))

    # ---- the four GEMMs -------------------------------------------------------
    rows = []
    for Bn in args.batches:
        M = Bn * args.seq
        for name, N, K in (("qkv", 3 * D, D), ("proj", D, D),
                           ("up", Dff, D), ("down", D, Dff)):
            x = torch.randn(M, K, generator=g).bfloat16().to(dev)
            w = (torch.randn(N, K, generator=g) * 0.02).bfloat16().to(dev)
            b = torch.zeros(N, dtype=torch.bfloat16, device=dev)
            qa, sa = ops.mx_quant_rows(x)
            qw, sw = ops.mx_quant_rows(w)
            ts = windows({"bf16": lambda: F.linear(x, w, b),
                          "mx": lambda: ops.mx_linear(qa, sa, qw, sw, b)},
                         args.iters * 4, args.repeats)
            mb, sb = summary(ts["bf16"])
            mm, sm = summary(ts["mx"])
            fl = 2.0 * M * N * K
            rows.append({"gemm": name, "M": M, "N": N, "K": K,
                         "bf16_us": round(mb * 1e6, 1),
                         "mx_us": round(mm * 1e6, 1),
                         "bf16_tflops": round(fl / mb / 1e12, 1),
                         "mx_tflops": round(fl / mm / 1e12, 1),
                         "mx_over_bf16": round(mb / mm, 3),
                         "bf16_spread": round(sb, 3),
                         "mx_spread": round(sm, 3)})
            print(rows[-1], flush=True)
    print(json.dumps({"metric": "mx_serving_gemms", **head, "rows": rows}))

    # ---- the quantising kernels -----------------------------------------------
    rows = []
    for Bn in args.batches:
        M = Bn * args.seq
        x = torch.randn(M, D, generator=g).bfloat16().to(dev)
        r = torch.randn(M, D, generator=g).bfloat16().to(dev)
        gamma = torch.ones(D, dtype=torch.bfloat16, device=dev)
        beta = torch.zeros(D, dtype=torch.bfloat16, device=dev)
        h = torch.randn(M, Dff, generator=g).bfloat16().to(dev)
        ub = torch.zeros(Dff, dtype=torch.bfloat16, device=dev)
        qbytes = 1 + 1 / 32
        cases = {
            "mx_quant_rows": (lambda: ops.mx_quant_rows(x),
                              M * D * (2 + qbytes)),
            "mx_add_layernorm": (
                lambda: ops.mx_add_layernorm(x, r, gamma, beta, 1e-5),
                M * D * (2 + 2 + 2 + qbytes)),
            "mx_bias_gelu": (lambda: ops.mx_bias_gelu(h, ub),
                             M * Dff * (2 + qbytes)),
            # today's kernels at the same shapes, for scale
            "fused_add_layernorm": (
                lambda: ops.fused_add_layernorm(x, r, gamma, beta, 1e-5),
                M * D * (2 + 2 + 2 + 2)),
            "fused_bias_gelu": (lambda: ops.fused_bias_gelu(h, ub),
                                M * Dff * (2 + 2)),
        }
        with torch.no_grad():
            ts = windows({k: v[0] for k, v in cases.items()},
                         args.iters * 4, args.repeats)
        for k, (_, nbytes) in cases.items():
            med, spread = summary(ts[k])
            rows.append({"kernel": k, "rows": M,
                         "us": round(med * 1e6, 1),
                         "required_bytes": int(nbytes),
                         "tb_per_s": round(nbytes / med / 1e12, 2),
                         "spread": round(spread, 3)})
            print(rows[-1], flush=True)
    print(json.dumps({"metric": "mx_serving_quantisers", **head,
                      "rows": rows}))


if __name__ == "__main__":
    main()
