"""Standalone flash-attention kernel microbench (for rocprofv3 PMC runs).

    python scripts/bench_flash.py [iters] [--zero-do-tail] [--bench-mask]

--zero-do-tail zeroes dO where the mask is padding (rows 400..511), as the
model's backward does, so the dead-query-tile skip has something to skip; the
three backward kernels (fa_dot, flash_bwd_fused, flash_dq_recompute) are
reported with and without the flags either way.  With random dO nothing is
skippable and the pair of figures is the cost of the flag test.

--bench-mask takes the padding mask of bench.py's batch instead of the fixed
400 live keys: synthetic_batch's per-row lengths, uniform in [256, 512], so
the workgroups of one launch see tails of different lengths as they do in
the model step."""
import sys, os; sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import time

import torch

from tosem2021_amd import ops


def main():
    B, H, L, dh = 128, 16, 512, 64
    args = [a for a in sys.argv[1:] if not a.startswith("--")]
    zero_tail = "--zero-do-tail" in sys.argv[1:]
    bench_mask = "--bench-mask" in sys.argv[1:]
    iters = int(args[0]) if args else 30
    torch.manual_seed(0)
    q = torch.randn(B, H, L, dh, device="cuda", dtype=torch.bfloat16)
    k = torch.randn_like(q)
    v = torch.randn_like(q)
    mask = torch.zeros(B, L, device="cuda")
    if bench_mask:
        from tosem2021_amd.data.synthetic import synthetic_batch
        from tosem2021_amd.models.classifier import CONFIGS
        _, live, _ = synthetic_batch(CONFIGS["mltc-base"], B, L, device="cuda")
        mask[~live] = -1e9
    else:
        mask[:, 400:] = -1e9
    mask = mask.contiguous()
    pad = (mask < 0).view(B, 1, L, 1)       # padded rows, over heads and dh
    scale = 0.125
    ext = ops.hip_ops()
    for _ in range(5):
        o, lse = ext.flash_fwd(q, k, v, mask, scale)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(iters):
        o, lse = ext.flash_fwd(q, k, v, mask, scale)
    torch.cuda.synchronize()
    dt = (time.perf_counter() - t0) / iters
    flops = 4 * B * H * L * L * dh
    print(f"flash_fwd {dt*1e6:.1f} us/call  {flops/dt/1e12:.1f} TF")
    # bwd stage (round-2 default: dk/dv only, no dS materialization)
    do = torch.randn_like(q)
    if zero_tail:
        do.masked_fill_(pad, 0)
    ddot = ext.fa_dot(do, o)

    # the three backward kernels, without and with the dead-tile flags
    def timed_us(fn):
        for _ in range(3):
            fn()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(iters):
            fn()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) / iters * 1e6

    _, dead = ext.fa_dot_flags(do, o)
    tag = "zero dO tail" if zero_tail else "random dO"
    print(f"[{tag}: {int(dead.sum())} of {dead.numel()} query tiles dead]")
    print(f"fa_dot (ddot + flags) {timed_us(lambda: ext.fa_dot(do, o)):.1f} us")
    # alternating, twice: the first measurement after a change of kernel
    # reads high, so a pair is compared within one pass
    for rep in range(2):
        for name, d in (("no flags", None), ("flags", dead)):
            t_f = timed_us(lambda: ext.flash_bwd_fused(
                q, k, v, do, mask, lse, ddot, scale, dead=d))
            t_q = timed_us(lambda: ext.flash_dq_recompute(
                q, k, v, do, mask, lse, ddot, scale, dead=d))
            print(f"pass {rep} {name}: flash_bwd_fused {t_f:.1f} us  "
                  f"flash_dq_recompute {t_q:.1f} us")
    for _ in range(3):
        dk, dv = ext.flash_bwd_fused(q, k, v, do, mask, lse, ddot, scale)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(iters):
        dk, dv = ext.flash_bwd_fused(q, k, v, do, mask, lse, ddot, scale)
    torch.cuda.synchronize()
    dt = (time.perf_counter() - t0) / iters
    print(f"flash_bwd_fused {dt*1e6:.1f} us/call  {3*flops/dt/1e12:.1f} TF-eq")
    for _ in range(3):
        dq = ext.flash_dq_recompute(q, k, v, do, mask, lse, ddot, scale)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(iters):
        dq = ext.flash_dq_recompute(q, k, v, do, mask, lse, ddot, scale)
    torch.cuda.synchronize()
    dt = (time.perf_counter() - t0) / iters
    print(f"flash_dq_recompute {dt*1e6:.1f} us/call  {3*flops/dt/1e12:.1f} TF-eq")
    # round-1 chain for comparison (dS round-trip + dq-from-ds)
    ds, dk, dv = ext.flash_bwd_fused(q, k, v, do, mask, lse, ddot, scale,
                                     emit_ds=True)
    for _ in range(3):
        dq = ext.flash_dq(ds, k)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(iters):
        ds, dk, dv = ext.flash_bwd_fused(q, k, v, do, mask, lse, ddot, scale,
                                         emit_ds=True)
        dq = ext.flash_dq(ds, k)
    torch.cuda.synchronize()
    dt = (time.perf_counter() - t0) / iters
    print(f"r1 bwd chain (fused+emit_ds + dq) {dt*1e6:.1f} us")
    del ds
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(iters):
        dk, dv = ext.flash_bwd_fused(q, k, v, do, mask, lse, ddot, scale)
        dq = ext.flash_dq_recompute(q, k, v, do, mask, lse, ddot, scale)
    torch.cuda.synchronize()
    dt = (time.perf_counter() - t0) / iters
    print(f"r2 bwd chain (fused + dq_recompute) {dt*1e6:.1f} us")
    del q, k, v, do, dq, dk, dv, o, lse, ddot

    # the training path: packed [B, L, 3D] layout, whole backward binding,
    # without and with the folded qkv bias gradient, and the reduction over
    # dqkv that the fold replaces
    def timed(fn):
        for _ in range(3):
            fn()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(iters):
            fn()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) / iters

    qkv = torch.randn(B, L, 3 * H * dh, device="cuda", dtype=torch.bfloat16)
    dop = torch.randn(B, L, H * dh, device="cuda", dtype=torch.bfloat16)
    if zero_tail:
        dop.masked_fill_(pad.view(B, L, 1), 0)
    o, lse = ext.flash_fwd_packed(qkv, H, mask, scale)
    dt0 = timed(lambda: ext.flash_bwd_packed(qkv, o, dop, mask, lse, H,
                                             scale))
    print(f"flash_bwd_packed {dt0*1e6:.1f} us")
    dtn = timed(lambda: ext.flash_bwd_packed(qkv, o, dop, mask, lse, H, scale,
                                             skip_zero_do=False))
    print(f"flash_bwd_packed skip_zero_do=False {dtn*1e6:.1f} us")
    dqkv = ext.flash_bwd_packed(qkv, o, dop, mask, lse, H, scale)
    dt2 = timed(lambda: dqkv.view(B * L, -1).sum(0))
    print(f"dqkv.sum(0) (the reduce the fold replaces) {dt2*1e6:.1f} us")
    if hasattr(ext, "flash_bwd_packed_bias"):
        dt1 = timed(lambda: ext.flash_bwd_packed_bias(qkv, o, dop, mask, lse,
                                                      H, scale))
        print(f"flash_bwd_packed_bias {dt1*1e6:.1f} us  "
              f"(+{(dt1-dt0)*1e6:.1f} us for the bias)")


if __name__ == "__main__":
    main()
