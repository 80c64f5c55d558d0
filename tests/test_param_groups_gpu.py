"""The grouped AdamW kernels (csrc/adamw.hip) on the GPU.

The main oracle is the existing kernel: for every distinct (lr_mult, wd) of
a table, ops.hip_ops().adamw_step runs on a copy of the whole buffer with the
scalars lr * lr_mult (the f32 product) and wd, the results are stitched by
segment, and the grouped kernel must match them bit for bit.  The second
oracle is the CPU reference, through the assert_close helper and the two
tolerances of tests/test_ops_gpu_scale.py (copied, not imported); a CPU test
shows that this check tells a table shifted by one element from the right
one.
"""
import functools
import math

import numpy as np
import pytest
import torch

from tosem2021_amd import ops
from tosem2021_amd.ops import reference as ref

BF16 = torch.bfloat16
F32 = torch.float32

# tests/test_ops_gpu_scale.py
TOL_MASTER = dict(atol=1e-4, rtol=1e-4)
# ~160 f32 ulps: FMA contraction in the kernel vs mul_/add_ in the reference
TOL_MOMENT = dict(atol=1e-6, rtol=1e-5)


def assert_close(got, want, name, *, atol, rtol):
    """got: kernel output (bf16 or f32); want: the fp32 reference, unrounded.

    f32 outputs get the allclose check alone; bf16 outputs also
    |got - want|_F / |want|_F <= 4 * |bf16(want) - want|_F / |want|_F."""
    assert got.shape == want.shape, (name, got.shape, want.shape)
    assert want.dtype == torch.float32, name
    want = want.to(got.device)
    g = got.float()
    worst = float((g - want).abs().max())
    if got.dtype == BF16:
        norm = float(want.norm())
        assert norm > 0, f"{name}: reference is all zeros"
        floor = float((want.to(BF16).float() - want).norm()) / norm
        rel = float((g - want).norm()) / norm
        print(f"{name}: rel {rel:.3e} floor {floor:.3e} ratio "
              f"{rel / floor:.2f} max|err| {worst:.3e}")
    else:
        print(f"{name}: max|err| {worst:.3e}")
    assert torch.allclose(g, want, atol=atol, rtol=rtol), \
        f"{name}: allclose failed, max|err| {worst:.3e}"
    if got.dtype == BF16:
        assert rel <= 4 * floor, \
            f"{name}: rel {rel:.3e} > 4 x bf16 floor {floor:.3e}"


HP = dict(beta1=0.9, beta2=0.999, eps=1e-8)
LRS = (1e-2, 7e-3, 4e-3)        # the scheduled rate of steps 1, 2, 3
GRAD_SCALE = 0.5
# distinct (lr_mult, wd); segment k takes PAIRS[k % 5], so neighbours differ
PAIRS = ((1.0, 0.05), (0.8, 0.0), (0.64, 0.05), (0.512, 0.01), (1.0, 0.0))

# test_adamw_scale's size: two full grid-stride passes of the 2048 x 1024
# cap plus a 148-element tail.  The clipped entry points take multiples of
# 8 only (the norm kernel's 16 B bf16 loads), so they get 4 more elements.
N_PLAIN = 4194452
N_CLIPPED = 4194456
PASS = 2048 * 1024


def big_ends(n):
    return [1, 2, 3,                # three boundaries inside the first group
            1001, 2002, 3003,       # = 1, 2, 3 mod 4
            5001, 5005,             # a 4-element segment starting at 1 mod 4
            PASS + 6,               # inside the second pass
            2 * PASS + 75,          # inside the tail
            n]


def scalar_lr(lr, mult):
    return float(np.float32(lr) * np.float32(mult))


@functools.lru_cache(maxsize=None)
def inputs(n, grad_dtype):
    """CPU inputs, never modified.  master = sign * (1 + |randn|): no
    element near zero, where a wrong wd would be invisible."""
    g = torch.Generator().manual_seed(n % 1000 + (grad_dtype == F32))
    r = torch.randn(n, generator=g)
    master = torch.where(r < 0, -1.0, 1.0) * (1 + r.abs())
    grads = torch.randn(n, generator=g).to(grad_dtype)
    return master, grads


def fresh(master, device="cuda"):
    """[p, m, v, master] at step 0."""
    mst = master.to(device)
    return [mst.to(BF16), torch.zeros_like(mst), torch.zeros_like(mst),
            mst.clone()]


def seg_pairs(ends):
    return [PAIRS[k % len(PAIRS)] for k in range(len(ends))]


def table_for(ends, n, device="cuda"):
    pairs = seg_pairs(ends)
    return ops.segment_table(ends, [a for a, _ in pairs],
                             [b for _, b in pairs], n, device=device)


def stitched(ends, n, master, grads, clip_state=None):
    """The oracle: the ungrouped kernel once per distinct pair on the whole
    buffer, three steps, stitched by segment."""
    pairs = seg_pairs(ends)
    distinct = sorted(set(pairs))
    lens = torch.diff(torch.tensor([0] + list(ends)))
    pair_of = torch.repeat_interleave(
        torch.tensor([distinct.index(pr) for pr in pairs]), lens).cuda()
    gg = grads.cuda()
    out = None
    for k, (mult, wd) in enumerate(distinct):
        bufs = fresh(master)
        for step, lr in enumerate(LRS, start=1):
            args = (scalar_lr(lr, mult), HP["beta1"], HP["beta2"], HP["eps"],
                    wd, step)
            if clip_state is None:
                ops.hip_ops().adamw_step(bufs[0], gg, *bufs[1:], *args,
                                         GRAD_SCALE)
            else:
                ops.hip_ops().adamw_step_clipped(bufs[0], gg, *bufs[1:],
                                                 *args, clip_state)
        if out is None:
            out = bufs
        else:
            sel = pair_of == k
            out = [torch.where(sel, b, o) for b, o in zip(bufs, out)]
    return out


def grouped(ends, n, master, grads, clip_state=None):
    table = table_for(ends, n)
    gg = grads.cuda()
    bufs = fresh(master)
    for step, lr in enumerate(LRS, start=1):
        if clip_state is None:
            ops.adamw_step_grouped(bufs[0], gg, *bufs[1:], *table, lr=lr,
                                   step=step, grad_scale=GRAD_SCALE, **HP)
        else:
            ops.adamw_step_grouped_clipped(bufs[0], gg, *bufs[1:], *table,
                                           lr=lr, step=step,
                                           clip_state=clip_state, **HP)
    return bufs


def bitwise(got, want):
    for name, a, b in zip(("p", "m", "v", "master"), got, want):
        bad = int((a != b).sum())
        first = int((a != b).nonzero()[0]) if bad else -1
        assert torch.equal(a, b), f"{name}: {bad} elements differ, the " \
                                  f"first at {first}"


@functools.lru_cache(maxsize=None)
def cpu_reference(grad_dtype, shift=0):
    """reference.adamw_step_grouped on the CPU, three steps, for the big
    table with every inner boundary moved up by `shift` elements."""
    n = N_PLAIN
    master, grads = inputs(n, grad_dtype)
    ends = big_ends(n)
    moved = [e + shift for e in ends[:-1]] + [n]
    pairs = seg_pairs(ends)
    table = ops.segment_table(moved, [a for a, _ in pairs],
                              [b for _, b in pairs], n)
    bufs = fresh(master, "cpu")
    for step, lr in enumerate(LRS, start=1):
        ref.adamw_step_grouped(bufs[0], grads, *bufs[1:], *table, lr=lr,
                               step=step, grad_scale=GRAD_SCALE, **HP)
    return bufs


# ---- CPU: the table and the check are what they claim -----------------------

def test_big_table_covers_the_cases():
    for n in (N_PLAIN, N_CLIPPED):
        ends = big_ends(n)
        assert n % 4 == 0 and n > 2 * PASS and n - 2 * PASS < PASS
        assert ends[:3] == [1, 2, 3]
        assert [e % 4 for e in ends[3:6]] == [1, 2, 3]
        assert ends[6] % 4 == 1 and ends[7] - ends[6] == 4
        assert PASS < ends[8] < PASS + 1024 and 2 * PASS < ends[9] < n
        assert ends[-1] == n
        pairs = seg_pairs(ends)
        assert len(set(pairs)) >= 4
        assert any(wd == 0.0 for _, wd in pairs)
        assert any(mult == 1.0 for mult, _ in pairs)
        assert all(a != b for a, b in zip(pairs, pairs[1:]))
    assert N_CLIPPED % 8 == 0


def test_reference_check_is_discriminating():
    """At TOL_MASTER the reference passes against itself and a table with
    every boundary one element late fails, at exactly the elements that
    changed segment."""
    want = cpu_reference(BF16)
    mutant = cpu_reference(BF16, shift=1)
    assert_close(want[3].clone(), want[3], "master control", **TOL_MASTER)
    assert_close(want[1].clone(), want[1], "m control", **TOL_MOMENT)
    assert_close(want[2].clone(), want[2], "v control", **TOL_MOMENT)
    assert torch.equal(want[0], want[3].to(BF16))
    with pytest.raises(AssertionError):
        assert_close(mutant[3], want[3], "master, shifted table",
                     **TOL_MASTER)
    err = (mutant[3] - want[3]).abs()
    bad = err > TOL_MASTER["atol"] + TOL_MASTER["rtol"] * want[3].abs()
    assert bad.nonzero().flatten().tolist() == big_ends(N_PLAIN)[:-1]


# ---- GPU --------------------------------------------------------------------

@pytest.mark.gpu
@pytest.mark.parametrize("grad_dtype", [BF16, F32], ids=["bf16grad", "f32grad"])
def test_grouped_is_bitwise_the_scalar_kernel(grad_dtype):
    n = N_PLAIN
    master, grads = inputs(n, grad_dtype)
    ends = big_ends(n)
    got = grouped(ends, n, master, grads)
    bitwise(got, stitched(ends, n, master, grads))
    # the stitched oracle is not trivially uniform
    assert not torch.equal(got[3], stitched([n], n, master, grads)[3])


@pytest.mark.gpu
@pytest.mark.parametrize("grad_dtype", [BF16, F32], ids=["bf16grad", "f32grad"])
def test_grouped_clipped_is_bitwise_the_scalar_kernel(grad_dtype):
    n = N_CLIPPED
    master, grads = inputs(n, grad_dtype)
    ends = big_ends(n)
    # |g| is about 2048
    state = ops.grad_clip_state(grads.cuda(), grad_scale=GRAD_SCALE,
                                max_norm=100.0)
    norm, scale, finite, _ = state.tolist()
    print(f"norm {norm:.2f} scale {scale:.5f}")
    assert finite == 1.0 and scale < 0.2 * GRAD_SCALE   # the clip is active
    got = grouped(ends, n, master, grads, clip_state=state)
    bitwise(got, stitched(ends, n, master, grads, clip_state=state))
    # and the scale was read from the state: by value it is the same step
    table = table_for(ends, n)
    bufs = fresh(master)
    for step, lr in enumerate(LRS, start=1):
        ops.hip_ops().adamw_step_grouped(
            bufs[0], grads.cuda(), *bufs[1:], *table, lr, HP["beta1"],
            HP["beta2"], HP["eps"], step, scale)
    bitwise(got, bufs)


@pytest.mark.gpu
@pytest.mark.parametrize("grad_dtype", [BF16, F32], ids=["bf16grad", "f32grad"])
def test_grouped_matches_cpu_reference(grad_dtype):
    n = N_PLAIN
    master, grads = inputs(n, grad_dtype)
    p, m, v, mst = grouped(big_ends(n), n, master, grads)
    _, m_w, v_w, mst_w = cpu_reference(grad_dtype)
    assert_close(mst, mst_w, "master", **TOL_MASTER)
    assert_close(m, m_w, "m", **TOL_MOMENT)
    assert_close(v, v_w, "v", **TOL_MOMENT)
    assert torch.equal(p, mst.to(BF16))


@pytest.mark.gpu
@pytest.mark.parametrize("grad_dtype", [BF16, F32], ids=["bf16grad", "f32grad"])
def test_one_segment_is_the_ungrouped_kernel(grad_dtype):
    n = N_PLAIN
    master, grads = inputs(n, grad_dtype)
    gg = grads.cuda()
    table = ops.segment_table([n], [1.0], [0.05], n, device="cuda")
    a, b = fresh(master), fresh(master)
    for step, lr in enumerate(LRS, start=1):
        ops.adamw_step_grouped(a[0], gg, *a[1:], *table, lr=lr, step=step,
                               grad_scale=GRAD_SCALE, **HP)
        ops.adamw_step(b[0], gg, *b[1:], lr=lr, wd=0.05, step=step,
                       grad_scale=GRAD_SCALE, **HP)
    bitwise(a, b)
    assert not torch.equal(a[3], master.cuda())


def _many_segments(n, S, seed):
    """S segments of mixed length over n elements."""
    rng = np.random.default_rng(seed)
    cuts = np.sort(rng.choice(np.arange(1, n), size=S - 1, replace=False))
    return [int(c) for c in cuts] + [n]


@pytest.mark.gpu
@pytest.mark.parametrize("n,S", [(512, 128), (8192, 1024)],
                         ids=["one-block-128x4", "1024-mixed"])
@pytest.mark.parametrize("grad_dtype", [BF16, F32], ids=["bf16grad", "f32grad"])
def test_small_and_large_tables(n, S, grad_dtype):
    ends = list(range(4, n + 1, 4)) if S == 128 else _many_segments(n, S, 3)
    assert len(ends) == S and ends[-1] == n
    if S == 1024:
        lens = np.diff([0] + ends)
        assert lens.min() == 1 and lens.max() > 16      # mixed indeed
    master, grads = inputs(n, grad_dtype)
    got = grouped(ends, n, master, grads)
    bitwise(got, stitched(ends, n, master, grads))
    state = ops.grad_clip_state(grads.cuda(), grad_scale=GRAD_SCALE,
                                max_norm=1.0)
    assert float(state[1]) < GRAD_SCALE
    got = grouped(ends, n, master, grads, clip_state=state)
    bitwise(got, stitched(ends, n, master, grads, clip_state=state))


@pytest.mark.gpu
def test_table_limits_raise():
    n = 4096
    bufs = fresh(inputs(n, BF16)[0])
    g = inputs(n, BF16)[1].cuda()
    before = [b.clone() for b in bufs]
    dev = dict(device="cuda")
    ends = torch.arange(1, 1026, dtype=torch.int64, **dev)
    ones, zeros = torch.ones(1025, **dev), torch.zeros(1025, **dev)
    hip = ops.hip_ops()
    args = (1e-3, 0.9, 0.999, 1e-8, 1, 1.0)
    state = ops.grad_clip_state(g, max_norm=1.0)
    for call, tail in ((hip.adamw_step_grouped, args),
                       (hip.adamw_step_grouped_clipped, args[:-1] + (state,))):
        with pytest.raises(RuntimeError, match="1 to 1024"):
            call(bufs[0], g, *bufs[1:], ends, ones, zeros, *tail)
        with pytest.raises(RuntimeError, match="1 to 1024"):
            call(bufs[0], g, *bufs[1:], ends[:0], ones[:0], zeros[:0], *tail)
        with pytest.raises(RuntimeError, match="one length"):
            call(bufs[0], g, *bufs[1:], ends[:4], ones[:3], zeros[:4], *tail)
        with pytest.raises(RuntimeError, match="int64"):
            call(bufs[0], g, *bufs[1:], ends[:4].int(), ones[:4], zeros[:4],
                 *tail)
        with pytest.raises(RuntimeError, match="GPU"):
            call(bufs[0], g, *bufs[1:], ends[:4].cpu(), ones[:4], zeros[:4],
                 *tail)
        with pytest.raises(RuntimeError, match="f32"):
            call(bufs[0], g, *bufs[1:], ends[:4], ones[:4].double(),
                 zeros[:4], *tail)
        with pytest.raises(RuntimeError, match="size mismatch"):
            call(bufs[0], g[:n - 8].clone(), *bufs[1:], ends[:4], ones[:4],
                 zeros[:4], *tail)
    with pytest.raises(ValueError, match="1025"):
        ops.adamw_step_grouped(bufs[0], g, *bufs[1:], ends, ones, zeros,
                               lr=1e-3, step=1)
    with pytest.raises(ValueError, match="on cuda"):
        ops.adamw_step_grouped(bufs[0], g, *bufs[1:], ends[:4].cpu(),
                               ones[:4], zeros[:4], lr=1e-3, step=1)
    torch.cuda.synchronize()
    bitwise(bufs, before)


@pytest.mark.gpu
def test_non_finite_gradient_skips():
    n = 8192
    master, grads = inputs(n, BF16)
    ends = _many_segments(n, 64, 4)
    table = table_for(ends, n)
    for bad in (math.nan, math.inf):
        g = grads.cuda().clone()
        g[n // 2 + 1] = bad
        state = ops.grad_clip_state(g, max_norm=1.0)
        assert float(state[2]) == 0.0
        bufs = fresh(master)
        bufs[1].uniform_(0.1, 1.0)
        bufs[2].uniform_(0.1, 1.0)
        before = [b.clone() for b in bufs]
        ops.adamw_step_grouped_clipped(bufs[0], g, *bufs[1:], *table,
                                       lr=1e-2, step=1, clip_state=state,
                                       **HP)
        torch.cuda.synchronize()
        bitwise(bufs, before)


@pytest.mark.gpu
def test_run_to_run_bitwise():
    n = N_PLAIN
    master, grads = inputs(n, BF16)
    ends = big_ends(n)
    first = grouped(ends, n, master, grads)
    for _ in range(4):
        bitwise(grouped(ends, n, master, grads), first)


@pytest.mark.gpu
def test_trainer_step_matches_reference():
    """mltc-tiny, bf16, both options on, one step: the trainer's buffers
    against reference.adamw_step_grouped with a table built here, one
    segment per parameter, from the parameter names."""
    from tosem2021_amd.data.synthetic import synthetic_batch
    from tosem2021_amd.models.classifier import CONFIGS
    from tosem2021_amd.train import TrainConfig, Trainer
    cfg = CONFIGS["mltc-tiny"]
    decay, wd = 0.8, 0.05
    torch.manual_seed(0)
    t = Trainer(TrainConfig(model="mltc-tiny", lr=1e-3, warmup_steps=0,
                            weight_decay=wd, no_decay_1d=True,
                            layer_decay=decay),
                device=torch.device("cuda"))
    f = t.flat
    ends, mults, wds = [], [], []
    off = 0
    for name, p in t.model.named_parameters():
        off += p.numel()
        if name.startswith(("tok_emb", "pos_emb")):
            depth = 0
        elif name.startswith("blocks."):
            depth = int(name.split(".")[1]) + 1
        else:
            depth = cfg.n_layers + 1
        ends.append(off)
        mults.append(decay ** (cfg.n_layers + 1 - depth))
        wds.append(0.0 if p.dim() == 1 else wd)
    assert off == f.numel and off % 4 == 1      # the heads end off the lattice
    ends[-1] = f.padded
    table = ops.segment_table(ends, mults, wds, f.padded)
    before = [x.detach().clone().cpu() for x in (f.flat, f.m, f.v, f.master)]
    start = [x.clone() for x in before]
    tokens, mask, labels = synthetic_batch(cfg, 8, 32, seed=42, device="cuda")
    t.step(tokens, mask, labels)
    assert t.step_num == t.opt_step == 1
    grad = f.grad_flat.detach().clone().cpu()    # left in place by the step
    assert grad.dtype == BF16 and float(grad.float().abs().sum()) > 0
    ref.adamw_step_grouped(before[0], grad, before[1], before[2], before[3],
                           *table, lr=t._lr(), beta1=t.cfg.beta1,
                           beta2=t.cfg.beta2, eps=t.cfg.eps, step=1,
                           grad_scale=t.ddp.grad_scale)
    assert_close(f.master, before[3], "master", **TOL_MASTER)
    assert_close(f.m, before[1], "m", **TOL_MOMENT)
    assert_close(f.v, before[2], "v", **TOL_MOMENT)
    assert torch.equal(f.flat, f.master.to(BF16))
    # the options are visible at TOL_MASTER: the plain step is far off
    ref.adamw_step(start[0], grad, start[1], start[2], start[3], lr=t._lr(),
                   beta1=t.cfg.beta1, beta2=t.cfg.beta2, eps=t.cfg.eps,
                   wd=wd, step=1, grad_scale=t.ddp.grad_scale)
    with pytest.raises(AssertionError):
        assert_close(f.master, start[3], "master, ungrouped", **TOL_MASTER)
