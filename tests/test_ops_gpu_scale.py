"""Elementwise kernels at training sizes, against the fp32 reference.

LayerNorm, bias+GeLU, softmax, the pools and AdamW are persistent
grid-stride kernels whose grids are capped by their launchers, each in the
kernel's own csrc/*.hip file.  The shapes here
are the smallest that send a wave round its loop a second time with a ragged
tail, at every config width (D = 128, 512, 1024, 2048), plus five-launch
bitwise reproducibility of the two reductions that merge across waves.

Every comparison goes through one helper, `assert_close`.  For a bf16 output
it asserts the op's usual allclose tolerances AND

    |got - want|_F / |want|_F  <=  4 * |bf16(want) - want|_F / |want|_F

The right-hand side is computed from the fp32 reference alone.  The kernels
read the same bf16 inputs, compute in f32 and round once, so their error is
that rounding floor (about 1.7e-3) plus f32 reordering and __expf noise,
orders of magnitude below it.  A dropped term or a wrong index is tens of
floors.  The CPU tests at the top prove that: reference mutants must be
rejected by the helper and the rounded reference itself accepted.

References are tosem2021_amd/ops/reference.py on fp32 copies of the bf16
inputs, on the CPU below 8M elements and on the GPU tensors (plain torch,
independent of the extension) from there on, to keep each case to seconds.
"""
import functools
import math

import pytest
import torch

from tosem2021_amd import ops
from tosem2021_amd.ops import reference as ref

BF16 = torch.bfloat16
EPS = 1e-5

# the project's allclose tolerances per op (tests/test_ops_gpu.py,
# tests/test_packing_gpu.py), unchanged
TOL_LN_Y = dict(atol=3e-2, rtol=2e-2)
TOL_LN_MEAN = dict(atol=2e-3, rtol=1e-3)
TOL_LN_RSTD = dict(atol=2e-3, rtol=2e-3)
TOL_LN_DX = dict(atol=4e-2, rtol=3e-2)
TOL_GELU = dict(atol=3e-2, rtol=2e-2)
TOL_SOFTMAX = dict(atol=8e-3, rtol=2e-2)
TOL_POOL = dict(atol=2e-2, rtol=2e-2)
TOL_MASTER = dict(atol=1e-4, rtol=1e-4)
# ~160 f32 ulps: FMA contraction in the kernel vs mul_/add_ in the reference
TOL_MOMENT = dict(atol=1e-6, rtol=1e-5)


def tol_dparam(N):
    return dict(atol=2e-2 + 2e-3 * math.sqrt(N), rtol=2e-2)


def tol_dbias(N):
    return dict(atol=0.1 + 0.01 * math.sqrt(N), rtol=2e-2)


def assert_close(got, want, name, *, atol, rtol):
    """got: kernel output (bf16 or f32); want: the fp32 reference, unrounded.

    f32 outputs get the allclose check alone; bf16 outputs also the relative
    Frobenius bound of the module docstring."""
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


def ref_device(numel):
    return "cuda" if numel >= 8 * 2 ** 20 else "cpu"


# ---- inputs that make a wrong term visible ----------------------------------

@functools.lru_cache(maxsize=2)
def ln_inputs(N, D):
    """x = 2.5 + 1.7 randn + per-row offset, gamma = 1 + 0.3 randn,
    dy = 0.5 + randn + 0.5 xhat: neither mean(dy gamma) nor
    mean(dy gamma xhat) is near zero, so dropping either term of dx is a
    relative error near 0.5, and an uncentred forward is far off."""
    g = torch.Generator().manual_seed(1000 * D + N)
    off = torch.linspace(-3.0, 3.0, N).unsqueeze(1)
    x = (2.5 + 1.7 * torch.randn(N, D, generator=g) + off).to(BF16)
    res = torch.randn(N, D, generator=g).to(BF16)
    gamma = (1 + 0.3 * torch.randn(D, generator=g)).to(BF16)
    beta = torch.randn(D, generator=g).to(BF16)
    xf = x.float()
    xhat = (xf - xf.mean(-1, keepdim=True)) * torch.rsqrt(
        xf.var(-1, unbiased=False, keepdim=True) + EPS)
    dy = (0.5 + torch.randn(N, D, generator=g) + 0.5 * xhat).to(BF16)
    ds = torch.randn(N, D, generator=g).to(BF16)
    return x, res, gamma, beta, dy, ds


def ln_bwd_reference(dy, x, gamma, ds):
    """fp32 stats and gradients of the reference on whatever device the
    inputs live on; ds (optional) is the residual-stream grad added to dx."""
    _, mean, rstd = ref.layernorm_fwd(x.float(), gamma.float(),
                                      torch.zeros_like(gamma).float(), EPS)
    dx, dg, db = ref.layernorm_bwd(dy.float(), x.float(), gamma.float(),
                                   mean, rstd)
    if ds is not None:
        dx = dx + ds.float()
    return mean, rstd, dx, dg, db


def pad_mask(B, Lk, pads):
    """Additive [B, Lk] key mask with a different pad length per batch row."""
    assert len(pads) == B and len(set(pads)) == B
    mask = torch.zeros(B, Lk)
    for b, p in enumerate(pads):
        mask[b, Lk - p:] = -1e9
    return mask


def softmax_inputs(B, H, Lq, Lk, pads, seed):
    g = torch.Generator().manual_seed(seed)
    s = (torch.randn(B, H, Lq, Lk, generator=g) * 3).to(BF16)
    dp = torch.randn(B, H, Lq, Lk, generator=g).to(BF16)
    return s, dp, pad_mask(B, Lk, pads)


def pool_reference(x, mask):
    """fp32 masked mean over L and the gradient map dpooled -> dx."""
    B, L, _ = x.shape
    w = (mask.float() if mask is not None else torch.ones(B, L)).unsqueeze(-1)
    counts = w.sum(1).clamp(min=1)
    pooled = (x.float() * w).sum(1) / counts

    def bwd(dp):
        return (dp.float() / counts).unsqueeze(1).expand(-1, L, -1) * w
    return pooled, counts.squeeze(-1), bwd


def adamw_reference(master, grads, steps, **hp):
    m = torch.zeros_like(master)
    v = torch.zeros_like(master)
    mst = master.clone()
    p = mst.to(BF16)
    for step in range(1, steps + 1):
        ref.adamw_step(p, grads.float(), m, v, mst, step=step, **hp)
    return p, m, v, mst


ADAMW_HP = dict(lr=1e-2, beta1=0.9, beta2=0.999, eps=1e-8, wd=0.05,
                grad_scale=0.5)


# ---- CPU: the helper rejects mutants and accepts the rounded reference ------

def rejects(got, want, name, **tol):
    with pytest.raises(AssertionError):
        assert_close(got, want, name, **tol)


def test_helper_layernorm_fwd_mutant():
    x, _, gamma, beta, _, _ = ln_inputs(64, 256)
    want, _, _ = ref.layernorm_fwd(x.float(), gamma.float(), beta.float(), EPS)
    assert_close(want.to(BF16), want, "ln y control", **TOL_LN_Y)
    xf = x.float()
    rstd = torch.rsqrt(xf.var(-1, unbiased=False, keepdim=True) + EPS)
    uncentred = xf * rstd * gamma.float() + beta.float()
    rejects(uncentred.to(BF16), want, "ln y uncentred", **TOL_LN_Y)


def test_helper_layernorm_bwd_mutants():
    x, _, gamma, _, dy, _ = ln_inputs(64, 256)
    mean, rstd, want, _, _ = ln_bwd_reference(dy, x, gamma, None)
    assert_close(want.to(BF16), want, "ln dx control", **TOL_LN_DX)
    xhat = (x.float() - mean[:, None]) * rstd[:, None]
    dyg = dy.float() * gamma.float()
    c1 = dyg.mean(-1, keepdim=True)
    c2 = (dyg * xhat).mean(-1, keepdim=True)
    no_c1 = rstd[:, None] * (dyg - xhat * c2)
    no_c2 = rstd[:, None] * (dyg - c1)
    rejects(no_c1.to(BF16), want, "ln dx without mean(dy g)", **TOL_LN_DX)
    rejects(no_c2.to(BF16), want, "ln dx without xhat mean(dy g xhat)",
            **TOL_LN_DX)


def test_helper_bias_gelu_mutant():
    g = torch.Generator().manual_seed(2)
    x = torch.randn(64, 256, generator=g).to(BF16)
    b = torch.randn(256, generator=g).to(BF16)
    want = ref.bias_gelu_fwd(x.float(), b.float())
    assert_close(want.to(BF16), want, "gelu control", **TOL_GELU)
    rolled = ref.bias_gelu_fwd(x.float(), b.float().roll(8))
    rejects(rolled.to(BF16), want, "gelu bias rolled by 8", **TOL_GELU)


def test_helper_softmax_mutants():
    B, H, Lq, Lk = 3, 2, 64, 64
    s, dp, mask = softmax_inputs(B, H, Lq, Lk, (16, 40, 8), seed=3)
    scale = 0.125
    want = ref.softmax_fwd(s.float(), mask, scale)
    assert_close(want.to(BF16), want, "softmax p control", **TOL_SOFTMAX)
    mask0 = mask[:1].expand(B, -1).contiguous()
    rejects(ref.softmax_fwd(s.float(), mask0, scale).to(BF16), want,
            "softmax p with batch 0's mask everywhere", **TOL_SOFTMAX)
    p = want.to(BF16)
    dwant = ref.softmax_bwd(dp.float(), p.float(), scale)
    assert_close(dwant.to(BF16), dwant, "softmax ds control", **TOL_SOFTMAX)
    rejects(torch.zeros_like(p), dwant, "softmax ds zeros", **TOL_SOFTMAX)
    no_dot = scale * p.float() * dp.float()
    rejects(no_dot.to(BF16), dwant, "softmax ds without dot", **TOL_SOFTMAX)


def test_helper_masked_pool_mutant():
    g = torch.Generator().manual_seed(4)
    B, L, D = 4, 64, 128
    x = torch.randn(B, L, D, generator=g).to(BF16)
    mask = torch.zeros(B, L, dtype=torch.bool)
    for b, n in enumerate((64, 5, 33, 50)):
        mask[b, :n] = True
    want, _, _ = pool_reference(x, mask)
    assert_close(want.to(BF16), want, "pool control", **TOL_POOL)
    by_len = (x.float() * mask.float().unsqueeze(-1)).sum(1) / L
    rejects(by_len.to(BF16), want, "pool divided by L", **TOL_POOL)


def test_helper_adamw_mutant():
    g = torch.Generator().manual_seed(5)
    n = 64
    master = torch.randn(n, generator=g)
    grads = torch.randn(n, generator=g)
    _, m, v, want = adamw_reference(master, grads, 3, **ADAMW_HP)
    assert_close(want.clone(), want, "adamw master control", **TOL_MASTER)
    assert_close(m.clone(), m, "adamw m control", **TOL_MOMENT)
    hp = dict(ADAMW_HP)
    gs = hp.pop("grad_scale")
    mm, vv, mst = torch.zeros(n), torch.zeros(n), master.clone()
    for _ in range(3):     # no bias correction
        gg = grads * gs
        mm.mul_(hp["beta1"]).add_(gg, alpha=1 - hp["beta1"])
        vv.mul_(hp["beta2"]).addcmul_(gg, gg, value=1 - hp["beta2"])
        mst.add_(-(hp["lr"] * (mm / (vv.sqrt() + hp["eps"]) +
                               hp["wd"] * mst)))
    rejects(mst, want, "adamw without bias correction", **TOL_MASTER)


# ---- GPU: LayerNorm ---------------------------------------------------------

# grid cap 4096 blocks x 4 rows: N = 16384 + 37 is a second pass with a
# ragged tail (the next-row prefetch of ln_fwd_t runs, then stops)
@pytest.mark.gpu
@pytest.mark.parametrize("N,D,residual", [
    (16421, 512, False), (16421, 1024, True), (16421, 2048, True),
    (16421, 128, False), (33, 2048, False), (37, 512, True)])
def test_layernorm_fwd_scale(N, D, residual):
    x, res, gamma, beta, _, _ = ln_inputs(N, D)
    dev = ref_device(N * D)            # reference device, see module docstring
    xg, rg, gg, bg = (t.cuda() for t in (x, res, gamma, beta))
    y, s, mean, rstd = ops.hip_ops().layernorm_fwd(
        xg, rg if residual else None, gg, bg, EPS)
    xr, rr, gr, br = (t.to(dev) for t in (xg, rg, gg, bg))
    if residual:
        s_want = (xr.float() + rr.float()).to(BF16)
        assert torch.equal(s.to(dev), s_want), \
            "fused residual sum must match the bf16 add"
    else:
        s_want = xr
        assert s.data_ptr() == xg.data_ptr()
    want, mean_w, rstd_w = ref.layernorm_fwd(s_want.float(), gr.float(),
                                             br.float(), EPS)
    assert_close(y, want, "y", **TOL_LN_Y)
    assert_close(mean, mean_w, "mean", **TOL_LN_MEAN)
    assert_close(rstd, rstd_w, "rstd", **TOL_LN_RSTD)


# grid cap 1024 blocks: N = 8192 + 37 is 2 passes of the two-rows-per-wave
# template kernel (D = 512, 1024) and 3 of the general one; N is odd, so the
# last wave's row B is off on its final pass.  D = 4104 is the wide kernel
# (one workspace row per wave in global memory), at one pass with idle waves
# and at three.
@pytest.mark.gpu
@pytest.mark.parametrize("with_ds", [False, True])
@pytest.mark.parametrize("N,D", [(8229, 512), (8229, 1024), (8229, 2048),
                                 (8229, 128), (37, 4104), (2085, 4104)])
def test_layernorm_bwd_scale(N, D, with_ds):
    x, _, gamma, _, dy, ds = ln_inputs(N, D)
    dev = ref_device(N * D)
    xg, gg, dyg = x.cuda(), gamma.cuda(), dy.cuda()
    dsg = ds.cuda() if with_ds else None
    mean, rstd, dx_w, dg_w, db_w = ln_bwd_reference(
        dyg.to(dev), xg.to(dev), gg.to(dev),
        dsg.to(dev) if with_ds else None)
    # the kernel gets the reference's own statistics: this test is about the
    # backward alone
    dx, dgamma, dbeta = ops.hip_ops().layernorm_bwd(
        dyg, xg, gg, mean.cuda(), rstd.cuda(), dsg)
    assert_close(dx, dx_w, "dx", **TOL_LN_DX)
    assert_close(dgamma, dg_w, "dgamma", **tol_dparam(N))
    assert_close(dbeta, db_w, "dbeta", **tol_dparam(N))


# ---- GPU: bias + GeLU -------------------------------------------------------

def gelu_inputs(N, D):
    g = torch.Generator().manual_seed(2000 + D)
    x = torch.randn(N, D, generator=g).to(BF16)
    b = torch.randn(D, generator=g).to(BF16)
    dy = torch.randn(N, D, generator=g).to(BF16)
    return x, b, dy


# grid cap 4096 blocks x 8192 elements: (8195, 4096) is 4097.5 tiles, block
# 1's second pass is a half tile (ok[p] false for p >= 2); (4099, 8192) ends
# on a full tile in block 2
@pytest.mark.gpu
@pytest.mark.parametrize("N,D", [(8195, 4096), (4099, 8192)])
def test_bias_gelu_fwd_scale(N, D):
    x, b, _ = gelu_inputs(N, D)
    xg, bg = x.cuda(), b.cuda()
    y = ops.hip_ops().bias_gelu_fwd(xg, bg)
    want = ref.bias_gelu_fwd(xg.float(), bg.float())   # on the GPU: >= 8M
    assert_close(y, want, "y", **TOL_GELU)


# grid cap 1024 blocks: each shape is a second pass ending in a partial tile;
# D = 4096 owns its columns per thread, D = 1024 and 256 share them between
# waves (the slab merge)
@pytest.mark.gpu
@pytest.mark.parametrize("N,D", [(2051, 4096), (8195, 1024), (32771, 256)])
def test_bias_gelu_bwd_scale(N, D):
    x, b, dy = gelu_inputs(N, D)
    xg, bg, dyg = x.cuda(), b.cuda(), dy.cuda()
    dx, dbias = ops.hip_ops().bias_gelu_bwd(dyg, xg, bg)
    # on the GPU: every case is >= 8M elements
    dx_w, db_w = ref.bias_gelu_bwd(dyg.float(), xg.float(), bg.float())
    assert_close(dx, dx_w, "dx", **TOL_GELU)
    assert_close(dbias, db_w, "dbias", **tol_dbias(N))


# ---- GPU: AdamW -------------------------------------------------------------

# grid cap 2048 blocks x 1024 elements: two full passes plus 148 elements
@pytest.mark.gpu
@pytest.mark.parametrize("grad_dtype", [BF16, torch.float32],
                         ids=["bf16grad", "f32grad"])
def test_adamw_scale(grad_dtype):
    n = 4194452
    g = torch.Generator().manual_seed(6)
    master = torch.randn(n, generator=g)
    grads = torch.randn(n, generator=g).to(grad_dtype)
    p = master.to(BF16).cuda()
    mst, gg = master.cuda(), grads.cuda()
    m, v = torch.zeros(n).cuda(), torch.zeros(n).cuda()
    hp = ADAMW_HP
    for step in range(1, 4):
        ops.hip_ops().adamw_step(p, gg, m, v, mst, hp["lr"], hp["beta1"],
                                 hp["beta2"], hp["eps"], hp["wd"], step,
                                 hp["grad_scale"])
    _, m_w, v_w, mst_w = adamw_reference(master, grads, 3, **hp)  # CPU
    assert_close(mst, mst_w, "master", **TOL_MASTER)
    assert_close(m, m_w, "m", **TOL_MOMENT)
    assert_close(v, v_w, "v", **TOL_MOMENT)
    assert torch.equal(p, mst.to(BF16))


# ---- GPU: softmax -----------------------------------------------------------

# grid cap 2048 blocks x 4 rows: 3*3*928 = 8352 rows is a second pass of 160
# rows; Lk = 512 is the register path, Lk = 64 the general one
@pytest.mark.gpu
@pytest.mark.parametrize("Lk,pads", [(512, (128, 320, 8)), (64, (16, 40, 8))])
def test_softmax_scale(Lk, pads):
    B, H, Lq = 3, 3, 928
    s, dp, mask = softmax_inputs(B, H, Lq, Lk, pads, seed=7)
    scale = 1.0 / math.sqrt(64)
    sg = s.cuda()
    p = ops.hip_ops().softmax_fwd(sg, mask.cuda(), scale)
    want = ref.softmax_fwd(s.float(), mask, scale)               # CPU
    assert_close(p, want, "p", **TOL_SOFTMAX)
    for b, pad in enumerate(pads):
        assert bool((p[b, :, :, Lk - pad:] == 0).all()), b
        assert bool((p[b, :, :, :Lk - pad] > 0).any())
    ds = ops.hip_ops().softmax_bwd(dp.cuda(), p, scale)
    dwant = ref.softmax_bwd(dp.float(), p.float().cpu(), scale)  # CPU
    assert_close(ds, dwant, "ds", **TOL_SOFTMAX)
    for b, pad in enumerate(pads):
        assert bool((ds[b, :, :, Lk - pad:] == 0).all()), b


# ---- GPU: pools -------------------------------------------------------------

# the backward's grid is capped at 2048 rows: 5 * 520 = 2600 loops
@pytest.mark.gpu
def test_masked_pool_scale():
    g = torch.Generator().manual_seed(8)
    B, L, D = 5, 520, 128
    x = torch.randn(B, L, D, generator=g).to(BF16)
    dp = torch.randn(B, D, generator=g).to(BF16)
    mask = torch.zeros(B, L, dtype=torch.bool)
    for b, n in enumerate((520, 1, 37, 300, 519)):
        mask[b, :n] = True
    mg = mask.cuda()
    pooled, counts = ops.hip_ops().masked_pool_fwd(x.cuda(), mg)
    want, counts_w, bwd = pool_reference(x, mask)                # CPU
    assert_close(pooled, want, "pooled", **TOL_POOL)
    assert torch.equal(counts.cpu(), counts_w)
    dx = ops.hip_ops().masked_pool_bwd(dp.cuda(), mg, counts, L)
    assert_close(dx, bwd(dp), "dx", **TOL_POOL)
    assert bool((dx[~mg] == 0).all())


# D = 2304 is a second d0 iteration for threads 0..31; L = 50 leaves the
# last 3 of the 16 sequence splits empty
@pytest.mark.gpu
def test_masked_pool_no_mask_wide():
    g = torch.Generator().manual_seed(9)
    B, L, D = 2, 50, 2304
    x = torch.randn(B, L, D, generator=g).to(BF16)
    dp = torch.randn(B, D, generator=g).to(BF16)
    pooled, counts = ops.hip_ops().masked_pool_fwd(x.cuda(), None)
    want, counts_w, bwd = pool_reference(x, None)                # CPU
    assert_close(pooled, want, "pooled", **TOL_POOL)
    assert torch.equal(counts.cpu(), counts_w)
    dx = ops.hip_ops().masked_pool_bwd(dp.cuda(), None, counts, L)
    assert_close(dx, bwd(dp), "dx", **TOL_POOL)


# the backward's grid is capped at 2048 positions
@pytest.mark.gpu
def test_segment_mean_pool_scale():
    from tosem2021_amd.data.packing import pack_examples
    g = torch.Generator().manual_seed(10)
    D, row_len = 128, 256
    lens = torch.randint(1, row_len + 1, (48,), generator=g).tolist()
    pb = pack_examples([torch.randint(8, 500, (n,), generator=g).tolist()
                        for n in lens], row_len)
    T = pb.n_positions
    assert T > 2048 and pb.n_segments == 48
    x = torch.randn(T, D, generator=g).to(BF16)
    dp = torch.randn(48, D, generator=g).to(BF16)
    dev = pb.to("cuda")
    xg = x.cuda().requires_grad_()
    pooled = ops.segment_mean_pool(xg, dev.seg_start, dev.seg_len,
                                   dev.pos2seg)
    pooled.backward(dp.cuda())
    want = ref.segment_pool_fwd(x.float(), pb.seg_start, pb.seg_len,
                                pb.pos2seg)                      # CPU
    dx_w = ref.segment_pool_bwd(dp.float(), pb.seg_len, pb.pos2seg)
    assert_close(pooled.detach(), want, "pooled", **TOL_POOL)
    assert_close(xg.grad, dx_w, "dx", **TOL_POOL)
    pad = (pb.pos2seg < 0).cuda()
    assert bool(pad.any()) and bool((xg.grad[pad] == 0).all())


# ---- GPU: reproducibility at the config widths ------------------------------
# All six cases differed from launch to launch while these widths merged
# their per-wave partials with LDS float atomics (docs/PERF.md).

def assert_reproducible(fn, launches=5):
    first = fn()
    for i in range(1, launches):
        for a, b in zip(first, fn()):
            assert torch.equal(a, b), f"launch {i} differs from launch 0"


@pytest.mark.gpu
@pytest.mark.parametrize("with_ds", [False, True])
@pytest.mark.parametrize("D", [128, 2048])
def test_layernorm_bwd_reproducible(D, with_ds):
    N = 8229
    x, _, gamma, _, dy, ds = ln_inputs(N, D)
    xg, gg, dyg = x.cuda(), gamma.cuda(), dy.cuda()
    dsg = ds.cuda() if with_ds else None
    mean, rstd, _, _, _ = ln_bwd_reference(dyg, xg, gg, None)
    assert_reproducible(
        lambda: ops.hip_ops().layernorm_bwd(dyg, xg, gg, mean, rstd, dsg))


@pytest.mark.gpu
@pytest.mark.parametrize("N,D", [(32771, 256), (8195, 1024)])
def test_bias_gelu_bwd_reproducible(N, D):
    x, b, dy = gelu_inputs(N, D)
    xg, bg, dyg = x.cuda(), b.cuda(), dy.cuda()
    assert_reproducible(lambda: ops.hip_ops().bias_gelu_bwd(dyg, xg, bg))
