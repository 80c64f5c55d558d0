"""Dropout on the attention probabilities inside the flash kernels
(csrc/flash_attn.hip, DROP instantiations) against reference.attn_dropout_keep
and the fp32 reference.

(B, H, L, p) — the smallest shapes at which the tile indexing can break:

  (1, 1, 32, .1)    one tile, less than a workgroup
  (2, 3, 64, .1)    bh indexing
  (2, 2, 96, .5)
  (2, 2, 160, .25)  second 128-row kv workgroup of flash_bwd_fused
  (1, 2, 288, .1)   second 256-row q workgroup, third kv workgroup

A tolerance cannot see a wrong mask bit (one bit moves dV by about 1/L), so
each kernel's mask is READ OUT exactly, 64 key (or query) columns at a time,
with inputs that turn one output element into one probability:

  forward       Q = 0, V[k, d] = 1 where d == k % 64 inside the chunk:
                O[q, d] = keep[q, 64c + d] * scale / L
  bwd_fused     Q = 0, V = 0, dO[q, d] = 1 where d == q % 64 inside the
                chunk: dV[k, d] = keep[64c + d, k] * scale / L
  dq_recompute  Q = 0, K one-hot per chunk, V[:, 0] = 1, dO = 1:
                dQ[q, d] = softmax_scale / L * (keep[q, 64c + d] * scale -
                D_q), classified against the midpoint with scale / 2, D_q
                taken from the forward's own O

The numeric checks use the tolerances of tests/test_packing_gpu.py's trio
check (o 3e-2 / 3e-2, gradients 5e-2 / 3e-2) with the absolute term times
the dropout scale, as tests/test_fused_dropout_gpu.py scales dres's.
"""
import copy
import dataclasses
import functools

import pytest
import torch

from test_ops_gpu_scale import BF16, assert_reproducible
from tosem2021_amd import ops
from tosem2021_amd.data.synthetic import synthetic_batch
from tosem2021_amd.models.classifier import MLTC, MLTCConfig
from tosem2021_amd.ops import reference as ref

pytestmark = pytest.mark.gpu

SEED, CALL, LAYER = (5 << 32) + 1234, 3, 1    # a seed with both key words set
SCALE = 0.125
CASES = [(1, 1, 32, 0.1), (2, 3, 64, 0.1), (2, 2, 96, 0.5),
         (2, 2, 160, 0.25), (1, 2, 288, 0.1)]


@functools.lru_cache(maxsize=None)
def keep_mask(B, H, L, p, seed=SEED, call=CALL, layer=LAYER):
    return ref.attn_dropout_keep(B, H, L, p, seed, call, layer)


def words(p, seed=SEED, call=CALL, layer=LAYER):
    """The bindings' keyword arguments."""
    return dict(drop_seed=seed, drop_call=call,
                drop_site=ref.ATTN_DROPOUT_SITE0 + layer,
                drop_thr=ref.attn_dropout_threshold(p)[0])


def dscale(p):
    return ref.attn_dropout_threshold(p)[1]


def zeros(B, H, L):
    return torch.zeros(B, H, L, 64, dtype=BF16, device="cuda")


def chunks(L):
    return [(c, min(64, L - c)) for c in range(0, L, 64)]


def assert_mask(got, B, H, L, p, what):
    want = keep_mask(B, H, L, p)
    wrong = int((got.cpu() != want).sum())
    assert wrong == 0, f"{what}: {wrong} of {want.numel()} mask bits differ"
    assert 0 < int((~want).sum()) < want.numel()


# ---- the mask of each kernel, bit by bit ------------------------------------

@pytest.mark.parametrize("B,H,L,p", CASES)
def test_forward_mask_readout(B, H, L, p):
    q = zeros(B, H, L)
    got = torch.zeros(B, H, L, L, dtype=torch.bool, device="cuda")
    kept = dscale(p) / L
    for c, n in chunks(L):
        v = zeros(B, H, L)
        idx = torch.arange(n, device="cuda")
        v[:, :, c + idx, idx] = 1
        o = ops.flash_attention(q, q, v, None, SCALE,
                                dropout=(p, SEED, CALL, LAYER)).float()
        got[..., c:c + n] = o[..., :n] != 0
        if n < 64:
            assert float(o[..., n:].abs().max()) == 0
        nz = o[..., :n][o[..., :n] != 0]
        assert torch.allclose(nz, torch.full_like(nz, kept), rtol=2e-2,
                              atol=0), "a kept probability is scale / L"
    assert_mask(got, B, H, L, p, "flash_fwd")


@pytest.mark.parametrize("B,H,L,p", CASES)
def test_bwd_fused_mask_readout(B, H, L, p):
    got = torch.zeros(B, H, L, L, dtype=torch.bool, device="cuda")
    for c, n in chunks(L):
        q = zeros(B, H, L)
        v = zeros(B, H, L).requires_grad_(True)
        do = zeros(B, H, L)
        idx = torch.arange(n, device="cuda")
        do[:, :, c + idx, idx] = 1
        o = ops.flash_attention(q, q, v, None, SCALE,
                                dropout=(p, SEED, CALL, LAYER))
        o.backward(do)
        dv = v.grad.float()                  # [k, d] = Pd[c + d, k]
        got[:, :, c:c + n, :] = (dv[..., :n] != 0).transpose(-1, -2)
        if n < 64:
            assert float(dv[..., n:].abs().max()) == 0
    assert_mask(got, B, H, L, p, "flash_bwd_fused")


@pytest.mark.parametrize("B,H,L,p", CASES)
def test_dq_recompute_mask_readout(B, H, L, p):
    got = torch.zeros(B, H, L, L, dtype=torch.bool, device="cuda")
    v = zeros(B, H, L)
    v[..., 0] = 1
    do = torch.ones(B, H, L, 64, dtype=BF16, device="cuda")
    for c, n in chunks(L):
        q = zeros(B, H, L).requires_grad_(True)
        k = zeros(B, H, L)
        idx = torch.arange(n, device="cuda")
        k[:, :, c + idx, idx] = 1
        o = ops.flash_attention(q, k, v, None, SCALE,
                                dropout=(p, SEED, CALL, LAYER))
        o.backward(do)
        d_q = o.detach().float()[..., :1]     # D = rowsum(dO * O) = O[:, 0]
        mid = SCALE / L * (dscale(p) / 2 - d_q)
        got[..., c:c + n] = q.grad.float()[..., :n] > mid
    assert_mask(got, B, H, L, p, "flash_dq_recompute")


# ---- numerics against the fp32 reference under the reference mask -----------

def trio(q, k, v, do, p, mask=None, seg=None, skip=True, **kw):
    ext = ops.hip_ops()
    w = words(p, **kw) if p else {}
    o, lse = ext.flash_fwd(q, k, v, mask, SCALE, seg=seg, **w)
    ddot, dead = ext.fa_dot_flags(do, o)
    if not skip:
        dead = None
    dk, dv = ext.flash_bwd_fused(q, k, v, do, mask, lse, ddot, SCALE,
                                 seg=seg, dead=dead, **w)
    dq = ext.flash_dq_recompute(q, k, v, do, mask, lse, ddot, SCALE, seg=seg,
                                dead=dead, **w)
    return o, lse, dq, dk, dv


def reference(q, k, v, do, keep_scale, mask=None, seg=None):
    """fp32, every position: O = Pd V with Pd = keep * scale * P, and
    dS = SCALE * P * (keep * scale * dP - rowsum(dO * O))."""
    qf, kf, vf, dof = (t.float().cpu() for t in (q, k, v, do))
    s = torch.matmul(qf, kf.transpose(-1, -2)) * SCALE
    if mask is not None:
        s = s + mask.cpu().view(mask.shape[0], 1, 1, -1)
    if seg is not None:
        s = s + ref.segment_bias(seg.cpu())
    p = torch.softmax(s, dim=-1)
    pd = p * keep_scale
    o = torch.matmul(pd, vf)
    dp = torch.matmul(dof, vf.transpose(-1, -2)) * keep_scale
    dd = (dof * o).sum(-1, keepdim=True)
    ds = SCALE * p * (dp - dd)
    return (o, torch.matmul(ds, kf), torch.matmul(ds.transpose(-1, -2), qf),
            torch.matmul(pd.transpose(-1, -2), dof))


def inputs(B, H, L, seed=40):
    g = torch.Generator().manual_seed(seed)
    return [torch.randn(B, H, L, 64, generator=g).to(BF16).cuda()
            for _ in range(4)]


def check_numerics(B, H, L, p, mask=None, seg=None):
    q, k, v, do = inputs(B, H, L)
    o, lse, dq, dk, dv = trio(q, k, v, do, p, mask, seg)
    _, lse0 = ops.hip_ops().flash_fwd(q, k, v, mask, SCALE, seg=seg)
    assert torch.equal(lse, lse0), "lse is the undropped softmax's"
    s = dscale(p)
    want = reference(q, k, v, do, keep_mask(B, H, L, p).float() * s, mask,
                     seg)
    tols = [("o", 3e-2, 3e-2)] + [(n, 5e-2, 3e-2) for n in ("dq", "dk", "dv")]
    for (name, atol, rtol), got, w in zip(tols, (o, dq, dk, dv), want):
        err = float((got.float().cpu() - w).abs().max())
        print(f"{name}: max|err| {err:.3e}")
        assert torch.allclose(got.float().cpu(), w, atol=atol * s,
                              rtol=rtol), f"{name}: max|err| {err:.3e}"
    return o, lse, dq, dk, dv


@pytest.mark.parametrize("B,H,L,p", CASES)
def test_trio_vs_reference(B, H, L, p):
    check_numerics(B, H, L, p)


def test_trio_with_padding_mask():
    """70 real tokens of 160: the tail kv tiles are skipped in all three
    kernels, and the mask of the tiles that run is still indexed right."""
    B, H, L, p = 2, 2, 160, 0.25
    mask = torch.zeros(B, L, dtype=torch.float32, device="cuda")
    mask[:, 70:] = -1e9
    check_numerics(B, H, L, p, mask=mask)


def test_trio_with_segments():
    """Two segments and the pad segment per row; segment edges off the tile
    grid, so tiles start above 0 and are skipped per wave."""
    B, H, L, p = 2, 2, 160, 0.25
    seg = torch.zeros(B, L, dtype=torch.int32)
    seg[0, 50:110], seg[0, 110:] = 1, 2
    seg[1, 100:130], seg[1, 130:] = 1, 2
    ops.check_segments(seg)
    check_numerics(B, H, L, p, seg=seg.cuda())


@pytest.mark.parametrize("B,H,L,p", CASES[1:])
def test_dead_query_tile_skip_is_exact(B, H, L, p):
    q, k, v, do = inputs(B, H, L)
    do[:, :, 32:64] = 0                      # a dead tile in every (b, h)
    do[0, 0, :32] = 0
    a = trio(q, k, v, do, p, skip=True)
    b = trio(q, k, v, do, p, skip=False)
    for name, x, y in zip(("o", "lse", "dq", "dk", "dv"), a, b):
        assert torch.equal(x, y), name
    assert float(a[2][:, :, 32:64].abs().max()) == 0


@pytest.mark.parametrize("B,H,L,p", CASES)
def test_packed_equals_bhld(B, H, L, p):
    D = H * 64
    g = torch.Generator().manual_seed(41)
    qkv = torch.randn(B, L, 3 * D, generator=g).to(BF16).cuda()
    gout = torch.randn(B, L, D, generator=g).to(BF16).cuda()
    drop = (p, SEED, CALL, LAYER)
    a = qkv.clone().requires_grad_(True)
    oa = ops.flash_attention_packed(a, H, None, SCALE, dropout=drop)
    oa.backward(gout)
    q, k, v = (t.view(B, L, H, 64).transpose(1, 2).contiguous()
               .requires_grad_(True) for t in qkv.split(D, dim=-1))
    ob = ops.flash_attention(q, k, v, None, SCALE, dropout=drop)
    ob.backward(gout.view(B, L, H, 64).transpose(1, 2).contiguous())
    assert torch.equal(oa, ob.transpose(1, 2).reshape(B, L, D))
    gb = torch.cat([t.grad.transpose(1, 2).reshape(B, L, D)
                    for t in (q, k, v)], dim=-1)
    assert torch.equal(a.grad, gb)


@pytest.mark.parametrize("B,H,L,p", [CASES[1], CASES[4]])
def test_reproducible(B, H, L, p):
    q, k, v, do = inputs(B, H, L)
    assert_reproducible(lambda: trio(q, k, v, do, p))


@pytest.mark.parametrize("B,H,L,p", [CASES[1], CASES[4]])
def test_every_word_changes_the_mask(B, H, L, p):
    q, k, v, do = inputs(B, H, L)
    base = trio(q, k, v, do, p)
    for other in (dict(seed=SEED + 1), dict(seed=SEED + (1 << 32)),
                  dict(call=CALL + 1), dict(layer=LAYER + 1)):
        got = trio(q, k, v, do, p, **other)
        assert torch.equal(got[1], base[1]), "lse"
        for name, x, y in zip(("o", "dq", "dk", "dv"),
                              got[:1] + got[2:], base[:1] + base[2:]):
            assert not torch.equal(x, y), (other, name)


@pytest.mark.parametrize("B,H,L,p", CASES)
def test_p_zero_is_todays_call(B, H, L, p):
    q, k, v, do = inputs(B, H, L)
    outs = []
    for kw in ({}, dict(dropout=(0.0, SEED, CALL, LAYER)),
               dict(dropout=None)):
        leaves = [t.clone().requires_grad_(True) for t in (q, k, v)]
        o = ops.flash_attention(*leaves, None, SCALE, **kw)
        o.backward(do)
        outs.append([o.detach()] + [t.grad for t in leaves])
    for other in outs[1:]:
        for x, y in zip(outs[0], other):
            assert torch.equal(x, y)
    # and the bindings' thr = 0 is the launch without the words
    a = trio(q, k, v, do, 0)
    ext = ops.hip_ops()
    o, lse = ext.flash_fwd(q, k, v, None, SCALE, drop_seed=SEED, drop_call=9,
                           drop_site=5, drop_thr=0)
    assert torch.equal(o, a[0]) and torch.equal(lse, a[1])
    assert torch.equal(o, outs[0][0])


def test_binding_validation():
    ext = ops.hip_ops()
    B, H, L = 1, 1, 32
    q, k, v, do = inputs(B, H, L)
    o, lse = ext.flash_fwd(q, k, v, None, SCALE)
    ddot = ext.fa_dot(do, o)
    with pytest.raises(RuntimeError, match="emit_ds"):
        ext.flash_bwd_fused(q, k, v, do, None, lse, ddot, SCALE, True,
                            **words(0.1))
    with pytest.raises(RuntimeError, match="threshold"):
        ext.flash_fwd(q, k, v, None, SCALE, drop_thr=256)
    with pytest.raises(ValueError):
        ops.flash_attention(q, k, v, None, SCALE, dropout=(1.0, 0, 0, 0))
    qkv = torch.zeros(B, L, 3 * 64, dtype=BF16, device="cuda")
    bias = torch.zeros(3 * 64, dtype=BF16, device="cuda", requires_grad=True)
    with pytest.raises(ValueError, match="qkv_bias"):
        ops.flash_attention_packed(qkv, H, None, SCALE, qkv_bias=bias,
                                   dropout=(0.1, 0, 0, 0))


# ---- model ------------------------------------------------------------------

CFG = MLTCConfig(vocab_size=512, d_model=128, n_heads=2, n_layers=2,
                 d_ff=256, max_seq=64, attn_dropout=0.1, dropout_seed=3)


def test_model_training_forward_vs_fp32_cpu():
    """Training-mode logits, GPU (bf16, flash kernels) against the CPU model
    (f32, reference mask), within the 0.05 of
    test_model_packed_and_unpacked_vs_fp32_cpu: possible only because both
    sides draw the same masks."""
    torch.manual_seed(0)
    model = MLTC(CFG).to(BF16).float().train()    # bf16-representable weights
    tokens, mask, _ = synthetic_batch(CFG, 4, 64, seed=7)
    out_cpu = model(tokens, mask)
    gm = copy.deepcopy(model).to(BF16).cuda().train()
    gm.dropout_call = 0
    out_gpu = gm(tokens.cuda(), mask.cuda())
    assert gm.dropout_call == model.dropout_call == 1
    for k in out_cpu:
        a, b = out_gpu[k].float().cpu(), out_cpu[k]
        assert torch.allclose(a, b, atol=0.05, rtol=0.05), \
            f"{k}: max diff {(a - b).abs().max()}"
    # the masks matter at this tolerance's scale or not, they do change bits
    gm.eval()
    out_eval = gm(tokens.cuda(), mask.cuda())
    assert any(not torch.equal(out_eval[k], out_gpu[k]) for k in out_gpu)


def test_model_backward_runs_and_counts():
    torch.manual_seed(0)
    gm = MLTC(CFG).to(BF16).cuda().train()
    tokens, mask, labels = synthetic_batch(CFG, 4, 64, device="cuda", seed=7)
    gm.loss(gm(tokens, mask), labels).backward()
    assert gm.dropout_call == 1
    for name, p in gm.named_parameters():
        assert p.grad is not None and bool(torch.isfinite(p.grad).all()), name


@pytest.mark.parametrize("over,L", [(dict(n_heads=4), 64), (dict(), 48)])
def test_off_lattice_shapes_raise_on_gpu(over, L):
    cfg = dataclasses.replace(CFG, **over)
    gm = MLTC(cfg).to(BF16).cuda().train()
    tokens, mask, _ = synthetic_batch(cfg, 2, L, device="cuda", seed=7)
    with pytest.raises(RuntimeError, match="attention dropout on the GPU"):
        gm(tokens, mask)
    gm.eval()
    gm(tokens, mask)                        # inactive in eval: today's path
