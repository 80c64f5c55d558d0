"""Flash backward: skipping query tiles whose output gradient is all +-0.

fa_dot writes one flag per (b, h, 32-row query tile) next to ddot: dead iff
every one of the tile's 32 x 64 dO elements has (bits & 0x7fff) == 0.  For
such a tile dP, D and dS are exact zeros, so it adds nothing to dK and dV and
its dQ rows are zero: flash_bwd_fused and flash_dq_recompute leave it out, and
the result is bitwise what the unskipped kernels give (finite inputs).

Every case here therefore asserts torch.equal between the skip run and the
run without it, in both geometries ([B, H, L, 64] and packed), with the folded
bias gradient, and additionally checks the skip run against the fp32 reference
with the tolerances tests/test_ops_gpu.py uses for the flash backward
(atol 5e-2, rtol 3e-2).

Shapes: B 2, H 2, dh 64, L 512 (flash_dq_recompute has two workgroups per
head, flash_bwd_fused four); L 96 covers the partial last workgroup.  The dO
patterns at L 512 and what they drive in flash_dq_recompute (workgroup 0 owns
tiles 0..7, wave w tiles w and 4 + w):
  tail256   workgroup 1 wholly dead: zero rows stored, no K/V load
  tail200   tile 7 dead: one block of wave 3 dead (runs, adds exact zeros)
  tail96    tiles 3..7 dead: wave 3 has both blocks dead (wave skip)
  interior  tile 2 (rows 64..95) dead with live tiles after it
  head0     every tile of head 0 dead, head 1 live
  one_bit   all zero but a single 0x0001 element: its tile must stay live
  negzero   tile 4 all 0x8000 (-0.0): dead
  zero      everything dead
"""
import functools

import pytest
import torch

from tosem2021_amd import ops
from tosem2021_amd.data.synthetic import synthetic_batch
from tosem2021_amd.models.classifier import MLTCConfig, build_model
from tosem2021_amd.ops import reference

pytestmark = pytest.mark.gpu

BF16 = torch.bfloat16
B, H, SCALE = 2, 2, 0.125
TOL = dict(atol=5e-2, rtol=3e-2)     # tests/test_ops_gpu.py, flash backward

PATTERNS = ("random", "tail256", "tail200", "tail96", "interior", "head0",
            "one_bit", "negzero", "zero")


def _packed(t):
    """[B, H, L, 64] -> [B, L, H * 64]"""
    return t.transpose(1, 2).reshape(t.shape[0], t.shape[2], -1).contiguous()


@functools.lru_cache(maxsize=None)
def _inputs(L):
    g = torch.Generator(device="cpu").manual_seed(1234 + L)
    q, k, v, do = (torch.randn(B, H, L, 64, generator=g).to(BF16).cuda()
                   for _ in range(4))
    qkv = torch.cat([_packed(t) for t in (q, k, v)], dim=-1).contiguous()
    return q, k, v, qkv, do


def _do(name, L=512):
    do = _inputs(L)[4].clone()
    bits = do.view(torch.int16)
    if name == "random":
        pass
    elif name.startswith("tail"):
        do[:, :, int(name[4:]):] = 0
    elif name == "interior":
        do[:, :, 64:96] = 0
    elif name == "head0":
        do[:, 0] = 0
    elif name == "one_bit":
        do.zero_()
        bits[1, 0, 300, 17] = 1                 # 0x0001, the smallest subnormal
    elif name == "negzero":
        bits[:, :, 128:160] = -32768            # 0x8000
    elif name == "zero":
        do.zero_()
    else:
        raise KeyError(name)
    return do


def _mask(name, L=512):
    if name == "none":
        return None
    m = torch.zeros(B, L, device="cuda")
    m[0, int(name[3:]):] = -1e9                  # row 1 stays unpadded
    return m.contiguous()


def _ddot_formula(do, o):
    """The kernel's sum, order included: 16 lanes x 4 elements per row, each
    lane adds its four products in order (a bf16 x bf16 product is exact in
    f32, so fused or not is the same number), then a 16-lane xor butterfly
    (8, 4, 2, 1)."""
    p = (do.float() * o.float()).view(*do.shape[:-1], 16, 4)
    s = torch.zeros_like(p[..., 0])
    for j in range(4):
        s = s + p[..., j]
    idx = torch.arange(16, device=do.device)
    for off in (8, 4, 2, 1):
        s = s + s[..., idx ^ off]
    return s[..., 0]


def _reference(q, k, v, do, o, lse, mask, seg):
    """fp32 dq, dk, dv as tests/test_ops_gpu.py forms them (the kernel's lse
    and o, everything else in f32)."""
    s = torch.matmul(q.float(), k.float().transpose(-1, -2)) * SCALE
    if mask is not None:
        s = s + mask.view(B, 1, 1, -1)
    if seg is not None:
        same = seg[:, :, None] == seg[:, None, :]
        s = s + torch.where(same, 0.0, -1e9)[:, None].float()
    p = torch.exp(s - lse.unsqueeze(-1))
    dd = (do.float() * o.float()).sum(-1)
    dp = torch.matmul(do.float(), v.float().transpose(-1, -2))
    ds = SCALE * p * (dp - dd.unsqueeze(-1))
    return (torch.matmul(ds, k.float()),
            torch.matmul(ds.transpose(-1, -2), q.float()),
            torch.matmul(p.transpose(-1, -2), do.float()))


def _close(got, want, what):
    err = float((got.float() - want).abs().max())
    print(f"{what}: max abs err {err:.3e}")
    assert torch.allclose(got.float(), want, **TOL), f"{what}: {err}"


def _check(L, do, mask=None, seg=None):
    """Flags, ddot and the skip-vs-no-skip equality in both geometries, the
    folded bias gradient, and the skip run against the fp32 reference.
    Returns the dead flags."""
    ext = ops.hip_ops()
    q, k, v, qkv, _ = _inputs(L)
    want_dead = reference.dead_q_tiles(do)

    # ---- [B, H, L, 64] ----
    o, lse = ext.flash_fwd(q, k, v, mask, SCALE, seg)
    ddot, dead = ext.fa_dot_flags(do, o)
    assert dead.dtype == torch.bool and dead.shape == (B, H, L // 32)
    assert torch.equal(dead, want_dead)
    assert torch.equal(ddot, _ddot_formula(do, o))
    assert torch.equal(ext.fa_dot(do, o), ddot)
    dk0, dv0 = ext.flash_bwd_fused(q, k, v, do, mask, lse, ddot, SCALE,
                                   False, seg)
    dq0 = ext.flash_dq_recompute(q, k, v, do, mask, lse, ddot, SCALE, seg)
    dk1, dv1 = ext.flash_bwd_fused(q, k, v, do, mask, lse, ddot, SCALE,
                                   False, seg, dead)
    dq1 = ext.flash_dq_recompute(q, k, v, do, mask, lse, ddot, SCALE, seg,
                                 dead)
    for n, a, b in (("dq", dq1, dq0), ("dk", dk1, dk0), ("dv", dv1, dv0)):
        assert torch.equal(a, b), f"{n} differs with the skip ([B, H, L, 64])"
    ref = _reference(q, k, v, do, o, lse, mask, seg)
    for n, a, r in zip(("dq", "dk", "dv"), (dq1, dk1, dv1), ref):
        _close(a, r, n)

    # ---- packed ----
    do_p = _packed(do)
    o_p, lse_p = ext.flash_fwd_packed(qkv, H, mask, SCALE, seg)
    ddot_p, dead_p = ext.fa_dot_packed_flags(do_p, o_p, H)
    assert torch.equal(dead_p, reference.dead_q_tiles(do_p, H))
    assert torch.equal(dead_p, want_dead)
    o4 = o_p.view(B, L, H, 64).transpose(1, 2)
    assert torch.equal(ddot_p, _ddot_formula(do, o4))
    g0 = ext.flash_bwd_packed(qkv, o_p, do_p, mask, lse_p, H, SCALE, seg,
                              skip_zero_do=False)
    g1 = ext.flash_bwd_packed(qkv, o_p, do_p, mask, lse_p, H, SCALE, seg)
    assert torch.equal(g1, g0), "dqkv differs with the skip (packed)"
    ref_p = _reference(q, k, v, do, o4, lse_p, mask, seg)
    for n, a, r in zip(("dq", "dk", "dv"), g1.split(H * 64, dim=-1), ref_p):
        _close(a.reshape(B, L, H, 64).transpose(1, 2), r, n + " packed")
    gb0, bias0 = ext.flash_bwd_packed_bias(qkv, o_p, do_p, mask, lse_p, H,
                                           SCALE, seg, skip_zero_do=False)
    gb1, bias1 = ext.flash_bwd_packed_bias(qkv, o_p, do_p, mask, lse_p, H,
                                           SCALE, seg)
    assert torch.equal(gb0, g0) and torch.equal(gb1, g0)
    assert torch.equal(bias1, bias0), "folded qkv bias gradient differs"
    return dead


@pytest.mark.parametrize("pattern", PATTERNS)
def test_patterns(pattern):
    dead = _check(512, _do(pattern))
    n_dead = int(dead.sum())
    want = {"random": 0, "tail256": 32, "tail200": 36, "tail96": 52,
            "interior": 4, "head0": 32, "one_bit": 63, "negzero": 4,
            "zero": 64}[pattern]
    assert n_dead == want
    if pattern == "one_bit":
        assert not bool(dead[1, 0, 300 // 32])


@pytest.mark.parametrize("mask", ["none", "pad128", "pad320"])
def test_mask_length_differs_from_live_length(mask):
    """dO lives in rows 0..199; the key padding starts before (128), after
    (320) or nowhere.  The skip follows dO, never the mask."""
    _check(512, _do("tail200"), mask=_mask(mask))


def test_segmented_with_dead_middle_segment():
    """Four segments per row; dO of the second one (rows 150..299) is zero,
    so tiles 5..8 are dead in the middle of the q range every kv workgroup
    of segments 1 and 2 walks."""
    L = 512
    seg = torch.zeros(B, L, dtype=torch.int32, device="cuda")
    seg[:, 150:] = 1
    seg[:, 300:] = 2
    seg[:, 450:] = 3
    do = _do("random")
    do[:, :, 150:300] = 0
    dead = _check(L, do, seg=seg.contiguous())
    assert dead[0, 0].nonzero().flatten().tolist() == [5, 6, 7, 8]


@pytest.mark.parametrize("live_rows", [96, 40, 0])
def test_partial_last_workgroup(live_rows):
    """L 96: one flash_dq_recompute workgroup with five of its eight tiles
    past L, a fused-backward workgroup with one empty wave."""
    L = 96
    do = _inputs(L)[4].clone()
    do[:, :, live_rows:] = 0
    mask = torch.zeros(B, L, device="cuda")
    mask[1, 70:] = -1e9
    _check(L, do, mask=mask.contiguous())


def test_emit_ds_ignores_the_flags():
    """The A/B path must write every dS tile: with emit_ds the flags are
    ignored and ds, dk, dv are what the call without flags returns."""
    ext = ops.hip_ops()
    q, k, v, _, _ = _inputs(512)
    do = _do("tail96")
    mask = _mask("pad320")
    o, lse = ext.flash_fwd(q, k, v, mask, SCALE)
    ddot, dead = ext.fa_dot_flags(do, o)
    assert int(dead.sum()) > 0
    want = ext.flash_bwd_fused(q, k, v, do, mask, lse, ddot, SCALE,
                               emit_ds=True)
    got = ext.flash_bwd_fused(q, k, v, do, mask, lse, ddot, SCALE,
                              emit_ds=True, dead=dead)
    assert len(got) == 3
    for n, a, b in zip(("ds", "dk", "dv"), got, want):
        assert torch.equal(a, b), n
    dq = ext.flash_dq(got[0], k)
    dq_r = ext.flash_dq_recompute(q, k, v, do, mask, lse, ddot, SCALE,
                                  dead=dead)
    assert bool((dq[:, :, 96:] == 0).all()) and bool((dq_r[:, :, 96:] == 0).all())


def test_flags_shape_is_checked():
    ext = ops.hip_ops()
    q, k, v, _, do = _inputs(96)
    o, lse = ext.flash_fwd(q, k, v, None, SCALE)
    ddot, dead = ext.fa_dot_flags(do, o)
    with pytest.raises(RuntimeError):
        ext.flash_dq_recompute(q, k, v, do, None, lse, ddot, SCALE,
                               dead=dead[:, :, :2].contiguous())
    with pytest.raises(RuntimeError):
        ext.flash_bwd_fused(q, k, v, do, None, lse, ddot, SCALE,
                            dead=dead.to(torch.uint8))


def test_model_gradients_equal_and_padded_tiles_dead(monkeypatch):
    """One forward and backward of a 2-layer model on a padded batch with the
    knob on and off: every gradient is bitwise equal.  A hook on each
    attention output checks the premise the gain rests on: the gradient
    reaching a padded query row is exactly zero in every layer, so every tile
    wholly past a row's length is flagged dead."""
    cfg = MLTCConfig(vocab_size=512, d_model=128, n_heads=2, n_layers=2,
                     d_ff=256, max_seq=64)
    L = 64
    torch.manual_seed(7)
    model = build_model(cfg).cuda()
    tokens, _, labels = synthetic_batch(cfg, 4, L, device="cuda")
    lengths = torch.tensor([20, 64, 32, 5], device="cuda")
    attn_mask = torch.arange(L, device="cuda")[None, :] < lengths[:, None]
    first_past = [(int(n) + 31) // 32 for n in lengths]

    seen = []
    real = ops.flash_attention_packed

    def hooked(qkv, n_heads, *args, **kw):
        out = real(qkv, n_heads, *args, **kw)

        def check(grad):
            dead = reference.dead_q_tiles(grad.contiguous(), n_heads)
            for b, t0 in enumerate(first_past):
                assert bool(dead[b, :, t0:].all()), \
                    f"row {b}: a tile past its length has a nonzero gradient"
            seen.append(int(dead.sum()))
        out.register_hook(check)
        return out

    monkeypatch.setattr(ops, "flash_attention_packed", hooked)

    def grads(skip):
        monkeypatch.setattr(ops, "_FLASH_QSKIP", skip)
        model.zero_grad(set_to_none=True)
        loss = model.loss(model(tokens, attn_mask), labels)
        loss.backward()
        return float(loss.detach()), {n: p.grad.clone()
                             for n, p in model.named_parameters()}

    loss_on, g_on = grads(True)
    loss_off, g_off = grads(False)
    # rows 0, 2 and 3 each have one tile wholly past their length
    assert len(seen) == 2 * cfg.n_layers and min(seen) >= 3 * cfg.n_heads
    assert loss_on == loss_off
    assert g_on.keys() == g_off.keys()
    for n in g_on:
        assert torch.equal(g_on[n], g_off[n]), n
    assert any(float(g.float().abs().sum()) > 0 for g in g_on.values())
