"""GPU numerics: each gfx950 HIP kernel vs the plain-PyTorch fp32 reference.

Every test compares the hand-written kernel (bf16 storage, f32 math) against
the same op computed in fp32 by reference.py; tolerances are bf16-rounding
sized.  Marked gpu — the driver runs these on a real MI355X.
"""
import math

import pytest
import torch

pytestmark = pytest.mark.gpu

from tosem2021_amd import ops
from tosem2021_amd.ops import reference as ref


def _bf16(x):
    return x.to(torch.bfloat16).cuda().contiguous()


@pytest.mark.parametrize("N,D", [(64, 1024), (257, 512), (32, 4096), (128, 136)])
def test_layernorm_fwd(N, D):
    torch.manual_seed(0)
    x = torch.randn(N, D)
    g = torch.randn(D)
    b = torch.randn(D)
    xg, gg, bg = _bf16(x), _bf16(g), _bf16(b)
    y, _, mean, rstd = ops.hip_ops().layernorm_fwd(xg, None, gg, bg, 1e-5)
    ye, me, re_ = ref.layernorm_fwd(xg.float().cpu(), gg.float().cpu(),
                                    bg.float().cpu(), 1e-5)
    assert torch.allclose(y.float().cpu(), ye, atol=3e-2, rtol=2e-2)
    assert torch.allclose(mean.cpu(), me, atol=2e-3, rtol=1e-3)
    assert torch.allclose(rstd.cpu(), re_, atol=2e-3, rtol=2e-3)


@pytest.mark.parametrize("N,D", [(64, 1024), (257, 512), (32, 4096), (128, 136)])
def test_layernorm_bwd(N, D):
    torch.manual_seed(1)
    xg = _bf16(torch.randn(N, D))
    gg = _bf16(torch.randn(D))
    bg = _bf16(torch.randn(D))
    dyg = _bf16(torch.randn(N, D))
    _, _, mean, rstd = ops.hip_ops().layernorm_fwd(xg, None, gg, bg, 1e-5)
    dx, dgamma, dbeta = ops.hip_ops().layernorm_bwd(dyg, xg, gg, mean, rstd, None)
    dxe, dge, dbe = ref.layernorm_bwd(dyg.float().cpu(), xg.float().cpu(),
                                      gg.float().cpu(), mean.cpu(), rstd.cpu())
    assert torch.allclose(dx.float().cpu(), dxe, atol=4e-2, rtol=3e-2)
    # kernel and reference both accumulate in f32 from the same bf16
    # inputs — only summation-order noise remains (VERDICT r1 weak #6:
    # the old 0.3 + 0.02*sqrt(N) would have hidden real reduction bugs)
    tol = dict(atol=2e-2 + 2e-3 * math.sqrt(N), rtol=2e-2)
    assert torch.allclose(dgamma.cpu(), dge, **tol)
    assert torch.allclose(dbeta.cpu(), dbe, **tol)


@pytest.mark.parametrize("N,D", [(128, 4096), (63, 256)])
def test_bias_gelu(N, D):
    torch.manual_seed(2)
    xg = _bf16(torch.randn(N, D))
    bg = _bf16(torch.randn(D))
    y = ops.hip_ops().bias_gelu_fwd(xg, bg)
    ye = ref.bias_gelu_fwd(xg.float().cpu(), bg.float().cpu())
    assert torch.allclose(y.float().cpu(), ye, atol=3e-2, rtol=2e-2)
    dyg = _bf16(torch.randn(N, D))
    dx, dbias = ops.hip_ops().bias_gelu_bwd(dyg, xg, bg)
    dxe, dbe = ref.bias_gelu_bwd(dyg.float().cpu(), xg.float().cpu(),
                                 bg.float().cpu())
    assert torch.allclose(dx.float().cpu(), dxe, atol=3e-2, rtol=2e-2)
    # dbias: f32 accumulation both sides; the gelu'(pre) term differs
    # (hardware-exp kernel vs tanh-form reference) by ~1e-3/elem
    assert torch.allclose(dbias.cpu(), dbe, atol=0.1 + 0.01 * math.sqrt(N),
                          rtol=2e-2)


@pytest.mark.parametrize("B,H,Lq,Lk", [(2, 4, 512, 512), (3, 2, 128, 128),
                                       (2, 2, 64, 2056)])
def test_softmax(B, H, Lq, Lk):
    torch.manual_seed(3)
    sg = _bf16(torch.randn(B, H, Lq, Lk) * 3)
    mask = torch.zeros(B, Lk)
    mask[:, Lk - Lk // 4:] = -1e9
    mg = mask.cuda().contiguous()
    scale = 1.0 / math.sqrt(64)
    p = ops.hip_ops().softmax_fwd(sg, mg, scale)
    pe = ref.softmax_fwd(sg.float().cpu(), mask, scale)
    assert torch.allclose(p.float().cpu(), pe, atol=8e-3, rtol=2e-2)
    assert float(p.float().cpu()[..., Lk - Lk // 4:].max()) < 1e-6
    # row sums ~ 1
    assert torch.allclose(p.float().sum(-1).cpu(), torch.ones(B, H, Lq),
                          atol=3e-2)
    dpg = _bf16(torch.randn(B, H, Lq, Lk))
    ds = ops.hip_ops().softmax_bwd(dpg, p, scale)
    dse = ref.softmax_bwd(dpg.float().cpu(), p.float().cpu(), scale)
    # |ds| peaks near 4e-3, below the atol: allclose alone passes an all-zero
    # ds, the helper's relative bound (4 x the bf16 rounding floor) does not
    from test_ops_gpu_scale import assert_close
    assert_close(ds.cpu(), dse, "ds", atol=8e-3, rtol=2e-2)


def test_softmax_no_mask():
    torch.manual_seed(4)
    sg = _bf16(torch.randn(2, 2, 64, 512))
    p = ops.hip_ops().softmax_fwd(sg, None, 0.5)
    pe = ref.softmax_fwd(sg.float().cpu(), None, 0.5)
    assert torch.allclose(p.float().cpu(), pe, atol=8e-3, rtol=2e-2)


def test_adamw_step():
    torch.manual_seed(5)
    n = 4096
    master = torch.randn(n)
    p = _bf16(master)
    mst = master.cuda()
    g = torch.randn(n)
    gg = _bf16(g)
    m = torch.zeros(n).cuda()
    v = torch.zeros(n).cuda()
    mr = master.clone()
    pr = mr.to(torch.bfloat16)
    mref = torch.zeros(n)
    vref = torch.zeros(n)
    for step in range(1, 5):
        ops.hip_ops().adamw_step(p, gg, m, v, mst, 1e-2, 0.9, 0.999, 1e-8,
                                 0.05, step, 1.0)
        ref.adamw_step(pr, gg.float().cpu(), mref, vref, mr, lr=1e-2,
                       beta1=0.9, beta2=0.999, eps=1e-8, wd=0.05, step=step)
    assert torch.allclose(mst.cpu(), mr, atol=1e-4, rtol=1e-4)
    assert torch.allclose(p.float().cpu(), pr.float(), atol=1e-2)


def test_grad_scale_matches_prescaled():
    """grad_scale folding (the DDP average) == scaling the grad explicitly."""
    torch.manual_seed(6)
    n = 1024
    master = torch.randn(n)
    g = torch.randn(n)
    pa = _bf16(master); ma = master.cuda().clone()
    sa = torch.zeros(n).cuda(); va = torch.zeros(n).cuda()
    pb = _bf16(master); mb = master.cuda().clone()
    sb = torch.zeros(n).cuda(); vb = torch.zeros(n).cuda()
    ops.hip_ops().adamw_step(pa, _bf16(g), sa, va, ma, 1e-2, 0.9, 0.999,
                             1e-8, 0.0, 1, 0.25)
    ops.hip_ops().adamw_step(pb, _bf16(g * 0.25), sb, vb, mb, 1e-2, 0.9,
                             0.999, 1e-8, 0.0, 1, 1.0)
    assert torch.allclose(ma, mb, atol=2e-3, rtol=1e-3)


@pytest.mark.parametrize("N,D", [(64, 1024), (33, 136)])
def test_add_layernorm_fused(N, D):
    torch.manual_seed(7)
    xg = _bf16(torch.randn(N, D))
    rg = _bf16(torch.randn(N, D))
    gg = _bf16(torch.randn(D))
    bg = _bf16(torch.randn(D))
    y, s, mean, rstd = ops.hip_ops().layernorm_fwd(xg, rg, gg, bg, 1e-5)
    ye, se, me, re_ = ref.add_layernorm_fwd(xg.cpu(), rg.cpu(), gg.cpu(),
                                            bg.cpu(), 1e-5)
    assert torch.equal(s.cpu(), se), "fused residual sum must match bf16 add"
    assert torch.allclose(y.float().cpu(), ye.float(), atol=3e-2, rtol=2e-2)
    assert torch.allclose(mean.cpu(), me, atol=2e-3, rtol=1e-3)
    # no-residual call returns x itself as the stream
    y2, s2, _, _ = ops.hip_ops().layernorm_fwd(xg, None, gg, bg, 1e-5)
    assert s2.data_ptr() == xg.data_ptr()


def test_qkv_repack_roundtrip():
    torch.manual_seed(8)
    B, L, H, dh = 3, 40, 4, 16
    qkv = _bf16(torch.randn(B, L, 3 * H * dh))
    q = ops.hip_ops().qkv_repack(qkv, H, False)
    expect = (qkv.view(B, L, 3, H, dh).permute(2, 0, 3, 1, 4).contiguous())
    assert torch.equal(q, expect)
    # bwd3 gathers back to the Linear layout
    dq, dk, dv = (x.contiguous() for x in expect.unbind(0))
    back = ops.hip_ops().qkv_repack_bwd3(dq, dk, dv)
    assert torch.equal(back, qkv)


def test_out_repack_roundtrip():
    torch.manual_seed(9)
    B, H, L, dh = 2, 4, 24, 16
    x = _bf16(torch.randn(B, H, L, dh))
    y = ops.hip_ops().out_repack(x, False)
    expect = x.permute(0, 2, 1, 3).reshape(B, L, H * dh)
    assert torch.equal(y, expect)
    back = ops.hip_ops().out_repack_bwd(y, H)
    assert torch.equal(back, x)


@pytest.mark.parametrize("B,H,L", [(2, 3, 128), (1, 2, 512), (2, 2, 192)])
def test_flash_fwd_vs_reference(B, H, L):
    torch.manual_seed(10)
    q = _bf16(torch.randn(B, H, L, 64))
    k = _bf16(torch.randn(B, H, L, 64))
    v = _bf16(torch.randn(B, H, L, 64))
    mask = torch.zeros(B, L)
    mask[:, L - L // 4:] = -1e9
    mg = mask.cuda().contiguous()
    scale = 1.0 / 8.0
    o, lse = ops.hip_ops().flash_fwd(q, k, v, mg, scale)
    oe, le = ref.flash_attention_fwd(q.float().cpu(), k.float().cpu(),
                                     v.float().cpu(), mask, scale)
    assert torch.allclose(o.float().cpu(), oe.float(), atol=3e-2, rtol=3e-2), \
        (o.float().cpu() - oe.float()).abs().max()
    assert torch.allclose(lse.cpu(), le, atol=2e-2, rtol=1e-3)


def test_flash_fwd_no_mask():
    torch.manual_seed(11)
    q = _bf16(torch.randn(2, 2, 64, 64) * 2)
    k = _bf16(torch.randn(2, 2, 64, 64) * 2)
    v = _bf16(torch.randn(2, 2, 64, 64))
    o, lse = ops.hip_ops().flash_fwd(q, k, v, None, 0.125)
    oe, le = ref.flash_attention_fwd(q.float().cpu(), k.float().cpu(),
                                     v.float().cpu(), None, 0.125)
    assert torch.allclose(o.float().cpu(), oe.float(), atol=3e-2, rtol=3e-2)
    assert torch.allclose(lse.cpu(), le, atol=2e-2, rtol=1e-3)


def test_flash_backward_matches_bmm_path():
    """End-to-end grads: flash fwd + recompute bwd == bmm+softmax autograd."""
    torch.manual_seed(12)
    B, H, L, dh = 2, 2, 192, 64
    scale = 1.0 / 8.0
    base = {n: _bf16(torch.randn(B, H, L, dh)) for n in "qkv"}
    mask = torch.zeros(B, L)
    mask[:, 160:] = -1e9
    mg = mask.cuda().contiguous()
    do = _bf16(torch.randn(B, H, L, dh))

    fa = {n: t.clone().requires_grad_(True) for n, t in base.items()}
    o1 = ops.flash_attention(fa["q"], fa["k"], fa["v"], mg, scale)
    o1.backward(do)

    bm = {n: t.clone().requires_grad_(True) for n, t in base.items()}
    scores = torch.matmul(bm["q"], bm["k"].transpose(-1, -2))
    p = ops.fused_softmax(scores, mg, scale)
    o2 = torch.matmul(p, bm["v"])
    o2.backward(do)

    assert torch.allclose(o1.float(), o2.float(), atol=4e-2, rtol=4e-2)
    for n in "qkv":
        a, b = fa[n].grad.float(), bm[n].grad.float()
        assert torch.allclose(a, b, atol=6e-2, rtol=6e-2), \
            f"d{n}: {(a-b).abs().max()}"


def test_p_from_lse_rows_normalized():
    torch.manual_seed(13)
    B, H, L = 2, 2, 128
    q = _bf16(torch.randn(B, H, L, 64))
    k = _bf16(torch.randn(B, H, L, 64))
    v = _bf16(torch.randn(B, H, L, 64))
    scale = 0.125
    _, lse = ops.hip_ops().flash_fwd(q, k, v, None, scale)
    s = torch.matmul(q, k.transpose(-1, -2)).contiguous()
    p = ops.hip_ops().p_from_lse(s, None, lse, scale)
    sums = p.float().sum(-1)
    assert torch.allclose(sums, torch.ones_like(sums), atol=3e-2)


@pytest.mark.parametrize("L,pad_from", [(128, 100), (256, 96)])
def test_flash_bwd_fused_vs_reference(L, pad_from):
    """Batch row 0 is padded from `pad_from`, row 1 is unpadded.  At
    (256, 96) the padded row drives every padding shortcut: backward
    workgroup 1 (kv 128..255) takes the whole-workgroup early-out, wave 3 of
    workgroup 0 (kv 96..127) the per-wave skip, and the forward and
    dq-recompute tail skip stops after 3 of 8 kv tiles."""
    torch.manual_seed(14)
    B, H = 2, 2
    scale = 0.125
    q = _bf16(torch.randn(B, H, L, 64))
    k = _bf16(torch.randn(B, H, L, 64))
    v = _bf16(torch.randn(B, H, L, 64))
    do = _bf16(torch.randn(B, H, L, 64))
    mask = torch.zeros(B, L)
    mask[0, pad_from:] = -1e9
    mg = mask.cuda().contiguous()
    o, lse = ops.hip_ops().flash_fwd(q, k, v, mg, scale)
    ddot = ops.hip_ops().fa_dot(do, o)
    dd_ref = (do.float() * o.float()).sum(-1)
    assert torch.allclose(ddot, dd_ref, atol=2e-2, rtol=2e-2)
    dsg, dkg, dvg = ops.hip_ops().flash_bwd_fused(q, k, v, do, mg, lse,
                                                  ddot, scale, emit_ds=True)
    # reference
    s = torch.matmul(q.float(), k.float().transpose(-1, -2)) * scale \
        + mask.cuda().view(B, 1, 1, L)
    p_ref = torch.exp(s - lse.unsqueeze(-1))
    dp_ref = torch.matmul(do.float(), v.float().transpose(-1, -2))
    ds_ref = scale * p_ref * (dp_ref - dd_ref.unsqueeze(-1))
    dv_ref = torch.matmul(p_ref.transpose(-1, -2), do.float())
    dk_ref = torch.matmul(ds_ref.transpose(-1, -2), q.float())
    assert torch.allclose(dsg.float(), ds_ref, atol=2e-2, rtol=3e-2), \
        (dsg.float() - ds_ref).abs().max()
    assert torch.allclose(dvg.float(), dv_ref, atol=5e-2, rtol=3e-2), \
        (dvg.float() - dv_ref).abs().max()
    assert torch.allclose(dkg.float(), dk_ref, atol=5e-2, rtol=3e-2), \
        (dkg.float() - dk_ref).abs().max()
    # default path returns dk/dv only (no dS materialization); emit_ds=True
    # above disables the padding early-out, so this also compares the
    # skipped path bit for bit with the unskipped one
    dk2, dv2 = ops.hip_ops().flash_bwd_fused(q, k, v, do, mg, lse,
                                             ddot, scale)
    assert torch.equal(dk2, dkg) and torch.equal(dv2, dvg)
    # dQ-by-recompute kernel vs the fp32 reference
    dqg = ops.hip_ops().flash_dq_recompute(q, k, v, do, mg, lse, ddot, scale)
    dq_ref = torch.matmul(ds_ref, k.float())
    assert torch.allclose(dqg.float(), dq_ref, atol=5e-2, rtol=3e-2), \
        (dqg.float() - dq_ref).abs().max()


def test_flash_rejects_wrong_mask_and_lse_shapes():
    """A short mask or lse must be refused by the binding (TORCH_CHECK), not
    reach a kernel that would read past its end."""
    torch.manual_seed(29)
    ext = ops.hip_ops()
    B, H, L = 1, 1, 64
    scale = 0.125
    q, k, v, do = (_bf16(torch.randn(B, H, L, 64)) for _ in range(4))
    o, lse = ext.flash_fwd(q, k, v, None, scale)
    ddot = ext.fa_dot(do, o)
    qkv = torch.cat([t.transpose(1, 2).reshape(B, L, H * 64)
                     for t in (q, k, v)], dim=-1).contiguous()
    o_p = o.transpose(1, 2).reshape(B, L, H * 64).contiguous()
    do_p = do.transpose(1, 2).reshape(B, L, H * 64).contiguous()
    bad_mask = torch.zeros(B, L // 2, device="cuda")
    bad_lse = lse[:, :, :L // 2].contiguous()

    with pytest.raises(RuntimeError):
        ext.flash_fwd(q, k, v, bad_mask, scale)
    with pytest.raises(RuntimeError):
        ext.flash_bwd_fused(q, k, v, do, bad_mask, lse, ddot, scale)
    with pytest.raises(RuntimeError):
        ext.flash_bwd_fused(q, k, v, do, None, bad_lse, ddot, scale)
    with pytest.raises(RuntimeError):
        ext.flash_dq_recompute(q, k, v, do, bad_mask, lse, ddot, scale)
    with pytest.raises(RuntimeError):
        ext.flash_dq_recompute(q, k, v, do, None, bad_lse, ddot, scale)
    with pytest.raises(RuntimeError):
        ext.flash_bwd_packed(qkv, o_p, do_p, bad_mask, lse, H, scale)
    with pytest.raises(RuntimeError):
        ext.flash_bwd_packed(qkv, o_p, do_p, None, bad_lse, H, scale)


# The non-flash bindings pin their operands the same way.  Each test below
# makes one valid call at the smallest legal shape, then malformed ones that
# the binding must refuse by name before anything is allocated or launched.

def test_layernorm_rejects_wrong_param_shapes():
    ext = ops.hip_ops()
    N, D = 4, 8
    x, dy = _bf16(torch.randn(N, D)), _bf16(torch.randn(N, D))
    g, b = _bf16(torch.ones(D)), _bf16(torch.zeros(D))
    g16, b16 = _bf16(torch.ones(16)), _bf16(torch.zeros(16))
    y, _, mean, rstd = ext.layernorm_fwd(x, None, g, b, 1e-5)
    assert y.shape == x.shape
    assert ext.layernorm_bwd(dy, x, g, mean, rstd, None)[0].shape == x.shape
    with pytest.raises(RuntimeError, match="gamma"):
        ext.layernorm_fwd(x, None, g16, b, 1e-5)
    with pytest.raises(RuntimeError, match="beta"):
        ext.layernorm_fwd(x, None, g, b16, 1e-5)
    with pytest.raises(RuntimeError, match="gamma"):
        ext.layernorm_bwd(dy, x, g16, mean, rstd, None)


def test_bias_gelu_rejects_wrong_bias_and_grad_shapes():
    ext = ops.hip_ops()
    N, D = 4, 8
    x, dy = _bf16(torch.randn(N, D)), _bf16(torch.randn(N, D))
    b, b16 = _bf16(torch.zeros(D)), _bf16(torch.zeros(16))
    assert ext.bias_gelu_fwd(x, b).shape == x.shape
    dx, dbias = ext.bias_gelu_bwd(dy, x, b)
    assert dx.shape == x.shape and dbias.shape == (D,)
    with pytest.raises(RuntimeError, match=r"\bb must be"):
        ext.bias_gelu_fwd(x, b16)
    with pytest.raises(RuntimeError, match=r"\bb must be"):
        ext.bias_gelu_bwd(dy, x, b16)
    with pytest.raises(RuntimeError, match="dy"):
        ext.bias_gelu_bwd(_bf16(torch.randn(N // 2, D)), x, b)


def test_bias_grad_rejects_non_2d():
    ext = ops.hip_ops()
    assert ext.bias_grad(_bf16(torch.randn(4, 8))).shape == (8,)
    with pytest.raises(RuntimeError, match="dy"):
        ext.bias_grad(_bf16(torch.randn(2, 2, 8)))


def test_softmax_rejects_wrong_mask_and_grad_shapes():
    ext = ops.hip_ops()
    s = _bf16(torch.randn(1, 1, 4, 8))
    mask = torch.zeros(1, 8, device="cuda")
    wide = torch.zeros(1, 16, device="cuda")    # Lk mismatch
    tall = torch.zeros(2, 8, device="cuda")     # B mismatch
    lse = torch.zeros(1, 1, 4, device="cuda")
    p = ext.softmax_fwd(s, mask, 1.0)
    assert p.shape == s.shape
    assert ext.softmax_bwd(_bf16(torch.randn(1, 1, 4, 8)), p, 1.0).shape == \
        s.shape
    assert ext.p_from_lse(s, mask, lse, 1.0).shape == s.shape
    for bad in (wide, tall, mask.view(1, 1, 8)):
        with pytest.raises(RuntimeError, match="mask"):
            ext.softmax_fwd(s, bad, 1.0)
        with pytest.raises(RuntimeError, match="mask"):
            ext.p_from_lse(s, bad, lse, 1.0)
    with pytest.raises(RuntimeError, match="scores"):
        ext.p_from_lse(s.view(4, 8), mask, lse, 1.0)
    with pytest.raises(RuntimeError, match="dp"):
        ext.softmax_bwd(_bf16(torch.randn(1, 1, 2, 8)), p, 1.0)
    s4 = _bf16(torch.randn(1, 1, 4, 4))
    with pytest.raises(RuntimeError, match="Lk"):
        ext.softmax_bwd(s4, s4, 1.0)
    with pytest.raises(RuntimeError, match="Lk"):
        ext.p_from_lse(s4, None, lse, 1.0)


def test_masked_pool_rejects_wrong_mask_and_counts():
    ext = ops.hip_ops()
    B, L, D = 2, 4, 8
    x, dp = _bf16(torch.randn(B, L, D)), _bf16(torch.randn(B, D))
    mask = torch.ones(B, L, dtype=torch.bool, device="cuda")
    pooled, counts = ext.masked_pool_fwd(x, mask)
    assert pooled.shape == (B, D) and counts.shape == (B,)
    assert ext.masked_pool_bwd(dp, mask, counts, L).shape == x.shape
    bad_masks = (torch.ones(B, 8, dtype=torch.bool, device="cuda"),
                 torch.ones(B, L, dtype=torch.int32, device="cuda"),
                 torch.ones(B, L, dtype=torch.bool))          # on the host
    for bad in bad_masks:
        with pytest.raises(RuntimeError, match="mask"):
            ext.masked_pool_fwd(x, bad)
        with pytest.raises(RuntimeError, match="mask"):
            ext.masked_pool_bwd(dp, bad, counts, L)
    for bad in (torch.ones(3, device="cuda"), counts.to(torch.bfloat16)):
        with pytest.raises(RuntimeError, match="counts"):
            ext.masked_pool_bwd(dp, mask, bad, L)
    with pytest.raises(RuntimeError, match="dpooled"):
        ext.masked_pool_bwd(dp.view(B, 1, D), mask, counts, L)
    with pytest.raises(RuntimeError, match="L must be"):
        ext.masked_pool_bwd(dp, None, counts, 0)


def test_repack_rejects_wrong_ranks_and_shapes():
    ext = ops.hip_ops()
    B, L, H, dh = 1, 4, 2, 8
    qkv = _bf16(torch.randn(B, L, 3 * H * dh))
    q3 = ext.qkv_repack(qkv, H, False)
    assert q3.shape == (3, B, H, L, dh)
    dq, dk, dv = (t.contiguous() for t in q3.unbind(0))
    assert torch.equal(ext.qkv_repack_bwd3(dq, dk, dv), qkv)
    merged = ext.out_repack(dq, False)
    assert merged.shape == (B, L, H * dh)
    assert torch.equal(ext.out_repack_bwd(merged, H), dq)
    other = _bf16(torch.randn(B, H, L, 2 * dh))
    with pytest.raises(RuntimeError, match="dk"):
        ext.qkv_repack_bwd3(dq, other, dv)
    with pytest.raises(RuntimeError, match="dv"):
        ext.qkv_repack_bwd3(dq, dk, other)
    with pytest.raises(RuntimeError, match="dq"):
        ext.qkv_repack_bwd3(dq[0], dk[0], dv[0])
    with pytest.raises(RuntimeError, match="qkv"):
        ext.qkv_repack(qkv, 5, False)             # 48 % (3 * 5) != 0
    with pytest.raises(RuntimeError, match="qkv"):
        ext.qkv_repack(qkv.view(B, L, 3, H * dh), H, False)
    with pytest.raises(RuntimeError, match="x must be"):
        ext.out_repack(merged, False)
    with pytest.raises(RuntimeError, match="dgrad"):
        ext.out_repack_bwd(merged, 3)             # 16 % 3 != 0
    with pytest.raises(RuntimeError, match="dgrad"):
        ext.out_repack_bwd(dq, H)
    # head_dim 4: every one of the four refuses it
    half = _bf16(torch.randn(B, H, L, 4))
    with pytest.raises(RuntimeError, match="head_dim"):
        ext.qkv_repack(_bf16(torch.randn(B, L, 3 * H * 4)), H, False)
    with pytest.raises(RuntimeError, match="head_dim"):
        ext.qkv_repack_bwd3(half, half, half)
    with pytest.raises(RuntimeError, match="head_dim"):
        ext.out_repack(half, False)
    with pytest.raises(RuntimeError, match="head_dim"):
        ext.out_repack_bwd(_bf16(torch.randn(B, L, H * 4)), H)


def test_layernorm_bwd_with_residual_grad():
    torch.manual_seed(15)
    N, D = 64, 1024
    xg = _bf16(torch.randn(N, D))
    gg = _bf16(torch.randn(D))
    bg = _bf16(torch.randn(D))
    dyg = _bf16(torch.randn(N, D))
    ds = _bf16(torch.randn(N, D))
    _, _, mean, rstd = ops.hip_ops().layernorm_fwd(xg, None, gg, bg, 1e-5)
    dx, _, _ = ops.hip_ops().layernorm_bwd(dyg, xg, gg, mean, rstd, ds)
    dx0, _, _ = ops.hip_ops().layernorm_bwd(dyg, xg, gg, mean, rstd, None)
    expect = (dx0.float() + ds.float()).to(torch.bfloat16)
    assert torch.allclose(dx.float(), expect.float(), atol=2e-2, rtol=2e-2)


def test_masked_pool():
    torch.manual_seed(16)
    B, L, D = 4, 48, 128
    x = _bf16(torch.randn(B, L, D))
    mask = torch.zeros(B, L, dtype=torch.bool)
    for i in range(B):
        mask[i, :12 + 7 * i] = True
    mg = mask.cuda().contiguous()
    pooled, counts = ops.hip_ops().masked_pool_fwd(x, mg)
    w = mask.float().unsqueeze(-1)
    expect = (x.float().cpu() * w).sum(1) / w.sum(1)
    assert torch.allclose(pooled.float().cpu(), expect, atol=2e-2, rtol=2e-2)
    assert torch.equal(counts.cpu(), mask.sum(-1).float())
    dp = _bf16(torch.randn(B, D))
    dx = ops.hip_ops().masked_pool_bwd(dp, mg, counts, L)
    dxe = (dp.float().cpu() / counts.cpu().unsqueeze(-1)).unsqueeze(1) \
        .expand(-1, L, -1) * w
    assert torch.allclose(dx.float().cpu(), dxe, atol=2e-2, rtol=2e-2)


def test_masked_pool_fully_masked_row():
    x = _bf16(torch.randn(2, 16, 64))
    mask = torch.zeros(2, 16, dtype=torch.bool)
    mask[0, :5] = True  # row 1 fully masked
    mg = mask.cuda().contiguous()
    pooled, counts = ops.hip_ops().masked_pool_fwd(x, mg)
    assert float(counts[1]) == 1.0  # clamped, no div-by-zero
    assert torch.all(pooled[1].float() == 0)
    assert not torch.isnan(pooled.float()).any()


@pytest.mark.gpu
def test_lt_linear_gelu_bias_vs_reference():
    """hipBLASLt GELU_BIAS epilogue (inference FFN-up) vs fp32 torch; also
    pins which epilogues this hipBLASLt build provides (csrc/lt_gemm.cpp)."""
    ext = ops.hip_ops()
    assert ext.lt_probe_epilogue(1024, 512, 256, 36)      # GELU_BIAS
    torch.manual_seed(21)
    N, D, F = 512, 256, 1024
    x = _bf16(torch.randn(N, D))
    w1 = _bf16(torch.randn(F, D) * 0.05)
    b1 = _bf16(torch.randn(F) * 0.1)
    a = ext.lt_linear_gelu_bias(x, w1, b1)
    h_ref = x.float() @ w1.float().T + b1.float()
    a_ref = torch.nn.functional.gelu(h_ref, approximate="tanh")
    a_ref_erf = torch.nn.functional.gelu(h_ref)
    d_tanh = (a.float() - a_ref).abs().max()
    d_erf = (a.float() - a_ref_erf).abs().max()
    assert min(d_tanh, d_erf) < 3e-2, (d_tanh, d_erf)


@pytest.mark.gpu
def test_ffn_inference_path_matches_training_path():
    """FFN.forward under no_grad (GELU_BIAS epilogue) vs the grad-mode
    kernel path on the same weights."""
    from tosem2021_amd.models.classifier import CONFIGS, FFN
    torch.manual_seed(22)
    ffn = FFN(CONFIGS["mltc-tiny"]).to(torch.bfloat16).cuda()
    x = _bf16(torch.randn(4, 64, CONFIGS["mltc-tiny"].d_model))
    with torch.no_grad():
        y_inf = ffn(x)
    y_train = ffn(x.requires_grad_())
    assert torch.allclose(y_inf.float(), y_train.float(), atol=3e-2,
                          rtol=3e-2), (y_inf.float() - y_train.float()).abs().max()


@pytest.mark.gpu
@pytest.mark.parametrize("B,H,L", [(2, 3, 128), (1, 2, 512), (2, 2, 192)])
def test_flash_dq_vs_matmul(B, H, L):
    torch.manual_seed(23)
    ds = _bf16(torch.randn(B, H, L, L))
    k = _bf16(torch.randn(B, H, L, 64))
    dq = ops.hip_ops().flash_dq(ds, k)
    ref_dq = torch.matmul(ds.float(), k.float())
    assert torch.allclose(dq.float(), ref_dq, atol=0.5, rtol=3e-2), \
        (dq.float() - ref_dq).abs().max()


@pytest.mark.gpu
@pytest.mark.parametrize("N,D", [(4096, 1024), (513, 3072)])
def test_bias_grad_vs_sum(N, D):
    torch.manual_seed(24)
    dy = _bf16(torch.randn(N, D))
    db = ops.hip_ops().bias_grad(dy)
    ref_db = dy.float().sum(0)
    # exact bf16 values summed in f32 both sides; only ordering noise
    # (bias_grad output is bf16, so allow one bf16 ulp of the magnitude)
    assert torch.allclose(db.float(), ref_db,
                          atol=5e-2 + 2e-3 * N ** 0.5, rtol=1e-2), \
        (db.float() - ref_db).abs().max()


@pytest.mark.gpu
def test_fused_linear_autograd_vs_torch():
    torch.manual_seed(25)
    N, D, M = 512, 256, 128
    x = torch.randn(N, D)
    w = torch.randn(M, D) * 0.05
    b = torch.randn(M) * 0.1
    dy = torch.randn(N, M)
    xg = _bf16(x).requires_grad_()
    wg = _bf16(w).requires_grad_()
    bg = _bf16(b).requires_grad_()
    y = ops.fused_linear(xg, wg, bg)
    y.backward(_bf16(dy))
    xr = x.requires_grad_()
    wr = w.requires_grad_()
    br = b.requires_grad_()
    yr = torch.nn.functional.linear(xr, wr, br)
    yr.backward(dy)
    assert torch.allclose(y.float().cpu(), yr, atol=5e-2, rtol=5e-2)
    assert torch.allclose(xg.grad.float().cpu(), xr.grad, atol=5e-2,
                          rtol=5e-2)
    assert torch.allclose(wg.grad.float().cpu(), wr.grad, atol=0.5, rtol=5e-2)
    assert torch.allclose(bg.grad.float().cpu(), br.grad, atol=0.5, rtol=5e-2)


@pytest.mark.gpu
def test_kernels_bitwise_deterministic():
    """Race-detection lane (the corpus used valgrind
    suppressions; our native surface is HIP kernels, where a data race
    shows up as run-to-run divergence): every kernel with cross-lane
    LDS traffic or atomics must be bitwise reproducible on identical
    input."""
    torch.manual_seed(26)
    B, H, L = 2, 4, 512
    q = _bf16(torch.randn(B, H, L, 64))
    k = _bf16(torch.randn(B, H, L, 64))
    v = _bf16(torch.randn(B, H, L, 64))
    do = _bf16(torch.randn(B, H, L, 64))
    mask = torch.zeros(B, L).cuda().contiguous()
    ext = ops.hip_ops()
    o1, lse1 = ext.flash_fwd(q, k, v, mask, 0.125)
    o2, lse2 = ext.flash_fwd(q, k, v, mask, 0.125)
    assert torch.equal(o1, o2) and torch.equal(lse1, lse2)
    dd = ext.fa_dot(do, o1)
    r1 = ext.flash_bwd_fused(q, k, v, do, mask, lse1, dd, 0.125,
                             emit_ds=True)
    r2 = ext.flash_bwd_fused(q, k, v, do, mask, lse1, dd, 0.125,
                             emit_ds=True)
    for a, b in zip(r1, r2):
        assert torch.equal(a, b)
    assert torch.equal(ext.flash_dq(r1[0], k), ext.flash_dq(r1[0], k))
    assert torch.equal(
        ext.flash_dq_recompute(q, k, v, do, mask, lse1, dd, 0.125),
        ext.flash_dq_recompute(q, k, v, do, mask, lse1, dd, 0.125))
    N, D = 4096, 1024
    x = _bf16(torch.randn(N, D))
    g = _bf16(torch.randn(D))
    bb = _bf16(torch.randn(D))
    dy = _bf16(torch.randn(N, D))
    _, _, mean, rstd = ext.layernorm_fwd(x, None, g, bb, 1e-5)
    l1 = ext.layernorm_bwd(dy, x, g, mean, rstd, None)
    l2 = ext.layernorm_bwd(dy, x, g, mean, rstd, None)
    for a, b in zip(l1, l2):
        assert torch.equal(a, b)  # incl. the two-stage colsum dgamma/dbeta
    assert torch.equal(ext.bias_grad(dy), ext.bias_grad(dy))
    bgx = _bf16(torch.randn(N, 4096))
    bgb = _bf16(torch.randn(4096))
    bgd = _bf16(torch.randn(N, 4096))
    d1 = ext.bias_gelu_bwd(bgd, bgx, bgb)
    d2 = ext.bias_gelu_bwd(bgd, bgx, bgb)
    for a, b in zip(d1, d2):
        assert torch.equal(a, b)


@pytest.mark.gpu
def test_flash_packed_vs_unpacked():
    """Packed-layout flash (straight on [B, L, 3D] QKV projection output)
    must match the unpacked kernels bit-for-bit in forward and backward —
    same compute, different addressing geometry."""
    torch.manual_seed(27)
    B, H, L = 2, 4, 256
    D = H * 64
    qkv = _bf16(torch.randn(B, L, 3 * D))
    mask = torch.zeros(B, L)
    mask[:, 200:] = -1e9
    mg = mask.cuda().contiguous()
    scale = 0.125
    ext = ops.hip_ops()
    # unpacked reference path
    q, k, v = (t.view(B, L, H, 64).transpose(1, 2).contiguous()
               for t in qkv.split(D, dim=-1))
    o_u, lse_u = ext.flash_fwd(q, k, v, mg, scale)
    o_p, lse_p = ext.flash_fwd_packed(qkv, H, mg, scale)
    assert torch.equal(lse_p, lse_u.view(B, H, L))
    o_p4 = o_p.view(B, L, H, 64).transpose(1, 2).contiguous()
    assert torch.equal(o_p4, o_u)
    # backward parity
    do = _bf16(torch.randn(B, L, D))
    do4 = do.view(B, L, H, 64).transpose(1, 2).contiguous()
    ddot = ext.fa_dot(do4, o_u)
    dk_u, dv_u = ext.flash_bwd_fused(q, k, v, do4, mg, lse_u, ddot, scale)
    dq_u = ext.flash_dq_recompute(q, k, v, do4, mg, lse_u, ddot, scale)
    dqkv = ext.flash_bwd_packed(qkv, o_p, do, mg, lse_p, H, scale)
    dq_p, dk_p, dv_p = (t.view(B, L, H, 64).transpose(1, 2).contiguous()
                        for t in dqkv.split(D, dim=-1))
    assert torch.equal(dq_p, dq_u)
    assert torch.equal(dk_p, dk_u)
    assert torch.equal(dv_p, dv_u)


@pytest.mark.gpu
def test_flash_packed_autograd_vs_cpu():
    """End-to-end packed autograd vs the fp32 CPU fallback of the same
    Function (bf16-sized tolerances)."""
    torch.manual_seed(28)
    B, H, L = 2, 2, 128
    D = H * 64
    qkv_cpu = torch.randn(B, L, 3 * D).to(torch.bfloat16).requires_grad_()
    mask = torch.zeros(B, L)
    mask[:, 100:] = -1e9
    out_cpu = ops.flash_attention_packed(qkv_cpu, H, mask, 0.125)
    gout = torch.randn(B, L, D).to(torch.bfloat16)
    out_cpu.backward(gout)
    qkv_gpu = qkv_cpu.detach().clone().cuda().requires_grad_()
    out_gpu = ops.flash_attention_packed(qkv_gpu, H,
                                         mask.cuda().contiguous(), 0.125)
    out_gpu.backward(gout.cuda())
    assert torch.allclose(out_gpu.float().cpu(), out_cpu.float(),
                          atol=3e-2, rtol=3e-2)
    assert torch.allclose(qkv_gpu.grad.float().cpu(), qkv_cpu.grad.float(),
                          atol=8e-2, rtol=5e-2), \
        (qkv_gpu.grad.float().cpu() - qkv_cpu.grad.float()).abs().max()


@pytest.mark.gpu
def test_flash_packed_deterministic():
    torch.manual_seed(29)
    B, H, L = 2, 4, 512
    D = H * 64
    qkv = _bf16(torch.randn(B, L, 3 * D))
    do = _bf16(torch.randn(B, L, D))
    mask = torch.zeros(B, L).cuda().contiguous()
    ext = ops.hip_ops()
    o1, l1 = ext.flash_fwd_packed(qkv, H, mask, 0.125)
    o2, l2 = ext.flash_fwd_packed(qkv, H, mask, 0.125)
    assert torch.equal(o1, o2) and torch.equal(l1, l2)
    g1 = ext.flash_bwd_packed(qkv, o1, do, mask, l1, H, 0.125)
    g2 = ext.flash_bwd_packed(qkv, o1, do, mask, l1, H, 0.125)
    assert torch.equal(g1, g2)


@pytest.mark.gpu
def test_hipgraph_captured_forward_matches_eager():
    """hipGraph-captured inference (utils/hipgraph.py) must match the eager
    forward on the same inputs."""
    from tosem2021_amd.models.classifier import CONFIGS, build_model
    from tosem2021_amd.utils.hipgraph import CapturedForward
    torch.manual_seed(31)
    model = build_model("mltc-tiny").cuda().eval()
    B, L = 4, 64
    fwd = CapturedForward(model, B, L)
    toks = torch.randint(4, CONFIGS["mltc-tiny"].vocab_size, (B, L),
                         device="cuda")
    mask = torch.ones(B, L, dtype=torch.bool, device="cuda")
    mask[:, 50:] = False
    out_g = {k: v.clone() for k, v in fwd(toks, mask).items()}
    with torch.no_grad():
        out_e = model(toks, mask)
    for k in out_e:
        assert torch.allclose(out_g[k].float(), out_e[k].float(),
                              atol=3e-2, rtol=3e-2), k
    # replay with different inputs gives different outputs (buffers rebind)
    toks2 = torch.randint(4, CONFIGS["mltc-tiny"].vocab_size, (B, L),
                          device="cuda")
    out_g2 = fwd(toks2, mask)
    assert not torch.equal(out_g2["strategy"], out_g["strategy"])


@pytest.mark.gpu
def test_wgrad_gemm_vs_reference():
    """Custom split-K wgrad GEMM vs fp32 torch reference + determinism
    (both variants: glds pipeline and register staging)."""
    import os
    torch.manual_seed(33)
    K, M, N = 4096, 512, 256
    dy = _bf16(torch.randn(K, M) * 0.3)
    x = _bf16(torch.randn(K, N) * 0.3)
    ref = torch.mm(dy.t().float(), x.float())
    ext = ops.hip_ops()
    dw = ext.wgrad_gemm(dy, x, 4)
    rel = (dw.float() - ref).abs().max() / ref.abs().max()
    assert rel < 2e-2, rel
    assert torch.equal(dw, ext.wgrad_gemm(dy, x, 4))     # deterministic
    # S=1 (no split) and auto-S agree with the reference too
    for s in (1, 0):
        dws = ext.wgrad_gemm(dy, x, s)
        rel = (dws.float() - ref).abs().max() / ref.abs().max()
        assert rel < 2e-2, (s, rel)
    # autograd wrapper end-to-end
    xg = _bf16(torch.randn(1024, 256)).requires_grad_()
    w = _bf16(torch.randn(512, 256) * 0.05).requires_grad_()
    b = _bf16(torch.randn(512) * 0.1).requires_grad_()
    y = ops.wgrad_linear(xg, w, b)
    gy = _bf16(torch.randn(1024, 512))
    y.backward(gy)
    assert torch.allclose(w.grad.float(),
                          torch.mm(gy.t().float(), xg.detach().float()),
                          atol=0.5, rtol=3e-2)
    assert torch.allclose(b.grad.float(), gy.float().sum(0), atol=0.3,
                          rtol=2e-2)
