"""Sequence packing on the GPU: the segment-aware flash trio, the segment
mean-pool and the packed model against the fp32 references.

All attention cases use B=2, H=2, randn bf16 inputs and scale 0.125:
  A  L=64   row 0 = segments [5, 40, 19]; row 1 = [1, 30] + 33 pad —
            segment edges off the 32-row tile grid, a 1-token segment, a
            pad tail that starts mid-tile
  B  L=320  row 0 = [120, 15, 115, 12, 58]; row 1 = one 320-token segment —
            two workgroups in the q-major kernels and three in
            flash_bwd_fused, segments straddling the 128- and 256-row
            workgroup edges (the tile-range skip starts above 0), a
            full-length segment
"""
import pytest
import torch

pytestmark = pytest.mark.gpu

from tosem2021_amd import ops
from tosem2021_amd.ops import reference as ref

B, H, SCALE = 2, 2, 0.125
CASES = {
    "A": (64, [[5, 40, 19], [1, 30]]),
    "B": (320, [[120, 15, 115, 12, 58], [320]]),
}


# model-level cases: the config and data of tests/test_packing.py's
# equivalence test (head_dim 64; seven texts of 1 .. 40 tokens; 64-token rows)
MODEL_CFG = dict(vocab_size=512, d_model=128, n_heads=2, n_layers=2,
                 d_ff=256, max_seq=64)
LENGTHS = [1, 40, 7, 23, 12, 31, 5]
ROW_LEN = 64


def make_texts():
    from tosem2021_amd.models.tokenizer import CodeTokenizer
    tok = CodeTokenizer(MODEL_CFG["vocab_size"])
    texts = [" ".join(f"w{i}x{j}" for j in range(n - 1))
             for i, n in enumerate(LENGTHS)]
    assert [len(tok.encode(t, ROW_LEN)) for t in texts] == LENGTHS
    return tok, texts


def _bf16(x):
    return x.to(torch.bfloat16).cuda().contiguous()


def make_seg(L, rows):
    """int32 [B, L] ids: 0, 1, ... per segment, then the pad tail's id."""
    seg = torch.zeros(len(rows), L, dtype=torch.int32)
    for r, lens in enumerate(rows):
        at = 0
        for s, n in enumerate(lens):
            seg[r, at:at + n] = s
            at += n
        seg[r, at:] = len(lens)
    ops.check_segments(seg)
    return seg


def _inputs(case, seed):
    L, rows = CASES[case]
    torch.manual_seed(seed)
    q, k, v, do = (_bf16(torch.randn(B, H, L, 64)) for _ in range(4))
    return L, make_seg(L, rows), q, k, v, do


def _run_trio(q, k, v, do, seg=None, mask=None):
    ext = ops.hip_ops()
    o, lse = ext.flash_fwd(q, k, v, mask, SCALE, seg=seg)
    ddot = ext.fa_dot(do, o)
    dk, dv = ext.flash_bwd_fused(q, k, v, do, mask, lse, ddot, SCALE,
                                 seg=seg)
    dq = ext.flash_dq_recompute(q, k, v, do, mask, lse, ddot, SCALE, seg=seg)
    return o, lse, dq, dk, dv


def _reference(q, k, v, do, seg):
    """fp32 reference with segment_bias, every position (pads included)."""
    qf, kf, vf, dof = (t.float().cpu() for t in (q, k, v, do))
    bias = ref.segment_bias(seg)
    o, lse = ref.flash_attention_fwd(qf, kf, vf, None, SCALE, bias)
    s = torch.matmul(qf, kf.transpose(-1, -2)) * SCALE + bias
    p = torch.exp(s - lse.unsqueeze(-1))
    dp = torch.matmul(dof, vf.transpose(-1, -2))
    dd = (dof * o).sum(-1)
    ds = SCALE * p * (dp - dd.unsqueeze(-1))
    return (o, lse, torch.matmul(ds, kf),
            torch.matmul(ds.transpose(-1, -2), qf),
            torch.matmul(p.transpose(-1, -2), dof))


@pytest.mark.parametrize("case", ["A", "B"])
def test_segmented_flash_trio_vs_reference(case):
    L, seg, q, k, v, do = _inputs(case, 40)
    o, lse, dq, dk, dv = _run_trio(q, k, v, do, seg=seg.cuda())
    oe, le, dqe, dke, dve = _reference(q, k, v, do, seg)
    assert torch.isfinite(o.float()).all() and torch.isfinite(lse).all()
    assert torch.allclose(o.float().cpu(), oe, atol=3e-2, rtol=3e-2), \
        (o.float().cpu() - oe).abs().max()
    assert torch.allclose(lse.cpu(), le, atol=2e-2, rtol=1e-3), \
        (lse.cpu() - le).abs().max()
    for name, got, want in (("dq", dq, dqe), ("dk", dk, dke),
                            ("dv", dv, dve)):
        assert torch.allclose(got.float().cpu(), want, atol=5e-2, rtol=3e-2), \
            f"{name}: {(got.float().cpu() - want).abs().max()}"


@pytest.mark.parametrize("case", ["A", "B"])
def test_flash_attention_packed_seg_autograd_vs_cpu(case):
    """ops.flash_attention_packed(seg=...) on the GPU against the same
    Function's CPU reference path (tolerances of
    test_flash_packed_autograd_vs_cpu)."""
    L, rows = CASES[case]
    seg = make_seg(L, rows)
    torch.manual_seed(41)
    D = H * 64
    qkv_cpu = torch.randn(B, L, 3 * D).to(torch.bfloat16).requires_grad_()
    gout = torch.randn(B, L, D).to(torch.bfloat16)
    out_cpu = ops.flash_attention_packed(qkv_cpu, H, None, SCALE, seg=seg)
    out_cpu.backward(gout)
    qkv_gpu = qkv_cpu.detach().clone().cuda().requires_grad_()
    out_gpu = ops.flash_attention_packed(qkv_gpu, H, None, SCALE,
                                         seg=seg.cuda())
    out_gpu.backward(gout.cuda())
    assert torch.allclose(out_gpu.float().cpu(), out_cpu.float(),
                          atol=3e-2, rtol=3e-2)
    assert torch.allclose(qkv_gpu.grad.float().cpu(), qkv_cpu.grad.float(),
                          atol=8e-2, rtol=5e-2), \
        (qkv_gpu.grad.float().cpu() - qkv_cpu.grad.float()).abs().max()


@pytest.mark.parametrize("row,which", [(0, 1), (0, 2), (1, 0), (1, 2)])
def test_no_leakage_between_segments_bitwise(row, which):
    """Replace q, k, v and dout of ONE segment (`which` of `row`; id 2 of
    row 1 is the pad tail): every output outside it is bit-identical,
    because an out-of-segment probability is exactly +0.0f."""
    L, seg, q, k, v, do = _inputs("A", 42)
    sg = seg.cuda()
    first = _run_trio(q, k, v, do, seg=sg)
    inside = (seg[row] == which)
    assert inside.any()
    torch.manual_seed(43)
    q2, k2, v2, do2 = (t.clone() for t in (q, k, v, do))
    for t in (q2, k2, v2, do2):
        t[row, :, inside.cuda()] = _bf16(
            torch.randn(H, int(inside.sum()), 64))
    second = _run_trio(q2, k2, v2, do2, seg=sg)
    keep = torch.ones(B, L, dtype=torch.bool)
    keep[row] = ~inside
    keep = keep.cuda()
    for name, a, b in zip(("o", "lse", "dq", "dk", "dv"), first, second):
        a, b = a.transpose(1, 2), b.transpose(1, 2)     # [B, L, H(, 64)]
        assert torch.equal(a[keep], b[keep]), f"{name} leaked"
    # and the replaced segment did change
    assert not torch.equal(first[0][row][:, inside.cuda()],
                           second[0][row][:, inside.cuda()])


@pytest.mark.parametrize("L,lens", [(64, [31, 64]), (320, [120, 290])])
def test_single_segment_rows_reproduce_mask_path(L, lens):
    """One real segment per row + the pad tail == the same lengths as the
    -1e9 padding mask: o and lse bit-equal at valid positions, gradients
    (dout zeroed at pads) within the gradient tolerance."""
    torch.manual_seed(44)
    q, k, v, do = (_bf16(torch.randn(B, H, L, 64)) for _ in range(4))
    seg = make_seg(L, [[n] for n in lens])
    mask = torch.zeros(B, L)
    valid = torch.zeros(B, L, dtype=torch.bool)
    for r, n in enumerate(lens):
        mask[r, n:] = -1e9
        valid[r, :n] = True
    do = do * valid.cuda()[:, None, :, None]
    got = _run_trio(q, k, v, do, seg=seg.cuda())
    want = _run_trio(q, k, v, do, mask=mask.cuda().contiguous())
    vg = valid.cuda()
    for name, a, b in zip(("o", "lse", "dq", "dk", "dv"), got, want):
        a, b = a.transpose(1, 2)[vg], b.transpose(1, 2)[vg]
        if name in ("o", "lse"):
            assert torch.equal(a, b), name
        else:
            assert torch.allclose(a.float(), b.float(), atol=5e-2,
                                  rtol=3e-2), \
                f"{name}: {(a.float() - b.float()).abs().max()}"


@pytest.mark.parametrize("case", ["A", "B"])
def test_segmented_flash_deterministic(case):
    L, rows = CASES[case]
    seg = make_seg(L, rows).cuda()
    torch.manual_seed(45)
    D = H * 64
    qkv = _bf16(torch.randn(B, L, 3 * D))
    do = _bf16(torch.randn(B, L, D))
    ext = ops.hip_ops()
    o1, l1 = ext.flash_fwd_packed(qkv, H, None, SCALE, seg=seg)
    o2, l2 = ext.flash_fwd_packed(qkv, H, None, SCALE, seg=seg)
    assert torch.equal(o1, o2) and torch.equal(l1, l2)
    g1 = ext.flash_bwd_packed(qkv, o1, do, None, l1, H, SCALE, seg=seg)
    g2 = ext.flash_bwd_packed(qkv, o1, do, None, l1, H, SCALE, seg=seg)
    assert torch.equal(g1, g2)


@pytest.mark.parametrize("D", [128, 1024])
def test_segment_mean_pool(D):
    from tosem2021_amd.data.packing import pack_examples
    g = torch.Generator().manual_seed(46)
    lens = [5, 40, 19, 1, 30, 22]
    pb = pack_examples([torch.randint(8, 500, (n,), generator=g).tolist()
                        for n in lens], 64)
    assert pb.tokens.shape == (2, 64)
    torch.manual_seed(47)
    x = torch.randn(pb.n_positions, D).to(torch.bfloat16)
    dp = torch.randn(pb.n_segments, D).to(torch.bfloat16)
    dev = pb.to("cuda")
    xg = x.cuda().requires_grad_()
    pooled = ops.segment_mean_pool(xg, dev.seg_start, dev.seg_len,
                                   dev.pos2seg)
    pooled.backward(dp.cuda())
    want = ref.segment_pool_fwd(x.float(), pb.seg_start, pb.seg_len,
                                pb.pos2seg)
    dx = ref.segment_pool_bwd(dp.float(), pb.seg_len, pb.pos2seg)
    assert torch.allclose(pooled.float().cpu(), want, atol=2e-2, rtol=2e-2)
    assert torch.allclose(xg.grad.float().cpu(), dx, atol=2e-2, rtol=2e-2)
    pad = pb.pos2seg < 0
    assert pad.any() and (xg.grad.cpu()[pad] == 0).all()


def test_model_packed_and_unpacked_vs_fp32_cpu():
    """Config and data of the CPU equivalence test, bf16 on the GPU: the
    packed logits (unpermuted) and the unpacked logits each meet
    test_model_gpu's tolerance against the fp32 CPU model."""
    from tosem2021_amd.models.classifier import MLTC, MLTCConfig
    cfg = MLTCConfig(**MODEL_CFG)
    torch.manual_seed(0)
    model = MLTC(cfg).to(torch.bfloat16)
    tok, texts = make_texts()
    toks, mask = tok.encode_batch(texts, 64)
    pb = tok.encode_packed(texts, 64, ROW_LEN)
    assert pb.tokens.shape[0] < len(texts)          # really shares rows
    cpu = MLTC(cfg).float()
    cpu.load_state_dict({k: v.float() for k, v in model.state_dict().items()})
    with torch.no_grad():
        want = cpu(toks, mask)
    gm = model.cuda()
    unpacked = gm(toks.cuda(), mask.cuda())
    dev = pb.to("cuda")
    packed = {h: dev.unpermute(x)
              for h, x in gm(dev.tokens, packing=dev).items()}
    for h in want:
        for name, got in (("unpacked", unpacked), ("packed", packed)):
            a = got[h].float().cpu()
            assert torch.allclose(a, want[h], atol=0.05, rtol=0.05), \
                f"{name} {h}: max diff {(a - want[h]).abs().max()}"


def test_packing_needs_flash_shapes_on_gpu():
    """head_dim != 64 under packing is an error on the GPU, not a silent
    O(L^2) fallback."""
    from tosem2021_amd.models.classifier import MLTC, MLTCConfig
    cfg = MLTCConfig(vocab_size=512, d_model=128, n_heads=4, n_layers=1,
                     d_ff=256, max_seq=64)
    model = MLTC(cfg).to(torch.bfloat16).cuda()
    tok, texts = make_texts()
    pb = tok.encode_packed(texts, 64, ROW_LEN, device="cuda")
    with pytest.raises(RuntimeError, match="head_dim"):
        model(pb.tokens, packing=pb)


def test_seg_binding_validation():
    """Every bad seg is refused on the host, before any launch."""
    ext = ops.hip_ops()
    L = 64
    torch.manual_seed(48)
    q, k, v, do = (_bf16(torch.randn(B, H, L, 64)) for _ in range(4))
    seg = make_seg(L, CASES["A"][1]).cuda()
    o, lse = ext.flash_fwd(q, k, v, None, SCALE, seg=seg)
    ddot = ext.fa_dot(do, o)
    D = H * 64
    qkv = _bf16(torch.randn(B, L, 3 * D))
    do_p = _bf16(torch.randn(B, L, D))
    o_p, lse_p = ext.flash_fwd_packed(qkv, H, None, SCALE, seg=seg)
    mask = torch.zeros(B, L, device="cuda")
    bad = {
        "dtype": seg.long(),
        "shape": seg[:, :L // 2].contiguous(),
        "batch": seg[:1].contiguous(),
        "device": seg.cpu(),
        "strided": seg.t().contiguous().t(),
    }
    for why, s in bad.items():
        with pytest.raises(RuntimeError):
            ext.flash_fwd(q, k, v, None, SCALE, seg=s)
        with pytest.raises(RuntimeError):
            ext.flash_bwd_fused(q, k, v, do, None, lse, ddot, SCALE, seg=s)
        with pytest.raises(RuntimeError):
            ext.flash_dq_recompute(q, k, v, do, None, lse, ddot, SCALE, seg=s)
        with pytest.raises(RuntimeError):
            ext.flash_fwd_packed(qkv, H, None, SCALE, seg=s)
        with pytest.raises(RuntimeError):
            ext.flash_bwd_packed(qkv, o_p, do_p, None, lse_p, H, SCALE, seg=s)
    # seg with mask
    with pytest.raises(RuntimeError):
        ext.flash_fwd(q, k, v, mask, SCALE, seg=seg)
    with pytest.raises(RuntimeError):
        ext.flash_bwd_fused(q, k, v, do, mask, lse, ddot, SCALE, seg=seg)
    with pytest.raises(RuntimeError):
        ext.flash_dq_recompute(q, k, v, do, mask, lse, ddot, SCALE, seg=seg)
    with pytest.raises(RuntimeError):
        ext.flash_fwd_packed(qkv, H, mask, SCALE, seg=seg)
    with pytest.raises(RuntimeError):
        ext.flash_bwd_packed(qkv, o_p, do_p, mask, lse_p, H, SCALE, seg=seg)
    with pytest.raises(ValueError):
        ops.flash_attention(q, k, v, mask, SCALE, seg=seg)
    # seg with emit_ds=True
    with pytest.raises(RuntimeError):
        ext.flash_bwd_fused(q, k, v, do, None, lse, ddot, SCALE,
                            emit_ds=True, seg=seg)
    # the existing call forms still work
    ext.flash_bwd_fused(q, k, v, do, None, lse, ddot, SCALE, emit_ds=True)
    ext.flash_bwd_fused(q, k, v, do, None, lse, ddot, SCALE, False, seg)
