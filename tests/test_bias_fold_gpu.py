"""Projection bias gradients folded into the LayerNorm backward (GPU).

`layernorm_bwd(..., want_dres=True)` returns a fourth tensor, dres_sum: the
column sum of the bf16 dx the same call returns.  That is the bias gradient
of the projection whose output was the LayerNorm's residual input, which
autograd otherwise computes with a separate sum(0) over dx.

Shapes: every kernel ln_bwd_launch can pick, at one row, at fewer rows than a
block has waves, and at a ragged second pass of the 1024-block grid:
ln_bwd_t2 (D = 512, 1024), ln_bwd_g (D = 128, 2048) and the wide kernel
(D = 4104 > LN_BWD_G_MAX_D).

Tolerances: dx, dgamma and dbeta keep those of tests/test_ops_gpu.py (through
the helpers of tests/test_ops_gpu_scale.py).  dres_sum against the reference
uses the same column-sum tolerance, atol = 2e-2 + 2e-3 sqrt(N), rtol = 2e-2.
dres_sum against the float64 sum of the RETURNED dx differs by f32
accumulation alone: N - 1 adds, each off by at most u = 2^-24 of a partial
sum that never exceeds sum|dx| of its column, so the error is at most
(N - 1) u / (1 - (N - 1) u) * sum|dx|, which for every N here is below

    |dres_sum - sum64(dx)|  <=  2 * N * 2^-24 * sum|dx|        per column.

`flash_bwd_packed_bias` returns dqkv and dqkv_bias, the column sum of that
dqkv over all B * L rows (bf16, rounded once from the f32 sum).  dqkv must be
bit-identical to flash_bwd_packed's; dqkv_bias goes against the float64
column sum of the returned dqkv with the same column-sum tolerance, N = B * L.
Cases (H = 2): one q-block and one kv-block (L = 32), a ragged last block
(L = 160: the dq kernel's B half does not exist, the last kv workgroup has
three empty waves), L = 384 (two dq workgroups, the second half-empty), the
same with a mask of valid lengths 384 and 200 (a wholly padded 128-row kv
block: skip_tile; partly padded waves: wave_skip) and a segmented batch.

The model-level tests run one config (head_dim 64, so the flash path) with the
routing on and off on the same weights and batch.
"""
import pytest
import torch

from test_ops_gpu_scale import (BF16, TOL_LN_DX, assert_close,
                                assert_reproducible, ln_bwd_reference,
                                ln_inputs, ref_device, tol_dparam)
from tosem2021_amd import ops
from tosem2021_amd.data.packing import pack_examples
from tosem2021_amd.data.synthetic import synthetic_batch
from tosem2021_amd.models.classifier import MLTCConfig, build_model

DRES_CASES = [(1, 1024), (3, 1024), (8229, 1024),
              (1, 512), (3, 512), (8229, 512),
              (1, 128), (3, 128), (2053, 128),
              (1, 2048), (3, 2048), (2053, 2048),
              (517, 4104)]


@pytest.mark.gpu
@pytest.mark.parametrize("with_ds", [False, True])
@pytest.mark.parametrize("N,D", DRES_CASES)
def test_layernorm_bwd_dres_sum(N, D, with_ds):
    x, _, gamma, _, dy, ds = ln_inputs(N, D)
    dev = ref_device(N * D)
    xg, gg, dyg = x.cuda(), gamma.cuda(), dy.cuda()
    dsg = ds.cuda() if with_ds else None
    mean, rstd, dx_w, dg_w, db_w = ln_bwd_reference(
        dyg.to(dev), xg.to(dev), gg.to(dev),
        dsg.to(dev) if with_ds else None)
    mean, rstd = mean.cuda(), rstd.cuda()
    ext = ops.hip_ops()
    plain = ext.layernorm_bwd(dyg, xg, gg, mean, rstd, dsg)
    out = ext.layernorm_bwd(dyg, xg, gg, mean, rstd, dsg, True)
    assert len(plain) == 3 and len(out) == 4
    dx, dgamma, dbeta, dres = out
    assert dres.shape == (D,) and dres.dtype == torch.float32

    assert_close(dx, dx_w, "dx", **TOL_LN_DX)
    assert_close(dgamma, dg_w, "dgamma", **tol_dparam(N))
    assert_close(dbeta, db_w, "dbeta", **tol_dparam(N))

    # against the reference: the f64 column sum of its bf16-rounded dx
    want = dx_w.to(BF16).double().sum(0).float()
    assert float(want.norm()) > 0 and float(dres.norm()) > 0
    assert_close(dres, want, "dres_sum", **tol_dparam(N))

    # against the dx this call returned: f32 accumulation order alone
    own = dx.double().sum(0)
    bound = 2 * N * 2.0 ** -24 * dx.double().abs().sum(0)
    err = (dres.double() - own).abs()
    print(f"dres_sum vs own dx: max err {float(err.max()):.3e}, "
          f"min slack {float((bound - err).min()):.3e}")
    assert bool((err <= bound).all())

    # asking for the third output changes none of the others
    for name, a, b in zip(("dx", "dgamma", "dbeta"), plain, out):
        assert torch.equal(a, b), f"{name} differs with dres_sum requested"

    # bf16 column outputs: the same f32 sums, rounded once by the last stage
    outb = ext.layernorm_bwd(dyg, xg, gg, mean, rstd, dsg, True, True)
    assert torch.equal(outb[0], dx)
    for name, a, b in zip(("dgamma", "dbeta", "dres_sum"), outb[1:], out[1:]):
        assert a.dtype == BF16, name
        assert torch.equal(a, b.to(BF16)), f"bf16 {name} is not the f32 one"
    plainb = ext.layernorm_bwd(dyg, xg, gg, mean, rstd, dsg, False, True)
    for a, b in zip(plainb, outb):
        assert torch.equal(a, b)


@pytest.mark.gpu
@pytest.mark.parametrize("N,D", [(8195, 1024), (2051, 4096)])
def test_bias_gelu_bwd_bf16_out(N, D):
    g = torch.Generator().manual_seed(3000 + D)
    xg = torch.randn(N, D, generator=g).to(BF16).cuda()
    bg = torch.randn(D, generator=g).to(BF16).cuda()
    dyg = torch.randn(N, D, generator=g).to(BF16).cuda()
    dx, dbias = ops.hip_ops().bias_gelu_bwd(dyg, xg, bg)
    dxb, dbiasb = ops.hip_ops().bias_gelu_bwd(dyg, xg, bg, True)
    assert dbias.dtype == torch.float32 and dbiasb.dtype == BF16
    assert float(dbias.norm()) > 0
    assert torch.equal(dx, dxb)
    assert torch.equal(dbiasb, dbias.to(BF16))


@pytest.mark.gpu
@pytest.mark.parametrize("with_ds", [False, True])
@pytest.mark.parametrize("N,D", [(8229, 1024), (8229, 512), (2053, 128),
                                 (2053, 2048), (517, 4104)])
def test_layernorm_bwd_dres_reproducible(N, D, with_ds):
    x, _, gamma, _, dy, ds = ln_inputs(N, D)
    xg, gg, dyg = x.cuda(), gamma.cuda(), dy.cuda()
    dsg = ds.cuda() if with_ds else None
    mean, rstd, _, _, _ = ln_bwd_reference(dyg, xg, gg, None)
    assert_reproducible(lambda: ops.hip_ops().layernorm_bwd(
        dyg, xg, gg, mean, rstd, dsg, True, True))


# ---- flash backward: dqkv_bias ----------------------------------------------

FLASH_H = 2


def flash_case(name):
    """(qkv, do, mask, seg) on the GPU for one named case."""
    B, L = {"L32": (2, 32), "L160": (3, 160), "L384": (2, 384),
            "L384-masked": (2, 384), "L256-seg": (2, 256)}[name]
    g = torch.Generator().manual_seed(4000 + 7 * L + B)
    D = FLASH_H * 64
    qkv = torch.randn(B, L, 3 * D, generator=g).to(BF16).cuda()
    do = torch.randn(B, L, D, generator=g).to(BF16).cuda()
    mask = seg = None
    if name == "L384-masked":
        mask = torch.zeros(B, L)
        mask[1, 200:] = -1e9
        mask = mask.cuda()
    if name == "L256-seg":
        seg = torch.zeros(B, L, dtype=torch.int32)
        for b, cuts in enumerate(((70, 150, 230), (33, 100, 192))):
            for c in cuts:          # three segments, then the padding tail
                seg[b, c:] += 1
        ops.check_segments(seg)
        seg = seg.cuda()
    return qkv, do, mask, seg


def flash_bwd_both(name):
    qkv, do, mask, seg = flash_case(name)
    ext = ops.hip_ops()
    scale = 0.125
    o, lse = ext.flash_fwd_packed(qkv, FLASH_H, mask, scale, seg)
    plain = ext.flash_bwd_packed(qkv, o, do, mask, lse, FLASH_H, scale, seg)
    fold = lambda: ext.flash_bwd_packed_bias(qkv, o, do, mask, lse, FLASH_H,
                                             scale, seg)
    return plain, fold


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["L32", "L160", "L384", "L384-masked",
                                  "L256-seg"])
def test_flash_bwd_packed_bias(name):
    plain, fold = flash_bwd_both(name)
    dqkv, dbias = fold()
    B, L, W = dqkv.shape
    assert dbias.shape == (W,) and dbias.dtype == BF16
    assert torch.equal(dqkv, plain), "dqkv differs with the bias requested"
    assert float(dqkv.float().abs().max()) > 0
    want = dqkv.double().reshape(B * L, W).sum(0).float()
    assert_close(dbias, want, "dqkv_bias", **tol_dparam(B * L))
    # each third on its own: q, k and v land in their own columns
    for i, third in enumerate("qkv"):
        sl = slice(i * W // 3, (i + 1) * W // 3)
        got, ref_ = dbias[sl].float(), want[sl]
        err = float((got - ref_).abs().max())
        print(f"d{third} bias: max|err| {err:.3e} max|want| "
              f"{float(ref_.abs().max()):.3e}")
        assert torch.allclose(got, ref_, **tol_dparam(B * L)), third
        if third != "k":    # the k-bias gradient is zero up to rounding
            assert float(got.abs().max()) > 0, third


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["L160", "L384-masked", "L256-seg"])
def test_flash_bwd_packed_bias_reproducible(name):
    _, fold = flash_bwd_both(name)
    assert_reproducible(fold)


# ---- model level ------------------------------------------------------------

CFG = MLTCConfig(vocab_size=512, d_model=128, n_heads=2, n_layers=2,
                 d_ff=256, max_seq=64)
BIAS_FAMILIES = ("attn.qkv.bias", "attn.proj.bias", "ffn.down.bias")


def model_pair():
    torch.manual_seed(0)
    off = build_model(CFG, fold_bias_grad=False)
    with torch.no_grad():
        for p in off.parameters():
            if p.dim() == 1:
                p.add_((0.1 * torch.randn(p.shape)).to(p.dtype))
    on = build_model(CFG, fold_bias_grad=True)
    on.load_state_dict(off.state_dict())
    return off.cuda(), on.cuda()


def grads_of(model, run):
    model.zero_grad(set_to_none=True)
    loss = run(model)
    loss.backward()
    return loss.detach(), {n: p.grad.clone()
                           for n, p in model.named_parameters()}


def check_routing(run, n_tokens):
    off, on = model_pair()
    loss0, g0 = grads_of(off, run)
    loss1, g1 = grads_of(on, run)
    assert torch.equal(loss0, loss1), "the forward must stay bit-identical"
    assert g0.keys() == g1.keys()
    tol = tol_dparam(n_tokens)
    n_bias = 0
    for name in g0:
        if name.endswith(BIAS_FAMILIES):
            n_bias += 1
            a, b = g1[name].float(), g0[name].float()
            err = float((a - b).abs().max())
            print(f"{name}: max|on - off| {err:.3e}, max|off| "
                  f"{float(b.abs().max()):.3e}")
            assert float(a.abs().max()) > 0 and float(b.abs().max()) > 0, name
            assert torch.allclose(a, b, **tol), name
        else:
            assert torch.equal(g1[name], g0[name]), name
    assert n_bias == 3 * CFG.n_layers


@pytest.mark.gpu
def test_model_routing_on_off():
    tokens, mask, labels = synthetic_batch(CFG, 4, 64, device="cuda", seed=3)
    assert len(set(mask.sum(1).tolist())) > 1, "the mask must be ragged"
    check_routing(lambda m: m.loss(m(tokens, mask), labels), 4 * 64)


@pytest.mark.gpu
def test_model_routing_on_off_packed():
    tokens, mask, labels = synthetic_batch(CFG, 6, 64, seed=4)
    lens = mask.sum(1).tolist()
    lens[0], lens[1] = 20, 30           # rows that hold several segments
    pb = pack_examples([tokens[i, :n].tolist() for i, n in enumerate(lens)],
                       64)
    R = pb.tokens.shape[0]
    assert R < 6
    plabels = {k: pb.gather(v).cuda() for k, v in labels.items()}
    dev = pb.to("cuda")
    check_routing(lambda m: m.loss(m(None, None, packing=dev), plabels),
                  R * 64)
