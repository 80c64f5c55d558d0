"""MXFP8 serving on the CPU: the format's bitwise contract
(ops.reference.mx_quantize / mx_dequantize), the quantised model's wiring,
and the entry points.  The helpers here (the exhaustive sweep, the float64
quantiser, the written-out forward) also serve tests/test_mx_gpu.py.

The format: a row is cut into blocks of 32 consecutive elements; per block,
with E the biased f32 exponent field of the largest magnitude, the scale
byte is s = clamp(E - 8, 0, 254) (e8m0, meaning 2^(s - 127)) and every
element is e4m3fn(clamp(x * 2^(127 - s), -448, 448)), round to nearest even,
subnormals kept.
"""
import functools

import pytest
import torch

from tosem2021_amd import ops
from tosem2021_amd.data.packing import pack_examples
from tosem2021_amd.models.classifier import MLTC, MLTCConfig
from tosem2021_amd.ops import reference

E4M3 = torch.float8_e4m3fn


def e4m3_values(q: torch.Tensor) -> torch.Tensor:
    """The f32 values of e4m3 bytes: +0 and -0 compare equal."""
    return q.view(E4M3).float()


# ---- an independent float64 quantiser, from the format's definition ---------

def _e4m3_table() -> torch.Tensor:
    """The 127 non-negative finite e4m3fn values by code 0..126 (code 127
    and its negative are NaN: 254 finite codes in all)."""
    vals = []
    for code in range(127):
        e, m = code >> 3, code & 7
        vals.append(m * 2.0 ** -9 if e == 0 else (8 + m) * 2.0 ** (e - 10))
    return torch.tensor(vals, dtype=torch.float64)


def quantize_f64(x: torch.Tensor):
    """(q, s) of x [R, K] computed in float64 without any float8 conversion:
    the shared exponent from frexp, the element by nearest-value search over
    the finite e4m3 codes with ties to the even code."""
    R, K = x.shape
    xb = x.double().reshape(R, K // 32, 32)
    amax = xb.abs().amax(-1)
    _, ex = torch.frexp(amax)                   # amax = m * 2^ex, m in [.5, 1)
    E = torch.where(amax >= 2.0 ** -126, ex - 1 + 127, torch.zeros_like(ex))
    s = (E - 8).clamp(0, 254).to(torch.int64)
    scaled = xb * torch.exp2((127 - s).double()).unsqueeze(-1)
    mag = scaled.abs().clamp(max=448.0)
    tab = _e4m3_table()
    hi = torch.searchsorted(tab, mag.reshape(-1)).clamp(max=126)
    lo = (hi - 1).clamp(min=0)
    dlo = mag.reshape(-1) - tab[lo]
    dhi = tab[hi] - mag.reshape(-1)
    take_hi = (dhi < dlo) | ((dhi == dlo) & (hi % 2 == 0))
    code = torch.where(take_hi, hi, lo)
    code = code.reshape(R, K) + 128 * torch.signbit(x.double()).long()
    return code.to(torch.uint8), s.to(torch.uint8)


# ---- the exhaustive sweep ----------------------------------------------------

SWEEP_PIVOTS = (1.0, 1.9375, 2.0 ** -126, 1.5 * 2.0 ** 127, -1.0)


@functools.lru_cache(maxsize=None)
def sweep_input(pivot: float) -> torch.Tensor:
    """bf16 [R, 32]: element 0 of every block is `pivot`, the other 31 run
    through every finite bf16 pattern of magnitude <= |pivot| (all 65,536
    patterns filtered), so the pivot is every block's maximum; the last
    block is filled up with zeros."""
    allp = torch.arange(65536, dtype=torch.int32).to(torch.int16).view(
        torch.bfloat16)
    keep = torch.isfinite(allp) & (allp.float().abs() <= abs(pivot))
    vals = allp[keep]
    pad = -vals.numel() % 31
    vals = torch.cat([vals, vals.new_zeros(pad)]).view(-1, 31)
    piv = torch.full((vals.shape[0], 1), pivot).to(torch.bfloat16)
    assert piv[0, 0].float().item() == pivot
    return torch.cat([piv, vals], dim=1).contiguous()


@functools.lru_cache(maxsize=None)
def sweep_expected(pivot: float):
    return quantize_f64(sweep_input(pivot))


def assert_mx_equal(q, s, q_ref, s_ref):
    assert q.dtype == torch.uint8 and s.dtype == torch.uint8
    assert torch.equal(s.cpu(), s_ref.cpu()), "scale bytes differ"
    a, b = e4m3_values(q.cpu()), e4m3_values(q_ref.cpu())
    assert not torch.isnan(a).any(), "a NaN element was produced"
    assert torch.equal(a, b), (
        f"{int((a != b).sum())} elements differ, first at "
        f"{torch.nonzero(a != b)[0].tolist()}")


# ---- the format ---------------------------------------------------------------

def _block(values):
    x = torch.zeros(1, 32)
    x[0, :len(values)] = torch.tensor(values, dtype=torch.float64).float()
    return x


def test_known_answers():
    x = _block([1.0, 17 / 256, 19 / 256, 21 / 256, 2.0 ** -17, 2.0 ** -18,
                3 * 2.0 ** -18])
    q, s = reference.mx_quantize(x)
    assert s.tolist() == [[119]]
    assert q[0, :7].tolist() == [120, 88, 90, 90, 1, 0, 2]
    assert q[0, 7:].tolist() == [0] * 25
    for amax in (1.8125, 1.9375):       # scaled 464 ties down, 496 saturates
        q, s = reference.mx_quantize(_block([0.5, amax]))
        assert s.tolist() == [[119]] and int(q[0, 1]) == 126
    q, s = reference.mx_quantize(torch.zeros(2, 64))
    assert not s.any() and not q.any()
    assert reference.mx_quantize(_block([2.0 ** -126]))[1].tolist() == [[0]]
    assert reference.mx_quantize(
        _block([1.5 * 2.0 ** 127]))[1].tolist() == [[246]]
    with pytest.raises(ValueError):
        reference.mx_quantize(torch.zeros(2, 48))


def test_known_answers_in_bf16_and_dequantised():
    x = _block([1.0, 17 / 256, 19 / 256, 21 / 256]).bfloat16()
    q, s = reference.mx_quantize(x)
    assert q[0, :4].tolist() == [120, 88, 90, 90]
    d = reference.mx_dequantize(q, s)
    assert d.dtype == torch.float32
    assert d[0, :4].tolist() == [1.0, 16 / 256, 20 / 256, 20 / 256]


@pytest.mark.parametrize("pivot", SWEEP_PIVOTS)
def test_exhaustive_conversion_sweep(pivot):
    x = sweep_input(pivot)
    assert x.shape[0] >= 9          # 258 patterns at the smallest pivot
    q, s = reference.mx_quantize(x)
    assert_mx_equal(q, s, *sweep_expected(pivot))
    assert int(s.max()) < 255


def test_round_trip_error_bound():
    """|dequantize(quantize(x)) - x| <= half an e4m3 step at the scaled
    value (the step of a binade [2^e, 2^(e+1)) is 2^(e-3), and 2^-9 below
    2^-6), or the distance to 448 where the scaled magnitude exceeds it."""
    g = torch.Generator().manual_seed(3)
    x = torch.randn(64, 256, generator=g) * torch.exp2(
        torch.randint(-30, 30, (64, 256), generator=g).float())
    x = x.bfloat16()
    q, s = reference.mx_quantize(x)
    d = reference.mx_dequantize(q, s).double()
    unit = torch.exp2(s.double() - 127).repeat_interleave(32, dim=1)
    scaled = x.double().abs() / unit
    assert float(scaled.max()) < 512 and float(scaled.max()) > 448
    _, ex = torch.frexp(scaled.clamp(min=2.0 ** -6))
    half_step = torch.exp2((ex - 1).double() - 3) / 2
    bound = torch.where(scaled > 448, scaled - 448, half_step) * unit
    err = (d - x.double()).abs()
    assert bool((err <= bound).all()), float((err - bound).max())
    # and the bound is not slack: some element sits on it
    assert bool((err == bound).any())


# ---- the model ----------------------------------------------------------------

MX_CFG = dict(vocab_size=512, d_model=128, n_heads=2, n_layers=2, d_ff=256,
              max_seq=64)
B, L = 2, 64


def make_model(dtype, device="cpu") -> MLTC:
    torch.manual_seed(0)
    m = MLTC(MLTCConfig(**MX_CFG))
    # biases and LayerNorm parameters are initialised to 0 and 1: move them,
    # so that a swapped bias or LayerNorm shows
    g = torch.Generator().manual_seed(1)
    with torch.no_grad():
        for name, p in m.named_parameters():
            if name.endswith("bias") or ".ln" in name or name.startswith(
                    "ln_f"):
                p.add_(torch.randn(p.shape, generator=g) * 0.1)
    return m.to(dtype).to(device).eval()


def make_inputs(device="cpu"):
    """(tokens, mask) padded, and the same examples packed."""
    g = torch.Generator().manual_seed(2)
    lens = [L, 23]
    tokens = torch.randint(1, MX_CFG["vocab_size"], (B, L), generator=g)
    mask = torch.arange(L)[None, :] < torch.tensor(lens)[:, None]
    tokens = tokens * mask
    pb = pack_examples([tokens[i, :n].tolist() for i, n in enumerate(lens)]
                       + [tokens[0, :17].tolist()], L)
    return tokens.to(device), mask.to(device), pb.to(device)


def composed_forward(model: MLTC, tokens, mask=None, packing=None):
    """The quantised forward written out from the public ops and the
    module's parameters: which weight, which scale, which bias and which
    LayerNorm goes where."""
    dt = model.tok_emb.weight.dtype
    if packing is not None:
        x = model.tok_emb(packing.tokens) + model.pos_emb(packing.pos)
        mask_bias, seg = None, packing.seg
    else:
        pos = torch.arange(tokens.shape[1], device=tokens.device)
        x = model.tok_emb(tokens) + model.pos_emb(pos)[None]
        mask_bias = torch.where(mask, 0.0, -1e9).float().contiguous()
        seg = None
    delta = None
    for blk in model.blocks:
        a, f = blk.attn, blk.ffn
        if delta is None:
            q, s = ops.mx_layernorm(x, blk.ln1.weight, blk.ln1.bias,
                                    blk.ln1.eps)
            s1 = x
        else:
            q, s, s1 = ops.mx_add_layernorm(x, delta, blk.ln1.weight,
                                            blk.ln1.bias, blk.ln1.eps)
        qkv = ops.mx_linear(q, s, *ops.mx_quant_rows(a.qkv.weight),
                            a.qkv.bias, dt)
        att = ops.flash_attention_packed(qkv, a.n_heads, mask_bias, a.scale,
                                         seg)
        h = ops.mx_linear(*ops.mx_quant_rows(att),
                          *ops.mx_quant_rows(a.proj.weight), a.proj.bias, dt)
        q, s, s2 = ops.mx_add_layernorm(s1, h, blk.ln2.weight, blk.ln2.bias,
                                        blk.ln2.eps)
        u = ops.mx_linear(q, s, *ops.mx_quant_rows(f.up.weight), None, dt)
        delta = ops.mx_linear(*ops.mx_bias_gelu(u, f.up_bias),
                              *ops.mx_quant_rows(f.down.weight), f.down.bias,
                              dt)
        x = s2
    x, _ = ops.fused_add_layernorm(x, delta, model.ln_f.weight,
                                   model.ln_f.bias, model.ln_f.eps)
    if packing is not None:
        pooled = ops.segment_mean_pool(
            x.reshape(-1, x.shape[-1]), packing.seg_start, packing.seg_len,
            packing.pos2seg)
    else:
        pooled = ops.masked_mean_pool(x, mask)
    return {name: head(pooled) for name, head in model.heads.items()}


def assert_logits_equal(a, b):
    assert a.keys() == b.keys()
    for k in a:
        assert a[k].dtype == b[k].dtype and torch.equal(a[k], b[k]), k


def check_composition(model, tokens, mask, pb):
    with torch.no_grad():
        plain = model(tokens, mask), model(None, packing=pb)
        model.quantize_mx()
        got = model(tokens, mask), model(None, packing=pb)
        want = (composed_forward(model, tokens, mask),
                composed_forward(model, None, packing=pb))
    for g, w, p in zip(got, want, plain):
        assert_logits_equal(g, w)
        # quantised, and still the same model: close to, not equal to, bf16
        d = (g["strategy"].float() - p["strategy"].float()).abs().max()
        assert 0 < float(d) < 0.25
    assert got[1]["strategy"].shape[0] == pb.n_segments


def check_raises_and_clear(model, tokens, mask):
    """Training mode, grad enabled and stale weights raise; clear_mx()
    restores the unquantised logits exactly; the state dict never changes."""
    keys = list(model.state_dict().keys())
    with torch.no_grad():
        before = model(tokens, mask)
    model.quantize_mx()
    assert model.mx_active and list(model.state_dict().keys()) == keys
    with pytest.raises(RuntimeError, match="no_grad"):
        model(tokens, mask)
    model.train()
    with torch.no_grad(), pytest.raises(RuntimeError, match="eval mode"):
        model(tokens, mask)
    model.eval()
    with torch.no_grad():
        model(tokens, mask)
        model.blocks[1].attn.proj.weight.mul_(1.0)      # values unchanged
        with pytest.raises(RuntimeError, match="quantize_mx"):
            model(tokens, mask)
        model.quantize_mx()                             # and again valid
        model(tokens, mask)
        model.clear_mx()
        assert not model.mx_active
        assert list(model.state_dict().keys()) == keys
        assert_logits_equal(model(tokens, mask), before)


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_quantised_forward_is_the_written_out_composition(dtype):
    check_composition(make_model(dtype), *make_inputs())


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_raises_clear_and_state_dict(dtype):
    tokens, mask, _ = make_inputs()
    check_raises_and_clear(make_model(dtype), tokens, mask)


def test_mx_ops_cpu_paths_are_the_reference():
    g = torch.Generator().manual_seed(4)
    x = torch.randn(6, 64, generator=g).bfloat16()
    r = torch.randn(6, 64, generator=g).bfloat16()
    gm = torch.randn(64, generator=g).bfloat16()
    bt = torch.randn(64, generator=g).bfloat16()
    y, sm = ops.fused_add_layernorm(x, r, gm, bt, 1e-5)
    q, s, sm2 = ops.mx_add_layernorm(x, r, gm, bt, 1e-5)
    assert torch.equal(sm, sm2)
    assert_mx_equal(q, s, *reference.mx_quantize(y))
    assert_mx_equal(*ops.mx_layernorm(x, gm, bt, 1e-5),
                    *reference.mx_quantize(ops.fused_layernorm(x, gm, bt)))
    assert_mx_equal(*ops.mx_bias_gelu(x, bt),
                    *reference.mx_quantize(ops.fused_bias_gelu(x, bt)))
    w = torch.randn(32, 64, generator=g).bfloat16()
    qa, sa = ops.mx_quant_rows(x)
    qw, sw = ops.mx_quant_rows(w)
    y = ops.mx_linear(qa, sa, qw, sw, bt[:32])
    want = torch.nn.functional.linear(reference.mx_dequantize(qa, sa),
                                      reference.mx_dequantize(qw, sw),
                                      bt[:32].float())
    assert y.dtype == torch.float32 and torch.equal(y, want)
    with pytest.raises(ValueError):
        ops.mx_linear(qa, sa, qw, sw[:, :1])
    assert ops.mx_supported(64, 384, 128)
    assert not ops.mx_supported(64, 384, 96)
    assert not ops.mx_supported(33, 384, 128)
    assert not ops.mx_supported(64, 40, 128)


# ---- entry points ---------------------------------------------------------------

def test_classify_and_serve_mx_end_to_end_cpu(tmp_path):
    import pandas as pd
    from test_packing import _write_tiny_taxonomy
    from tosem2021_amd.classify.neural import (apply_classifier,
                                               train_classifier)
    from tosem2021_amd.serve import ClassifierService
    tax = str(tmp_path / "tax.csv")
    ck = str(tmp_path / "ck")
    _write_tiny_taxonomy(tax)
    train_classifier(tax, model="mltc-tiny", steps=4, batch=8, seq=32,
                     lr=1e-3, device="cpu", ckpt_dir=ck)
    src = pd.read_csv(tax)
    for pack in (False, True):
        out = apply_classifier(ck, tax, str(tmp_path / f"mx{int(pack)}.csv"),
                               model="mltc-tiny", seq=32, batch=16,
                               device="cpu", pack=pack, mx=True)
        got = pd.read_csv(out)
        assert got["Labels"].tolist() == src["Labels"].tolist()
    texts = [f"assertTrue(x_{i})" + " # pad" * (i % 7) for i in range(11)]
    svc = ClassifierService(ck, model="mltc-tiny", seq=32, device="cpu",
                            mx=True)
    assert svc.trainer.model.mx_active
    assert svc.precision == {"precision": "mxfp8",
                             "mx_gemm_backend": "reference"}
    res = svc.classify(texts)
    assert len(res) == len(texts)
    assert res == svc.classify(texts[:5]) + svc.classify(texts[5:])
    plain = ClassifierService(ck, model="mltc-tiny", seq=32, device="cpu")
    assert not plain.trainer.model.mx_active
    assert plain.precision == {"precision": "f32", "mx_gemm_backend": None}


def check_stale_under_trainer(device, tmp_path):
    """Under a Trainer every parameter is a view into one flat buffer and
    keeps a version counter of its own, so the writers that matter (an EMA
    swap, a checkpoint load, load_ema_weights, an optimizer step) write
    through the buffer without touching it.  Each must make the quantised
    forward raise, and re-quantising must serve the NEW weights."""
    from tosem2021_amd.classify.neural import load_ema_weights
    from tosem2021_amd.train import TrainConfig, Trainer
    dev = torch.device(device)
    tr = Trainer(TrainConfig(model="mltc-tiny", warmup_steps=0,
                             ema_decay=0.5, ckpt_dir=str(tmp_path),
                             dtype="f32" if dev.type == "cpu" else "bf16"),
                 device=dev, model_cfg=MLTCConfig(**MX_CFG))
    model = tr.model
    tokens, mask, _ = make_inputs(dev)
    g = torch.Generator().manual_seed(7)
    labels = {
        "strategy": (torch.rand(B, 19, generator=g) > 0.8).float().to(dev),
        "property": (torch.rand(B, 21, generator=g) > 0.8).float().to(dev),
        "stage": torch.randint(0, 9, (B,), generator=g).to(dev),
        "method": torch.randint(0, 4, (B,), generator=g).to(dev)}
    for _ in range(3):                  # weights, master and average part ways
        tr.step(tokens, mask, labels)
    path = tr.save()

    def forward():
        model.eval()
        with torch.no_grad():
            return model(tokens, mask)

    def assert_stale():
        with pytest.raises(RuntimeError, match="quantize_mx"):
            forward()

    model.quantize_mx()
    raw = forward()
    with tr.ema_weights():              # the swap in ...
        assert_stale()
        model.quantize_mx()
        ema = forward()
    assert_stale()                      # ... and the swap back
    assert not torch.equal(ema["strategy"], raw["strategy"])
    model.quantize_mx()
    assert_logits_equal(forward(), raw)

    tr.flat.flat.mul_(1.5)
    assert_stale()
    model.quantize_mx()
    moved = forward()
    assert not torch.equal(moved["strategy"], raw["strategy"])
    tr.load(path)                       # a checkpoint load
    assert_stale()
    model.quantize_mx()
    assert_logits_equal(forward(), raw)

    load_ema_weights(tr, path)
    assert_stale()
    model.quantize_mx()
    assert_logits_equal(forward(), ema)

    # an optimizer step: it cannot run while quantised (training mode
    # raises), but one taken in between must not go unnoticed either
    stamps = model._mx_versions
    model.clear_mx()
    model.train()
    tr.step(tokens, mask, labels)
    assert model._mx_weight_versions() != stamps


def test_stale_weights_raise_under_a_trainer(tmp_path):
    check_stale_under_trainer("cpu", tmp_path)


def test_service_mx_without_a_model_raises():
    from tosem2021_amd.serve import ClassifierService
    with pytest.raises(ValueError, match="ckpt_dir"):
        ClassifierService(None, mx=True)
    assert ClassifierService(None).precision == {"precision": None,
                                                 "mx_gemm_backend": None}


def test_cli_classify_carries_mx_flag(monkeypatch):
    from tosem2021_amd import cli
    from tosem2021_amd.classify import neural
    seen = {}
    monkeypatch.setattr(neural, "apply_classifier",
                        lambda *a, **kw: seen.update(kw) or "out.csv")
    base = ["classify", "--taxonomy", "t.csv", "--ckpt-dir", "ck", "--out",
            "o.csv"]
    cli.main(base)
    assert seen["mx"] is False
    cli.main(base + ["--mx", "--ema"])
    assert seen["mx"] is True and seen["use_ema"] is True
