"""Dropout on the attention probabilities, CPU reference path: the 4 x 4
block mask (reference.attn_dropout_keep), the two flash ops against the
composition they fuse, the model switch (MLTCConfig.attn_dropout) and
bit-exact trainer resume.

The flash kernels draw the same mask from csrc/philox.h;
tests/test_attn_dropout_gpu.py reads it out of each of them bit by bit.
"""
import dataclasses
import math

import numpy as np
import pytest
import torch

from tosem2021_amd import ops
from tosem2021_amd.data.synthetic import synthetic_batch
from tosem2021_amd.models import classifier
from tosem2021_amd.models.classifier import MLTCConfig, build_model
from tosem2021_amd.ops import reference as ref
from tosem2021_amd.train import TrainConfig, Trainer

SEED, CALL, LAYER = (5 << 32) + 1234, 3, 1    # a seed with both key words set
# the shapes of tests/test_attn_dropout_gpu.py
CASES = [(1, 1, 32, 0.1), (2, 3, 64, 0.1), (2, 2, 96, 0.5),
         (2, 2, 160, 0.25), (1, 2, 288, 0.1)]

# head_dim 64: the packed flash path of the encoder
CFG = MLTCConfig(vocab_size=512, d_model=128, n_heads=2, n_layers=2,
                 d_ff=256, max_seq=64, attn_dropout=0.1, dropout_seed=11)


# ---- the mask ---------------------------------------------------------------

def test_threshold_and_scale():
    assert ref.attn_dropout_threshold(0.1) == (26, 256 / 230)
    assert ref.attn_dropout_threshold(0.5) == (128, 2.0)
    assert ref.attn_dropout_threshold(0.25) == (64, 256 / 192)
    assert ref.attn_dropout_threshold(1e-9)[0] == 1         # clamped, not 0
    assert ref.attn_dropout_threshold(1 - 1e-9)[0] == 255   # clamped, not 256
    for p in (0.0, 1.0, -0.1, 1.5):
        with pytest.raises(ValueError):
            ref.attn_dropout_threshold(p)


@pytest.mark.parametrize("B,H,L,p", CASES)
def test_keep_rate(B, H, L, p):
    keep = ref.attn_dropout_keep(B, H, L, p, SEED, CALL, LAYER)
    assert keep.dtype == torch.bool and keep.shape == (B, H, L, L)
    q = 1 - ref.attn_dropout_threshold(p)[0] / 256
    rate = float(keep.float().mean())
    z = (rate - q) / math.sqrt(q * (1 - q) / keep.numel())
    print(f"keep rate {rate:.5f}, expected {q:.5f}, z = {z:.2f}")
    assert abs(z) < 4
    assert bool(keep.any(dim=-1).all()), "a query row lost every key"


def test_keep_is_the_documented_function():
    """One element at a time from philox4x32_10, at a shape whose blk is not
    the flat index of a simpler layout (H = 3, nb = 9 with a ragged edge)."""
    B, H, L, p = 2, 3, 34, 0.3
    keep = ref.attn_dropout_keep(B, H, L, p, SEED, CALL, LAYER)
    thr, _ = ref.attn_dropout_threshold(p)
    nb = (L + 3) // 4
    for b, h, q, k in [(0, 0, 0, 0), (1, 2, 33, 33), (0, 1, 5, 30),
                       (1, 0, 17, 2), (1, 2, 3, 4), (0, 2, 32, 7)]:
        blk = ((b * H + h) * nb + q // 4) * nb + k // 4
        w = ref.philox4x32_10(
            (blk & 0xffffffff, blk >> 32, 0x10000 + LAYER, CALL),
            (SEED & 0xffffffff, SEED >> 32))
        byte = (int(w[q & 3]) >> (8 * (k & 3))) & 0xff
        assert bool(keep[b, h, q, k]) == (byte >= thr), (b, h, q, k)


def test_mask_depends_on_every_word():
    B, H, L, p = 2, 2, 64, 0.25
    keep = ref.attn_dropout_keep(B, H, L, p, SEED, CALL, LAYER)
    assert torch.equal(keep,
                       ref.attn_dropout_keep(B, H, L, p, SEED, CALL, LAYER))
    for other in [(SEED + 1, CALL, LAYER), (SEED + (1 << 32), CALL, LAYER),
                  (SEED, CALL + 1, LAYER), (SEED, CALL, LAYER + 1)]:
        assert not torch.equal(
            keep, ref.attn_dropout_keep(B, H, L, p, *other)), other
    flat = keep.reshape(B * H, L, L)
    for i in range(B * H):
        for j in range(i + 1, B * H):
            assert not torch.equal(flat[i], flat[j]), (i, j)
    # the first (b, h) does not depend on how many follow it
    assert torch.equal(keep[0, 0], ref.attn_dropout_keep(
        1, 1, L, p, SEED, CALL, LAYER)[0, 0])


def test_site_is_disjoint_from_the_residual_sites():
    """Residual sites run 0 .. 2 * n_layers - 1; layer l's attention site is
    0x10000 + l.  With the same counter words otherwise, the Philox outputs
    of the two families differ."""
    n_layers = max(c.n_layers for c in classifier.CONFIGS.values())
    assert ref.ATTN_DROPOUT_SITE0 == 0x10000 > 2 * n_layers - 1
    key = (SEED & 0xffffffff, SEED >> 32)
    blk = np.arange(64, dtype=np.uint64)
    attn = ref.philox4x32_10((blk, 0, ref.ATTN_DROPOUT_SITE0 + 1, CALL), key)
    for site in range(4):
        res = ref.philox4x32_10((blk, 0, site, CALL), key)
        assert not (attn == res).all(axis=-1).any(), site


# ---- the ops against the composition they fuse ------------------------------

def composition(q, k, v, mask, scale, keep, dscale):
    s = torch.matmul(q, k.transpose(-1, -2)) * scale
    if mask is not None:
        s = s + mask.view(mask.shape[0], 1, 1, -1)
    p = torch.softmax(s, dim=-1)
    return torch.matmul(p * keep * dscale, v)


@pytest.mark.parametrize("p,with_mask", [(0.1, False), (0.5, True)])
def test_op_matches_composition(p, with_mask):
    B, H, L, scale = 2, 2, 32, 0.125
    g = torch.Generator().manual_seed(3)
    q, k, v, w = (torch.randn(B, H, L, 64, generator=g) for _ in range(4))
    mask = None
    if with_mask:
        mask = torch.zeros(B, L)
        mask[1, 20:] = -1e9
    keep = ref.attn_dropout_keep(B, H, L, p, SEED, CALL, LAYER)
    dscale = ref.attn_dropout_threshold(p)[1]

    def run(fused):
        leaves = [t.clone().requires_grad_(True) for t in (q, k, v)]
        if fused:
            o = ops.flash_attention(*leaves, mask, scale,
                                    dropout=(p, SEED, CALL, LAYER))
        else:
            o = composition(*leaves, mask, scale, keep, dscale)
        (o * w).sum().backward()
        return o.detach(), [t.grad for t in leaves]

    o0, g0 = run(False)
    o1, g1 = run(True)
    assert torch.allclose(o1, o0, atol=1e-5, rtol=1e-5)
    for name, a, b in zip(("dq", "dk", "dv"), g1, g0):
        assert torch.allclose(a, b, atol=1e-5, rtol=1e-4), \
            (name, float((a - b).abs().max()))
    # and the mask matters: the undropped op differs
    assert not torch.allclose(ops.flash_attention(q, k, v, mask, scale), o1,
                              atol=1e-3)


def test_packed_op_matches_bhld_op():
    B, H, L, scale, p = 2, 2, 32, 0.125, 0.25
    D = H * 64
    g = torch.Generator().manual_seed(4)
    qkv = torch.randn(B, L, 3 * D, generator=g)
    w = torch.randn(B, L, D, generator=g)
    drop = (p, SEED, CALL, LAYER)
    a = qkv.clone().requires_grad_(True)
    oa = ops.flash_attention_packed(a, H, None, scale, dropout=drop)
    (oa * w).sum().backward()
    b = qkv.clone().requires_grad_(True)
    q, k, v = (t.view(B, L, H, 64).transpose(1, 2) for t in b.split(D, -1))
    ob = ops.flash_attention(q, k, v, None, scale, dropout=drop)
    ob = ob.transpose(1, 2).reshape(B, L, D)
    (ob * w).sum().backward()
    assert torch.equal(oa, ob)
    assert torch.allclose(a.grad, b.grad, atol=1e-6, rtol=1e-6)


def test_p_zero_is_the_call_without_dropout():
    B, H, L, scale = 1, 2, 32, 0.125
    g = torch.Generator().manual_seed(5)
    q, k, v, w = (torch.randn(B, H, L, 64, generator=g) for _ in range(4))
    qkv = torch.randn(B, L, 3 * H * 64, generator=g)

    def grads(fn, *ts):
        leaves = [t.clone().requires_grad_(True) for t in ts]
        o = fn(*leaves)
        o.sum().backward()
        return [o.detach()] + [t.grad for t in leaves]

    for drop in (None, (0.0, SEED, CALL, LAYER)):
        a = grads(lambda *t: ops.flash_attention(*t, None, scale), q, k, v)
        b = grads(lambda *t: ops.flash_attention(*t, None, scale,
                                                 dropout=drop), q, k, v)
        for x, y in zip(a, b):
            assert torch.equal(x, y)
        a = grads(lambda t: ops.flash_attention_packed(t, H, None, scale),
                  qkv)
        b = grads(lambda t: ops.flash_attention_packed(t, H, None, scale,
                                                       dropout=drop), qkv)
        for x, y in zip(a, b):
            assert torch.equal(x, y)


def test_ops_reject_bad_arguments():
    B, H, L = 1, 1, 32
    q = torch.randn(B, H, L, 64)
    qkv = torch.randn(B, L, 3 * H * 64)
    bias = torch.zeros(3 * H * 64, requires_grad=True)
    for p in (1.0, -0.5, 1.5):
        with pytest.raises(ValueError):
            ops.flash_attention(q, q, q, None, 1.0, dropout=(p, 0, 0, 0))
        with pytest.raises(ValueError):
            ops.flash_attention_packed(qkv, H, None, 1.0,
                                       dropout=(p, 0, 0, 0))
    with pytest.raises(ValueError, match="qkv_bias"):
        ops.flash_attention_packed(qkv, H, None, 1.0, qkv_bias=bias,
                                   dropout=(0.1, 0, 0, 0))


# ---- the model switch -------------------------------------------------------

def dropped_and_plain(**over):
    cfg = dataclasses.replace(CFG, **over)
    torch.manual_seed(0)
    model = build_model(cfg, dtype=torch.float32)
    plain = build_model(dataclasses.replace(cfg, attn_dropout=0.0),
                        dtype=torch.float32)
    plain.load_state_dict(model.state_dict())
    return model, plain


def spy(monkeypatch, name):
    seen = []
    real = getattr(ops, name)

    def wrapper(*args, **kw):
        seen.append((args, kw))
        return real(*args, **kw)
    monkeypatch.setattr(classifier.ops, name, wrapper)
    return seen


def test_config_validation():
    assert MLTCConfig().attn_dropout == 0.0
    for p in (1.0, -0.1, 2.0):
        with pytest.raises(ValueError):
            MLTCConfig(attn_dropout=p)


def test_model_eval_is_todays_path():
    model, plain = dropped_and_plain()
    tokens, mask, labels = synthetic_batch(CFG, 4, 64, seed=5)
    outs = []
    for m in (model, plain):
        m.eval()
        m.zero_grad(set_to_none=True)
        logits = m(tokens, mask)
        m.loss(logits, labels).backward()
        outs.append((logits, {n: p.grad for n, p in m.named_parameters()}))
    assert model.dropout_call == 0          # eval forwards are not counted
    (l0, g0), (l1, g1) = outs
    for k in l0:
        assert torch.equal(l0[k], l1[k]), k
    for n in g0:
        assert torch.equal(g0[n], g1[n]), n
    # and in training mode the switch does change the result
    model.train(), plain.train()
    a, b = model(tokens, mask), plain(tokens, mask)
    assert any(not torch.equal(a[k], b[k]) for k in a)


def test_model_masks_follow_the_call_counter():
    """attn_dropout WITHOUT fused_dropout advances the counter by itself."""
    model, plain = dropped_and_plain()
    assert not CFG.fused_dropout and not CFG.dropout
    tokens, mask, _ = synthetic_batch(CFG, 4, 64, seed=5)
    model.train(), plain.train()
    assert model.dropout_call == 0
    a = model(tokens, mask)
    assert model.dropout_call == 1
    b = model(tokens, mask)                 # call 1: other masks
    assert model.dropout_call == 2
    model.dropout_call = 0
    torch.manual_seed(12345)                # torch's generator plays no part
    c = model(tokens, mask)
    for k in a:
        assert torch.equal(a[k], c[k]), k
    assert any(not torch.equal(a[k], b[k]) for k in a)
    plain(tokens, mask)
    assert plain.dropout_call == 0          # nothing active, nothing counted


def test_counter_advances_once_with_both_dropouts(monkeypatch):
    model, _ = dropped_and_plain(dropout=0.1, fused_dropout=True)
    tokens, mask, labels = synthetic_batch(CFG, 2, 64, seed=5)
    attn_calls = spy(monkeypatch, "flash_attention_packed")
    res_calls = spy(monkeypatch, "fused_dropout_add_layernorm")
    model.train()
    model.dropout_call = 6
    model.loss(model(tokens, mask), labels).backward()
    assert model.dropout_call == 7
    n = len(model.blocks)
    # (p, seed, call, layer): one mask per layer, the residual masks' call
    assert [kw.get("dropout", args[6] if len(args) > 6 else None)
            for args, kw in attn_calls] == \
        [(0.1, 11 * 65536, 6, i) for i in range(n)]
    assert {args[5:8] for args, _ in res_calls} == {(0.1, 11 * 65536, 6)}
    for name, p in model.named_parameters():
        assert p.grad is not None and bool(torch.isfinite(p.grad).all()), name


def test_fold_is_off_while_attention_dropout_is_active():
    cfg = dataclasses.replace(CFG)
    model = classifier.MLTC(cfg, fold_bias_grad=True)
    x = torch.zeros(1)
    model.train()
    assert not model._fold_active(x)
    model.eval()
    assert model._fold_active(x)
    # the folded path stays reachable, and exact, with the switch at 0
    plain = classifier.MLTC(dataclasses.replace(cfg, attn_dropout=0.0),
                            fold_bias_grad=True).train()
    assert plain._fold_active(x)


def test_ranks_draw_different_masks():
    model, _ = dropped_and_plain()
    tokens, mask, _ = synthetic_batch(CFG, 2, 64, seed=5)
    model.train()
    a = model(tokens, mask)
    model.dropout_call, model.dropout_rank = 0, 1
    b = model(tokens, mask)
    assert any(not torch.equal(a[k], b[k]) for k in a)


def test_off_lattice_cpu_fallback_draws_the_reference_mask(monkeypatch):
    """head_dim 32 has no flash path: the bmm fallback multiplies P by the
    same reference mask, one per layer."""
    cfg = dataclasses.replace(CFG, n_heads=4)
    torch.manual_seed(0)
    model = build_model(cfg, dtype=torch.float32).train()
    tokens, mask, _ = synthetic_batch(cfg, 2, 48, seed=5)
    seen = []
    real = ref.attn_dropout_keep

    def wrapper(*args):
        seen.append(args)
        return real(*args)
    monkeypatch.setattr(ref, "attn_dropout_keep", wrapper)
    a = model(tokens, mask)
    assert seen == [(2, 4, 48, 0.1, 11 * 65536, 0, i) for i in range(2)]
    model.eval()
    b = model(tokens, mask)
    assert len(seen) == 2
    assert any(not torch.equal(a[k], b[k]) for k in a)


# ---- trainer: resume == uninterrupted ---------------------------------------

def test_trainer_resume_is_bit_exact(tmp_path):
    tcfg = TrainConfig(model="mltc-tiny", lr=1e-3, warmup_steps=0,
                       total_steps=8, dtype="f32")
    cpu = torch.device("cpu")
    batches = [synthetic_batch(CFG, 4, 64, seed=20 + i) for i in range(8)]

    torch.manual_seed(0)
    one = Trainer(tcfg, device=cpu, model_cfg=CFG)
    for b in batches[:4]:
        one.step(*b)
    path = one.save(str(tmp_path / "ckpt.pt"))
    assert one.state_dict()["dropout_call"] == 4
    for b in batches[4:]:
        one.step(*b)

    torch.manual_seed(1)                    # another init: load must replace it
    two = Trainer(tcfg, device=cpu, model_cfg=CFG)
    two.load(path)
    assert two.model.dropout_call == 4
    for b in batches[4:]:
        two.step(*b)
    for name in ("flat", "master", "m", "v"):
        assert torch.equal(one.state_dict()[name], two.state_dict()[name]), \
            name

    # without the counter the resumed run draws other masks
    three = Trainer(tcfg, device=cpu, model_cfg=CFG)
    three.load(path)
    three.model.dropout_call = 0
    for b in batches[4:]:
        three.step(*b)
    assert not torch.equal(three.flat.master, one.flat.master)


def test_cli_and_train_classifier_validate_the_rate():
    from tosem2021_amd import cli
    from tosem2021_amd.classify.neural import train_classifier
    with pytest.raises(SystemExit):
        cli.main(["train", "--taxonomy", "x.csv", "--attn-dropout", "1.0"])
    with pytest.raises(ValueError, match="attn_dropout"):
        train_classifier("does-not-exist.csv", attn_dropout=1.5)
