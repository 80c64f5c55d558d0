"""Fused residual dropout on the CPU reference path: the counter-based mask
(Philox4x32-10, reference.dropout_keep), the op against its composition, the
model switch (MLTCConfig.fused_dropout) and bit-exact trainer resume.

The GPU kernels draw the same mask from csrc/philox.h;
tests/test_fused_dropout_gpu.py compares them element by element.
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

# head_dim 64: the packed flash path of the encoder
CFG = MLTCConfig(vocab_size=512, d_model=128, n_heads=2, n_layers=2,
                 d_ff=256, max_seq=64, dropout=0.1, fused_dropout=True,
                 dropout_seed=11)

# Random123's known-answer vectors for philox4x32_10: counter, key, output
KAT = [
    ((0, 0, 0, 0), (0, 0),
     (0x6627e8d5, 0xe169c58d, 0xbc57ac4c, 0x9b00dbd8)),
    ((0xffffffff,) * 4, (0xffffffff,) * 2,
     (0x408f276d, 0x41c83b0e, 0xa20bc7c6, 0x6d5451fd)),
    ((0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344),
     (0xa4093822, 0x299f31d0),
     (0xd16cfe09, 0x94fdcceb, 0x5001e420, 0x24126ea1)),
]


@pytest.mark.parametrize("counter,key,want", KAT)
def test_philox_known_answers(counter, key, want):
    got = ref.philox4x32_10(counter, key)
    assert got.dtype == np.uint32 and got.shape == (4,)
    assert tuple(int(w) for w in got) == want


def test_philox_broadcasts_over_counters():
    """An array of counters gives what one call per counter gives."""
    c0 = np.array([0, 0xffffffff, 0x243f6a88], dtype=np.uint64)
    got = ref.philox4x32_10((c0, 7, 8, 9), (1, 2))
    assert got.shape == (3, 4)
    for i, c in enumerate(c0):
        one = ref.philox4x32_10((int(c), 7, 8, 9), (1, 2))
        assert (got[i] == one).all()


def test_threshold_and_scale():
    assert ref.dropout_threshold(0.1) == (6554, 65536 / (65536 - 6554))
    assert ref.dropout_threshold(0.5) == (32768, 2.0)
    assert ref.dropout_threshold(1e-9)[0] == 1          # clamped, not 0
    assert ref.dropout_threshold(1 - 1e-9)[0] == 65535  # clamped, not 65536
    for p in (0.0, 1.0, -0.1, 1.5):
        with pytest.raises(ValueError):
            ref.dropout_threshold(p)


@pytest.mark.parametrize("N,D,p,seed,call,site", [
    (64, 1024, 0.1, 1234, 0, 0), (37, 136, 0.5, 7, 5, 1)])
def test_keep_rate_and_dependence(N, D, p, seed, call, site):
    keep = ref.dropout_keep(N, D, p, seed, call, site)
    assert keep.dtype == torch.bool and keep.shape == (N, D)
    thr, _ = ref.dropout_threshold(p)
    q = 1 - thr / 65536
    rate = float(keep.float().mean())
    z = (rate - q) / math.sqrt(q * (1 - q) / (N * D))
    print(f"keep rate {rate:.5f}, expected {q:.5f}, z = {z:.2f}")
    assert abs(z) < 4
    assert torch.equal(keep, ref.dropout_keep(N, D, p, seed, call, site))
    for other in [(seed + 1, call, site), (seed, call + 1, site),
                  (seed, call, site + 1), (seed + (1 << 32), call, site)]:
        assert not torch.equal(keep, ref.dropout_keep(N, D, p, *other)), other


def test_keep_is_indexed_by_element_not_by_shape():
    """The packet index is (row * D + col) / 8 of the flattened tensor: the
    same elements keep their bits when the rows are cut elsewhere."""
    a = ref.dropout_keep(6, 64, 0.3, 5, 2, 3)
    b = ref.dropout_keep(3, 128, 0.3, 5, 2, 3)
    assert torch.equal(a.reshape(-1), b.reshape(-1))


# ---- the op against the composition it fuses --------------------------------

def op_inputs(N=37, D=136):
    g = torch.Generator().manual_seed(3)
    x = torch.randn(N, D, generator=g)
    res = torch.randn(N, D, generator=g)
    gamma = 1 + 0.3 * torch.randn(D, generator=g)
    beta = torch.randn(D, generator=g)
    wy = torch.randn(N, D, generator=g)     # weights of the scalar loss
    ws = torch.randn(N, D, generator=g)
    return x, res, gamma, beta, wy, ws


@pytest.mark.parametrize("p", [0.1, 0.5])
def test_op_matches_composition(p):
    seed, call, site = 99, 4, 3
    x, res, gamma, beta, wy, ws = op_inputs()
    N, D = x.shape
    keep = ref.dropout_keep(N, D, p, seed, call, site)
    _, scale = ref.dropout_threshold(p)

    def run(fused):
        leaves = [t.clone().requires_grad_(True)
                  for t in (x, res, gamma, beta)]
        xl, rl, gl, bl = leaves
        if fused:
            y, s = ops.fused_dropout_add_layernorm(xl, rl, gl, bl, 1e-5, p,
                                                   seed, call, site)
        else:
            y, s = ops.fused_add_layernorm(xl, rl * keep * scale, gl, bl,
                                           1e-5)
        ((y * wy).sum() + (s * ws).sum()).backward()
        return y.detach(), s.detach(), [t.grad for t in leaves]

    y0, s0, g0 = run(False)
    y1, s1, g1 = run(True)
    assert torch.equal(y1, y0) and torch.equal(s1, s0)
    for name, a, b in zip(("dx", "dres", "dgamma", "dbeta"), g1, g0):
        assert torch.allclose(a, b, atol=1e-5, rtol=0), name
    dres = g1[1]
    assert float(dres[~keep].abs().max()) == 0.0, "dres where dropped"
    assert float(dres[keep].abs().min()) > 0.0
    assert 0 < int((~keep).sum()) < keep.numel()


def test_op_rejects_bad_p():
    x, res, gamma, beta, _, _ = op_inputs(3, 16)
    for p in (0.0, 1.0, -0.5):
        with pytest.raises(ValueError):
            ops.fused_dropout_add_layernorm(x, res, gamma, beta, 1e-5, p,
                                            0, 0, 0)


# ---- the model switch -------------------------------------------------------

def fused_and_plain():
    torch.manual_seed(0)
    fused = build_model(CFG, dtype=torch.float32)
    plain = build_model(dataclasses.replace(CFG, fused_dropout=False),
                        dtype=torch.float32)
    plain.load_state_dict(fused.state_dict())
    return fused, plain


def spy(monkeypatch, name):
    seen = []
    real = getattr(ops, name)

    def wrapper(*args, **kw):
        seen.append(args)
        return real(*args, **kw)
    monkeypatch.setattr(classifier.ops, name, wrapper)
    return seen


def test_model_masks_follow_the_call_counter():
    model, _ = fused_and_plain()
    tokens, mask, _ = synthetic_batch(CFG, 4, 64, seed=5)
    model.train()
    assert model.dropout_call == 0
    a = model(tokens, mask)
    assert model.dropout_call == 1
    b = model(tokens, mask)                 # call 1: other masks
    assert model.dropout_call == 2
    model.dropout_call = 0
    c = model(tokens, mask)                 # call 0 again
    for k in a:
        assert torch.equal(a[k], c[k]), k
    assert any(not torch.equal(a[k], b[k]) for k in a)
    # torch's global generator plays no part
    model.dropout_call = 0
    torch.manual_seed(12345)
    d = model(tokens, mask)
    for k in a:
        assert torch.equal(a[k], d[k]), k


def test_model_eval_is_todays_path(monkeypatch):
    fused, plain = fused_and_plain()
    tokens, mask, labels = synthetic_batch(CFG, 4, 64, seed=5)
    outs = []
    for m in (fused, plain):
        m.eval()
        m.zero_grad(set_to_none=True)
        logits = m(tokens, mask)
        m.loss(logits, labels).backward()
        outs.append((logits, {n: p.grad for n, p in m.named_parameters()}))
    assert fused.dropout_call == 0          # eval forwards are not counted
    (l0, g0), (l1, g1) = outs
    for k in l0:
        assert torch.equal(l0[k], l1[k]), k
    for n in g0:
        assert torch.equal(g0[n], g1[n]), n


def test_model_routing(monkeypatch):
    model, _ = fused_and_plain()
    tokens, mask, labels = synthetic_batch(CFG, 4, 64, seed=5)
    plain_calls = spy(monkeypatch, "fused_add_layernorm")
    drop_calls = spy(monkeypatch, "fused_dropout_add_layernorm")
    model.train()
    model.dropout_call = 6
    model.loss(model(tokens, mask), labels).backward()
    n = len(model.blocks)
    assert not plain_calls
    assert len(drop_calls) == 2 * n
    # (x, residual, gamma, beta, eps, p, seed, call, site): block i's ln2
    # drops at site 2i, the consumer of its ffn delta at 2i + 1
    assert [c[8] for c in drop_calls] == [0, 1, 2, 3][:2 * n]
    assert {c[5:8] for c in drop_calls} == {(0.1, 11 * 65536, 6)}
    for name, p in model.named_parameters():
        assert p.grad is not None and bool(torch.isfinite(p.grad).all()), name
    del plain_calls[:], drop_calls[:]
    model.eval()
    model(tokens, mask)
    assert len(plain_calls) == 2 * n and not drop_calls


def test_default_config_does_not_route(monkeypatch):
    """fused_dropout is a switch: off by default, F.dropout as before."""
    cfg = dataclasses.replace(CFG, fused_dropout=False)
    assert MLTCConfig().fused_dropout is False
    torch.manual_seed(0)
    model = build_model(cfg, dtype=torch.float32)
    tokens, mask, _ = synthetic_batch(cfg, 2, 64, seed=5)
    drop_calls = spy(monkeypatch, "fused_dropout_add_layernorm")
    model.train()
    model(tokens, mask)
    assert not drop_calls and model.dropout_call == 0


def test_ranks_draw_different_masks():
    model, _ = fused_and_plain()
    tokens, mask, _ = synthetic_batch(CFG, 2, 64, seed=5)
    model.train()
    a = model(tokens, mask)
    model.dropout_call, model.dropout_rank = 0, 1
    b = model(tokens, mask)
    assert any(not torch.equal(a[k], b[k]) for k in a)


# ---- trainer: resume == uninterrupted ---------------------------------------

def test_trainer_resume_is_bit_exact(tmp_path):
    tcfg = TrainConfig(model="mltc-tiny", lr=1e-3, warmup_steps=0,
                       total_steps=8, dtype="f32")
    cpu = torch.device("cpu")
    batches = [synthetic_batch(CFG, 4, 64, seed=20 + i) for i in range(8)]

    torch.manual_seed(0)
    one = Trainer(tcfg, device=cpu, model_cfg=CFG)
    init = {k: v.clone() for k, v in one.state_dict().items()
            if torch.is_tensor(v)}
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
        a, b = one.state_dict()[name], two.state_dict()[name]
        assert torch.equal(a, b), name
        assert not torch.equal(a, init[name]), name

    # without the counter the resumed run draws other masks
    three = Trainer(tcfg, device=cpu, model_cfg=CFG)
    three.load(path)
    three.model.dropout_call = 0
    for b in batches[4:]:
        three.step(*b)
    assert not torch.equal(three.flat.master, one.flat.master)


def test_old_checkpoint_loads_with_counter_zero(tmp_path):
    tcfg = TrainConfig(model="mltc-tiny", dtype="f32")
    tr = Trainer(tcfg, device=torch.device("cpu"), model_cfg=CFG)
    sd = tr.state_dict()
    del sd["dropout_call"]
    path = str(tmp_path / "old.pt")
    torch.save(sd, path)
    tr.model.dropout_call = 9
    tr.load(path)
    assert tr.model.dropout_call == 0
