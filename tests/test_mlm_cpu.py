"""Masked-LM pretraining on the CPU: the cross-entropy reference behind
ops.fused_cross_entropy, data.mlm.mlm_corrupt, MLTC.encode / mlm_loss,
Trainer.step_mlm (also resumed, also data parallel), train_classifier's MLM
stage and the CLI flags."""
import csv
import os

import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp
import torch.nn.functional as F

from tosem2021_amd import ops
from tosem2021_amd.data.mlm import mlm_corrupt
from tosem2021_amd.data.packing import pack_examples
from tosem2021_amd.extract.schema import TAXONOMY_COLUMNS
from tosem2021_amd.models.classifier import CONFIGS, MLTC
from tosem2021_amd.models.tokenizer import CLS, MASK, N_RESERVED, PAD
from tosem2021_amd.train import TrainConfig, Trainer

PORT = 29931
TINY = CONFIGS["mltc-tiny"]


# ---- cross-entropy reference ------------------------------------------------

def _ce_case(n=37, v=51, seed=0):
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(n, v, generator=g) * 3
    t = torch.randint(0, v, (n,), generator=g)
    t[::5] = -100
    return x, t


def test_cross_entropy_matches_torch_value_and_gradient():
    x, t = _ce_case()
    a = x.clone().requires_grad_()
    b = x.clone().requires_grad_()
    la = ops.fused_cross_entropy(a, t)
    lb = F.cross_entropy(b.float(), t, ignore_index=-100)
    assert la.dim() == 0 and la.dtype == torch.float32
    assert torch.allclose(la, lb, rtol=1e-6, atol=1e-6)
    (la * 3.7).backward()       # an upstream gradient that is not 1
    (lb * 3.7).backward()
    assert torch.allclose(a.grad, b.grad, rtol=1e-5, atol=1e-7)
    assert torch.equal(a.grad[::5], torch.zeros_like(a.grad[::5]))


def test_cross_entropy_all_rows_ignored_is_zero_not_nan():
    x, t = _ce_case()
    a = x.clone().requires_grad_()
    loss = ops.fused_cross_entropy(a, torch.full_like(t, -100))
    assert float(loss.detach()) == 0.0
    loss.backward()
    assert torch.equal(a.grad, torch.zeros_like(a))


@pytest.mark.parametrize("bad", [51, -1, 10 ** 9])
def test_cross_entropy_out_of_range_target_raises(bad):
    x, t = _ce_case()
    t[3] = bad
    with pytest.raises(IndexError):
        ops.fused_cross_entropy(x, t)


def test_cross_entropy_other_ignore_index():
    x, t = _ce_case()
    t2 = torch.where(t == -100, torch.full_like(t, -7), t)
    assert torch.equal(ops.fused_cross_entropy(x, t2, ignore_index=-7),
                       ops.fused_cross_entropy(x, t))


# ---- mlm_corrupt ------------------------------------------------------------

def _batch(b=8, length=64, seed=0, vocab=TINY.vocab_size):
    """A padded batch as the tokenizer makes it: CLS first, PAD tail."""
    g = torch.Generator().manual_seed(seed)
    tokens = torch.randint(N_RESERVED, vocab, (b, length), generator=g)
    lengths = torch.randint(length // 2, length + 1, (b,), generator=g)
    mask = torch.arange(length)[None, :] < lengths[:, None]
    tokens[:, 0] = CLS
    tokens[~mask] = PAD
    return tokens, mask


def test_corrupt_is_a_function_of_seed_and_step():
    tokens, _ = _batch()
    a = mlm_corrupt(tokens, 0.15, 3, 11, TINY.vocab_size)
    b = mlm_corrupt(tokens.clone(), 0.15, 3, 11, TINY.vocab_size)
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])
    c = mlm_corrupt(tokens, 0.15, 3, 12, TINY.vocab_size)
    assert not torch.equal(a[1] != -100, c[1] != -100)
    d = mlm_corrupt(tokens, 0.15, 4, 11, TINY.vocab_size)
    assert not torch.equal(a[1] != -100, d[1] != -100)
    assert a[0].shape == tokens.shape and a[0].dtype == tokens.dtype


@pytest.mark.parametrize("p", [0.15, 0.5, 0.001])
def test_corrupt_selection_count_and_reserved_ids(p):
    tokens, _ = _batch()
    corrupted, targets = mlm_corrupt(tokens, p, 0, 0, TINY.vocab_size)
    maskable = tokens >= N_RESERVED
    sel = targets != -100
    assert int(sel.sum()) == max(1, round(p * int(maskable.sum())))
    # no reserved id (PAD, CLS) is ever selected or changed
    assert not bool((sel & ~maskable).any())
    assert torch.equal(corrupted[~maskable], tokens[~maskable])
    # off the selection: target -100 exactly, tokens untouched
    assert torch.equal(targets[~sel], torch.full_like(targets[~sel], -100))
    assert torch.equal(corrupted[~sel], tokens[~sel])
    # on it: the target is the original id
    assert torch.equal(targets[sel], tokens[sel])
    assert bool(((corrupted[sel] == MASK) |
                 (corrupted[sel] >= N_RESERVED)).all())


def test_corrupt_nothing_maskable():
    tokens = torch.tensor([[CLS, PAD, PAD, PAD]])
    corrupted, targets = mlm_corrupt(tokens, 0.15, 0, 0, TINY.vocab_size)
    assert torch.equal(corrupted, tokens)
    assert torch.equal(targets, torch.full_like(tokens, -100))


def test_corrupt_shares_80_10_10():
    """>= 2,000 selected positions: the MASK share lies in [0.75, 0.85] and
    the kept share in [0.05, 0.15], both more than 5 sigma of the binomial
    (sigma <= sqrt(.8 * .2 / 2000) = 0.009).  vocab 32768, so a random
    replacement hits the original id with probability 3e-5."""
    tokens, _ = _batch(b=64, length=512, seed=5, vocab=32768)
    corrupted, targets = mlm_corrupt(tokens, 0.15, 0, 0, 32768)
    sel = targets != -100
    n = int(sel.sum())
    assert n >= 2000
    masked = float((corrupted[sel] == MASK).sum()) / n
    kept = float((corrupted[sel] == tokens[sel]).sum()) / n
    print(f"selected {n}: MASK {masked:.3f}, kept {kept:.3f}")
    assert 0.75 <= masked <= 0.85
    assert 0.05 <= kept <= 0.15


def _packed(seed=0):
    g = torch.Generator().manual_seed(seed)
    rows = []
    for _ in range(12):
        n = int(torch.randint(3, 40, (1,), generator=g))
        rows.append([CLS] + torch.randint(N_RESERVED, TINY.vocab_size, (n,),
                                          generator=g).tolist())
    return pack_examples(rows, 64, pad_id=PAD)


def test_corrupt_packed_batch_never_masks_cls_or_pad():
    pb = _packed()
    for step in range(5):
        corrupted, targets = mlm_corrupt(pb.tokens, 0.5, 0, step,
                                         TINY.vocab_size)
        special = (pb.tokens == CLS) | (pb.tokens == PAD)
        assert bool(special.any())
        assert torch.equal(corrupted[special], pb.tokens[special])
        assert bool((targets[special] == -100).all())
        assert bool((targets[pb.pos2seg.view_as(targets) < 0] == -100).all())


# ---- model ------------------------------------------------------------------

def _expected_state(cfg):
    """State-dict keys and parameter count of MLTC, from the config."""
    d, f = cfg.d_model, cfg.d_ff
    shapes = {"tok_emb.weight": cfg.vocab_size * d,
              "pos_emb.weight": cfg.max_seq * d}
    for i in range(cfg.n_layers):
        b = f"blocks.{i}."
        shapes.update({
            b + "ln1.weight": d, b + "ln1.bias": d,
            b + "attn.qkv.weight": 3 * d * d, b + "attn.qkv.bias": 3 * d,
            b + "attn.proj.weight": d * d, b + "attn.proj.bias": d,
            b + "ln2.weight": d, b + "ln2.bias": d,
            b + "ffn.up_bias": f, b + "ffn.up.weight": f * d,
            b + "ffn.down.weight": d * f, b + "ffn.down.bias": d})
    shapes.update({"ln_f.weight": d, "ln_f.bias": d})
    for name, n in cfg.heads.items():
        shapes.update({f"heads.{name}.weight": n * d,
                       f"heads.{name}.bias": n})
    return shapes


def test_mlm_adds_no_parameter():
    torch.manual_seed(0)
    model = MLTC(TINY)
    tokens, mask = _batch(4, 32)
    corrupted, targets = mlm_corrupt(tokens, 0.15, 0, 0, TINY.vocab_size)
    model.mlm_loss(corrupted, mask, targets).backward()
    want = _expected_state(TINY)
    assert list(model.state_dict().keys()) == list(want.keys())
    assert sum(p.numel() for p in model.parameters()) == sum(want.values())
    assert [n for n, _ in model.named_parameters()] == list(want.keys())


@pytest.mark.parametrize("packed", [False, True], ids=["padded", "packed"])
def test_mlm_loss_is_encode_index_linear_cross_entropy(packed):
    torch.manual_seed(0)
    model = MLTC(TINY)
    if packed:
        pb = _packed(1)
        corrupted, targets = mlm_corrupt(pb.tokens, 0.15, 0, 0,
                                         TINY.vocab_size)
        args = (corrupted, None)
        kw = dict(packing=pb)
    else:
        tokens, mask = _batch(4, 32)
        corrupted, targets = mlm_corrupt(tokens, 0.15, 0, 0, TINY.vocab_size)
        args = (corrupted, mask)
        kw = {}
    got = model.mlm_loss(*args, targets, **kw)
    h = model.encode(*args, **kw)
    sel = targets.reshape(-1) != -100
    logits = F.linear(h.reshape(-1, h.shape[-1])[sel], model.tok_emb.weight)
    want = F.cross_entropy(logits.float(), targets.reshape(-1)[sel])
    assert torch.allclose(got, want, rtol=1e-6, atol=1e-6), (got, want)


def test_forward_is_encode_then_pool():
    torch.manual_seed(0)
    model = MLTC(TINY)
    tokens, mask = _batch(4, 32)
    out = model(tokens, mask)
    pooled = ops.masked_mean_pool(model.encode(tokens, mask), mask)
    for name, head in model.heads.items():
        assert torch.equal(out[name], head(pooled))


def test_tied_embedding_gradient_is_the_sum_of_both_paths():
    torch.manual_seed(0)
    model = MLTC(TINY)
    tokens, mask = _batch(4, 32)
    corrupted, targets = mlm_corrupt(tokens, 0.15, 0, 0, TINY.vocab_size)
    model.mlm_loss(corrupted, mask, targets).backward()
    tied = model.tok_emb.weight.grad.clone()
    # the same loss with the decoder reading an untied clone of the weight
    dec = model.tok_emb.weight.detach().clone().requires_grad_()
    model.zero_grad()
    h = model.encode(corrupted, mask)
    sel = targets.reshape(-1) != -100
    logits = F.linear(h.reshape(-1, h.shape[-1])[sel], dec)
    F.cross_entropy(logits, targets.reshape(-1)[sel]).backward()
    want = model.tok_emb.weight.grad + dec.grad
    assert float(dec.grad.abs().max()) > 0
    assert float(model.tok_emb.weight.grad.abs().max()) > 0
    # f32 sums in another order; the gradients are of order 1e-2
    assert torch.allclose(tied, want, rtol=1e-5, atol=1e-6)


# ---- trainer ----------------------------------------------------------------

def _trainer(**kw):
    torch.manual_seed(0)
    return Trainer(TrainConfig(model="mltc-tiny", lr=1e-3, warmup_steps=0,
                               dtype="f32", **kw),
                   device=torch.device("cpu"))


def test_step_mlm_learns_a_fixed_batch():
    trainer = _trainer()
    tokens, mask = _batch(8, 32)
    corrupted, targets = mlm_corrupt(tokens, 0.15, 0, 0, TINY.vocab_size)
    losses = [trainer.step_mlm(corrupted, mask, targets) for _ in range(30)]
    assert all(l == l for l in losses), "NaN loss"
    assert losses[-1] < 0.8 * losses[0], losses[::10]


def test_step_mlm_accepts_a_packed_batch():
    trainer = _trainer()
    pb = _packed(2)
    pb.tokens, targets = mlm_corrupt(pb.tokens, 0.15, 0, 0, TINY.vocab_size)
    l0 = trainer.step_mlm(pb, None, targets)
    l1 = trainer.step_mlm(pb, None, targets)
    assert l0 == l0 and l1 < l0


def _mlm_steps(trainer, upto):
    tokens, mask = _batch(8, 32)
    while trainer.step_num < upto:
        corrupted, targets = mlm_corrupt(tokens, 0.15, 7, trainer.step_num,
                                         TINY.vocab_size)
        trainer.step_mlm(corrupted, mask, targets)


def test_step_mlm_resume_is_exact(tmp_path):
    whole = _trainer()
    _mlm_steps(whole, 6)
    first = _trainer()
    _mlm_steps(first, 3)
    path = first.save(str(tmp_path / "ck.pt"))
    torch.manual_seed(123)      # another init: the checkpoint overrides it
    resumed = Trainer(TrainConfig(model="mltc-tiny", lr=1e-3, warmup_steps=0,
                                  dtype="f32"), device=torch.device("cpu"))
    resumed.load(path)
    _mlm_steps(resumed, 6)
    assert torch.equal(resumed.flat.flat, whole.flat.flat)
    assert torch.equal(resumed.flat.master, whole.flat.master)


# ---- library and CLI --------------------------------------------------------

def _write_tiny_taxonomy(path, n=48):
    with open(path, "w", newline="") as f:
        w = csv.DictWriter(f, fieldnames=TAXONOMY_COLUMNS)
        w.writeheader()
        for i in range(n):
            row = {c: "" for c in TAXONOMY_COLUMNS}
            for c in ("regression", "Integration", "end_to_end", "status_test",
                      "negative_test", "value_range", "null_pointer",
                      "logical_statement", "logical_expression",
                      "error_handling", "Approximation", "basic_comparizon"):
                row[c] = 0
            if i % 2:
                row.update(Labels=f"assertTrue(ok_{i}())", status_test=1,
                           Category="Model", Repo="Ray", Model="Correctness")
            else:
                row.update(Labels=f"assertAlmostEqual(a_{i}, b)",
                           Approximation=1,
                           Approximation_Type="rounding_tolence",
                           Category="Data Preprocessing", Repo="tpot",
                           Data="Validity")
            row["Index"] = i
            w.writerow(row)


@pytest.mark.parametrize("pack", [False, True], ids=["padded", "packed"])
def test_train_classifier_mlm_stage(tmp_path, pack):
    from tosem2021_amd.classify.neural import train_classifier
    tax = str(tmp_path / "gold.csv")
    mined = str(tmp_path / "mined.csv")
    _write_tiny_taxonomy(tax)
    _write_tiny_taxonomy(mined, n=64)
    kw = dict(model="mltc-tiny", steps=3, batch=8, seq=32, lr=1e-3,
              device="cpu", pack=pack)
    res = train_classifier(tax, mlm_path=mined, mlm_steps=3, **kw)
    assert res["steps"] == 3 and res["mlm_steps"] == 3
    assert res["mlm_time_s"] >= 0
    for k in ("mlm_loss_first10_mean", "mlm_final_loss", "final_loss"):
        assert res[k] == res[k] and abs(res[k]) < float("inf"), (k, res[k])
    # the fine-tune starts from the MLM weights
    cold = train_classifier(tax, **kw)
    assert "mlm_steps" not in cold
    assert res["final_loss"] != cold["final_loss"]


def test_cli_parses_the_mlm_flags(monkeypatch):
    from tosem2021_amd import cli
    from tosem2021_amd.classify import neural
    seen = {}
    monkeypatch.setattr(neural, "train_classifier",
                        lambda *a, **kw: seen.update(kw) or {})
    cli.main(["train", "--taxonomy", "t.csv"])
    assert seen["mlm_path"] is None and seen["mlm_steps"] == 0
    assert seen["mlm_prob"] == 0.15
    cli.main(["train", "--taxonomy", "t.csv", "--mlm", "mined.csv",
              "--mlm-steps", "40", "--mlm-prob", "0.2"])
    assert (seen["mlm_path"], seen["mlm_steps"], seen["mlm_prob"]) == \
        ("mined.csv", 40, 0.2)


# ---- data parallel ----------------------------------------------------------

def _ddp_worker(rank, world, port, out):
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        torch.manual_seed(100 + rank)   # rank 0's init is broadcast
        trainer = Trainer(TrainConfig(model="mltc-tiny", lr=1e-3,
                                      warmup_steps=0, dtype="f32",
                                      bucket_mb=1),
                          device=torch.device("cpu"))
        tokens, mask = _batch(8, 32)
        per = 8 // world
        sl = slice(rank * per, rank * per + per)
        for step in range(2):
            corrupted, targets = mlm_corrupt(tokens[sl], 0.15, 5 + rank,
                                             step, TINY.vocab_size)
            trainer.step_mlm(corrupted, mask[sl], targets)
        out[rank] = trainer.flat.flat.clone()
    finally:
        dist.destroy_process_group()


@pytest.mark.timeout(300)
def test_ddp_step_mlm_ranks_agree():
    """World size 2 over gloo: the classification heads get no gradient in an
    MLM step, their buckets are reduced by finalize all the same, nothing
    hangs and the ranks end with equal weights that have moved."""
    world = 2
    ctx = mp.get_context("spawn")
    with ctx.Manager() as mgr:
        out = mgr.dict()
        mp.start_processes(_ddp_worker, args=(world, PORT, out),
                           nprocs=world, join=True, start_method="spawn")
        flats = {r: out[r] for r in range(world)}
    assert torch.equal(flats[0], flats[1])
    torch.manual_seed(100)
    init = Trainer(TrainConfig(model="mltc-tiny", dtype="f32"),
                   device=torch.device("cpu")).flat.flat
    assert not torch.equal(flats[0], init)
