"""Sequence packing on the CPU: packer properties, packed-vs-unpacked model
equivalence through the fp32 reference path, dataset/classifier plumbing."""
import pytest
import torch

from tosem2021_amd import ops
from tosem2021_amd.data.dataset import TaxonomyDataset
from tosem2021_amd.data.packing import (PackedBatch, pack_examples,
                                        pack_lengths)
from tosem2021_amd.models.classifier import MLTC, MLTCConfig
from tosem2021_amd.models.tokenizer import CLS, PAD, CodeTokenizer

CFG = MLTCConfig(vocab_size=512, d_model=128, n_heads=2, n_layers=2, d_ff=256,
                 max_seq=64)
# token lengths (CLS included) 1 .. 40
LENGTHS = [1, 40, 7, 23, 12, 31, 5]
ROW_LEN = 64


def make_texts(lengths=LENGTHS):
    """One text per requested token length: CLS + (n - 1) identifiers."""
    tok = CodeTokenizer(CFG.vocab_size)
    texts = [" ".join(f"w{i}x{j}" for j in range(n - 1))
             for i, n in enumerate(lengths)]
    assert [len(tok.encode(t, ROW_LEN)) for t in texts] == list(lengths)
    return tok, texts


def _random_examples(seed, n, row_len):
    g = torch.Generator().manual_seed(seed)
    lens = torch.randint(1, row_len + 1, (n,), generator=g).tolist()
    return [torch.randint(8, 500, (k,), generator=g).tolist() for k in lens]


@pytest.mark.parametrize("seed,n,row_len", [(0, 1, 64), (1, 50, 64),
                                            (2, 200, 128), (3, 97, 256)])
def test_packer_properties(seed, n, row_len):
    examples = _random_examples(seed, n, row_len)
    pb = pack_examples(examples, row_len, pad_id=PAD)
    R = pb.tokens.shape[0]
    assert pb.tokens.shape == pb.seg.shape == pb.pos.shape == (R, row_len)
    assert pb.seg.dtype == torch.int32 and pb.pos2seg.dtype == torch.int32
    assert pb.seg_start.dtype == torch.int32 and pb.seg_len.dtype == torch.int32
    ops.check_segments(pb.seg)
    # order is a permutation; every example appears exactly once, intact
    assert sorted(pb.order.tolist()) == list(range(n))
    flat_tok = pb.tokens.reshape(-1)
    flat_pos = pb.pos.reshape(-1)
    flat_seg = pb.seg.reshape(-1)
    for s in range(n):
        a, k = int(pb.seg_start[s]), int(pb.seg_len[s])
        ex = examples[int(pb.order[s])]
        assert flat_tok[a:a + k].tolist() == ex
        # no segment crosses a row; no row exceeds row_len
        assert a // row_len == (a + k - 1) // row_len
        # pos restarts per segment
        assert flat_pos[a:a + k].tolist() == list(range(k))
        # seg_start / seg_len / pos2seg agree with seg
        assert (pb.pos2seg[a:a + k] == s).all()
        assert len(set(flat_seg[a:a + k].tolist())) == 1
        if a % row_len:
            assert int(flat_seg[a - 1]) == int(flat_seg[a]) - 1
        else:
            assert int(flat_seg[a]) == 0
    assert int((pb.pos2seg >= 0).sum()) == int(pb.seg_len.sum()) == \
        sum(len(e) for e in examples)
    # padding: PAD tokens, one id above the row's last real id, pos2seg -1
    pad = pb.pos2seg.view(R, row_len) < 0
    assert (pb.tokens[pad] == PAD).all()
    for r in range(R):
        real = pb.seg[r][~pad[r]]
        assert (pb.seg[r][pad[r]] == int(real.max()) + 1).all()
    # first-fit guarantee: at most one row is filled to <= row_len / 2
    fill = (~pad).sum(1)
    assert int((fill <= row_len // 2).sum()) <= 1
    # unpermute puts per-segment values back into input order
    assert pb.unpermute(pb.order.clone()).tolist() == list(range(n))
    assert pb.gather(torch.arange(n)).tolist() == pb.order.tolist()


def test_pack_lengths_is_deterministic_ffd():
    rows = pack_lengths([10, 30, 30, 64, 4, 34], 64)
    # decreasing length, ties by index, first row that fits
    assert rows == [[3], [5, 1], [2, 0, 4]]
    assert pack_lengths([10, 30, 30, 64, 4, 34], 64) == rows


def test_packer_truncates_and_validates():
    pb = pack_examples([list(range(8, 108))], 64)
    assert int(pb.seg_len[0]) == 64
    with pytest.raises(ValueError):
        pack_examples([[1, 2, 3]], 48)          # row_len % 64 != 0
    with pytest.raises(ValueError):
        pack_examples([[]], 64)


def test_check_segments_rejects_non_monotone():
    ops.check_segments(torch.tensor([[0, 0, 1, 2, 2]], dtype=torch.int32))
    with pytest.raises(ValueError):
        ops.check_segments(torch.tensor([[0, 1, 0, 2]], dtype=torch.int32))
    with pytest.raises(ValueError):
        ops.check_segments(torch.zeros(4, dtype=torch.int32))


def test_encode_packed_matches_encode():
    tok, texts = make_texts()
    pb = tok.encode_packed(texts, 64, ROW_LEN)
    assert isinstance(pb, PackedBatch) and pb.n_segments == len(texts)
    flat = pb.tokens.reshape(-1)
    for s in range(pb.n_segments):
        a, k = int(pb.seg_start[s]), int(pb.seg_len[s])
        assert flat[a:a + k].tolist() == tok.encode(texts[int(pb.order[s])], 64)
        assert int(flat[a]) == CLS


def _model_and_inputs():
    torch.manual_seed(0)
    model = MLTC(CFG).float()
    tok, texts = make_texts()
    toks, mask = tok.encode_batch(texts, 64)
    pb = tok.encode_packed(texts, 64, ROW_LEN)
    g = torch.Generator().manual_seed(5)
    n = len(texts)
    labels = {
        "strategy": (torch.rand(n, CFG.heads["strategy"], generator=g) > .7)
        .float(),
        "property": (torch.rand(n, CFG.heads["property"], generator=g) > .7)
        .float(),
        "stage": torch.randint(0, CFG.heads["stage"], (n,), generator=g),
        "method": torch.randint(0, CFG.heads["method"], (n,), generator=g),
    }
    return model, toks, mask, pb, labels


def test_model_packed_equals_unpacked_f32():
    """Packed logits (unpermuted) and every parameter gradient equal the
    unpacked path's; the only difference is f32 summation order.
    Observed on two machines: max |dlogit| 6.0e-8 and 8.9e-8, max |dgrad|
    1.3e-7 and 1.5e-7 (bound 1e-4)."""
    model, toks, mask, pb, labels = _model_and_inputs()
    assert pb.tokens.shape[0] < len(LENGTHS)        # really shares rows

    ref = model(toks, mask)
    model.loss(ref, labels).backward()
    ref_grads = {n: p.grad.clone() for n, p in model.named_parameters()}
    model.zero_grad()

    out = model(pb.tokens, packing=pb)
    seg_labels = {k: pb.gather(v) for k, v in labels.items()}
    model.loss(out, seg_labels).backward()

    worst = 0.0
    for h in ref:
        got = pb.unpermute(out[h])
        assert got.shape == ref[h].shape
        worst = max(worst, float((got - ref[h]).detach().abs().max()))
        assert torch.allclose(got, ref[h], atol=1e-4, rtol=1e-4), h
    gworst = 0.0
    for n, p in model.named_parameters():
        gworst = max(gworst, float((p.grad - ref_grads[n]).abs().max()))
        assert torch.allclose(p.grad, ref_grads[n], atol=1e-4, rtol=1e-4), n
    print(f"max |dlogit| {worst:.3e}  max |dgrad| {gworst:.3e}")


def test_model_packed_any_head_dim_on_cpu():
    """head_dim != 64 has no flash-shaped reference; the CPU path still
    handles packing (the GPU raises instead of falling back)."""
    torch.manual_seed(1)
    cfg = MLTCConfig(vocab_size=512, d_model=128, n_heads=4, n_layers=1,
                     d_ff=256, max_seq=64)
    model = MLTC(cfg).float()
    tok, texts = make_texts()
    toks, mask = tok.encode_batch(texts, 64)
    pb = tok.encode_packed(texts, 64, ROW_LEN)
    ref = model(toks, mask)
    out = model(None, packing=pb)
    for h in ref:
        assert torch.allclose(pb.unpermute(out[h]), ref[h], atol=1e-4,
                              rtol=1e-4), h


def test_mask_and_seg_together_raise():
    model, toks, mask, pb, _ = _model_and_inputs()
    with pytest.raises(ValueError):
        model(pb.tokens, torch.ones_like(pb.tokens, dtype=torch.bool),
              packing=pb)
    qkv = torch.randn(1, 64, 3 * 128)
    seg = torch.zeros(1, 64, dtype=torch.int32)
    with pytest.raises(ValueError):
        ops.flash_attention_packed(qkv, 2, torch.zeros(1, 64), 0.125, seg=seg)
    q = torch.randn(1, 2, 64, 64)
    with pytest.raises(ValueError):
        ops.flash_attention(q, q, q, torch.zeros(1, 64), 0.125, seg=seg)


def test_segment_mean_pool_reference():
    torch.manual_seed(2)
    pb = pack_examples(_random_examples(7, 9, 64), 64)
    T = pb.n_positions
    x = torch.randn(T, 16, requires_grad=True)
    pooled = ops.segment_mean_pool(x, pb.seg_start, pb.seg_len, pb.pos2seg)
    for s in range(pb.n_segments):
        a, k = int(pb.seg_start[s]), int(pb.seg_len[s])
        assert torch.allclose(pooled[s], x[a:a + k].mean(0), atol=1e-6)
    g = torch.randn_like(pooled)
    pooled.backward(g)
    pad = pb.pos2seg < 0
    assert (x.grad[pad] == 0).all()
    for s in range(pb.n_segments):
        a, k = int(pb.seg_start[s]), int(pb.seg_len[s])
        assert torch.allclose(x.grad[a:a + k], (g[s] / k).expand(k, -1),
                              atol=1e-6)


def _dataset(n=23):
    tok = CodeTokenizer(CFG.vocab_size)
    g = torch.Generator().manual_seed(11)
    lens = torch.randint(1, 50, (n,), generator=g).tolist()
    texts = [" ".join(f"t{i}y{j}" for j in range(k)) for i, k in
             enumerate(lens)]
    ds = TaxonomyDataset(
        texts,
        (torch.rand(n, 19, generator=g) > 0.7).float(),
        (torch.rand(n, 21, generator=g) > 0.7).float(),
        torch.randint(0, 9, (n,), generator=g),
        torch.arange(n) % 4)
    return tok, ds


def test_packed_batches_cover_dataset_once():
    tok, ds = _dataset()
    ds.stage = torch.arange(len(ds))        # stage doubles as the example id
    seen = []
    for pb, labels in ds.packed_batches(tok, 8, 64, 64, shuffle=True, seed=3):
        assert labels["stage"].shape[0] == pb.n_segments
        flat = pb.tokens.reshape(-1)
        for s, ex in enumerate(labels["stage"].tolist()):
            a, k = int(pb.seg_start[s]), int(pb.seg_len[s])
            assert flat[a:a + k].tolist() == tok.encode(ds.texts[ex], 64)
            assert torch.equal(labels["strategy"][s], ds.strategy[ex])
        seen += labels["stage"].tolist()
    assert sorted(seen) == list(range(len(ds)))


def test_head_probs_packed_matches_unpacked():
    from tosem2021_amd.classify.neural import _head_probs
    from tosem2021_amd.train import TrainConfig, Trainer
    torch.manual_seed(4)
    tok, ds = _dataset()
    trainer = Trainer(TrainConfig(model="custom", dtype="f32"),
                      device=torch.device("cpu"), model_cfg=CFG)
    p0, g0 = _head_probs(trainer, ds, tok, 64, batch=8, pack=False)
    p1, g1 = _head_probs(trainer, ds, tok, 64, batch=8, pack=True)
    for h in p0:
        assert torch.equal(g0[h], g1[h])
        assert torch.allclose(p0[h], p1[h], atol=1e-4, rtol=1e-4), h


def test_trainer_step_accepts_packed_batch():
    from tosem2021_amd.train import TrainConfig, Trainer
    torch.manual_seed(6)
    tok, ds = _dataset()
    trainer = Trainer(TrainConfig(model="custom", dtype="f32",
                                  warmup_steps=0),
                      device=torch.device("cpu"), model_cfg=CFG)
    pb, labels = next(ds.packed_batches(tok, 8, 64, 64, shuffle=False))
    l0 = trainer.step(pb, None, labels)
    l1 = trainer.step_accum([(pb, None, labels)])
    assert l0 == l0 and l1 == l1 and l1 < l0


def _write_tiny_taxonomy(path, n=40):
    import csv
    from tosem2021_amd.extract.schema import TAXONOMY_COLUMNS
    flags = ("regression", "Integration", "end_to_end", "status_test",
             "negative_test", "value_range", "null_pointer",
             "logical_statement", "logical_expression", "error_handling",
             "Approximation", "basic_comparizon")
    with open(path, "w", newline="") as f:
        w = csv.DictWriter(f, fieldnames=TAXONOMY_COLUMNS)
        w.writeheader()
        for i in range(n):
            row = {c: "" for c in TAXONOMY_COLUMNS}
            row.update({c: 0 for c in flags})
            if i % 2:
                row.update(Labels="assertTrue(" + "ok_%d() and " % i * (i % 5)
                           + "done)", status_test=1, Category="Model",
                           Repo="Ray", Model="Correctness")
            else:
                row.update(Labels=f"assertAlmostEqual(a_{i}, b)",
                           Approximation=1,
                           Approximation_Type="rounding_tolence",
                           Category="Data Preprocessing", Repo="tpot",
                           Data="Validity")
            row["Index"] = i
            w.writerow(row)


def test_pack_flag_end_to_end_cpu(tmp_path):
    """train --pack, then classify and serve with and without pack: same
    labels, in input order."""
    from tosem2021_amd.classify.neural import (apply_classifier,
                                               train_classifier)
    from tosem2021_amd.serve import ClassifierService
    tax = str(tmp_path / "tax.csv")
    ck = str(tmp_path / "ck")
    _write_tiny_taxonomy(tax)
    res = train_classifier(tax, model="mltc-tiny", steps=4, batch=8, seq=32,
                           lr=1e-3, device="cpu", ckpt_dir=ck, pack=True)
    assert res["steps"] == 4 and res["final_loss"] == res["final_loss"]
    outs = []
    for pack in (False, True):
        out = apply_classifier(ck, tax, str(tmp_path / f"out{int(pack)}.csv"),
                               model="mltc-tiny", seq=32, batch=16,
                               device="cpu", pack=pack)
        outs.append(open(out).read())
    assert outs[0] == outs[1]
    texts = [f"assertTrue(x_{i})" + " # pad" * (i % 7) for i in range(11)]
    plain = ClassifierService(ck, model="mltc-tiny", seq=32, device="cpu")
    packed = ClassifierService(ck, model="mltc-tiny", seq=32, device="cpu",
                               pack=True)
    assert plain.classify(texts) == packed.classify(texts)


def test_cli_verbs_carry_pack_flag(monkeypatch, capsys):
    from tosem2021_amd import cli
    from tosem2021_amd.classify import neural
    seen = {}
    monkeypatch.setattr(neural, "apply_classifier",
                        lambda *a, **kw: seen.update(apply=kw) or "out.csv")
    monkeypatch.setattr(neural, "train_classifier",
                        lambda *a, **kw: seen.update(train=kw) or {})
    base = ["--taxonomy", "t.csv"]
    cli.main(["classify"] + base + ["--ckpt-dir", "ck", "--out", "o.csv"])
    cli.main(["train"] + base)
    assert seen["apply"]["pack"] is False and seen["train"]["pack"] is False
    cli.main(["classify"] + base + ["--ckpt-dir", "ck", "--out", "o.csv",
                                    "--pack"])
    cli.main(["train"] + base + ["--pack"])
    assert seen["apply"]["pack"] is True and seen["train"]["pack"] is True
