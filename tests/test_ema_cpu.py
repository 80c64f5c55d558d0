"""The weight EMA of the fused AdamW step on the CPU: the warm-up schedule,
the reference recurrence against a float64 closed form, the trainer's
bookkeeping (off by default, skipped steps, resume, ema_weights, gradient
accumulation), train_classifier / apply_classifier / the CLI / YAML, and the
gloo DP path."""
import math
import os

import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

from tosem2021_amd import ops
from tosem2021_amd.data.synthetic import synthetic_batch
from tosem2021_amd.models.classifier import CONFIGS
from tosem2021_amd.ops import reference as ref
from tosem2021_amd.train import TrainConfig, Trainer

PORT = 29951          # 29871..29879 and 29931.. belong to other files
F32 = torch.float32


def _trainer(**kw):
    return Trainer(TrainConfig(model="mltc-tiny", lr=1e-3, warmup_steps=0,
                               dtype="f32", **kw), device=torch.device("cpu"))


def _batch(seed=42):
    return synthetic_batch(CONFIGS["mltc-tiny"], 8, 32, seed=seed)


def _state(t):
    f = t.flat
    return [x.clone() for x in (f.flat, f.master, f.m, f.v)]


def _same(a, b):
    return all(torch.equal(x, y) for x, y in zip(a, b))


def _recurrence(ema0, masters, decays):
    """ema * d + master_t * (1 - d) with separate f32 torch ops."""
    e = ema0.clone()
    for w, d in zip(masters, decays):
        d32 = torch.tensor(d, dtype=F32)
        omd = torch.ones((), dtype=F32) - d32
        a = e * d32
        b = w * omd
        e = a + b
    return e


# ---- the schedule -----------------------------------------------------------

def test_ema_decay_at():
    assert ref.ema_decay_at(0.999, 1) == 2 / 11
    assert ref.ema_decay_at(0.999, 2) == 3 / 12
    assert ref.ema_decay_at(0.999, 10 ** 6) == 0.999
    assert ref.ema_decay_at(0.5, 8) == 0.5           # 9 / 18 reaches it
    assert ref.ema_decay_at(0.5, 7) == 8 / 17
    for t in (1, 2, 50, 10 ** 6):
        assert ref.ema_decay_at(0.0, t) == 0.0
    ds = [ref.ema_decay_at(0.9999, t) for t in range(1, 200)]
    assert all(0 < a < b < 1 for a, b in zip(ds, ds[1:]))


# ---- the reference against the closed form ----------------------------------

def _closed_form(ema0, masters, decays):
    """float64: ema_T = (prod d_t) ema_0 + sum_t (1 - d_t)(prod_{s>t} d_s) w_t
    with the f32 decays the ops round their argument to."""
    d = [float(torch.tensor(x, dtype=F32)) for x in decays]
    out = math.prod(d) * ema0.double()
    for t, w in enumerate(masters):
        out += (1 - d[t]) * math.prod(d[t + 1:]) * w.double()
    return out


def _six_steps(decays, grouped):
    n = 1024
    g = torch.Generator().manual_seed(5)
    master = torch.randn(n, generator=g)
    ema0 = torch.randn(n, generator=g)
    p, m, v = master.clone(), torch.zeros(n), torch.zeros(n)
    ema = ema0.clone()
    masters = []
    table = ops.segment_table([101, 202, n], [1.0, 0.5, 0.25],
                              [0.01, 0.0, 0.01], n)
    for step, d in enumerate(decays, start=1):
        grad = torch.randn(n, generator=g)
        if grouped:
            ops.adamw_step_grouped(p, grad, m, v, master, *table, lr=1e-2,
                                   step=step, ema=ema, ema_decay=d)
        else:
            ops.adamw_step(p, grad, m, v, master, lr=1e-2, step=step,
                           ema=ema, ema_decay=d)
        masters.append(master.clone())
    return ema0, masters, ema


@pytest.mark.parametrize("grouped", [False, True], ids=["plain", "grouped"])
def test_reference_matches_closed_form(grouped):
    """rtol 1e-5, atol 1e-7: a few f32 roundings (6e-8 relative each) per
    step over six steps."""
    decays = [ref.ema_decay_at(0.9, t) for t in range(1, 6)] + [0.9]
    ema0, masters, ema = _six_steps(decays, grouped)
    assert masters[0].ne(masters[5]).all()
    want = _closed_form(ema0, masters, decays)
    assert torch.allclose(ema.double(), want, rtol=1e-5, atol=1e-7), \
        float((ema.double() - want).abs().max())
    # and bitwise the three-operation recurrence
    assert torch.equal(ema, _recurrence(ema0, masters, decays))
    # the check tells a schedule that starts one update late from this one
    shifted = [ref.ema_decay_at(0.9, t + 1) for t in range(1, 6)] + [0.9]
    wrong = _closed_form(ema0, masters, shifted)
    assert not torch.allclose(ema.double(), wrong, rtol=1e-5, atol=1e-7)


def test_reference_clipped_skips_ema():
    n = 64
    g = torch.Generator().manual_seed(1)
    master = torch.randn(n, generator=g)
    ema0 = torch.randn(n, generator=g)
    grad = torch.randn(n, generator=g)
    table = ops.segment_table([n], [1.0], [0.01], n)
    for grouped in (False, True):
        for bad in (math.inf, math.nan, None):
            gg = grad.clone()
            if bad is not None:
                gg[3] = bad
            state = ops.grad_clip_state(gg, max_norm=1.0)
            p, m, v, w = master.clone(), torch.zeros(n), torch.zeros(n), \
                master.clone()
            ema = ema0.clone()
            if grouped:
                ops.adamw_step_grouped_clipped(
                    p, gg, m, v, w, *table, lr=1e-2, step=1,
                    clip_state=state, ema=ema, ema_decay=0.5)
            else:
                ops.adamw_step_clipped(p, gg, m, v, w, lr=1e-2, step=1,
                                       clip_state=state, ema=ema,
                                       ema_decay=0.5)
            if bad is None:
                assert torch.equal(ema, _recurrence(ema0, [w], [0.5]))
                assert not torch.equal(w, master)
            else:
                assert torch.equal(ema, ema0) and torch.equal(w, master)


def test_ops_validation():
    n = 64
    p, g, m, v, w = (torch.zeros(n) for _ in range(5))
    table = ops.segment_table([n], [1.0], [0.0], n)
    state = ops.grad_clip_state(torch.ones(n), max_norm=1.0)
    calls = [
        lambda **kw: ops.adamw_step(p, g, m, v, w, lr=1e-3, step=1, **kw),
        lambda **kw: ops.adamw_step_clipped(p, g, m, v, w, lr=1e-3, step=1,
                                            clip_state=state, **kw),
        lambda **kw: ops.adamw_step_grouped(p, g, m, v, w, *table, lr=1e-3,
                                            step=1, **kw),
        lambda **kw: ops.adamw_step_grouped_clipped(
            p, g, m, v, w, *table, lr=1e-3, step=1, clip_state=state, **kw),
    ]
    for call in calls:
        with pytest.raises(ValueError, match="f32"):
            call(ema=torch.zeros(n, dtype=torch.float64), ema_decay=0.5)
        with pytest.raises(ValueError, match="length"):
            call(ema=torch.zeros(n - 4), ema_decay=0.5)
        with pytest.raises(ValueError, match="contiguous"):
            call(ema=torch.zeros(2 * n)[::2], ema_decay=0.5)
        with pytest.raises(ValueError, match="go together"):
            call(ema=torch.zeros(n))
        with pytest.raises(ValueError, match="go together"):
            call(ema_decay=0.5)
        for bad in (1.0, -0.01, math.nan):
            with pytest.raises(ValueError, match=r"\[0, 1\)"):
                call(ema=torch.zeros(n), ema_decay=bad)
    assert all(float(x.abs().sum()) == 0 for x in (p, m, v, w))


# ---- trainer ----------------------------------------------------------------

def test_config_validation():
    assert TrainConfig().ema_decay == 0.0
    assert TrainConfig(ema_decay=0.999).ema_decay == 0.999
    for bad in (1.0, -0.1, 1.5):
        with pytest.raises(ValueError, match="ema_decay"):
            TrainConfig(ema_decay=bad)


def test_off_by_default_and_on_changes_nothing_else():
    tokens, mask, labels = _batch()
    torch.manual_seed(100)
    off = _trainer()
    assert off.flat.ema is None and "ema" not in off.state_dict()
    torch.manual_seed(100)
    on = _trainer(ema_decay=0.99)
    assert on.flat.ema.dtype == F32
    assert on.flat.ema.shape == (on.flat.padded,)
    assert torch.equal(on.flat.ema, on.flat.master)
    assert on.flat.ema.data_ptr() != on.flat.master.data_ptr()
    ema0 = on.flat.ema.clone()
    masters = []
    for _ in range(5):
        off.step(tokens, mask, labels)
        on.step(tokens, mask, labels)
        masters.append(on.flat.master.clone())
    assert _same(_state(on), _state(off))
    assert off.flat.ema is None and "ema" not in off.state_dict()
    assert "ema" in on.state_dict()
    decays = [ref.ema_decay_at(0.99, t) for t in range(1, 6)]
    assert torch.equal(on.flat.ema, _recurrence(ema0, masters, decays))
    assert not torch.equal(on.flat.ema, on.flat.master)


def test_off_takes_todays_op_calls(monkeypatch):
    """With the option off no op sees an ema keyword at all."""
    seen = []
    real = ops.adamw_step
    monkeypatch.setattr(ops, "adamw_step",
                        lambda *a, **kw: seen.append(set(kw)) or real(*a, **kw))
    t = _trainer()
    t.step(*_batch())
    assert seen and not any("ema" in k or "ema_decay" in k for k in seen)
    seen.clear()
    t = _trainer(ema_decay=0.9)
    t.step(*_batch())
    assert seen and all({"ema", "ema_decay"} <= k for k in seen)


@pytest.mark.parametrize("groups", [False, True], ids=["plain", "grouped"])
def test_non_finite_step_leaves_ema_and_warmup(monkeypatch, groups):
    tokens, mask, labels = _batch()
    kw = dict(max_grad_norm=6.0, ema_decay=0.99)
    if groups:
        kw.update(no_decay_1d=True, layer_decay=0.8)
    torch.manual_seed(100)
    t = _trainer(**kw)
    ema0 = t.flat.ema.clone()
    t.step(tokens, mask, labels)
    w1 = t.flat.master.clone()
    before = t.flat.ema.clone()
    assert torch.equal(before, _recurrence(ema0, [w1], [2 / 11]))
    loss_fn = t.model.loss
    with monkeypatch.context() as mp_:
        mp_.setattr(t.model, "loss",
                    lambda lg, lb: loss_fn(lg, lb) * float("nan"))
        t.step(tokens, mask, labels)
    assert (t.step_num, t.opt_step, t.skipped_steps) == (2, 1, 1)
    assert torch.equal(t.flat.ema, before)
    assert torch.equal(t.flat.master, w1)
    # the next applied update is number 2: decay 3 / 12, not 4 / 13
    t.step(tokens, mask, labels)
    assert (t.step_num, t.opt_step, t.skipped_steps) == (3, 2, 1)
    w2 = t.flat.master.clone()
    assert torch.equal(t.flat.ema, _recurrence(before, [w2], [3 / 12]))
    assert not torch.equal(t.flat.ema, _recurrence(before, [w2], [4 / 13]))


def test_resume_is_exact(tmp_path):
    batches = [_batch(40 + i) for i in range(5)]
    torch.manual_seed(100)
    a = _trainer(ema_decay=0.99)
    for i, b in enumerate(batches):
        a.step(*b)
        if i == 2:
            path = a.save(str(tmp_path / "s3.pt"))
    assert "ema" in torch.load(path, weights_only=True)
    torch.manual_seed(7)
    b_ = _trainer(ema_decay=0.99)
    b_.load(path)
    for b in batches[3:]:
        b_.step(*b)
    assert _same(_state(a), _state(b_))
    assert torch.equal(a.flat.ema, b_.flat.ema)


def test_checkpoint_without_ema_seeds_from_master(tmp_path):
    torch.manual_seed(100)
    plain = _trainer()
    plain.step(*_batch())
    path = plain.save(str(tmp_path / "plain.pt"))
    assert "ema" not in torch.load(path, weights_only=True)
    torch.manual_seed(7)
    t = _trainer(ema_decay=0.99)
    assert not torch.equal(t.flat.ema, plain.flat.master)
    t.load(path)
    assert torch.equal(t.flat.master, plain.flat.master)
    assert torch.equal(t.flat.ema, plain.flat.master)
    # and an EMA checkpoint loads into a trainer without the average
    t.step(*_batch())
    with_ema = t.save(str(tmp_path / "ema.pt"))
    plain.load(with_ema)
    assert plain.flat.ema is None
    assert torch.equal(plain.flat.master, t.flat.master)


def test_reset_ema():
    t = _trainer(ema_decay=0.9)
    t.step(*_batch())
    assert not torch.equal(t.flat.ema, t.flat.master)
    buf = t.flat.ema
    t.reset_ema()
    assert t.flat.ema is buf and torch.equal(t.flat.ema, t.flat.master)
    with pytest.raises(RuntimeError, match="ema_decay"):
        _trainer().reset_ema()


def test_ema_weights_context():
    t = _trainer(ema_decay=0.9)
    for _ in range(2):
        t.step(*_batch())
    f = t.flat
    flat_before, ema_before = f.flat.clone(), f.ema.clone()
    master_before = f.master.clone()
    first = next(t.model.parameters())
    for training in (True, False):
        t.model.train(training)
        with t.ema_weights() as model:
            assert model is t.model
            assert torch.equal(f.flat, f.ema.to(f.flat.dtype))
            assert not torch.equal(f.flat, flat_before)
            # the model's parameters are views of the flat buffer
            assert torch.equal(first.data.reshape(-1),
                               f.flat[:first.numel()])
            assert t.model.training == training
        assert torch.equal(f.flat, flat_before)
        assert t.model.training == training
    # restored when the body raises, too
    with pytest.raises(KeyError):
        with t.ema_weights():
            raise KeyError("x")
    assert torch.equal(f.flat, flat_before)
    assert torch.equal(f.ema, ema_before)
    assert torch.equal(f.master, master_before)
    with pytest.raises(RuntimeError, match="ema_decay"):
        with _trainer().ema_weights():
            pass


def test_step_accum_updates_once():
    tokens, mask, labels = _batch()
    torch.manual_seed(100)
    t = _trainer(ema_decay=0.99)
    ema0 = t.flat.ema.clone()
    micros = [(tokens[s], mask[s], {k: v[s] for k, v in labels.items()})
              for s in (slice(0, 4), slice(4, 8))]
    t.step_accum(micros)
    assert t.opt_step == 1
    w1 = t.flat.master.clone()
    assert torch.equal(t.flat.ema, _recurrence(ema0, [w1], [2 / 11]))
    t.step_accum(micros)
    assert t.opt_step == 2
    assert torch.equal(
        t.flat.ema,
        _recurrence(ema0, [w1, t.flat.master], [2 / 11, 3 / 12]))


# ---- classifier, CLI, YAML --------------------------------------------------

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


def test_train_classifier_end_to_end(tmp_path):
    from tosem2021_amd.classify.neural import (apply_classifier,
                                               train_classifier)
    from tosem2021_amd.serve import ClassifierService
    tax = str(tmp_path / "tax.csv")
    _write_tiny_taxonomy(tax)
    kw = dict(model="mltc-tiny", steps=6, batch=8, seq=32, lr=1e-3,
              device="cpu")
    ck, ck_off = str(tmp_path / "ck"), str(tmp_path / "ck_off")
    probs = str(tmp_path / "probs.pt")
    torch.manual_seed(3)        # the model's init draws from the global RNG
    res = train_classifier(tax, ckpt_dir=ck, ema_decay=0.9,
                           dump_probs_path=probs, **kw)
    torch.manual_seed(3)
    off = train_classifier(tax, ckpt_dir=ck_off, **kw)
    # the unprefixed keys report the raw weights: exactly the run without
    assert not any(k.startswith("ema_") for k in off)
    timing = {"train_time_s", "pretrain_time_s"}
    assert {k: v for k, v in res.items()
            if not k.startswith("ema_") and k not in timing} == \
        {k: v for k, v in off.items() if k not in timing}
    evals = [k for k in off if k.endswith(("_f1", "_acc", "_tuned", "_t0.3"))]
    assert "strategy_micro_f1" in evals and "property_micro_f1_tuned" in evals
    for k in evals:
        assert f"ema_{k}" in res, k
    dumped = torch.load(probs, weights_only=True)
    for k in ("val_probs", "train_probs", "ema_val_probs", "ema_train_probs",
              "val_gold", "train_gold"):
        assert k in dumped, k
    assert any(not torch.equal(dumped["val_probs"][h],
                               dumped["ema_val_probs"][h])
               for h in dumped["val_probs"])
    sd = torch.load(Trainer.latest_checkpoint(ck), weights_only=True)
    sd_off = torch.load(Trainer.latest_checkpoint(ck_off), weights_only=True)
    assert "ema" in sd and "ema" not in sd_off
    assert torch.equal(sd["flat"], sd_off["flat"])
    assert not torch.equal(sd["ema"], sd["master"])

    raw = apply_classifier(ck, tax, str(tmp_path / "raw.csv"),
                           model="mltc-tiny", seq=32, device="cpu")
    ema = apply_classifier(ck, tax, str(tmp_path / "ema.csv"),
                           model="mltc-tiny", seq=32, device="cpu",
                           use_ema=True)
    assert len(open(ema).readlines()) == len(open(raw).readlines()) == 41
    with pytest.raises(ValueError, match="ck_off"):
        apply_classifier(ck_off, tax, str(tmp_path / "no.csv"),
                         model="mltc-tiny", seq=32, device="cpu",
                         use_ema=True)
    svc = ClassifierService(ck, model="mltc-tiny", seq=32, device="cpu",
                            use_ema=True)
    assert torch.equal(svc.trainer.flat.flat, sd["ema"])
    assert len(svc.classify(["assertTrue(x)"])) == 1
    with pytest.raises(ValueError, match="ck_off"):
        ClassifierService(ck_off, model="mltc-tiny", seq=32, device="cpu",
                          use_ema=True)


def test_warm_start_reseeds_the_average(tmp_path):
    """After an MLM stage the average starts from the warm-started weights:
    with decay 0 from update 1 on it would equal master, so instead check
    the seed through reset_ema's call."""
    from tosem2021_amd.classify import neural
    tax = str(tmp_path / "tax.csv")
    _write_tiny_taxonomy(tax)
    calls = []
    real = Trainer.reset_ema

    def spy(self):
        calls.append((self.step_num,
                      torch.equal(self.flat.master, self.flat.flat.float())))
        before = None if self.flat.ema is None else self.flat.ema.clone()
        real(self)
        if before is not None:
            calls.append(torch.equal(before, self.flat.ema))
    Trainer.reset_ema = spy
    try:
        neural.train_classifier(tax, model="mltc-tiny", steps=2, batch=8,
                                seq=32, lr=1e-3, device="cpu", mlm_path=tax,
                                mlm_steps=2, ema_decay=0.9)
    finally:
        Trainer.reset_ema = real
    # once at construction, once after the warm start, where it changed ema
    assert calls[0] == (0, True)
    assert calls[-2] == (0, True) and calls[-1] is False


def test_cli_flags_parse(monkeypatch):
    from tosem2021_amd import cli
    from tosem2021_amd.classify import neural
    seen = {}
    monkeypatch.setattr(neural, "train_classifier",
                        lambda **kw: seen.update(kw) or {})
    cli.main(["train", "--taxonomy", "x.csv", "--ema-decay", "0.999"])
    assert seen["ema_decay"] == 0.999
    cli.main(["train", "--taxonomy", "x.csv"])
    assert seen["ema_decay"] == 0.0
    with pytest.raises(SystemExit):
        cli.main(["train", "--taxonomy", "x.csv", "--ema-decay", "1.0"])
    got = {}
    monkeypatch.setattr(neural, "apply_classifier",
                        lambda *a, **kw: got.update(kw) or "out.csv")
    base = ["classify", "--taxonomy", "x.csv", "--ckpt-dir", "ck", "--out",
            "o.csv"]
    cli.main(base + ["--ema"])
    assert got["use_ema"] is True
    cli.main(base)
    assert got["use_ema"] is False


def test_train_classifier_argument_reaches_train_config(monkeypatch):
    from tosem2021_amd.classify import neural

    class Stop(Exception):
        pass

    class FakeDataset:
        def split(self, **kw):
            return self, self

    seen = []

    def fake_trainer(tcfg, **kw):
        seen.append(tcfg)
        raise Stop

    monkeypatch.setattr(neural, "_load_dataset", lambda *a: FakeDataset())
    monkeypatch.setattr(neural, "Trainer", fake_trainer)
    with pytest.raises(Stop):
        neural.train_classifier("x.csv", model="mltc-tiny", device="cpu",
                                ema_decay=0.5)
    assert seen[0].ema_decay == 0.5
    with pytest.raises(Stop):
        neural.train_classifier("x.csv", model="mltc-tiny", device="cpu")
    assert seen[1].ema_decay == 0.0


def test_yaml_key(tmp_path):
    from tosem2021_amd.utils.config import load_config
    p = tmp_path / "exp.yaml"
    p.write_text("train:\n  model: mltc-tiny\n  ema_decay: 0.999\n")
    assert load_config(str(p)).train.ema_decay == 0.999
    p.write_text("train:\n  model: mltc-tiny\n  ema_decay: 1.0\n")
    with pytest.raises(ValueError, match="ema_decay"):
        load_config(str(p))


# ---- DP (gloo, world 2) -----------------------------------------------------

def _worker(rank, world, port, out):
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        torch.manual_seed(100 + rank)   # rank-0 init is broadcast
        t = Trainer(TrainConfig(model="mltc-tiny", lr=1e-3, warmup_steps=0,
                                dtype="f32", bucket_mb=1, ema_decay=0.99),
                    device=torch.device("cpu"))
        ema0 = t.flat.ema.clone()
        tokens, mask, labels = _batch()
        per = 8 // world
        sl = slice(rank * per, rank * per + per)
        masters = []
        for _ in range(3):
            t.step(tokens[sl], mask[sl], {k: v[sl] for k, v in labels.items()})
            masters.append(t.flat.master.clone())
        out[rank] = (ema0, masters, t.flat.ema.clone())
    finally:
        dist.destroy_process_group()


@pytest.mark.timeout(300)
def test_ddp_ranks_agree_on_ema():
    world = 2
    ctx = mp.get_context("spawn")
    with ctx.Manager() as mgr:
        out = mgr.dict()
        mp.start_processes(_worker, args=(world, PORT, out), nprocs=world,
                           join=True, start_method="spawn")
        res = {r: out[r] for r in range(world)}
    # seeded from the broadcast weights, not from each rank's own init
    assert torch.equal(res[0][0], res[1][0])
    assert torch.equal(res[0][2], res[1][2])
    decays = [ref.ema_decay_at(0.99, t) for t in (1, 2, 3)]
    assert torch.equal(res[0][2], _recurrence(res[0][0], res[0][1], decays))
    assert not torch.equal(res[0][2], res[0][1][-1])
