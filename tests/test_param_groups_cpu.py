"""Parameter groups in the fused AdamW on the CPU: the segment table the
trainer builds, the grouped reference against torch.optim.AdamW with real
param groups, the trainer against a twin stepped by torch.optim.AdamW, the
default path, resume, the skip and the validation."""
import math
import re

import numpy as np
import pytest
import torch

from tosem2021_amd import ops
from tosem2021_amd.data.synthetic import synthetic_batch
from tosem2021_amd.models.classifier import CONFIGS
from tosem2021_amd.ops import reference as ref
from tosem2021_amd.train import TrainConfig, Trainer, param_group_table

TINY = CONFIGS["mltc-tiny"]
WD = 0.01           # TrainConfig's default
DECAY = 0.8
# tests/test_grad_clip_cpu.py::test_reference_matches_torch_clip_and_adamw:
# torch.allclose(master, torch's, atol=1e-5) at allclose's default rtol
TOL = dict(atol=1e-5, rtol=1e-5)


def _trainer(**kw):
    return Trainer(TrainConfig(model="mltc-tiny", lr=1e-3, warmup_steps=0,
                               dtype="f32", **kw), device=torch.device("cpu"))


def _batch():
    return synthetic_batch(TINY, 8, 32, seed=42)


def _state(t):
    f = t.flat
    return [x.clone() for x in (f.flat, f.master, f.m, f.v)]


def _same(a, b):
    # bitwise: NaN-safe and sign-of-zero-safe, unlike torch.equal
    return all(torch.equal(x.view(torch.int32), y.view(torch.int32))
               for x, y in zip(a, b))


def _expected(name, p, n_layers, layer_decay=DECAY, no_decay_1d=True):
    """(lr_mult, wd) of a parameter from its name and dim(), written out
    here independently of train.param_depth / param_group_table."""
    if name in ("tok_emb.weight", "pos_emb.weight"):
        depth = 0
    else:
        blk = re.match(r"blocks\.(\d+)\.", name)
        if blk:
            depth = int(blk.group(1)) + 1
        else:
            assert name.startswith(("ln_f.", "heads.")), name
            depth = n_layers + 1
    wd = 0.0 if (no_decay_1d and p.dim() == 1) else WD
    return layer_decay ** (n_layers + 1 - depth), wd


# ---- the table --------------------------------------------------------------

def test_table_maps_every_parameter_of_tiny():
    t = _trainer(no_decay_1d=True, layer_decay=DECAY)
    ends, mults, wds = param_group_table(
        t.model, TINY.n_layers, t.flat.padded, weight_decay=WD,
        no_decay_1d=True, layer_decay=DECAY)
    S = len(ends)
    assert len(mults) == len(wds) == S
    assert S == 24      # counted by hand: 1 (embeddings) + 7 + 7 + 9
    assert all(b > a for a, b in zip([0] + ends, ends))
    assert ends[-1] == t.flat.padded
    # the merge: neighbours differ
    assert all((mults[i], wds[i]) != (mults[i + 1], wds[i + 1])
               for i in range(S - 1))
    seg_of = np.searchsorted(np.asarray(ends), np.arange(t.flat.padded),
                             side="right")
    mult_e, wd_e = np.asarray(mults)[seg_of], np.asarray(wds)[seg_of]
    off = 0
    seen = set()
    for (name, p), want_off in zip(t.model.named_parameters(),
                                   t.flat.offsets):
        assert off == want_off, name
        mult, wd = _expected(name, p, TINY.n_layers)
        seen.add((mult, wd))
        n = p.numel()
        assert (mult_e[off:off + n] == mult).all(), name
        assert (wd_e[off:off + n] == wd).all(), name
        off += n
    assert off == t.flat.numel
    # the padding tail joins the last segment
    assert (seg_of[off:] == S - 1).all()
    assert len(seen) == 7   # depths 0..3, 1-D and 2-D, no 1-D at depth 0
    # heads at the scheduled rate, embeddings at the smallest
    assert mults[-1] == 1.0 and mults[0] == DECAY ** 3 == min(mults)
    # what the trainer uploaded is this table
    se, sm, sw = t._seg_table
    assert se.dtype == torch.int64 and se.tolist() == ends
    assert torch.equal(sm, torch.tensor(mults, dtype=torch.float32))
    assert torch.equal(sw, torch.tensor(wds, dtype=torch.float32))


def test_table_head_offsets_are_off_the_lattice():
    """The boundaries the kernel must handle: head tensors start at offsets
    that are no multiple of 4, and heads.method.bias is a 4-element segment
    across two 4-wide groups."""
    t = _trainer(no_decay_1d=True, layer_decay=DECAY)
    off = dict(zip((n for n, _ in t.model.named_parameters()),
                   t.flat.offsets))
    assert off["heads.property.weight"] == 341395
    assert off["heads.property.bias"] == 344083
    assert off["heads.method.weight"] == 345265
    assert off["heads.method.bias"] == 345777
    ends = t._seg_table[0].tolist()
    for o in (341395, 344083, 345265, 345777):
        assert o % 4 and o in ends


def test_table_with_both_options_off_is_one_segment():
    t = _trainer()
    assert t._seg_table is None
    ends, mults, wds = param_group_table(
        t.model, TINY.n_layers, t.flat.padded, weight_decay=0.03)
    assert (ends, mults, wds) == ([t.flat.padded], [1.0], [0.03])


# ---- the reference ----------------------------------------------------------

def test_reference_matches_torch_param_groups():
    torch.manual_seed(7)
    n = 64
    # a 1-element segment first and at [11, 12); ends = 1, 2, 3 mod 4
    ends = [1, 6, 11, 12, 40, n]
    mults = [1.0, 0.8, 0.64, 0.5, 1.0, 0.3]
    wds = [0.05, 0.0, 0.05, 0.1, 0.0, 0.02]
    assert {e % 4 for e in ends} >= {1, 2, 3}
    table = ops.segment_table(ends, mults, wds, n)
    hp = dict(beta1=0.9, beta2=0.999, eps=1e-8)
    grad_scale = 0.25
    master = torch.randn(n)
    p, m, v = master.clone(), torch.zeros(n), torch.zeros(n)
    starts = [0] + ends[:-1]
    tps = [master[a:b].clone().requires_grad_(True)
           for a, b in zip(starts, ends)]
    opt = torch.optim.AdamW(
        [dict(params=[tp], weight_decay=wd) for tp, wd in zip(tps, wds)],
        lr=1.0, betas=(0.9, 0.999), eps=1e-8)
    for step, lr in enumerate((1e-2, 7e-3, 1.2e-2, 3e-3, 9e-3), start=1):
        g = torch.randn(n)
        for tp, group, mult, a, b in zip(tps, opt.param_groups, mults,
                                         starts, ends):
            tp.grad = g[a:b] * grad_scale
            group["lr"] = lr * mult
        opt.step()
        ops.adamw_step_grouped(p, g, m, v, master, *table, lr=lr, step=step,
                               grad_scale=grad_scale, **hp)
    want = torch.cat([tp.detach() for tp in tps])
    print("max|err|", float((master - want).abs().max()))
    assert torch.allclose(master, want, **TOL)
    assert torch.equal(p, master)
    # the groups matter at this tolerance: one lr and wd for all is far off
    one = master.clone()
    ref.adamw_step(one.clone(), g, m.clone(), v.clone(), one, lr=9e-3,
                   wd=0.05, step=6, **hp)
    two = master.clone()
    ref.adamw_step_grouped(two.clone(), g, m.clone(), v.clone(), two, *table,
                           lr=9e-3, step=6, **hp)
    assert not torch.allclose(one, two, **TOL)


def test_reference_one_segment_is_the_ungrouped_step():
    torch.manual_seed(8)
    n = 40
    master = torch.randn(n)
    g = torch.randn(n)
    a = [master.clone(), torch.zeros(n), torch.zeros(n), master.clone()]
    b = [x.clone() for x in a]
    table = ops.segment_table([n], [1.0], [0.05], n)
    for step in (1, 2, 3):
        ops.adamw_step(a[0], g, a[1], a[2], a[3], lr=1e-2, wd=0.05,
                       step=step, grad_scale=0.5)
        ops.adamw_step_grouped(b[0], g, b[1], b[2], b[3], *table, lr=1e-2,
                               step=step, grad_scale=0.5)
    assert _same(a, b)


def test_reference_clipped_skip_leaves_buffers():
    torch.manual_seed(5)
    n = 64
    bufs = [torch.randn(n), torch.rand(n), torch.rand(n), torch.randn(n)]
    p, m, v, master = (b.clone() for b in bufs)
    g = torch.randn(n)
    g[-1] = math.nan
    st = ops.grad_clip_state(g, max_norm=1.0)
    assert float(st[2]) == 0.0
    table = ops.segment_table([3, 17, n], [1.0, 0.5, 0.25], [0.0, 0.1, 0.0],
                              n)
    ops.adamw_step_grouped_clipped(p, g, m, v, master, *table, lr=1e-2,
                                   step=1, clip_state=st)
    assert _same([p, m, v, master], bufs)
    # and a finite gradient steps at the clipped scale
    g[-1] = 0.5
    st = ops.grad_clip_state(g, max_norm=1.0)
    assert float(st[2]) == 1.0 and float(st[1]) < 1.0
    q = [b.clone() for b in bufs]
    ops.adamw_step_grouped_clipped(p, g, m, v, master, *table, lr=1e-2,
                                   step=1, clip_state=st)
    ops.adamw_step_grouped(q[0], g, q[1], q[2], q[3], *table, lr=1e-2,
                           step=1, grad_scale=float(st[1]))
    assert _same([p, m, v, master], q)
    assert not torch.equal(master, bufs[3])


# ---- the trainer ------------------------------------------------------------

@pytest.mark.parametrize("max_norm", [0.0, 6.0], ids=["noclip", "clip"])
def test_trainer_matches_torch_param_groups(max_norm):
    """A twin model stepped by torch.optim.AdamW with one param group per
    parameter, built here from the names.  The unclipped norm of step 1 is
    11.10 (tests/test_grad_clip_cpu.py): 6.0 clips."""
    tokens, mask, labels = _batch()
    torch.manual_seed(100)
    a = _trainer(no_decay_1d=True, layer_decay=DECAY, max_grad_norm=max_norm)
    torch.manual_seed(100)
    b = _trainer()
    assert _same(_state(a), _state(b))
    names = [n for n, _ in b.model.named_parameters()]
    groups, group_mult = [], []
    for name, p in zip(names, b.flat.params):
        mult, wd = _expected(name, p, TINY.n_layers)
        groups.append(dict(params=[p], weight_decay=wd))
        group_mult.append(mult)
    opt = torch.optim.AdamW(groups, lr=1.0, betas=(b.cfg.beta1, b.cfg.beta2),
                            eps=b.cfg.eps)
    clipped = []
    for _ in range(4):
        a.step(tokens, mask, labels)
        # the same gradients: a's, which its step leaves unscaled in place.
        # (Gradients of b's own would differ in the last bits, and Adam
        # turns that into +-lr where the true gradient is zero, such as the
        # key bias of attn.qkv.)
        b.flat.grad_flat.copy_(a.flat.grad_flat)
        if max_norm:
            norm = float(torch.nn.utils.clip_grad_norm_(b.flat.params,
                                                        max_norm))
            assert a.metrics["grad_norm"] == pytest.approx(norm, rel=1e-5)
            clipped.append(norm > max_norm)
        b.step_num += 1
        for group, mult in zip(opt.param_groups, group_mult):
            group["lr"] = b._lr() * mult
        opt.step()
    if max_norm:
        assert any(clipped), clipped
    live = slice(0, b.flat.numel)
    diff = float((a.flat.flat[live] - b.flat.flat[live]).abs().max())
    print(f"max|a - b| {diff:.3e}")
    assert torch.allclose(a.flat.flat[live], b.flat.flat[live], **TOL)
    assert torch.equal(a.flat.flat, a.flat.master)
    assert a.opt_step == a.step_num == 4
    # the options matter at this tolerance
    torch.manual_seed(100)
    c = _trainer(max_grad_norm=max_norm)
    for _ in range(4):
        c.step(tokens, mask, labels)
    assert not torch.allclose(a.flat.flat, c.flat.flat, **TOL)
    # the logged rate is the scheduled base rate
    from tosem2021_amd.utils.metrics import get_metrics
    assert get_metrics()._history[-1]["lr"] == c._lr()


@pytest.mark.parametrize("max_norm", [0.0, 6.0], ids=["noclip", "clip"])
def test_defaults_take_the_old_path(monkeypatch, max_norm):
    calls = []
    for name in ("adamw_step_grouped", "adamw_step_grouped_clipped"):
        monkeypatch.setattr(
            ops, name, lambda *a, _n=name, **kw: calls.append(_n))
    tokens, mask, labels = _batch()
    torch.manual_seed(100)
    new = _trainer(max_grad_norm=max_norm, no_decay_1d=False,
                   layer_decay=1.0)
    torch.manual_seed(100)
    old = _trainer(max_grad_norm=max_norm)
    for _ in range(3):
        new.step(tokens, mask, labels)
        old.step(tokens, mask, labels)
    assert calls == []
    assert new._seg_table is None
    assert _same(_state(new), _state(old))
    # and with an option on, the grouped op is what runs
    on = _trainer(max_grad_norm=max_norm, no_decay_1d=True)
    before = _state(on)
    on.step(tokens, mask, labels)
    assert calls == ["adamw_step_grouped_clipped" if max_norm
                     else "adamw_step_grouped"]
    assert _same(_state(on), before)    # the spy swallowed the step


def test_resume_rebuilds_the_table(tmp_path):
    tokens, mask, labels = _batch()
    kw = dict(no_decay_1d=True, layer_decay=DECAY, max_grad_norm=6.0)
    torch.manual_seed(100)
    whole = _trainer(**kw)
    for _ in range(4):
        whole.step(tokens, mask, labels)
    torch.manual_seed(100)
    first = _trainer(**kw)
    for _ in range(2):
        first.step(tokens, mask, labels)
    path = first.save(str(tmp_path / "a.pt"))
    assert set(torch.load(path, weights_only=True)) == {
        "step", "opt_step", "skipped_steps", "dropout_call", "flat",
        "master", "m", "v", "model"}          # checkpoints are unchanged
    torch.manual_seed(1)                      # another init, overwritten
    second = _trainer(**kw)
    second.load(path)
    for _ in range(2):
        second.step(tokens, mask, labels)
    assert _same(_state(second), _state(whole))
    assert second.step_num == second.opt_step == 4


# ---- validation and plumbing ------------------------------------------------

@pytest.mark.parametrize("bad", [0.0, 1.5, -1.0, math.nan])
def test_layer_decay_out_of_range_raises(bad):
    with pytest.raises(ValueError, match="layer_decay"):
        TrainConfig(layer_decay=bad)


def test_layer_decay_bounds_accepted():
    assert TrainConfig(layer_decay=1.0).layer_decay == 1.0
    assert TrainConfig(layer_decay=1e-3).layer_decay == 1e-3
    assert TrainConfig().no_decay_1d is False
    assert TrainConfig().layer_decay == 1.0


def test_bad_tables_raise():
    n = 2048
    good = (list(range(2, n + 1, 2)), [1.0] * 1024, [0.0] * 1024)
    assert ops.MAX_SEGMENTS == 1024
    ops.check_segment_table(*good, n)                       # S = 1024 passes
    too_many = list(range(1, 1025)) + [n]
    with pytest.raises(ValueError, match="1025"):
        ops.check_segment_table(too_many, [1.0] * 1025, [0.0] * 1025, n)
    with pytest.raises(ValueError):
        ops.check_segment_table([], [], [], n)
    for ends in ([4, 4, n], [8, 4, n], [0, 4, n], [-4, 4, n]):
        with pytest.raises(ValueError, match="increasing"):
            ops.check_segment_table(ends, [1.0] * 3, [0.0] * 3, n)
    for last in (n - 4, n + 4):
        with pytest.raises(ValueError, match="end at n"):
            ops.check_segment_table([4, last], [1.0] * 2, [0.0] * 2, n)
    with pytest.raises(ValueError, match="one length"):
        ops.check_segment_table([4, n], [1.0], [0.0] * 2, n)
    with pytest.raises(ValueError):
        ops.segment_table([8, 4, n], [1.0] * 3, [0.0] * 3, n)
    # the step itself checks what it can see: all of a CPU table
    bufs = [torch.zeros(n) for _ in range(5)]
    i64, f32 = torch.int64, torch.float32

    def step(ends, mults, wds):
        ops.adamw_step_grouped(*bufs, ends, mults, wds, lr=1e-3, step=1)

    with pytest.raises(ValueError, match="1025"):
        step(torch.tensor(too_many), torch.ones(1025), torch.zeros(1025))
    with pytest.raises(ValueError, match="increasing"):
        step(torch.tensor([8, 4, n]), torch.ones(3), torch.zeros(3))
    with pytest.raises(ValueError, match="end at n"):
        step(torch.tensor([4, n - 4]), torch.ones(2), torch.zeros(2))
    with pytest.raises(ValueError, match="int64"):
        step(torch.tensor([4, n], dtype=torch.int32), torch.ones(2),
             torch.zeros(2))
    with pytest.raises(ValueError, match="f32"):
        step(torch.tensor([4, n]), torch.ones(2, dtype=torch.float64),
             torch.zeros(2))
    with pytest.raises(ValueError, match="one length"):
        step(torch.tensor([4, n]), torch.ones(3), torch.zeros(2))
    se, sm, sw = ops.segment_table([4, n], [1.0, 0.5], [0.0, 0.1], n)
    assert (se.dtype, sm.dtype, sw.dtype) == (i64, f32, f32)
    assert all(float(b.abs().max()) == 0.0 for b in bufs)   # nothing ran


def test_cli_flags_reach_train_classifier(monkeypatch, capsys):
    from tosem2021_amd import cli
    from tosem2021_amd.classify import neural
    seen = {}
    monkeypatch.setattr(neural, "train_classifier",
                        lambda **kw: seen.update(kw) or {})
    cli.main(["train", "--taxonomy", "x.csv", "--weight-decay", "0.1",
              "--no-decay-1d", "--layer-decay", "0.75"])
    assert (seen["weight_decay"], seen["no_decay_1d"],
            seen["layer_decay"]) == (0.1, True, 0.75)
    cli.main(["train", "--taxonomy", "x.csv"])
    assert (seen["weight_decay"], seen["no_decay_1d"],
            seen["layer_decay"]) == (0.01, False, 1.0)
    with pytest.raises(SystemExit):
        cli.main(["train", "--help"])
    text = " ".join(capsys.readouterr().out.split())
    assert "final fine-tune stage only" in text


def test_layer_decay_reaches_the_fine_tune_stage_only(monkeypatch):
    from tosem2021_amd.classify import neural

    class Stop(Exception):
        pass

    class FakeDataset:
        def split(self, **kw):
            return self, self

        def pos_weights(self):
            return {}

    seen = []

    class FakeTrainer(Trainer):
        def __init__(self, tcfg, **kw):
            seen.append(tcfg)
            super().__init__(tcfg, **kw)

    def stop(*a, **kw):
        raise Stop

    monkeypatch.setattr(neural, "_load_dataset", lambda *a: FakeDataset())
    monkeypatch.setattr(neural, "Trainer", FakeTrainer)
    monkeypatch.setattr(neural, "_run_mlm_steps", lambda tr, *a: [1.0])
    monkeypatch.setattr(neural, "_run_steps", lambda tr, *a, **kw: ([1.0], 0))
    monkeypatch.setattr(neural, "evaluate", stop)
    with pytest.raises(Stop):
        neural.train_classifier(
            "x.csv", model="mltc-tiny", device="cpu", seq=32, steps=10,
            mlm_path="m.csv", mlm_steps=10, pretrain_path="p.csv",
            pretrain_steps=10, weight_decay=0.1, no_decay_1d=True,
            layer_decay=0.75)
    fine, mlm, pre = seen
    assert [c.total_steps for c in seen] == [10, 10, 10]
    assert all(c.weight_decay == 0.1 and c.no_decay_1d for c in seen)
    assert fine.layer_decay == 0.75
    assert mlm.layer_decay == pre.layer_decay == 1.0
    seen.clear()
    with pytest.raises(Stop):
        neural.train_classifier("x.csv", model="mltc-tiny", device="cpu",
                                seq=32, steps=10)
    assert (seen[0].weight_decay, seen[0].no_decay_1d,
            seen[0].layer_decay) == (0.01, False, 1.0)


def test_yaml_keys_reach_train_config(tmp_path):
    from tosem2021_amd.utils.config import load_config
    p = tmp_path / "exp.yaml"
    p.write_text("train:\n  model: mltc-tiny\n  weight_decay: 0.1\n"
                 "  no_decay_1d: true\n  layer_decay: 0.9\n")
    tc = load_config(str(p)).train
    assert (tc.weight_decay, tc.no_decay_1d, tc.layer_decay) == (0.1, True,
                                                                 0.9)
    p.write_text("train:\n  layer_decay: 1.5\n")
    with pytest.raises(ValueError, match="layer_decay"):
        load_config(str(p))
