"""Gradient-norm clipping and non-finite step skipping on the CPU: the
reference ops against PyTorch, the trainer against a hand-driven loop, the
skip/checkpoint bookkeeping, the gloo DP path and the plumbing."""
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

PORT = 29931          # tests/test_ddp_cpu.py owns 29871..29879
F32_REORDER = 5e-5    # tests/test_ddp_cpu.py's bound for f32 reordering


def _trainer(**kw):
    return Trainer(TrainConfig(model="mltc-tiny", lr=1e-3, warmup_steps=0,
                               dtype="f32", **kw), device=torch.device("cpu"))


def _batch():
    return synthetic_batch(CONFIGS["mltc-tiny"], 8, 32, seed=42)


def _state(t):
    f = t.flat
    return [x.clone() for x in (f.flat, f.master, f.m, f.v)]


def _same(a, b):
    # bitwise: NaN-safe and sign-of-zero-safe, unlike torch.equal
    return all(torch.equal(x.view(torch.int32), y.view(torch.int32))
               for x, y in zip(a, b))


# ---- reference ops ----------------------------------------------------------

def test_reference_state_formulas():
    g = torch.tensor([3.0, 4.0] + [0.0] * 6)
    norm, scale, finite, sumsq = ref.grad_clip_state(g, 0.5, 1.0).tolist()
    assert (norm, finite, sumsq) == (2.5, 1.0, 25.0)
    assert scale == pytest.approx(0.5 / (2.5 + 1e-6), rel=1e-6)
    # no clip: scale is bitwise grad_scale, for a finite and an infinite bound
    gs = 1.0 / 6
    for max_norm in (1e9, math.inf):
        st = ref.grad_clip_state(g, gs, max_norm)
        assert st.dtype == torch.float32
        assert float(st[1]) == float(torch.tensor(gs, dtype=torch.float32))
    for bad in (math.inf, -math.inf, math.nan):
        h = g.clone()
        h[-1] = bad
        assert float(ref.grad_clip_state(h, 1.0, 1.0)[2]) == 0.0
    # an f32 overflow of the sum counts as non-finite too
    big = torch.full((8,), 3e19)
    assert float(ref.grad_clip_state(big, 1.0, 1.0)[2]) == 0.0
    for bad in (0.0, -1.0, math.nan):
        with pytest.raises(ValueError):
            ops.grad_clip_state(g, max_norm=bad)


def test_reference_matches_torch_clip_and_adamw():
    torch.manual_seed(4)
    n, max_norm = 1024, 32.0
    hp = dict(lr=1e-2, beta1=0.9, beta2=0.999, eps=1e-8, wd=0.05)
    master = torch.randn(n)
    p, m, v = master.clone(), torch.zeros(n), torch.zeros(n)
    tp = master.clone().requires_grad_(True)
    opt = torch.optim.AdamW([tp], lr=hp["lr"], betas=(0.9, 0.999), eps=1e-8,
                            weight_decay=hp["wd"])
    clipped = []
    # |g| is about 32 * magnitude
    for step, mag in enumerate((3.0, 0.2, 2.0, 0.1, 0.5), start=1):
        g = torch.randn(n) * mag
        tp.grad = g.clone()
        want_norm = torch.nn.utils.clip_grad_norm_([tp], max_norm)
        opt.step()
        st = ops.grad_clip_state(g, max_norm=max_norm)
        ops.adamw_step_clipped(p, g, m, v, master, step=step, clip_state=st,
                               **hp)
        assert float(st[0]) == pytest.approx(float(want_norm), rel=1e-6)
        assert float(st[2]) == 1.0
        clipped.append(float(st[1]) < 1.0)
        assert clipped[-1] == (float(want_norm) > max_norm)
    assert any(clipped) and not all(clipped), clipped
    assert torch.allclose(master, tp.detach(), atol=1e-5)
    assert torch.equal(p, master)


def test_reference_skip_leaves_buffers():
    torch.manual_seed(5)
    n = 64
    bufs = [torch.randn(n), torch.rand(n), torch.rand(n), torch.randn(n)]
    p, m, v, master = (b.clone() for b in bufs)
    g = torch.randn(n)
    g[-1] = math.nan
    st = ops.grad_clip_state(g, max_norm=1.0)
    ops.adamw_step_clipped(p, g, m, v, master, lr=1e-2, step=1, clip_state=st)
    assert _same([p, m, v, master], bufs)


# ---- trainer ----------------------------------------------------------------

def test_trainer_matches_hand_loop():
    """clip_grad_norm_ on flat.params + the existing ops.adamw_step.  The
    unclipped step norms of this run are 11.10, 6.65, 6.15, 5.32, ...: 6.0
    clips the early steps and not the late ones."""
    max_norm = 6.0
    tokens, mask, labels = _batch()
    torch.manual_seed(100)
    a = _trainer(max_grad_norm=max_norm)
    torch.manual_seed(100)
    b = _trainer()
    norms = []
    for _ in range(4):
        a.step(tokens, mask, labels)
        b.flat.zero_grad()
        b.model.loss(b._forward(tokens, mask), labels).backward()
        norm = float(torch.nn.utils.clip_grad_norm_(b.flat.params, max_norm))
        b.step_num += 1
        ops.adamw_step(b.flat.flat, b.flat.grad_flat, b.flat.m, b.flat.v,
                       b.flat.master, lr=b._lr(), beta1=b.cfg.beta1,
                       beta2=b.cfg.beta2, eps=b.cfg.eps,
                       wd=b.cfg.weight_decay, step=b.step_num)
        print(f"step {b.step_num}: norm {norm:.4f} "
              f"trainer {a.metrics['grad_norm']:.4f}")
        assert a.metrics["grad_norm"] == pytest.approx(norm, rel=1e-5)
        norms.append(norm)
    assert any(x > max_norm for x in norms), norms
    assert any(x <= max_norm for x in norms), norms
    diff = float((a.flat.flat - b.flat.flat).abs().max())
    assert diff < F32_REORDER, diff
    assert a.opt_step == a.step_num == 4 and a.skipped_steps == 0


def test_huge_max_norm_is_bitwise_off():
    tokens, mask, labels = _batch()
    torch.manual_seed(100)
    off = _trainer()
    torch.manual_seed(100)
    on = _trainer(max_grad_norm=1e9)
    for _ in range(3):
        off.step(tokens, mask, labels)
        on.step(tokens, mask, labels)
    assert _same(_state(on), _state(off))
    assert "grad_norm" in on.metrics and "grad_norm" not in off.metrics
    assert off.opt_step == on.opt_step == 3


def test_step_accum_matches_step():
    tokens, mask, labels = _batch()
    torch.manual_seed(100)
    big = _trainer(max_grad_norm=6.0)
    big.step(tokens, mask, labels)
    torch.manual_seed(100)
    acc = _trainer(max_grad_norm=6.0)
    acc.step_accum(
        [(tokens[s], mask[s], {k: v[s] for k, v in labels.items()})
         for s in (slice(0, 4), slice(4, 8))])
    assert big.metrics["grad_norm"] > 6.0      # the clip is active
    assert acc.metrics["grad_norm"] == pytest.approx(
        big.metrics["grad_norm"], rel=1e-5)
    diff = float((big.flat.flat - acc.flat.flat).abs().max())
    assert diff < F32_REORDER, diff
    assert acc.opt_step == 1


def test_non_finite_step_is_skipped(monkeypatch):
    from tosem2021_amd.utils.metrics import get_metrics
    tokens, mask, labels = _batch()
    torch.manual_seed(100)
    t = _trainer(max_grad_norm=6.0)
    t.step(tokens, mask, labels)
    before = _state(t)
    loss_fn = t.model.loss
    with monkeypatch.context() as mp_:
        mp_.setattr(t.model, "loss",
                    lambda lg, lb: loss_fn(lg, lb) * float("nan"))
        t.step(tokens, mask, labels)
    assert _same(_state(t), before)
    assert (t.step_num, t.opt_step, t.skipped_steps) == (2, 1, 1)
    assert math.isnan(t.metrics["grad_norm"])
    rec = get_metrics()._history[-1]
    assert rec["step"] == 2 and rec["skipped"] is True
    # the next step runs, with the bias correction of the SECOND update
    torch.manual_seed(100)
    clean = _trainer(max_grad_norm=6.0)
    clean.step(tokens, mask, labels)
    clean.step_num += 1            # same LR schedule position as t
    loss = t.step(tokens, mask, labels)
    clean.step(tokens, mask, labels)
    assert math.isfinite(loss) and bool(torch.isfinite(t.flat.flat).all())
    assert (t.step_num, t.opt_step, t.skipped_steps) == (3, 2, 1)
    assert _same(_state(t), _state(clean))


def test_checkpoint_round_trips_counters(tmp_path):
    tokens, mask, labels = _batch()
    t = _trainer(max_grad_norm=6.0)
    t.step(tokens, mask, labels)
    t.skipped_steps, t.step_num = 2, 3          # as after two skipped steps
    path = t.save(str(tmp_path / "a.pt"))
    u = _trainer(max_grad_norm=6.0)
    u.load(path)
    assert (u.step_num, u.opt_step, u.skipped_steps) == (3, 1, 2)
    # a checkpoint from before the counters existed
    sd = t.state_dict()
    del sd["opt_step"], sd["skipped_steps"]
    old = str(tmp_path / "old.pt")
    torch.save(sd, old)
    u.load(old)
    assert (u.step_num, u.opt_step, u.skipped_steps) == (3, 3, 0)


# ---- DP (gloo, world 2) -----------------------------------------------------

def _worker(rank, world, port, out):
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        torch.manual_seed(100 + rank)   # rank-0 init is broadcast
        t = Trainer(TrainConfig(model="mltc-tiny", lr=1e-3, warmup_steps=0,
                                dtype="f32", bucket_mb=1, max_grad_norm=6.0),
                    device=torch.device("cpu"))
        tokens, mask, labels = _batch()
        per = 8 // world
        sl = slice(rank * per, rank * per + per)
        norms = []
        for _ in range(2):
            t.step(tokens[sl], mask[sl], {k: v[sl] for k, v in labels.items()})
            norms.append(t.metrics["grad_norm"])
        out[rank] = (t.flat.flat.clone(), norms, t.opt_step)
    finally:
        dist.destroy_process_group()


@pytest.mark.timeout(300)
def test_ddp_clipping_matches_single_process():
    world = 2
    ctx = mp.get_context("spawn")
    with ctx.Manager() as mgr:
        out = mgr.dict()
        mp.start_processes(_worker, args=(world, PORT, out), nprocs=world,
                           join=True, start_method="spawn")
        res = {r: out[r] for r in range(world)}
    assert torch.equal(res[0][0], res[1][0])
    assert res[0][1] == res[1][1]           # grad_norm, bitwise
    assert res[0][2] == res[1][2] == 2
    torch.manual_seed(100)
    solo = _trainer(max_grad_norm=6.0)
    tokens, mask, labels = _batch()
    for want in res[0][1]:
        solo.step(tokens, mask, labels)
        assert solo.metrics["grad_norm"] == pytest.approx(want, rel=1e-5)
    assert max(res[0][1]) > 6.0             # clipping was active
    diff = float((solo.flat.flat - res[0][0]).abs().max())
    assert diff < F32_REORDER, diff


# ---- plumbing ---------------------------------------------------------------

def test_cli_flag_reaches_train_classifier(monkeypatch):
    from tosem2021_amd import cli
    from tosem2021_amd.classify import neural
    seen = {}
    monkeypatch.setattr(neural, "train_classifier",
                        lambda **kw: seen.update(kw) or {})
    cli.main(["train", "--taxonomy", "x.csv", "--clip-grad-norm", "0.5"])
    assert seen["max_grad_norm"] == 0.5
    cli.main(["train", "--taxonomy", "x.csv"])
    assert seen["max_grad_norm"] == 0.0


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
                                max_grad_norm=2.5)
    assert seen[0].max_grad_norm == 2.5
    with pytest.raises(Stop):
        neural.train_classifier("x.csv", model="mltc-tiny", device="cpu")
    assert seen[1].max_grad_norm == 0.0


def test_yaml_key_reaches_train_config(tmp_path):
    from tosem2021_amd.utils.config import load_config
    p = tmp_path / "exp.yaml"
    p.write_text("train:\n  model: mltc-tiny\n  max_grad_norm: 1.5\n")
    assert load_config(str(p)).train.max_grad_norm == 1.5
    assert TrainConfig().max_grad_norm == 0.0
