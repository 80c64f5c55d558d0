"""Per-tile side data of the flash kernels travels with its tile.

flash_fwd and flash_dq_recompute stage the 32 mask biases or kv segment ids
of a kv tile through a 128-byte LDS slot, flash_bwd_fused the lse, ddot and q
segment ids of a q tile: loaded with the tile's prefetch, stored at the loop
top, read by register row (docs/KERNELS.md, "Side data").  What can go wrong
is a value from the wrong key, the wrong register-row slot, the wrong tile or
the wrong batch row, a first tile that misses the prologue load, and a q
tile paired with its neighbour's lse / ddot when the live-tile scan jumps.

Everything is measured with the float64 reference and the budgets of
tests/test_flash_numerics.py; none of them involves a kernel's output.  The
CPU test at the top shows that the emulated reference itself passes every
case, so the budgets are not void at these inputs.  B = 2, H = 2 throughout.

L 32 is one tile, 96 fewer tiles than a workgroup's q rows, 288 one tile past
a 256-row workgroup, 544 one tile past two of them and long enough for a
steady state after the prologue's first tile.
"""
import functools

import pytest
import torch

from tosem2021_amd import ops
from tosem2021_amd.ops import reference
from test_flash_numerics import (BF16, DROPOUT, F64, OUTPUTS, SCALE,
                                 assert_flash_close, assert_lse_close,
                                 assert_packed_equal, both, check_outputs,
                                 cuda, inputs, key_bias, run_kernels,
                                 run_packed)

B, H = 2, 2
LENGTHS = (32, 96, 288, 544)


# ---- inputs -----------------------------------------------------------------

def distinct_bias(L):
    """[2, L] f32: every key a different finite bias, the two rows differ.
    A 0 / -1e9 mask would hide a value taken from the wrong key."""
    k = torch.arange(L, dtype=torch.float32)
    return torch.stack([-0.37 * (k % 7) - 0.01 * k,
                        -0.29 * (k % 5) - 0.013 * k]).contiguous()


def short_segments(L):
    """[2, L] int32: several short segments and a trailing pad segment, no
    boundary on a tile edge (where L allows one off it), the rows differ."""
    rows = []
    for lens, pad in (((13, 37, 50, 7, 22), 11), ((9, 45, 5, 61, 30), 3)):
        out, i = [], 0
        while len(out) < L - pad:
            out += [i] * lens[i % len(lens)]
            i += 1
        out = out[:L - pad]
        out += [out[-1] + 1] * pad
        rows.append(out)
    seg = torch.tensor(rows, dtype=torch.int32)
    ops.check_segments(seg)
    edges = (seg[:, 1:] != seg[:, :-1]).nonzero()[:, 1] + 1
    assert bool((edges % 32 != 0).all())
    return seg


def dropout_args(L):
    p, seed, call, layer = DROPOUT
    thr, dscale = reference.attn_dropout_threshold(p)
    drop = dict(drop_seed=seed, drop_call=call, drop_thr=thr,
                drop_site=reference.ATTN_DROPOUT_SITE0 + layer)
    keep = reference.attn_dropout_keep(B, H, L, *DROPOUT)
    return drop, keep.to(F64) * dscale


@functools.lru_cache(maxsize=None)
def side_case(kind, L, drop):
    """kind 'bias': distinct_bias as the key mask; 'seg': short_segments."""
    q, k, v, do = inputs(B, H, L, 9000 + L)
    mask = distinct_bias(L) if kind == "bias" else None
    seg = short_segments(L) if kind == "seg" else None
    bias = reference.segment_bias(seg) if seg is not None else key_bias(mask)
    hd, keep_scale = dropout_args(L) if drop else (None, None)
    exact, emul = both(q, k, v, do, bias, keep_scale)
    return dict(L=L, q=q, k=k, v=v, do=do, mask=mask, seg=seg, drop=hd,
                exact=exact, emul=emul)


# The live-scan cases move lse from q tile to q tile by a common component:
# column 0 of every key is K_COMMON + randn and column 0 of q tile t is
# Q_COMMON[t % 3], which adds scale * Q_COMMON * K_COMMON = 0, 8, 16 to every
# score of the tile's rows.  The softmax does not see a row-wise shift, so P
# stays as well conditioned as with plain randn, while lse moves by about 8
# between adjacent tiles and between tiles two apart (the neighbours in the
# alternating pattern).  A plain gain on q that moves lse as far (x 8) makes
# P one-hot, and the float64 reference rounded to bf16 then misses the older
# allclose tolerance on dK by itself.
K_COMMON = 8.0
Q_COMMON = (0.0, 8.0, 16.0)

# name -> live q tiles (the rest have dO zeroed), per L
LIVE = {
    288: {"first": [0], "last": [8], "alternating": [0, 2, 4, 6, 8],
          # tiles 2..7 dead up to row 256, the live tile lies across it
          "run-after-gap": [0, 1, 8]},
    544: {"first": [0], "last": [16], "alternating": list(range(0, 17, 2)),
          # tiles 6..9 dead: rows 192..319 cross row 256
          "run-after-gap": list(range(6)) + list(range(10, 17))},
}


@functools.lru_cache(maxsize=None)
def scan_case(L, pattern):
    q, k, v, do = inputs(B, H, L, 7000 + L)
    n_t = L // 32
    q, k = q.clone(), k.clone()
    q[..., 0] = torch.tensor([Q_COMMON[t % 3] for t in range(n_t)]) \
        .repeat_interleave(32).to(BF16)
    k[..., 0] = (k[..., 0].float() + K_COMMON).to(BF16)
    live = torch.zeros(n_t, dtype=torch.bool)
    live[LIVE[L][pattern]] = True
    do = (do.float() * live.repeat_interleave(32).view(1, 1, L, 1)).to(BF16)
    mask = distinct_bias(L)
    exact, emul = both(q, k, v, do, key_bias(mask))
    # the premise: a neighbour's lse is a different number altogether
    tile_lse = exact["lse"].view(B, H, n_t, 32).mean(-1)
    for d in (1, 2):
        gap = (tile_lse[..., d:] - tile_lse[..., :-d]).abs().min()
        assert float(gap) > 5, (L, d, float(gap))
    return dict(L=L, q=q, k=k, v=v, do=do, mask=mask, live=live,
                exact=exact, emul=emul)


# ---- CPU: the emulated reference passes the cases' own budgets --------------

def _accepts_emulated(c, what):
    for n in OUTPUTS:
        assert_flash_close(c["emul"][n].to(BF16), c["exact"][n], c["emul"][n],
                           f"{what} control {n}")
    assert_lse_close(c["exact"]["lse"].float(), c["exact"]["lse"],
                     f"{what} control lse")


def test_budgets_accept_emulated_reference():
    for L in LENGTHS:
        _accepts_emulated(side_case("bias", L, False), f"bias L{L}")
        _accepts_emulated(side_case("bias", L, True), f"bias drop L{L}")
        _accepts_emulated(side_case("seg", L, False), f"seg L{L}")
        _accepts_emulated(side_case("seg", L, True), f"seg drop L{L}")
    for L in LIVE:
        for pattern in LIVE[L]:
            _accepts_emulated(scan_case(L, pattern), f"scan L{L} {pattern}")


def test_budget_rejects_neighbour_bias():
    """The bias shifted by one key, and the other batch row's bias, are
    outside the budget: the distinct biases do what they are there for."""
    c = side_case("bias", 96, False)
    for wrong in (torch.roll(c["mask"], 1, dims=1), c["mask"].flip(0)):
        _, mut = both(c["q"], c["k"], c["v"], c["do"], key_bias(wrong))
        for n in OUTPUTS:
            with pytest.raises(AssertionError):
                assert_flash_close(mut[n].to(BF16), c["exact"][n],
                                   c["emul"][n], f"mutant {n}")


# ---- GPU --------------------------------------------------------------------

def _run_both_geometries(c, what, **kw):
    q, k, v, do, mask, seg = (cuda(c[n]) for n in
                              ("q", "k", "v", "do", "mask", "seg"))
    got = run_kernels(q, k, v, do, mask, seg, c["drop"], **kw)
    check_outputs(got, c["exact"], c["emul"], what)
    pk = run_packed(q, k, v, do, mask, seg, H, c["drop"])
    assert_packed_equal(pk, got, what)
    return got


@pytest.mark.gpu
@pytest.mark.parametrize("L", LENGTHS)
def test_distinct_biases(L):
    _run_both_geometries(side_case("bias", L, False), f"bias L{L}")


@pytest.mark.gpu
@pytest.mark.parametrize("L", LENGTHS)
@pytest.mark.parametrize("kind,drop", [("seg", False), ("seg", True),
                                       ("bias", True)])
def test_segments_and_dropout(kind, drop, L):
    _run_both_geometries(side_case(kind, L, drop),
                         f"{kind}{' drop' if drop else ''} L{L}")


@pytest.mark.gpu
@pytest.mark.parametrize("L", sorted(LIVE))
@pytest.mark.parametrize("pattern", ["first", "last", "alternating",
                                     "run-after-gap"])
def test_backward_side_data_follows_live_scan(pattern, L):
    c = scan_case(L, pattern)
    what = f"scan L{L} {pattern}"
    q, k, v, do, mask = (cuda(c[n]) for n in ("q", "k", "v", "do", "mask"))
    got = run_kernels(q, k, v, do, mask, None, dead_flags=True)
    assert torch.equal(got["dead"].view(B, H, -1).cpu() == 0,
                       c["live"].expand(B, H, -1))
    check_outputs(got, c["exact"], c["emul"], what)
    plain = run_kernels(q, k, v, do, mask, None)
    for n in ("dq", "dk", "dv"):
        assert torch.equal(got[n], plain[n]), f"{what}: {n} with the flags"
    pk = run_packed(q, k, v, do, mask, None, H)
    assert_packed_equal(pk, got, what)
    off = run_packed(q, k, v, do, mask, None, H, skip_zero_do=False)
    assert torch.equal(off["dqkv"], pk["dqkv"]), f"{what}: skip_zero_do=False"


def _zero_extend(t, L):
    out = torch.zeros(*t.shape[:2], L, t.shape[3], dtype=t.dtype)
    out[:, :, :t.shape[2]] = t
    return out


@pytest.mark.gpu
def test_tail_invariance_bitwise():
    """L 256 without padding against the same tensors zero-extended to 512
    with keys >= 256 at -1e9 and dO rows >= 256 zero: the rows below 256 are
    the same bits (docs/KERNELS.md on the tile skips; the last prefetch's
    guards).  With and without the dead-tile flags."""
    Ls, Ll = 256, 512
    small = inputs(B, H, Ls, 256512)
    mask = torch.zeros(B, Ll)
    mask[:, Ls:] = -1e9
    a_in = [cuda(t) for t in small]
    b_in = [cuda(_zero_extend(t, Ll)) for t in small]
    for flags in (False, True):
        a = run_kernels(*a_in, None, None, dead_flags=flags)
        b = run_kernels(*b_in, cuda(mask), None, dead_flags=flags)
        for n in ("o", "dq", "dk", "dv"):
            assert torch.equal(a[n], b[n][:, :, :Ls]), (n, flags)
        assert torch.equal(a["lse"].view(B, H, Ls),
                           b["lse"].view(B, H, Ll)[:, :, :Ls]), flags
    pa = run_packed(*a_in, None, None, H)
    pb = run_packed(*b_in, cuda(mask), None, H)
    assert torch.equal(pa["dqkv"], pb["dqkv"][:, :Ls])
    assert torch.equal(pa["o_p"], pb["o_p"][:, :Ls])


@pytest.mark.gpu
@pytest.mark.parametrize("kind", ["bias", "seg"])
def test_two_launches_are_bitwise_equal(kind):
    c = side_case(kind, 288, False)
    q, k, v, do, mask, seg = (cuda(c[n]) for n in
                              ("q", "k", "v", "do", "mask", "seg"))
    one = run_kernels(q, k, v, do, mask, seg)
    two = run_kernels(q, k, v, do, mask, seg)
    for n in ("o", "lse", "ddot", "dq", "dk", "dv"):
        assert torch.equal(one[n], two[n]), n
