"""Flash kernels against an independent float64 reference.

`flash_reference` computes o, lse, ds, dq, dk and dv of one attention call in
float64 from the bf16 inputs alone: nothing a kernel produced enters it.  With
`emulate=True` it rounds where the kernels round (docs/KERNELS.md,
"Validation") and nowhere else:

  * exp(s - rowmax) goes to bf16 before the P V product; the row sum is taken
    from the unrounded values,
  * D = rowsum(dO * O) is taken from the bf16 o,
  * P and dS go to bf16 before P^T dO, dS^T Q and dS K.

Every bf16 output goes through `assert_flash_close(got, exact, emul, name)`:

    floor  = |bf16(exact) - exact|_F / |exact|_F
    E_emul = |bf16(emul)  - exact|_F / |exact|_F
    rel    = |got         - exact|_F / |exact|_F
    assert rel <= max(4 floor, 2 E_emul)

Four floors is the factor tests/test_ops_gpu_scale.py uses.  The factor two
over the emulation is room for what the emulation does not model: __expf and
__logf, P rounded against the running instead of the final row max, and the
f32 accumulation order, all of them f32-sized.  Neither side of the inequality
involves the code under test.  The allclose tolerances the older flash tests
use stay as a second assertion.  lse is f32 with no bf16 rounding on its way:
|lse - exact| <= 1e-4 + 1e-6 |exact| (the __expf argument error at |s| < 30
and one __logf are a few 1e-6; measured on an MI355X: 4.6e-6 with q, k x 3,
at most 1.2e-6 in every other case, table in docs/KERNELS.md).

fa_dot is checked on the reference's own bf16 o, so that its expected value
needs no kernel output: the 64 products of a row are exact in f32 and every
one of them passes through at most seven f32 additions (three in the lane,
four butterfly steps): (1 + 2^-24)^7 - 1 < 8 * 2^-24, so

    |ddot - sum64(dO * o)| <= 8 * 2^-24 * sum|dO * o|        per row.

The CPU tests at the top prove that the helper bites: bf16(emul) must be
accepted, reference mutants (softmax scale off by 2 %, a mask off by one key,
the D term dropped, the wrong batch row's mask, one query tile of 65 left out
of dK and dV) must be rejected, and the old allclose must be shown to accept
the scale mutant, which is the gap this file closes.

The GPU cases are listed at CASES.  All rows are compared, padded query rows
included: they are defined.  The packed kernels run on the same data and must
equal the [B, H, L, 64] results bitwise, which carries the bound over to the
packed geometry.  The legacy dS path (emit_ds, flash_dq) and p_from_lse get
the bf16 bound at the two smallest cases that go through the general
reference, one without a mask (one-tile) and one with (ragged-96).
"""
import functools
import math
import zlib

import pytest
import torch

from tosem2021_amd import ops
from tosem2021_amd.ops import reference
from test_ops_gpu_scale import assert_close, tol_dparam

BF16 = torch.bfloat16
F64 = torch.float64
SCALE = 0.125

# the allclose tolerances of tests/test_ops_gpu.py and
# tests/test_flash_qskip_gpu.py, unchanged
TOL_O = dict(atol=3e-2, rtol=3e-2)
TOL_GRAD = dict(atol=5e-2, rtol=3e-2)
TOL_DS = dict(atol=2e-2, rtol=3e-2)
TOL_P = dict(atol=8e-3, rtol=2e-2)
OLD_TOL = {"o": TOL_O, "dq": TOL_GRAD, "dk": TOL_GRAD, "dv": TOL_GRAD,
           "ds": TOL_DS, "p": TOL_P}
OUTPUTS = ("o", "dq", "dk", "dv")


def rb(t):
    """Round to bf16, back in float64."""
    return t.to(BF16).to(F64)


# ---- the reference ----------------------------------------------------------

def _flash_math(q, k, v, do, bias, scale, keep_scale, emulate,
                softmax_scale=None, drop_d=False):
    """flash_reference plus the two knobs the mutant tests turn:
    softmax_scale replaces scale inside the softmax only, drop_d leaves the
    D term out of dS."""
    q, k, v, do = (t.to(F64) for t in (q, k, v, do))
    ss = scale if softmax_scale is None else softmax_scale
    s = ss * torch.matmul(q, k.transpose(-1, -2))
    if bias is not None:
        s = s + bias.to(F64)
    m = s.max(dim=-1, keepdim=True).values
    e = torch.exp(s - m)
    l = e.sum(dim=-1, keepdim=True)
    lse = (m + torch.log(l)).squeeze(-1)
    p = e / l
    ks = 1.0 if keep_scale is None else keep_scale.to(F64)
    if emulate:
        o = torch.matmul(rb(e) * ks, v) / l
        o_d = rb(o)
    else:
        o = torch.matmul(p * ks, v)
        o_d = o
    d = (do * o_d).sum(dim=-1, keepdim=True)
    if drop_d:
        d = torch.zeros_like(d)
    dp = torch.matmul(do, v.transpose(-1, -2)) * ks
    ds = scale * p * (dp - d)
    p_mm, ds_mm = (rb(p), rb(ds)) if emulate else (p, ds)
    dq = torch.matmul(ds_mm, k)
    dk = torch.matmul(ds_mm.transpose(-1, -2), q)
    dv = torch.matmul((p_mm * ks).transpose(-1, -2), do)
    return o, lse, ds, dq, dk, dv


def flash_reference(q, k, v, do, bias, scale, keep_scale=None, emulate=False):
    """float64 attention forward and backward of the bf16 inputs q, k, v, do
    [B, H, L, 64].  bias: additive, broadcastable to [B, H, L, L] (a key mask
    viewed [B, 1, 1, L], reference.segment_bias(seg)) or None.  keep_scale:
    optional [B, H, L, L], reference.attn_dropout_keep times the dropout
    scale; as in reference.flash_attention_fwd and docs/KERNELS.md it
    multiplies the probabilities after the softmax, and lse stays the
    undropped softmax's.  Returns o, lse, ds, dq, dk, dv in float64;
    emulate=True rounds at the kernels' rounding points (module docstring)."""
    return _flash_math(q, k, v, do, bias, scale, keep_scale, emulate)


# ---- the budget -------------------------------------------------------------

def flash_budget(got, exact, emul):
    """(rel, floor, E_emul) of the module docstring."""
    exact = exact.to(F64)
    norm = float(exact.norm())
    assert norm > 0, "reference is all zeros"
    floor = float((rb(exact) - exact).norm()) / norm
    e_emul = float((rb(emul.to(F64)) - exact).norm()) / norm
    rel = float((got.detach().cpu().to(F64) - exact).norm()) / norm
    return rel, floor, e_emul


def old_allclose(got, exact, kind):
    return torch.allclose(got.detach().cpu().float(), exact.float(),
                          **OLD_TOL[kind])


def assert_flash_close(got, exact, emul, name):
    """got: a bf16 kernel output; exact, emul: flash_reference's float64
    value of it without and with emulate.  name's last word picks the old
    allclose tolerance (o, dq, dk, dv, ds, p)."""
    assert got.dtype == BF16, name
    assert got.shape == exact.shape == emul.shape, (name, got.shape,
                                                    exact.shape)
    rel, floor, e_emul = flash_budget(got, exact, emul)
    worst = float((got.detach().cpu().to(F64) - exact).abs().max())
    print(f"{name}: rel {rel:.3e} floor {floor:.3e} E_emul {e_emul:.3e} "
          f"rel/floor {rel / floor:.2f} rel/E_emul {rel / e_emul:.2f} "
          f"max|err| {worst:.3e}")
    assert rel <= max(4 * floor, 2 * e_emul), \
        (f"{name}: rel {rel:.3e} > max(4 x floor {floor:.3e}, "
         f"2 x E_emul {e_emul:.3e})")
    assert old_allclose(got, exact, name.split()[-1]), \
        f"{name}: allclose failed, max|err| {worst:.3e}"


def assert_lse_close(got, exact, name):
    assert got.dtype == torch.float32, name
    err = (got.detach().cpu().to(F64).reshape(exact.shape) - exact).abs()
    print(f"{name}: max|err| {float(err.max()):.3e}")
    assert bool((err <= 1e-4 + 1e-6 * exact.abs()).all()), \
        f"{name}: max|err| {float(err.max()):.3e}"


# ---- inputs -----------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def inputs(B, H, L, seed, qk_gain=1.0):
    """randn q, k, v, dO in bf16 from a seeded CPU generator.  v and dO are
    zero-mean on purpose: with a common offset in v, o is dominated by that
    offset and a wrong softmax hides in the relative norm."""
    g = torch.Generator().manual_seed(seed)
    q, k, v, do = (torch.randn(B, H, L, 64, generator=g) for _ in range(4))
    return ((q * qk_gain).to(BF16), (k * qk_gain).to(BF16), v.to(BF16),
            do.to(BF16))


def suffix_mask(L, pads):
    """Additive [B, L] key mask, pads[b] trailing keys of row b at -1e9."""
    m = torch.zeros(len(pads), L)
    for b, p in enumerate(pads):
        if p:
            m[b, L - p:] = -1e9
    return m


def key_bias(mask):
    return None if mask is None else mask.view(mask.shape[0], 1, 1, -1)


def both(q, k, v, do, bias, keep_scale=None, big=False):
    """(exact, emul) as dicts; ds is left out where it is [*, 2080, 2080]."""
    out = []
    for emulate in (False, True):
        o, lse, ds, dq, dk, dv = flash_reference(q, k, v, do, bias, SCALE,
                                                 keep_scale, emulate)
        out.append(dict(o=o, lse=lse, ds=None if big else ds, dq=dq, dk=dk,
                        dv=dv))
    return out


# ---- CPU: the helper rejects mutants and accepts the emulated reference -----

CPU_PADS = (28, 0)


@functools.lru_cache(maxsize=None)
def cpu_case():
    q, k, v, do = inputs(2, 2, 128, 101)
    bias = key_bias(suffix_mask(128, CPU_PADS))
    exact, emul = both(q, k, v, do, bias)
    return (q, k, v, do), bias, exact, emul


def mutant(softmax_scale=None, drop_d=False, pads=CPU_PADS):
    """bf16 outputs of the EMULATED reference with one thing wrong; with no
    argument it is the emulated reference itself."""
    (q, k, v, do), _, _, _ = cpu_case()
    bias = key_bias(suffix_mask(128, pads))
    o, _, _, dq, dk, dv = _flash_math(q, k, v, do, bias, SCALE, None, True,
                                      softmax_scale, drop_d)
    return dict(o=o.to(BF16), dq=dq.to(BF16), dk=dk.to(BF16),
                dv=dv.to(BF16))


def rejects(got, exact, emul, name):
    with pytest.raises(AssertionError):
        assert_flash_close(got, exact, emul, name)


def check_mutant(mut, names, what):
    _, _, exact, emul = cpu_case()
    for n in names:
        rejects(mut[n], exact[n], emul[n], f"{what} {n}")


def test_helper_accepts_emulated_reference():
    _, _, exact, emul = cpu_case()
    ctrl = mutant()
    for n in OUTPUTS:
        assert torch.equal(ctrl[n], emul[n].to(BF16))
        assert_flash_close(ctrl[n], exact[n], emul[n], f"control {n}")
        rel, floor, e_emul = flash_budget(ctrl[n], exact[n], emul[n])
        # each rounding point adds an error no larger than the output's own
        # rounding and independent of it, so at this well-conditioned input
        # the emulation stays below two floors and the bound in force is
        # the four floors; an emulation above that would be what loosens it
        assert rel == e_emul and floor <= e_emul < 2 * floor, n
    assert_flash_close(emul["ds"].to(BF16), exact["ds"], emul["ds"],
                       "control ds")
    assert_lse_close(exact["lse"].float(), exact["lse"], "control lse")


def test_helper_rejects_softmax_scale_mutant():
    check_mutant(mutant(softmax_scale=1.02 * SCALE), OUTPUTS, "scale x 1.02")


def test_old_allclose_accepts_softmax_scale_mutant():
    """The gap: a softmax scale wrong by 2 % is within atol 3e-2 .. 5e-2 of
    every output the older tests compare, and ten floors outside the new
    bound."""
    _, _, exact, emul = cpu_case()
    mut = mutant(softmax_scale=1.02 * SCALE)
    for n in OUTPUTS:
        assert old_allclose(mut[n], exact[n], n), n
        rel, floor, e_emul = flash_budget(mut[n], exact[n], emul[n])
        print(f"{n}: scale mutant at {rel / floor:.1f} floors")
        assert rel > 8 * floor and rel > 4 * e_emul, n


def test_helper_rejects_mask_off_by_one():
    """One more live key in the padded row."""
    check_mutant(mutant(pads=(27, 0)), OUTPUTS, "mask off by one")


def test_helper_rejects_dropped_d_term():
    check_mutant(mutant(drop_d=True), ("dq", "dk"), "no D")


def test_helper_rejects_batch_0_mask_everywhere():
    check_mutant(mutant(pads=(28, 28)), OUTPUTS, "row 0's mask on row 1")


def test_helper_rejects_lse_error():
    _, _, exact, _ = cpu_case()
    with pytest.raises(AssertionError):
        assert_lse_close((exact["lse"] + 3e-4).float(), exact["lse"], "lse")


def do_pattern(do, name):
    """dO of the window case with whole 32-row query tiles zeroed."""
    do = do.clone()
    if name == "cross":            # tiles 60..63 dead, tile 64 live
        do[:, :, 60 * 32:64 * 32] = 0
    elif name == "jump":           # tiles 0..63 dead, tile 64 live
        do[:, :, :64 * 32] = 0
    elif name == "last":           # tile 64 dead, the rest live
        do[:, :, 64 * 32:] = 0
    else:
        assert name == "random"
    return do


@functools.lru_cache(maxsize=None)
def window_case(pattern):
    q, k, v, do = inputs(1, 1, 2080, 2080)
    do = do_pattern(do, pattern)
    exact, emul = both(q, k, v, do, None, big=True)
    return (q, k, v, do), exact, emul


def test_helper_rejects_missing_query_tile_64():
    """L 2080 is 65 query tiles.  dK and dV without the last one: a query row
    enters them through its own row of dO alone, so the emulated reference
    of the dO with that tile zeroed is exactly that mutant."""
    _, exact, emul = window_case("random")
    _, _, mut = window_case("last")
    for n in ("dk", "dv"):
        assert_flash_close(emul[n].to(BF16), exact[n], emul[n],
                           f"L2080 control {n}")
        rejects(mut[n].to(BF16), exact[n], emul[n], f"L2080 no tile 64 {n}")


# ---- GPU: the cases ---------------------------------------------------------

def _bias_left_pad(B, L, n):
    m = torch.zeros(B, L)
    m[0, :n] = -1e9
    return m


def _bias_holes(L):
    m = torch.zeros(2, L)
    m[0, 5:9] = -1e9
    m[0, 40:140] = -1e9
    m[1, L - 1] = -1e9
    return m


def _bias_finite(L):
    g = torch.Generator().manual_seed(77)
    return torch.randn(2, L, generator=g) * 2


def _seg_long(L):
    seg = torch.cat([torch.full((n,), i, dtype=torch.int32)
                     for i, n in enumerate((300, 7, 513, 200, 36))])
    assert seg.numel() == L
    seg = seg.view(1, L).contiguous()
    ops.check_segments(seg)
    return seg


DROPOUT = (0.1, 0x1234567, 5, 1)        # (p, seed, call, layer)

# name -> (B, H, L, what beyond randn q, k, v, dO at scale 0.125)
#   one-tile    smallest launch; every wave's second q-block absent
#   ragged-*    pads (1, L - 1): L - 1 and 1 live keys; partial last workgroup
#               of all three kernels; packed stride 192; skip boundaries
#   tile-edge   31 and 33 live keys: one key either side of the first tile
#               boundary, where the tail skip and the wave skip switch
#   left-pad    keys 0..36 of row 0 masked: mrow[0] switches the backward
#               skips off; the forward's first tile is all-masked and
#               alpha = 0 must wipe it
#   holes       interior holes, a whole masked wave inside a live block, the
#               last live key is not the live count
#   finite      the bias as a number: 2 randn per key, no -1e9
#   hot         q, k x 3: the running max moves in most tiles, P concentrates
#   long        33 kv tiles, 5 / 9 workgroups per head, left pad 37
#   long-seg    segments [300, 7, 513, 200] + 36 pad across workgroups
#   dropout     pad 40 and attention dropout through the same helper
CASES = {
    "one-tile": (2, 2, 32),
    "ragged-96": (2, 3, 96),
    "ragged-160": (2, 3, 160),
    "ragged-288": (2, 3, 288),
    "tile-edge": (2, 2, 96),
    "left-pad": (2, 2, 288),
    "holes": (2, 3, 160),
    "finite": (2, 2, 96),
    "hot": (2, 2, 96),
    "long": (1, 2, 1056),
    "long-seg": (1, 2, 1056),
    "dropout": (1, 2, 288),
}


@functools.lru_cache(maxsize=None)
def case(name):
    """Inputs (CPU), mask / seg / dropout and both references of one case."""
    B, H, L = CASES[name]
    seed = zlib.crc32(name.encode())          # stable when cases are added
    q, k, v, do = inputs(B, H, L, seed, 3.0 if name == "hot" else 1.0)
    mask = seg = drop = keep_scale = None
    if name.startswith("ragged"):
        mask = suffix_mask(L, (1, L - 1))
    elif name == "tile-edge":
        mask = suffix_mask(L, (L - 31, L - 33))
    elif name == "left-pad":
        mask = _bias_left_pad(B, L, 37)
    elif name == "holes":
        mask = _bias_holes(L)
    elif name == "finite":
        mask = _bias_finite(L)
    elif name == "long":
        mask = _bias_left_pad(B, L, 37)
    elif name == "long-seg":
        seg = _seg_long(L)
    elif name == "dropout":
        mask = suffix_mask(L, (40,))
        p, seed, call, layer = DROPOUT
        thr, dscale = reference.attn_dropout_threshold(p)
        drop = dict(drop_seed=seed, drop_call=call, drop_thr=thr,
                    drop_site=reference.ATTN_DROPOUT_SITE0 + layer)
        keep = reference.attn_dropout_keep(B, H, L, *DROPOUT)
        keep_scale = keep.to(F64) * dscale
        assert 0.85 < float(keep.float().mean()) < 0.95
    bias = reference.segment_bias(seg) if seg is not None else key_bias(mask)
    exact, emul = both(q, k, v, do, bias, keep_scale)
    return dict(B=B, H=H, L=L, q=q, k=k, v=v, do=do, mask=mask, seg=seg,
                drop=drop, exact=exact, emul=emul)


def packed(t):
    """[B, H, L, 64] -> [B, L, H * 64]"""
    return t.transpose(1, 2).reshape(t.shape[0], t.shape[2], -1).contiguous()


def unpacked(t, H):
    """[B, L, H * 64] -> [B, H, L, 64]"""
    return t.view(t.shape[0], t.shape[1], H, 64).transpose(1, 2).contiguous()


def cuda(t):
    return None if t is None else t.cuda().contiguous()


def run_kernels(q, k, v, do, mask, seg, drop=None, dead_flags=False):
    """The default pipeline on GPU tensors in the [B, H, L, 64] geometry:
    flash_fwd, fa_dot, flash_bwd_fused, flash_dq_recompute.  With dead_flags
    the backward kernels get fa_dot's flags.  drop: the bindings' drop_*
    keywords."""
    ext = ops.hip_ops()
    hd = drop or {}
    o, lse = ext.flash_fwd(q, k, v, mask, SCALE, seg, **hd)
    ddot, dead = ext.fa_dot_flags(do, o)
    assert torch.equal(ext.fa_dot(do, o), ddot)
    assert torch.equal(dead, reference.dead_q_tiles(do))
    flags = dead if dead_flags else None
    dk, dv = ext.flash_bwd_fused(q, k, v, do, mask, lse, ddot, SCALE, False,
                                 seg, flags, **hd)
    dq = ext.flash_dq_recompute(q, k, v, do, mask, lse, ddot, SCALE, seg,
                                flags, **hd)
    return dict(o=o, lse=lse, ddot=ddot, dead=dead, dq=dq, dk=dk, dv=dv)


def run_packed(q, k, v, do, mask, seg, H, drop=None, skip_zero_do=True):
    ext = ops.hip_ops()
    hd = drop or {}
    qkv = torch.cat([packed(t) for t in (q, k, v)], dim=-1).contiguous()
    do_p = packed(do)
    o_p, lse_p = ext.flash_fwd_packed(qkv, H, mask, SCALE, seg, **hd)
    ddot_p, dead_p = ext.fa_dot_packed_flags(do_p, o_p, H)
    dqkv = ext.flash_bwd_packed(qkv, o_p, do_p, mask, lse_p, H, SCALE, seg,
                                skip_zero_do, **hd)
    dq, dk, dv = (unpacked(t, H) for t in dqkv.split(H * 64, dim=-1))
    return dict(o=unpacked(o_p, H), lse=lse_p, ddot=ddot_p, dead=dead_p,
                dq=dq, dk=dk, dv=dv, qkv=qkv, o_p=o_p, do_p=do_p, dqkv=dqkv)


def assert_packed_equal(pk, got, what):
    for n in ("o", "dq", "dk", "dv", "dead"):
        assert torch.equal(pk[n], got[n]), f"{what}: packed {n} differs"
    for n in ("lse", "ddot"):
        assert torch.equal(pk[n], got[n].view(pk[n].shape)), \
            f"{what}: packed {n} differs"


def check_fa_dot(do, o_ref, what):
    """fa_dot on the reference's bf16 o (module docstring)."""
    o16 = o_ref.to(BF16)
    got = ops.hip_ops().fa_dot(do, o16.cuda()).cpu().to(F64)
    terms = do.cpu().to(F64) * o16.to(F64)
    err = (got.reshape(terms.shape[:-1]) - terms.sum(-1)).abs()
    bound = 8 * 2.0 ** -24 * terms.abs().sum(-1)
    print(f"{what} ddot: max|err| {float(err.max()):.3e}, "
          f"min slack {float((bound - err).min()):.3e}")
    assert bool((err <= bound).all()), what


def check_outputs(got, exact, emul, what, names=OUTPUTS):
    for n in names:
        assert_flash_close(got[n], exact[n], emul[n], f"{what} {n}")
    if "o" in names:
        assert_lse_close(got["lse"], exact["lse"], f"{what} lse")


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(CASES))
def test_flash_vs_float64(name):
    c = case(name)
    q, k, v, do, mask, seg = (cuda(c[n]) for n in
                              ("q", "k", "v", "do", "mask", "seg"))
    got = run_kernels(q, k, v, do, mask, seg, c["drop"])
    check_outputs(got, c["exact"], c["emul"], name)
    check_fa_dot(do, c["exact"]["o"], name)
    pk = run_packed(q, k, v, do, mask, seg, c["H"], c["drop"])
    assert_packed_equal(pk, got, name)
    # masked keys take no gradient and add none
    if name.startswith("ragged"):
        L = c["L"]
        assert bool((got["dk"][0, :, L - 1:] == 0).all())
        assert bool((got["dv"][1, :, 1:] == 0).all())
    if name == "left-pad":
        assert bool((got["dk"][0, :, :37] == 0).all())
        assert bool((got["dv"][0, :, :37] == 0).all())


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["one-tile", "ragged-96"])
def test_legacy_ds_path_vs_float64(name):
    """emit_ds, flash_dq on that dS, and p_from_lse.  p_from_lse gets the
    bf16 scores and the f32 lse of the reference, and its expected value is
    the float64 formula of those inputs: it has no inner rounding point, so
    exact and emul coincide and the bound is four floors."""
    c = case(name)
    ext = ops.hip_ops()
    q, k, v, do, mask = (cuda(c[n]) for n in ("q", "k", "v", "do", "mask"))
    o, lse = ext.flash_fwd(q, k, v, mask, SCALE)
    ddot = ext.fa_dot(do, o)
    ds, dk, dv = ext.flash_bwd_fused(q, k, v, do, mask, lse, ddot, SCALE,
                                     emit_ds=True)
    dq = ext.flash_dq(ds, k)
    got = dict(ds=ds, dk=dk, dv=dv, dq=dq)
    check_outputs(got, c["exact"], c["emul"], f"{name} emit_ds",
                  ("ds", "dq", "dk", "dv"))
    dk2, dv2 = ext.flash_bwd_fused(q, k, v, do, mask, lse, ddot, SCALE)
    assert torch.equal(dk2, dk) and torch.equal(dv2, dv)

    s16 = torch.matmul(c["q"].to(F64), c["k"].to(F64).transpose(-1, -2)) \
        .to(BF16)
    lse32 = c["exact"]["lse"].float()
    want = SCALE * s16.to(F64) + lse32.to(F64).neg().unsqueeze(-1)
    if c["mask"] is not None:
        want = want + key_bias(c["mask"]).to(F64)
    want = torch.exp(want)
    p = ext.p_from_lse(s16.cuda(), mask, lse32.cuda(), SCALE)
    assert_flash_close(p, want, want, f"{name} p_from_lse p")


@pytest.mark.gpu
def test_all_pad_row():
    """Row 0 is padding throughout.  In f32, s * scale - 1e9 is exactly -1e9
    for |s * scale| < 32 (half an ulp at 1e9), so the defined result is the
    uniform average: o = mean_k v and lse = -1e9 + log L.  Row 1 has no
    padding and must not notice its neighbour."""
    B, H, L = 2, 2, 64
    q, k, v, do = inputs(B, H, L, 640)
    s = SCALE * torch.matmul(q.to(F64), k.to(F64).transpose(-1, -2))
    assert float(s.abs().max()) < 31            # the premise above
    mask = torch.zeros(B, L)
    mask[0] = -1e9
    qg, kg, vg, dog, mg = (cuda(t) for t in (q, k, v, do, mask))
    got = run_kernels(qg, kg, vg, dog, mg, None)
    pk = run_packed(qg, kg, vg, dog, mg, None, H)
    assert_packed_equal(pk, got, "all-pad")

    mean_v = v[0].to(F64).mean(dim=1, keepdim=True).expand(H, L, 64)
    assert_flash_close(got["o"][0], mean_v, mean_v, "all-pad row 0 o")
    lse0 = got["lse"].view(B, H, L)[0].cpu().to(F64)
    want = -1e9 + math.log(L)
    assert bool(((lse0 - want).abs() <= 1e-6 * abs(want)).all())
    for n in ("dq", "dk", "dv"):
        assert bool(torch.isfinite(got[n][0].float()).all()), n

    alone = run_kernels(qg[1:].contiguous(), kg[1:].contiguous(),
                        vg[1:].contiguous(), dog[1:].contiguous(),
                        mg[1:].contiguous(), None)
    for n in ("o", "dq", "dk", "dv"):
        assert torch.equal(got[n][1:], alone[n]), f"row 1 {n}"
    for n in ("lse", "ddot"):
        assert torch.equal(got[n].view(B, H, L)[1:],
                           alone[n].view(1, H, L)), f"row 1 {n}"
    exact, emul = both(q[1:], k[1:], v[1:], do[1:], None)
    check_outputs(alone, exact, emul, "all-pad row 1")


@pytest.mark.gpu
@pytest.mark.parametrize("pattern", ["random", "cross", "jump", "last"])
def test_window(pattern):
    """L 2080 = 65 query tiles: FaLiveScan fetches a second 64-tile flag
    window, crosses into it (cross), jumps over an all-dead first window
    (jump) and finds the second window dead (last)."""
    (q, k, v, do), exact, emul = window_case(pattern)
    H = 1
    qg, kg, vg, dog = (cuda(t) for t in (q, k, v, do))
    plain = run_kernels(qg, kg, vg, dog, None, None)
    got = run_kernels(qg, kg, vg, dog, None, None, dead_flags=True)
    dead = got["dead"].flatten().nonzero().flatten().tolist()
    assert dead == {"random": [], "cross": [60, 61, 62, 63],
                    "jump": list(range(64)), "last": [64]}[pattern]
    for n in ("dq", "dk", "dv"):
        assert torch.equal(got[n], plain[n]), f"{n} differs with the flags"
    check_outputs(got, exact, emul, f"window-{pattern}")
    check_fa_dot(dog, exact["o"], f"window-{pattern}")

    pk = run_packed(qg, kg, vg, dog, None, None, H)
    assert_packed_equal(pk, got, f"window-{pattern}")
    ext = ops.hip_ops()
    off = ext.flash_bwd_packed(pk["qkv"], pk["o_p"], pk["do_p"], None,
                               pk["lse"], H, SCALE, None, skip_zero_do=False)
    assert torch.equal(off, pk["dqkv"])
    dqkv, dbias = ext.flash_bwd_packed_bias(pk["qkv"], pk["o_p"], pk["do_p"],
                                            None, pk["lse"], H, SCALE)
    assert torch.equal(dqkv, pk["dqkv"])
    B, L, W = dqkv.shape
    want = dqkv.double().reshape(B * L, W).sum(0).float()
    assert_close(dbias, want, "dqkv_bias", **tol_dparam(B * L))
    for i, third in enumerate("qkv"):
        sl = slice(i * W // 3, (i + 1) * W // 3)
        assert torch.allclose(dbias[sl].float(), want[sl],
                              **tol_dparam(B * L)), third


@pytest.mark.gpu
def test_packed_autograd_vs_float64():
    c = case("ragged-160")
    H = c["H"]
    qkv = torch.cat([packed(c[n]) for n in ("q", "k", "v")], dim=-1) \
        .cuda().requires_grad_()
    out = ops.flash_attention_packed(qkv, H, cuda(c["mask"]), SCALE)
    out.backward(packed(c["do"]).cuda())
    got = dict(o=unpacked(out.detach(), H))
    for n, t in zip(("dq", "dk", "dv"), qkv.grad.split(H * 64, dim=-1)):
        got[n] = unpacked(t, H)
    for n in OUTPUTS:
        assert_flash_close(got[n], c["exact"][n], c["emul"][n],
                           f"autograd {n}")
