"""MXFP8 serving on the GPU: the quantising kernels against the bitwise
contracts, the block-scaled GEMM against float64, and the quantised model.

Kernel geometry (csrc/mx_quant.hip, csrc/mx.h): a lane holds one 16-byte
packet of 8 bf16 values, so a 32-element block is the four packets of a lane
quad and its maximum takes two cross-lane steps; a lane stores 8 bytes of q
and the quad's first lane the scale byte.  mx_quant_rows and mx_bias_gelu
see the tensor as a flat run of packets: 256 threads per block, one packet
per thread, grid capped at 2048 blocks = 524,288 packets = 4,194,304
elements, grid-stride beyond that; R = 4100 at K = 1024 (4,198,400 elements)
is the case past the cap.  The LayerNorm MX mode keeps the bf16 kernels'
geometry (one wave per row, packet p of lane l at element (p * 64 + l) * 8):
D = 512, 1024, 2048 take the templated kernel, D = 4096 the register-cached
path of the general kernel, D = 128 and 480 its two-pass path with idle
lanes (16 and 60 of 64 active: whole quads).
"""
import pytest
import torch

from tosem2021_amd import ops
from tosem2021_amd.ops import reference

from test_mx_cpu import (SWEEP_PIVOTS, assert_logits_equal, assert_mx_equal,
                         check_composition, check_raises_and_clear,
                         check_stale_under_trainer, make_inputs, make_model,
                         sweep_expected, sweep_input)

pytestmark = pytest.mark.gpu

BF16 = torch.bfloat16
EPS = 1e-5


def dev():
    return torch.device("cuda", 0)


# ---- mx_quant_rows against the reference -------------------------------------

def _plants():
    """Block patterns, each a function of a block's 32 normal values."""
    def amax_at(j, v=5.0):
        def f(b):
            b = b * 0.1
            b[j] = v
            return b
        return f

    def subnormals(b):
        bits = torch.arange(1, 33, dtype=torch.int16) * 3        # 3 .. 96
        bits[1::2] |= -0x8000                                    # some negative
        return bits.view(BF16).float()

    return [
        lambda b: torch.zeros(32),                  # an all-zero block
        subnormals,                                 # bf16 subnormals only
        amax_at(0), amax_at(7), amax_at(8), amax_at(31),    # the lane edges
        amax_at(13, -7.0),                          # a negative maximum
        amax_at(3, 1.8125 * 8), amax_at(20, 1.9375 * 8),    # mantissa > 1.75
        amax_at(9, -1.96875 * 0.25),
        lambda b: b * 2.0 ** 126,                   # a 2^127-scale block ...
        lambda b: b * 2.0 ** -120,                  # ... next to a 2^-120 one
    ]


def planted(R, K, seed):
    """Seeded normal bf16 [R, K] with the patterns above planted into
    consecutive blocks, as many as fit, starting at the last block of row 0
    so that they straddle a row boundary where there is one.  Block 0 always
    keeps its normal data, so the smallest shapes (one or two blocks) still
    test ordinary values."""
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(R * K // 32, 32, generator=g)
    start = max(K // 32 - 1, 1)
    n = 0
    for i, f in enumerate(_plants()):
        if start + i < x.shape[0]:
            x[start + i] = f(x[start + i].clone())
            n += 1
    return x.view(R, K).to(BF16), n


@pytest.mark.parametrize("K", [32, 64, 128, 480, 512, 544, 1024, 4096, 4128])
@pytest.mark.parametrize("R", [1, 3, 130])
def test_quant_rows_matches_reference(R, K):
    x, n = planted(R, K, seed=R * 10000 + K)
    if R == 130:
        assert n == len(_plants())
    assert x[0, :32].float().abs().max() > 0.5      # block 0 is ordinary
    assert x[0, :32].count_nonzero() > 28
    assert torch.isfinite(x.float()).all()
    q, s = ops.mx_quant_rows(x.to(dev()))
    assert q.shape == (R, K) and s.shape == (R, K // 32)
    assert_mx_equal(q, s, *reference.mx_quantize(x))


def test_quant_rows_past_the_grid_cap():
    R, K = 4100, 1024
    assert R * K // 8 > 2048 * 256
    x, n = planted(R, K, seed=5)
    assert n == len(_plants())
    q, s = ops.mx_quant_rows(x.to(dev()))
    assert_mx_equal(q, s, *reference.mx_quantize(x))


@pytest.mark.parametrize("pivot", SWEEP_PIVOTS)
def test_quant_rows_exhaustive_sweep(pivot):
    q, s = ops.mx_quant_rows(sweep_input(pivot).to(dev()))
    assert_mx_equal(q, s, *sweep_expected(pivot))


def test_quant_rows_leading_dims_and_bad_k():
    x, _ = planted(6, 64, seed=6)
    q, s = ops.mx_quant_rows(x.view(2, 3, 64).to(dev()))
    assert q.shape == (2, 3, 64) and s.shape == (2, 3, 2)
    qr, sr = reference.mx_quantize(x)
    assert_mx_equal(q.view(6, 64), s.view(6, 2), qr, sr)
    with pytest.raises(RuntimeError, match="multiple of 32"):
        ops.mx_quant_rows(torch.zeros(4, 48, dtype=BF16, device=dev()))


# ---- the fused producers against mx_quant_rows of today's kernels ------------

def _ln_operands(N, D, seed):
    g = torch.Generator().manual_seed(seed)
    x = (torch.randn(N, D, generator=g) * 2).to(BF16)
    # a residual with outliers: block maxima with every mantissa
    r = (torch.randn(N, D, generator=g)
         * torch.exp2(torch.randint(-3, 4, (N, D), generator=g).float())
         ).to(BF16)
    gamma = (1 + 0.3 * torch.randn(D, generator=g)).to(BF16)
    beta = (0.2 * torch.randn(D, generator=g)).to(BF16)
    return tuple(t.to(dev()) for t in (x, r, gamma, beta))


@pytest.mark.parametrize("D", [128, 480, 512, 1024, 2048, 4096])
@pytest.mark.parametrize("N", [1, 3, 130])
def test_layernorm_mx_is_quant_rows_of_layernorm(N, D):
    x, r, gamma, beta = _ln_operands(N, D, seed=N * 10000 + D)
    y, s_out = ops.fused_add_layernorm(x, r, gamma, beta, EPS)
    q, s, sm = ops.mx_add_layernorm(x, r, gamma, beta, EPS)
    assert torch.equal(sm, s_out)
    assert_mx_equal(q, s, *ops.mx_quant_rows(y))
    y = ops.fused_layernorm(x, gamma, beta, EPS)
    assert_mx_equal(*ops.mx_layernorm(x, gamma, beta, EPS),
                    *ops.mx_quant_rows(y))


def test_layernorm_mx_grid_stride_rows():
    """More rows than the forward grid holds at once (4096 blocks of 4
    waves): the row loop and the next-row prefetch of the MX mode."""
    N, D = 4 * 4096 + 37, 512
    x, r, gamma, beta = _ln_operands(N, D, seed=8)
    y, s_out = ops.fused_add_layernorm(x, r, gamma, beta, EPS)
    q, s, sm = ops.mx_add_layernorm(x, r, gamma, beta, EPS)
    assert torch.equal(sm, s_out)
    assert_mx_equal(q, s, *ops.mx_quant_rows(y))


def test_layernorm_mx_width_limits():
    for D in (8192, 4128):
        x, r, gamma, beta = _ln_operands(2, D, seed=9)
        with pytest.raises(RuntimeError, match="4096"):
            ops.mx_layernorm(x, gamma, beta, EPS)
    x, r, gamma, beta = _ln_operands(2, 72, seed=9)
    with pytest.raises(RuntimeError, match="multiple of 32"):
        ops.mx_add_layernorm(x, r, gamma, beta, EPS)


@pytest.mark.parametrize("F", [256, 4096])
@pytest.mark.parametrize("N", [1, 3, 130])
def test_bias_gelu_mx_is_quant_rows_of_bias_gelu(N, F):
    g = torch.Generator().manual_seed(N * 10000 + F)
    h = (torch.randn(N, F, generator=g) * 3).to(BF16).to(dev())
    b = torch.randn(F, generator=g).to(BF16).to(dev())
    assert_mx_equal(*ops.mx_bias_gelu(h, b),
                    *ops.mx_quant_rows(ops.fused_bias_gelu(h, b)))


@pytest.mark.parametrize("N,F", [(1030, 4096), (8800, 480)])
def test_bias_gelu_mx_past_the_grid_cap(N, F):
    """More than 524,288 packets: threads go round the grid-stride loop and
    carry the bias column along it.  F = 4096 divides the stride (the column
    stays put); F = 480 does not (it moves by 64 per round and wraps)."""
    assert N * F // 8 > 2048 * 256
    g = torch.Generator().manual_seed(N + F)
    h = (torch.randn(N, F, generator=g) * 3).to(BF16).to(dev())
    b = torch.randn(F, generator=g).to(BF16).to(dev())
    assert_mx_equal(*ops.mx_bias_gelu(h, b),
                    *ops.mx_quant_rows(ops.fused_bias_gelu(h, b)))


# ---- mx_linear against float64 ------------------------------------------------

def _gemm_operand(R, K, g):
    """bf16 [R, K] whose blocks carry scales 2^-20, 1 or 2^20, drawn per
    (row, block): neighbours differ by up to 2^40 within a row and between
    rows, so a scale taken from another block or row misses by orders of
    magnitude."""
    e = torch.randint(-1, 2, (R, K // 32), generator=g).float() * 20
    e[:, 0], e[:, -1] = 20, -20         # both extremes in every row
    return (torch.randn(R, K, generator=g)
            * torch.exp2(e).repeat_interleave(32, 1)).to(BF16)


@pytest.mark.parametrize("with_bias", [False, True])
@pytest.mark.parametrize("M,N,K", [(32, 32, 128), (64, 384, 128),
                                   (64, 3072, 1024), (64, 1024, 4096),
                                   (96, 4096, 1024)])
def test_mx_linear_against_float64(M, N, K, with_bias):
    """Budget per output: 2^-8 |y| for the bf16 rounding (or its neighbour)
    plus K 2^-24 sum_k |a_k w_k| for an f32 accumulation in any order, both
    from float64 of the same dequantised operands."""
    g = torch.Generator().manual_seed(M + N + K)
    qa, sa = reference.mx_quantize(_gemm_operand(M, K, g))
    qw, sw = reference.mx_quantize(_gemm_operand(N, K, g))
    a64 = reference.mx_dequantize(qa, sa).double()
    w64 = reference.mx_dequantize(qw, sw).double()
    y64 = a64 @ w64.t()
    bias = None
    if with_bias:
        # of the outputs' size, so that it matters
        bias = (torch.randn(N, generator=g) * y64.std()).to(BF16)
        y64 = y64 + bias.double()
    budget = 2.0 ** -8 * y64.abs() + K * 2.0 ** -24 * (a64.abs()
                                                       @ w64.abs().t())
    y = ops.mx_linear(qa.to(dev()), sa.to(dev()), qw.to(dev()), sw.to(dev()),
                      None if bias is None else bias.to(dev()))
    assert y.dtype == BF16 and y.shape == (M, N)
    err = (y.double().cpu() - y64).abs()
    worst = float((err / budget).max())
    print(f"mx_linear {M}x{N}x{K} bias={with_bias} "
          f"backend={ops.mx_gemm_backend()} worst err/budget {worst:.3f}")
    assert worst <= 1.0


@pytest.mark.parametrize("with_bias", [False, True])
@pytest.mark.parametrize("M,N,K", [(32, 32, 128), (96, 160, 256),
                                   (256, 384, 1024)])
def test_block_scaled_gemm_branch(M, N, K, with_bias, monkeypatch):
    """The torch._scaled_mm branch of mx_linear, which the probe may turn
    down (it does on the library this was written against, whose MX kernels
    truncate their bf16 output): run it forced, so that its operand views,
    the scale rows filled up to a multiple of 128 (M = 32 and 96, N = 32 and
    160) and the bias add stay right.  A scale taken from another block or
    row misses by orders of magnitude (2^20 between neighbours).

    Budget, from the formats alone: a truncated bf16 result is off by less
    than one ulp, at most 2^-7 |acc|; the f32 accumulation in any order by
    K 2^-24 sum |a w|; with the bias added to the bf16 result by torch, one
    more rounding to nearest of the sum, at most 2^-8 |y|."""
    monkeypatch.setattr(ops, "_MX_BACKEND", ("scaled_mm", False))
    monkeypatch.setattr(ops, "_MX_REFUSED", set())
    g = torch.Generator().manual_seed(M + N + K + 1)
    qa, sa = reference.mx_quantize(_gemm_operand(M, K, g))
    qw, sw = reference.mx_quantize(_gemm_operand(N, K, g))
    a64 = reference.mx_dequantize(qa, sa).double()
    w64 = reference.mx_dequantize(qw, sw).double()
    acc64 = a64 @ w64.t()
    budget = 2.0 ** -7 * acc64.abs() + K * 2.0 ** -24 * (a64.abs()
                                                         @ w64.abs().t())
    y64, bias = acc64, None
    if with_bias:
        bias = (torch.randn(N, generator=g) * acc64.std()).to(BF16)
        y64 = acc64 + bias.double()
        budget = budget + 2.0 ** -8 * y64.abs()
    import warnings
    with warnings.catch_warnings():
        warnings.simplefilter("error")      # a refused shape would warn
        y = ops.mx_linear(qa.to(dev()), sa.to(dev()), qw.to(dev()),
                          sw.to(dev()),
                          None if bias is None else bias.to(dev()))
    assert not ops._MX_REFUSED
    err = (y.double().cpu() - y64).abs()
    worst = float((err / budget).max())
    print(f"scaled_mm branch {M}x{N}x{K} bias={with_bias} worst err/budget "
          f"{worst:.3f}")
    assert worst <= 1.0


def test_mx_linear_off_lattice_raises_and_backend_is_named():
    assert ops.mx_gemm_backend() in ("scaled_mm", "hipblaslt", "dequant")
    for M, N, K in [(33, 32, 128), (32, 40, 128), (32, 32, 96)]:
        assert not ops.mx_supported(M, N, K)
        q = torch.zeros(M, K, dtype=torch.uint8, device=dev())
        s = torch.zeros(M, K // 32, dtype=torch.uint8, device=dev())
        wq = torch.zeros(N, K, dtype=torch.uint8, device=dev())
        ws = torch.zeros(N, K // 32, dtype=torch.uint8, device=dev())
        with pytest.raises(ValueError, match="multiples of 32"):
            ops.mx_linear(q, s, wq, ws)


def test_mx_linear_leading_dims():
    g = torch.Generator().manual_seed(11)
    qa, sa = reference.mx_quantize(_gemm_operand(64, 128, g))
    qw, sw = reference.mx_quantize(_gemm_operand(32, 128, g))
    args = [t.to(dev()) for t in (qa, sa, qw, sw)]
    flat = ops.mx_linear(*args)
    y = ops.mx_linear(args[0].view(2, 32, 128), args[1].view(2, 32, 4),
                      args[2], args[3])
    assert y.shape == (2, 32, 32) and torch.equal(y.view(64, 32), flat)


# ---- the model ----------------------------------------------------------------

def test_quantised_forward_is_the_written_out_composition_gpu():
    check_composition(make_model(BF16, dev()), *make_inputs(dev()))


def test_quantised_forward_is_deterministic():
    model = make_model(BF16, dev()).quantize_mx()
    tokens, mask, pb = make_inputs(dev())
    with torch.no_grad():
        a = model(tokens, mask), model(None, packing=pb)
        b = model(tokens, mask), model(None, packing=pb)
    for x, y in zip(a, b):
        assert_logits_equal(x, y)


def test_raises_clear_and_state_dict_gpu():
    tokens, mask, _ = make_inputs(dev())
    check_raises_and_clear(make_model(BF16, dev()), tokens, mask)


def test_stale_weights_raise_under_a_trainer_gpu(tmp_path):
    """On the GPU the optimizer step writes through raw pointers: the
    Trainer counts that write itself."""
    check_stale_under_trainer("cuda", tmp_path)


def test_gpu_weights_quantise_like_the_reference():
    """A weight [N, K] goes through the same kernel along K: the quantised
    copies equal the CPU reference's bit for bit."""
    model = make_model(BF16, dev()).quantize_mx()
    for lin in model._mx_linears():
        assert_mx_equal(lin.mx_q, lin.mx_s,
                        *reference.mx_quantize(lin.weight.detach().cpu()))
    assert "mx_q" not in "".join(model.state_dict().keys())
