"""reference.dead_q_tiles on hand-made inputs (no GPU): the flag definition
the flash backward's dead-query-tile skip rests on.  A 32-row tile of one head
is dead iff every bf16 element has (bits & 0x7fff) == 0."""
import pytest
import torch

from tosem2021_amd.ops import reference

BF16 = torch.bfloat16


def _bits(t):
    return t.view(torch.int16)


def test_all_zero_and_all_live():
    z = torch.zeros(2, 3, 64, 64, dtype=BF16)
    assert reference.dead_q_tiles(z).shape == (2, 3, 2)
    assert reference.dead_q_tiles(z).dtype == torch.bool
    assert bool(reference.dead_q_tiles(z).all())
    assert not bool(reference.dead_q_tiles(torch.ones_like(z)).any())


def test_tile_boundaries_and_heads():
    d = torch.zeros(2, 2, 96, 64, dtype=BF16)
    d[0, 0, 31, 63] = 1.0        # last element of tile 0
    d[0, 1, 32, 0] = -2.0        # first element of tile 1
    d[1, 0, 95, 5] = 0.5         # last row of tile 2
    want = torch.ones(2, 2, 3, dtype=torch.bool)
    want[0, 0, 0] = want[0, 1, 1] = want[1, 0, 2] = False
    assert torch.equal(reference.dead_q_tiles(d), want)


def test_negative_zero_is_dead_subnormal_is_live():
    d = torch.zeros(1, 1, 64, 64, dtype=BF16)
    _bits(d)[0, 0, :32] = -32768            # 0x8000: a tile of -0.0
    _bits(d)[0, 0, 40, 17] = 1              # 0x0001: the smallest subnormal
    assert float(d[0, 0, 40, 17]) != 0.0 and float(d[0, 0, 3, 3]) == 0.0
    assert reference.dead_q_tiles(d).tolist() == [[[True, False]]]
    _bits(d)[0, 0, 40, 17] = -32767         # 0x8001: the negative subnormal
    assert reference.dead_q_tiles(d).tolist() == [[[True, False]]]


def test_nan_and_inf_are_live():
    d = torch.zeros(1, 1, 64, 64, dtype=BF16)
    d[0, 0, 0, 0] = float("nan")
    d[0, 0, 63, 63] = float("-inf")
    assert reference.dead_q_tiles(d).tolist() == [[[False, False]]]


def test_packed_layout_matches_bhld():
    torch.manual_seed(0)
    B, H, L = 2, 3, 64
    d4 = torch.randn(B, H, L, 64).to(BF16)
    d4[0, 1, 32:] = 0
    d4[1, 2, :32] = 0
    d4[1, 0] = 0
    packed = d4.permute(0, 2, 1, 3).reshape(B, L, H * 64).contiguous()
    got = reference.dead_q_tiles(packed, H)
    assert torch.equal(got, reference.dead_q_tiles(d4))
    assert int(got.sum()) == 4


def test_rejects_bad_inputs():
    with pytest.raises(ValueError):
        reference.dead_q_tiles(torch.zeros(1, 1, 32, 64))            # f32
    with pytest.raises(ValueError):
        reference.dead_q_tiles(torch.zeros(1, 1, 48, 64, dtype=BF16))
    with pytest.raises(ValueError):
        reference.dead_q_tiles(torch.zeros(1, 32, 128, dtype=BF16), 3)
    with pytest.raises(ValueError):
        reference.dead_q_tiles(torch.zeros(1, 32, 128, dtype=BF16))
