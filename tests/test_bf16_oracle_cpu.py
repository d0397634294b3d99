"""The bf16 oracle's per-element bound (bf16_oracle.py), kept honest without a GPU: a torch emulation of a layer
(bf16 operands, fp32 accumulation in two orders, fp32 bias, ReLU, one rounding) stays inside it, and each subtly
wrong variant of the same emulation leaves it. Shapes are cut down in M only: the conv has Conv2's K = 2400 on 7x7
pixels of 2 images, the FC has FC6's K = 9216 with 64 outputs on 6 rows."""
import pytest
import torch
import torch.nn.functional as F

from bf16_oracle import (C_ACC, U, assert_pool_bracket, assert_within, bf16_bound, conv_ref, f32_bound, fc_ref, maxpool,
                         quant, worst)


def _bf16_values(shape, gen, scale=1.0):
    return (torch.randn(shape, generator=gen) * scale).to(torch.bfloat16).float()


def _bias(n, gen):
    """fp32, none of it bf16-representable, one channel clipped by ReLU."""
    b = torch.randn(n, generator=gen) * 0.1
    b.view(torch.int32).bitwise_or_(1)
    b[1] = -100.0 - 2.0 ** -10
    assert (b.to(torch.bfloat16).float() != b).all()
    return b


def _sum_blas(a, w):  # fp32 accumulation, the BLAS's order
    return a @ w.T


def _sum_tiles(a, w):  # fp32 accumulation, 64-wide K tiles one after another
    acc = torch.zeros(a.shape[0], w.shape[0])
    for k in range(0, a.shape[1], 64):
        acc = acc + a[:, k:k + 64] @ w[:, k:k + 64].T
    return acc


def _truncate(v):  # fp32 -> bf16 by dropping the low 16 bits
    return (v.contiguous().view(torch.int32) & ~0xFFFF).view(torch.float32)


def _rne(v):
    return v.to(torch.bfloat16).float()


SUMS = {"blas": _sum_blas, "tiles64": _sum_tiles}


def _case(kind):
    """-> (a [M, K] fp32 of bf16 values, wq [out, K] fp32 of bf16 values, b fp32, images, ref, T, out shape)"""
    g = torch.Generator().manual_seed(11 if kind == "conv" else 12)
    if kind == "conv":
        x = _bf16_values((2, 11, 11, 96), g).abs()  # post-ReLU, post-pool activations are >= 0
        w = (torch.rand((16, 96, 5, 5), generator=g) * 2 - 1) * (6.0 / 2400) ** 0.5
        b = _bias(16, g)
        ref, T = conv_ref(x, w, b)
        a = F.unfold(x.permute(0, 3, 1, 2), 5).permute(0, 2, 1).reshape(2 * 49, 2400)
        wq = quant(w).float().reshape(16, 2400)
        return a, wq, b, 2, ref.reshape(98, 16), T.reshape(98, 16), (2, 7, 7, 16)
    x = _bf16_values((6, 9216), g).abs()
    w = (torch.rand((64, 9216), generator=g) * 2 - 1) * (6.0 / 9216) ** 0.5
    b = _bias(64, g)
    ref, T = fc_ref(x, w, b)
    return x, quant(w).float(), b, 6, ref, T, (6, 64)


@pytest.fixture(scope="module", params=["conv", "fc"])
def case(request):
    return _case(request.param)


def _emulate(case, order, mutation=None):
    a, wq, b, images, _, _, _ = case
    if mutation == "drop_product":
        a = a.clone()
        a[:, 1234] = 0
    acc = SUMS[order](a, wq)
    bias = {None: b, "no_bias": torch.zeros_like(b), "neighbour_bias": b.roll(1), "bias_twice": 2 * b}.get(mutation, b)
    v = F.relu(acc + bias)
    y = _truncate(v) if mutation == "truncate" else _rne(v)
    if mutation == "swap_images":
        y = y.reshape(images, -1, y.shape[1]).flip(0).reshape(y.shape)
    return y


@pytest.mark.parametrize("order", list(SUMS))
def test_emulation_is_inside_the_bound(case, order):
    want, tol = bf16_bound(case[4], case[5])
    ratio = assert_within(_emulate(case, order), want, tol, order)
    assert ratio <= 1.0
    # the fp32 form (FC8): the accumulation alone is far inside C_ACC * T
    acc = SUMS[order](case[0], case[1]) + case[2]
    fr = assert_within(acc, *f32_bound(case[4], case[5]), order)
    assert fr <= 0.25, fr  # <= 5e-7 * T, the figure the GPU test reports


@pytest.mark.parametrize("order", list(SUMS))
@pytest.mark.parametrize("mutation", ["drop_product", "no_bias", "neighbour_bias", "bias_twice", "swap_images",
                                      "truncate"])
def test_mutation_leaves_the_bound(case, order, mutation):
    want, tol = bf16_bound(case[4], case[5])
    got = _emulate(case, order, mutation)
    bad, ratio = worst(got, want, tol)
    assert bad > 0 and ratio > 1.0, (mutation, bad, ratio)
    with pytest.raises(AssertionError):
        assert_within(got, want, tol, mutation)


def test_f32_bound_catches_a_dropped_product_and_bias_errors(case):
    ref, tol = f32_bound(case[4], case[5])
    a, wq, b = case[0], case[1], case[2]
    d = a.clone()
    d[:, 1234] = 0
    for got in (d @ wq.T + b, a @ wq.T, a @ wq.T + b.roll(1), a @ wq.T + 2 * b):
        assert worst(got, ref, tol)[0] > 0


def test_clipped_channel_must_be_zero(case):
    """A channel ReLU clips everywhere has want = 0 and a bound of (1 + U) * C_ACC * T: a kernel that dropped its
    bias (so the channel is not clipped) cannot hide there."""
    want, tol = bf16_bound(case[4], case[5])
    assert want[:, 1].abs().max() == 0 and tol[:, 1].max() < 1e-3
    assert _emulate(case, "blas")[:, 1].abs().max() == 0


def test_pool_bracket_passes_the_exact_pool_and_fails_a_short_window():
    case = _case("conv")
    want, tol = bf16_bound(case[4], case[5])
    shape = case[6]
    want, tol = want.reshape(shape), tol.reshape(shape)
    y = _emulate(case, "tiles64").reshape(shape)
    pooled = maxpool(y)
    assert assert_pool_bracket(pooled, want, tol, "pool") <= 1.0
    # the max over each 3x3 window without its last pixel
    win = y.unfold(1, 3, 2).unfold(2, 3, 2).reshape(2, 3, 3, 16, 9)
    short = win[..., :8].amax(-1)
    assert not torch.equal(short, pooled)
    with pytest.raises(AssertionError):
        assert_pool_bracket(short, want, tol, "short window")


def test_bound_constants():
    assert C_ACC == 2e-6 and U == 2.0 ** -8
