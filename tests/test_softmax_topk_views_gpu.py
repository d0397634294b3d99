"""The view-averaging head kernel (softmax_topk_views.hip) against the fp64 mean of softmaxes
(softmax_topk_views_cases.py has the bound; expf differs between host and device, so the kernel is not compared with
the host definition's bits), and the bit identities between its own routes: slabs against logits, vector loads
against scalar loads."""
import pytest
import torch

from anx.ops import softmax_topk_views
from softmax_topk_cases import random_rows
from softmax_topk_views_cases import assert_order, assert_views, confident_minority, one_hot_votes, repeated_crafted

pytestmark = pytest.mark.gpu

K_SIZES = (1, 2, 63, 64, 65, 257, 1000, 1001, 4099, 7680)
V_SIZES = (1, 2, 3, 10, 32)


def bits(t):
    return t.contiguous().view(torch.int32)


def same(a, b):
    return all(torch.equal(bits(x), bits(y)) for x, y in zip(a, b))


@pytest.mark.parametrize("V", V_SIZES)
@pytest.mark.parametrize("K", K_SIZES)
def test_random_rows_against_fp64(cuda, K, V):
    for N in (1, 3):
        z = random_rows(N * V, K, seed=1000 * V + K + N)
        zd = z.to(cuda)
        for k in sorted({1, min(K, 5), min(K, 16)}):
            idx, prob, probs = softmax_topk_views(zd, V, k, return_probs=True)
            assert_views(idx, prob, probs, z, V, k, f"K={K} V={V} N={N} k={k}")
            assert same(softmax_topk_views(zd, V, k), (idx, prob))


def test_too_many_classes_raise(cuda):
    with pytest.raises(ValueError):
        softmax_topk_views(torch.zeros(2, 7681, device=cuda), 2, 5)
    idx, prob = softmax_topk_views(torch.zeros(2, 7680, device=cuda), 2, 5)
    assert idx.tolist() == [[0, 1, 2, 3, 4]]


@pytest.mark.parametrize("K", (64, 1000, 7680))
def test_offset_logits_take_the_scalar_loads_and_give_the_same_bits(cuda, K):
    N, V = 3, 10
    z = random_rows(N * V, K, seed=K + 1).to(cuda)
    flat = torch.empty(z.numel() + 1, device=cuda)
    shifted = flat[1:].view(N * V, K)
    shifted.copy_(z)
    assert z.data_ptr() % 16 == 0 and shifted.data_ptr() % 16 == 4 and shifted.is_contiguous()
    assert same(softmax_topk_views(shifted, V, 16, return_probs=True), softmax_topk_views(z, V, 16, return_probs=True))


@pytest.mark.parametrize("K", (63, 1001, 4099))
def test_rows_of_no_whole_vectors_give_the_bits_of_their_padded_rows(cuda, K):
    """K % 4 != 0 takes the scalar loads. The same rows padded to K + pad columns of -inf take the vector loads:
    a padded class adds exp(-inf) = 0 to its thread's sum and can never be the maximum, so every other class must
    come out with the same bits, and the padding ranks last."""
    N, V = 3, 10
    pad = 4 - K % 4
    z = random_rows(N * V, K, seed=K + 2)
    padded = torch.cat([z, torch.full((N * V, pad), float("-inf"))], dim=1).to(cuda)
    a = softmax_topk_views(z.to(cuda), V, 16, return_probs=True)
    b = softmax_topk_views(padded, V, 16, return_probs=True)
    assert same((a[0], a[1], a[2]), (b[0], b[1], b[2][:, :K]))
    assert (b[2][:, K:] == 0).all()


@pytest.mark.parametrize("ksplit", (1, 2, 3, 4))
@pytest.mark.parametrize("with_bias", (True, False))
def test_slabs_equal_logits_bit_for_bit(cuda, ksplit, with_bias):
    for K in (1000, 257):  # vector and scalar loads
        N, V = 3, 10
        M = N * V
        g = torch.Generator().manual_seed(10 + ksplit + K)
        ws = torch.randn(ksplit, M, K, generator=g) * torch.logspace(-3, 1, ksplit)[:, None, None]  # order matters
        bias = torch.randn(K, generator=g) if with_bias else None
        z = bias.expand(M, K).clone() if with_bias else ws[0].clone()
        for s in range(0 if with_bias else 1, ksplit):
            z = z + ws[s]
        a = softmax_topk_views(None, V, 5, slabs=ws.to(cuda), bias=bias.to(cuda) if with_bias else None,
                               return_probs=True)
        b = softmax_topk_views(z.to(cuda), V, 5, return_probs=True)
        assert same(a, b), f"K={K} ksplit={ksplit} bias={with_bias}"
        assert_views(*a, z, V, 5, f"K={K} ksplit={ksplit} bias={with_bias}")


def test_crafted_votes(cuda):
    for (z, order), k in ((one_hot_votes(), 3), (confident_minority(), 2)):
        idx, prob, probs = softmax_topk_views(z.to(cuda), 10, k, return_probs=True)
        assert_views(idx, prob, probs, z, 10, k, "crafted votes")
        want = torch.sort(torch.softmax(z.double(), 1).mean(0), descending=True, stable=True).indices[:k].tolist()
        assert idx[0].tolist() == want == order


@pytest.mark.parametrize("K", (2, 65, 1000))
@pytest.mark.parametrize("V", (1, 3, 10))
def test_crafted_rows_repeated_per_view(cuda, K, V):
    rows = repeated_crafted(K, V)
    z = torch.cat(list(rows.values()))
    k = min(K, 16)
    idx, prob, probs = softmax_topk_views(z.to(cuda), V, k, return_probs=True)
    assert_views(idx, prob, probs, z, V, k, f"crafted K={K} V={V}")
    assert idx[list(rows).index("all_equal")].tolist() == list(range(k))


def test_nan_row_still_gives_distinct_indices(cuda):
    K, V, k = 100, 3, 16
    z = random_rows(3 * V, K, seed=5)
    z[V + 1, ::7] = float("nan")  # a view of image 1
    idx, prob, probs = softmax_topk_views(z.to(cuda), V, k, return_probs=True)
    got = idx[1].tolist()
    assert len(set(got)) == k and all(0 <= i < K for i in got)
    assert_order(idx, prob, probs, k, "the NaN image and its neighbours")  # also where no bound is defined
    keep = torch.tensor([0, 2])
    rows = torch.cat([torch.arange(V), torch.arange(2 * V, 3 * V)])
    assert_views(idx.cpu()[keep], prob.cpu()[keep], probs.cpu()[keep], z[rows], V, k, "neighbours of the NaN image")
