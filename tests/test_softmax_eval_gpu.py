"""The evaluation head kernel (softmax_eval.hip) against softmax_eval_cases.py's fp64 reference and bounds (expf and
logf differ between host and device, so the kernel is not compared with the host definition's bits), the bit
identities between its own routes (vector against scalar loads, slabs against logits) and against the two other head
kernels on the same rows, and the running counters: exact, and the same bits from run to run on two streams."""
import pytest
import torch

from anx import _native as nat
from anx.ops import softmax_eval, softmax_topk, softmax_topk_views
from softmax_eval_cases import (assert_eval, assert_rank_in_head, crafted_eval_rows, expected_confusion, expected_stats,
                                labels_for, special_value_rows)
from softmax_topk_cases import random_rows

pytestmark = pytest.mark.gpu

K_SIZES = (1, 5, 255, 257, 1000, 1001, 7680)
V_SIZES = (None, 1, 2, 10)


def bits(t):
    return t.contiguous().view(torch.int32)


def same(a, b):
    return all(torch.equal(bits(x), bits(y)) for x, y in zip(a, b))


def head_of(zd, V, k):
    """(idx, probs or None) of the other head kernel on the same rows."""
    if V is None:
        return softmax_topk(zd, k)[0], None
    idx, _, probs = softmax_topk_views(zd, V, k, return_probs=True)
    return idx, probs


def check_against_heads(rank, pred, y, idx, k, what):
    """pred == idx[:, 0]; idx[i, rank[i]] == y wherever rank < 16; rank >= k wherever y is absent from idx."""
    rank, pred, y, idx = rank.cpu(), pred.cpu(), y.cpu(), idx.cpu()
    assert torch.equal(pred, idx[:, 0]), f"{what}: pred is not the head's first class"
    kk = idx.shape[1]
    for i in range(y.shape[0]):
        r, yi = int(rank[i]), int(y[i])
        if 0 <= r < kk:
            assert int(idx[i, r]) == yi, f"{what}: image {i}: idx[rank] is not the label"
        if yi not in idx[i, :k].tolist():
            assert r >= k or r == -1, f"{what}: image {i}: rank {r} < k but the label is not among the k"
        else:
            assert 0 <= r < k, f"{what}: image {i}: the label is among the k but rank is {r}"


# 15360 classes are the limit of the call without views; 7680 that of the call with views
@pytest.mark.parametrize("K,V", [(K, V) for K in K_SIZES for V in V_SIZES] + [(15360, None)])
def test_random_rows_against_fp64(cuda, K, V):
    v = V or 0
    for N in (1, 7):
        z = random_rows(N * max(v, 1), K, seed=2000 * v + K + N)
        y = labels_for(z, v, seed=K + N)
        zd, yd = z.to(cuda), y.to(cuda)
        k = min(K, 5)
        rank, nll, pred = softmax_eval(zd, yd, k, views=V)
        idx, probs = head_of(zd, V, min(K, 16))
        what = f"K={K} V={V} N={N}"
        assert_eval(rank, nll, pred, z, y, v, probs, what)
        check_against_heads(rank, pred, y, idx, k, what)


@pytest.mark.parametrize("V", (None, 3), ids=lambda v: f"V{v}")
@pytest.mark.parametrize("K", (5, 257, 1000))
def test_crafted_rows(cuda, K, V):
    z1, y, _ = crafted_eval_rows(K)
    v = V or 0
    z = z1.repeat_interleave(max(v, 1), dim=0)
    zd, yd = z.to(cuda), y.to(cuda)
    rank, nll, pred = softmax_eval(zd, yd, 1, views=V)
    idx, probs = head_of(zd, V, min(K, 16))
    assert_eval(rank, nll, pred, z, y, v, probs, f"crafted K={K} V={V}")
    check_against_heads(rank, pred, y, idx, 1, f"crafted K={K} V={V}")
    z1, y = special_value_rows(K)  # the first round on +inf, -inf, NaN and ties: the other heads' order, bit for bit
    zd, yd = z1.repeat_interleave(max(v, 1), dim=0).to(cuda), y.to(cuda)
    rank, _, pred = softmax_eval(zd, yd, 1, views=V)
    assert_rank_in_head(rank, pred, y, head_of(zd, V, min(K, 16))[0], f"special values K={K} V={V}")
    if V is None:  # by logit: the lone +inf at K // 2 wins, a row of -inf goes by index
        assert pred.tolist()[:6] == [K // 2] * 3 + [0] * 3


@pytest.mark.parametrize("K,V", [(1000, None), (7680, None), (15360, None), (1000, 10), (7680, 10)])
def test_offset_logits_take_the_scalar_loads_and_give_the_same_bits(cuda, K, V):
    N = 3
    M = N * (V or 1)
    z = random_rows(M, K, seed=K + 1)
    y = labels_for(z, V or 0, seed=K).to(cuda)
    z = z.to(cuda)
    flat = torch.empty(z.numel() + 1, device=cuda)
    shifted = flat[1:].view(M, K)
    shifted.copy_(z)
    assert z.data_ptr() % 16 == 0 and shifted.data_ptr() % 16 == 4 and shifted.is_contiguous()
    assert same(softmax_eval(shifted, y, 5, views=V, return_logits=True), softmax_eval(z, y, 5, views=V, return_logits=True))


@pytest.mark.parametrize("V", (None, 2), ids=lambda v: f"V{v}")
@pytest.mark.parametrize("ksplit", (1, 3))
def test_slabs_plus_bias_equal_logits_and_the_logits_are_the_heads_bits(cuda, ksplit, V):
    for K in (1000, 257):  # vector and scalar loads
        N = 7
        M = N * (V or 1)
        g = torch.Generator().manual_seed(10 + ksplit + K)
        ws = torch.randn(ksplit, M, K, generator=g) * torch.logspace(-3, 1, ksplit)[:, None, None]  # order matters
        bias = torch.randn(K, generator=g)
        z = bias.expand(M, K).clone()
        for s in range(ksplit):
            z = z + ws[s]
        y = labels_for(z, V or 0, seed=ksplit).to(cuda)
        wsd, bd = ws.to(cuda), bias.to(cuda)
        a = softmax_eval(None, y, 5, views=V, slabs=wsd, bias=bd, return_logits=True)
        b = softmax_eval(z.to(cuda), y, 5, views=V)
        what = f"K={K} ksplit={ksplit} V={V}"
        assert same(a[:3], b), what
        assert torch.equal(bits(a[3]), bits(z.to(cuda))), f"{what}: logits_out is not the slab sum"
        zt = softmax_topk(None, 5, slabs=wsd, bias=bd, return_logits=True)[2]
        assert torch.equal(bits(a[3]), bits(zt)), f"{what}: logits_out is not softmax_topk's"
        assert_eval(*a[:3], z, y.cpu(), V or 0, head_of(z.to(cuda), V, 1)[1], what)


def test_counters_are_exact_and_the_same_bits_from_run_to_run(cuda):
    """Three calls on two streams into the same counters, twice: exact against Python integers, and identical."""
    K, k = 257, 5
    calls = []
    for c, (N, V) in enumerate(((7, None), (5, 10), (7, 2))):
        z = random_rows(N * (V or 1), K, seed=70 + c)
        y = labels_for(z, V or 0, seed=c)
        y[1] = -1
        calls.append((z.to(cuda), y.to(cuda), V))
    streams = [torch.cuda.Stream(cuda), torch.cuda.Stream(cuda)]
    runs = []
    for _ in range(2):
        stats = torch.zeros(4, dtype=torch.int64, device=cuda)
        conf = torch.zeros(K, K, dtype=torch.int32, device=cuda)
        torch.cuda.synchronize()
        outs = []
        for c, (zd, yd, V) in enumerate(calls):
            with torch.cuda.stream(streams[c % 2]):
                outs.append(softmax_eval(zd, yd, k, views=V, stats=stats, confusion=conf))
        torch.cuda.synchronize()
        runs.append((stats.cpu(), conf.cpu(), [tuple(t.cpu() for t in o) for o in outs]))
    stats, conf, outs = runs[0]
    want, want_conf = [0, 0, 0, 0], torch.zeros(K, K, dtype=torch.int32)
    for (zd, yd, V), (rank, nll, pred) in zip(calls, outs):
        want = [a + b for a, b in zip(want, expected_stats(rank, nll, k))]
        want_conf += expected_confusion(yd, pred, K)
    assert stats.tolist() == want and want[0] == 16
    assert torch.equal(conf, want_conf)
    assert torch.equal(runs[1][0], stats) and torch.equal(runs[1][1], conf)
    for a, b in zip(outs, runs[1][2]):
        assert same(a, b)


@pytest.mark.parametrize("V", (None, 2), ids=lambda v: f"V{v}")
def test_outputs_are_slices_and_their_neighbours_stay(cuda, V):
    K, N = 1001, 7
    z = random_rows(N * (V or 1), K, seed=9).to(cuda)
    y = labels_for(z.cpu(), V or 0, seed=9).to(cuda)
    big = (torch.full((N + 2,), -77, dtype=torch.int32, device=cuda), torch.full((N + 2,), -77.0, device=cuda),
           torch.full((N + 2,), -77, dtype=torch.int32, device=cuda))
    stats = torch.full((6,), -77, dtype=torch.int64, device=cuda)
    stats[1:5] = 0
    conf = torch.zeros(K + 2, K, dtype=torch.int32, device=cuda)
    conf[0], conf[-1] = -77, -77
    got = softmax_eval(z, y, 5, views=V, stats=stats[1:5], confusion=conf[1:-1], out=tuple(t[1:-1] for t in big))
    want = softmax_eval(z, y, 5, views=V)
    torch.cuda.synchronize()
    assert same(got, want)
    for t in big:
        assert t[0] == -77 and t[-1] == -77
    assert stats[0] == -77 and stats[5] == -77 and stats[1] == N
    assert (conf[0] == -77).all() and (conf[-1] == -77).all() and int(conf[1:-1].sum()) == N


def test_limits_are_refused_without_a_launch(cuda):
    y = torch.zeros(2, dtype=torch.int32, device=cuda)
    with pytest.raises(ValueError):
        softmax_eval(torch.zeros(2, 15361, device=cuda), y, 5)
    with pytest.raises(ValueError):
        softmax_eval(torch.zeros(4, 7681, device=cuda), y, 5, views=2)
    # the native entry refuses them too, with a message, before anything is launched
    lib = nat.lib()
    z = torch.zeros(4, 15364, device=cuda)
    out = torch.full((2,), -5, dtype=torch.int32, device=cuda)
    for V, K in ((0, 15361), (2, 7681), (33, 100), (0, 0)):
        assert lib.anx_softmax_eval(z.data_ptr(), 1, 0, None, 2, V, K, 1, y.data_ptr(), out.data_ptr(), None, None, None,
                                    None, None, nat.stream_ptr(cuda)) != 0
        assert "anx_softmax_eval" in lib.anx_last_error().decode()
    torch.cuda.synchronize()
    assert out.tolist() == [-5, -5]
    rank, _, pred = softmax_eval(torch.zeros(2, 15360, device=cuda), y, 5)
    assert rank.tolist() == [0, 0] and pred.tolist() == [0, 0]
    rank, _, pred = softmax_eval(torch.zeros(4, 7680, device=cuda), y, 5, views=2)
    assert rank.tolist() == [0, 0] and pred.tolist() == [0, 0]
