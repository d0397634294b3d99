"""The view-averaging head without a GPU: the host definition (cpu::softmax_topk_views through
anx.ops.softmax_topk_views on CPU tensors) against the fp64 mean of softmaxes (softmax_topk_views_cases.py has the
bound), the slab route against the logits route bit for bit, one view against softmax_topk, the crafted rows, and the
argument errors. The device tests (test_softmax_topk_views_gpu.py) hold the kernel to the same reference."""
import ctypes as C

import pytest
import torch

from anx import _native as nat
from anx.ops import softmax_topk, softmax_topk_views
from softmax_topk_cases import random_rows
from softmax_topk_views_cases import assert_order, assert_views, confident_minority, one_hot_votes, repeated_crafted

K_SIZES = (1, 2, 63, 64, 65, 257, 1000, 1001, 4099, 9000)
V_SIZES = (1, 2, 3, 10, 32)


def bits(t):
    return t.contiguous().view(torch.int32)


@pytest.mark.parametrize("V", V_SIZES)
@pytest.mark.parametrize("K", K_SIZES)
def test_random_rows_against_fp64(K, V):
    for N in (1, 3):
        z = random_rows(N * V, K, seed=1000 * V + K + N)
        for k in sorted({1, min(K, 5), min(K, 16)}):
            idx, prob, probs = softmax_topk_views(z, V, k, return_probs=True)
            assert_views(idx, prob, probs, z, V, k, f"K={K} V={V} N={N} k={k}")
            idx2, prob2 = softmax_topk_views(z, V, k)
            assert torch.equal(idx, idx2) and torch.equal(bits(prob), bits(prob2))


@pytest.mark.parametrize("ksplit", (1, 2, 3, 4))
@pytest.mark.parametrize("with_bias", (True, False))
def test_slabs_equal_logits_bit_for_bit(ksplit, with_bias):
    N, V, K = 3, 4, 257
    M = N * V
    g = torch.Generator().manual_seed(10 + ksplit)
    ws = torch.randn(ksplit, M, K, generator=g) * torch.logspace(-3, 1, ksplit)[:, None, None]  # order matters
    bias = torch.randn(K, generator=g) if with_bias else None
    z = bias.expand(M, K).clone() if with_bias else ws[0].clone()
    for s in range(0 if with_bias else 1, ksplit):
        z = z + ws[s]
    a = softmax_topk_views(None, V, 5, slabs=ws, bias=bias, return_probs=True)
    b = softmax_topk_views(z, V, 5, return_probs=True)
    assert torch.equal(a[0], b[0]) and torch.equal(bits(a[1]), bits(b[1])) and torch.equal(bits(a[2]), bits(b[2]))
    assert_views(*a, z, V, 5, f"ksplit={ksplit} bias={with_bias}")


@pytest.mark.parametrize("K", (1, 2, 65, 1000, 4099))
def test_one_view_has_softmax_topk_probabilities(K):
    """V = 1 divides by 1.0f: the probabilities are softmax_topk's bits. The ORDER is by probability, so it may
    differ from softmax_topk's (by logit) among classes whose probabilities underflow to one value."""
    z = random_rows(6, K, seed=K)
    k = min(K, 16)
    idx1, prob1 = softmax_topk(z, k)
    idx, prob, probs = softmax_topk_views(z, 1, k, return_probs=True)
    assert torch.equal(bits(probs.gather(1, idx1.long())), bits(prob1))
    assert torch.equal(bits(prob), bits(prob1))  # the k best values agree even where their order does not
    assert_views(idx, prob, probs, z, 1, k, f"one view K={K}")


def test_one_view_orders_underflow_ties_by_index():
    z = torch.tensor([[0.0, -300.0, -200.0, 1.0]])  # both small ones underflow to 0: logit order 2, 1; index order 1, 2
    assert softmax_topk(z, 4)[0].tolist() == [[3, 0, 2, 1]]
    assert softmax_topk_views(z, 1, 4)[0].tolist() == [[3, 0, 1, 2]]


def test_crafted_votes():
    z, order = one_hot_votes()
    idx, prob, probs = softmax_topk_views(z, 10, 3, return_probs=True)
    assert_views(idx, prob, probs, z, 10, 3, "one-hot votes")
    want = torch.sort(torch.softmax(z.double(), 1).mean(0), descending=True, stable=True).indices[:3].tolist()
    assert idx[0].tolist() == want == order
    z, order = confident_minority()
    idx, prob, probs = softmax_topk_views(z, 10, 2, return_probs=True)
    assert_views(idx, prob, probs, z, 10, 2, "confident minority")
    want = torch.sort(torch.softmax(z.double(), 1).mean(0), descending=True, stable=True).indices[:2].tolist()
    assert idx[0].tolist() == want == order
    assert (z[:9].argmax(1) == 4).all()  # the majority of the views votes for the loser


@pytest.mark.parametrize("K", (2, 65, 1000))
@pytest.mark.parametrize("V", (1, 3, 10))
def test_crafted_rows_repeated_per_view(K, V):
    rows = repeated_crafted(K, V)
    z = torch.cat(list(rows.values()))
    k = min(K, 16)
    idx, prob, probs = softmax_topk_views(z, V, k, return_probs=True)
    assert_views(idx, prob, probs, z, V, k, f"crafted K={K} V={V}")
    assert idx[list(rows).index("all_equal")].tolist() == list(range(k))


def test_nan_row_still_gives_distinct_indices():
    K, V, k = 100, 3, 16
    z = random_rows(3 * V, K, seed=5)
    z[V + 1, ::7] = float("nan")  # a view of image 1
    idx, prob, probs = softmax_topk_views(z, V, k, return_probs=True)
    got = idx[1].tolist()
    assert len(set(got)) == k and all(0 <= i < K for i in got)
    assert_order(idx, prob, probs, k, "the NaN image and its neighbours")  # also where no bound is defined
    keep = torch.tensor([0, 2])
    rows = torch.cat([torch.arange(V), torch.arange(2 * V, 3 * V)])
    assert_views(idx[keep], prob[keep], probs[keep], z[rows], V, k, "neighbours of the NaN image")


def test_python_argument_checks():
    z = torch.zeros(6, 20)
    for bad in dict(views=0), dict(views=33), dict(views=4), dict(views=None), dict(views=2.0), dict(views=True), \
            dict(views=2, k=0), dict(views=2, k=17), dict(views=2, k=21):
        with pytest.raises(ValueError):
            softmax_topk_views(z, **bad)
    with pytest.raises(ValueError):
        softmax_topk_views(z, 2, 5, slabs=torch.zeros(1, 6, 20))
    with pytest.raises(ValueError):
        softmax_topk_views(z, 2, 5, bias=torch.zeros(20))
    with pytest.raises(ValueError):
        softmax_topk_views(z.double(), 2, 5)
    with pytest.raises(ValueError):
        softmax_topk_views(None, 2, 5, slabs=torch.zeros(2, 5, 20))  # 5 rows, 2 views
    i, p, q = softmax_topk_views(torch.zeros(0, 20), 2, 5, return_probs=True)
    assert tuple(i.shape) == tuple(p.shape) == (0, 5) and tuple(q.shape) == (0, 20)


def test_abi_version_7_and_symbols():
    assert nat.lib().anx_abi_version() >= 7
    for lib, sigs, names in ((nat.lib(), nat._SIGS, ("anx_softmax_topk_views", "anx_cpu_softmax_topk_views")),
                             (nat.bf16(), nat._BF16_SIGS, ("anx_full_run",))):
        for name in names:
            fn = getattr(lib, name)  # AttributeError: the library does not export it
            assert fn.argtypes == sigs[name][1] and fn.restype is sigs[name][0]


def test_rejected_arguments_name_the_function():
    lib = nat.lib()
    z = torch.zeros(6, 20)
    idx = torch.zeros(3, 16, dtype=torch.int32)
    prob = torch.zeros(3, 16)
    ok = dict(src=z.data_ptr(), N=3, V=2, K=20, k=5, idx=idx.data_ptr(), prob=prob.data_ptr())
    cases = {"V = 0": dict(V=0), "V = 33": dict(V=33), "k = 0": dict(k=0), "k = 17": dict(k=17),
             "k > K": dict(K=4, k=5), "null idx": dict(idx=None), "null src": dict(src=None)}
    for what, change in cases.items():
        a = {**ok, **change}
        args = (a["src"], 1, 120, None, a["N"], a["V"], a["K"], a["k"], a["idx"], a["prob"], None, None)
        for name, full in (("anx_cpu_softmax_topk_views", args), ("anx_softmax_topk_views", args + (None,))):
            assert getattr(lib, name)(*full) != 0, (name, what)
            assert name in lib.anx_last_error().decode(), (name, what)
    # more classes than two LDS rows hold: refused by the device entry before anything is launched
    assert lib.anx_softmax_topk_views(z.data_ptr(), 1, 0, None, 3, 2, 7681, 5, idx.data_ptr(), prob.data_ptr(), None,
                                      None, None) != 0
    assert "7680" in lib.anx_last_error().decode()
    assert lib.anx_cpu_softmax_topk_views(ok["src"], 1, 120, None, 3, 2, 20, 5, ok["idx"], ok["prob"], None, None) == 0


def test_null_engine_is_an_error_with_a_message():
    lib = nat.bf16()
    for u8 in (0, 1):  # with views, floats and bytes
        call = nat.FullCallC(rows=10, views=10, k=5, u8=u8)
        assert lib.anx_full_run(None, C.byref(call), None) != 0, u8
        msg = nat.lib().anx_last_error().decode()
        assert "anx_full_run" in msg and "no engine" in msg, (u8, msg)
