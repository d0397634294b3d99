"""The classifier-head kernel (softmax_topk.hip through anx.ops.softmax_topk on CUDA tensors) against the host
definition (the same op on CPU tensors): indices equal, every probability inside the bound of softmax_topk_cases.py
against the fp64 softmax, the returned logits equal bit for bit. The sizes are the smallest that cross each boundary
of a 64-lane, 256-thread kernel with 16-B loads: K around 64 and 256, K % 4 != 0, several elements per thread
(1000, 4099), more rows than one (3, 257), a row past the LDS budget (20000), split-K slabs with a bias, and a source
that starts 4 bytes off a 16-B boundary."""
import pytest
import torch

from anx.ops import softmax_topk
from softmax_topk_cases import K_SIZES, assert_head, crafted_rows, random_rows

pytestmark = pytest.mark.gpu


def bits(t):
    return t.cpu().contiguous().view(torch.int32)


def same_bits(a, b):
    return a.shape == b.shape and torch.equal(bits(a), bits(b))


def check_against_host(z, k, got, what, host=None):
    """got = (idx, prob[, logits]) from the GPU for the host fp32 logits z; host = the definition's (idx, prob) at
    some k' >= k (its first k columns are its answer for k)."""
    hi = (host or softmax_topk(z, k))[0][:, :k]
    assert torch.equal(got[0].cpu(), hi), f"{what}: indices differ from the host definition"
    assert_head(got[0], got[1], z, k, what)
    if len(got) == 3:
        assert same_bits(got[2], z), f"{what}: returned logits differ"


@pytest.mark.parametrize("K", K_SIZES)
def test_sizes(cuda, K):
    kmax = min(K, 16)
    for M in (1, 3, 257):
        z = random_rows(M, K, seed=1000 * M + K)
        host = softmax_topk(z, kmax)
        zd = z.to(cuda)
        for k in sorted({1, min(K, 5), kmax}):
            check_against_host(z, k, softmax_topk(zd, k, return_logits=True), f"K={K} M={M} k={k}", host)
        check_against_host(z, kmax, softmax_topk(zd, kmax), f"K={K} M={M} no logits", host)


def test_row_past_the_lds_budget(cuda):
    K, M = 20000, 2
    z = random_rows(M, K, seed=5)
    z[1] *= 0.01  # a flat row: thousands of terms carry the sum
    host = softmax_topk(z, 16)
    for k in (1, 5, 16):
        check_against_host(z, k, softmax_topk(z.to(cuda), k, return_logits=True), f"K={K} k={k}", host)
    check_against_host(z, 16, softmax_topk(z.to(cuda), 16), f"K={K} no logits asked", host)
    # scalar loads on the staged path
    z1 = random_rows(M, K + 1, seed=6)
    check_against_host(z1, 16, softmax_topk(z1.to(cuda), 16, return_logits=True), f"K={K + 1}")


@pytest.mark.parametrize("ksplit", (1, 2, 7))
@pytest.mark.parametrize("K", (1000, 1001))
def test_slabs_with_bias(cuda, ksplit, K):
    M = 3
    g = torch.Generator().manual_seed(10 * ksplit + K)
    ws = torch.randn(ksplit, M, K, generator=g) * torch.logspace(-3, 3, ksplit)[:, None, None]
    bias = torch.randn(K, generator=g)
    hi, hp, hz = softmax_topk(None, 5, slabs=ws, bias=bias, return_logits=True)
    gi, gp, gz = softmax_topk(None, 5, slabs=ws.to(cuda), bias=bias.to(cuda), return_logits=True)
    assert same_bits(gz, hz), "reduced logits differ from the host's bias-first, slabs-ascending sum"
    check_against_host(hz, 5, (gi, gp), f"ksplit={ksplit} K={K}", (hi, hp))
    gi2, gp2 = softmax_topk(None, 5, slabs=ws.to(cuda))  # no bias: the sum starts from slab 0
    hi2, hp2, hz2 = softmax_topk(None, 5, slabs=ws, return_logits=True)
    check_against_host(hz2, 5, (gi2, gp2), f"ksplit={ksplit} K={K} no bias", (hi2, hp2))


@pytest.mark.parametrize("K", (1000, 256, 63))
def test_source_four_bytes_off_alignment(cuda, K):
    M = 3
    z = random_rows(M, K, seed=K)
    buf = torch.empty(M * K + 1, device=cuda)
    zs = buf[1:].view(M, K)  # a slice: K % 4 == 0 rows that no 16-B load may touch
    zs.copy_(z)
    assert zs.data_ptr() % 16 == 4 and zs.is_contiguous()
    got = softmax_topk(zs, min(K, 16), return_logits=True)
    check_against_host(z, min(K, 16), got, f"offset K={K}")
    ref = softmax_topk(z.to(cuda), min(K, 16))
    assert torch.equal(got[0], ref[0]) and same_bits(got[1], ref[1]), "the load width changed the answer"


@pytest.mark.parametrize("K", (65, 257, 1000))
def test_crafted_rows(cuda, K):
    rows = crafted_rows(K)
    names = list(rows)
    z = torch.stack(list(rows.values()))
    k = min(K, 16)
    idx, prob, out = softmax_topk(z.to(cuda), k, return_logits=True)
    check_against_host(z, k, (idx, prob, out), f"crafted K={K}")
    idx, prob = idx.cpu(), prob.cpu()
    assert idx[names.index("all_equal")].tolist() == list(range(k))
    assert torch.allclose(prob[names.index("all_equal")].double(), torch.full((k,), 1.0 / K, dtype=torch.float64),
                          rtol=32 * 2.0 ** -24, atol=0)
    assert idx[names.index("max_first"), 0] == 0 and idx[names.index("max_last"), 0] == K - 1
    assert idx[names.index("ramp_up")].tolist() == list(range(K - 1, K - 1 - k, -1))
    if K > 256:
        assert idx[names.index("equal_maxima"), :4].tolist() == [63, 64, 255, 256]
    zero = idx[names.index("signed_zeros")].tolist()
    assert zero == sorted(zero) and zero[:3] == [0, 1, 2]  # +0.0, -0.0, +0.0: by index, not by sign bit


def test_a_rows_answer_depends_only_on_its_bits(cuda):
    K, ksplit = 1000, 7
    g = torch.Generator().manual_seed(77)
    ws = torch.randn(ksplit, 1, K, generator=g)
    bias = torch.randn(K, generator=g)
    i1, p1, z1 = softmax_topk(None, 16, slabs=ws.to(cuda), bias=bias.to(cuda), return_logits=True)
    i2, p2 = softmax_topk(z1, 16)  # the logits those slabs reduce to
    assert torch.equal(i1, i2) and same_bits(p1, p2), "slabs and their logits disagree"
    big = random_rows(257, K, seed=78).to(cuda)
    for at in (0, 5, 256):
        big[at] = z1[0]
    ib, pb = softmax_topk(big, 16)
    for at in (0, 5, 256):
        assert torch.equal(ib[at], i1[0]) and same_bits(pb[at], p1[0]), f"row position {at} changed the answer"
    # and inside a slab launch of many rows
    wsb = torch.randn(ksplit, 257, K, generator=g)
    wsb[:, 100] = ws[:, 0]
    i3, p3 = softmax_topk(None, 16, slabs=wsb.to(cuda), bias=bias.to(cuda))
    assert torch.equal(i3[100], i1[0]) and same_bits(p3[100], p1[0])


@pytest.mark.parametrize("row", ("nan", "all_minus_inf", "plus_inf"))
@pytest.mark.parametrize("K", (100, 1000))
def test_bad_rows_still_give_distinct_indices(cuda, row, K):
    k = 16
    z = random_rows(3, K, seed=3)
    if row == "nan":
        z[1, ::7] = float("nan")
    elif row == "all_minus_inf":
        z[1] = float("-inf")
    else:
        z[1, 40] = float("inf")
    idx, prob = softmax_topk(z.to(cuda), k)
    got = idx[1].tolist()
    assert len(set(got)) == k and all(0 <= i < K for i in got), got
    keep = torch.tensor([0, 2])
    check_against_host(z[keep], k, (idx.cpu()[keep], prob.cpu()[keep]), f"neighbours of the {row} row")


def test_no_rows_and_bad_k(cuda):
    i, p = softmax_topk(torch.zeros(0, 10, device=cuda), 5)
    assert tuple(i.shape) == tuple(p.shape) == (0, 5)
    for bad in (0, 17, 11):
        with pytest.raises(ValueError):
            softmax_topk(torch.zeros(2, 10, device=cuda), bad)
