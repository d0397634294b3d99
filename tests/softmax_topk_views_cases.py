"""Shared by the view-averaging head's tests (test_softmax_topk_views_cpu.py, test_softmax_topk_views_gpu.py): the
fp64 reference, the bound on the mean probability, and the crafted rows.

The reference is pbar64 = softmax(z.double()).view(N, V, K).mean(1). The bound on a returned mean pbar is
    |pbar - pbar64| <= mean_v( p64_v (2 |z - m_v| + 32) ) 2^-24 + (V + 1) 2^-24 pbar64 + 2^-120,   m_v = max of view v:

* every view's fp32 probability p_v carries softmax_topk_cases.py's one-row allowance,
  |p_v - p64_v| <= p64_v (2 |z - m_v| + 32) 2^-24 + 2^-120 (the 32 is that file's: the exponential, the K-term sum
  and the division). The mean passes the V allowances on with weight 1 / V each: their mean, and 2^-120 once.
* the V - 1 fp32 additions each round a partial sum to half an ulp, at most 2^-24 of a value that is at most the
  sum of all V terms, V pbar64 (1 + e) with e the views' own relative error, under 2^-10 wherever p does not
  underflow: (V - 1) 2^-24 V pbar64 (1 + e) on the sum, so (V - 1) 2^-24 pbar64 (1 + e) on the mean.
* the division by float(V) (exact for V <= 2^24) rounds once more: 2^-24 pbar64 (1 + e).
  Together V 2^-24 pbar64 (1 + e); the (V + 1) leaves one 2^-24 pbar64 for the e terms (V e < 32 * 2^-10 < 1).
* a mean in the fp32 subnormal range is off by at most 2^-150 more, far inside the 2^-120.
Nothing here comes from what a kernel returns: the tests print the worst ratio to the bound before they assert."""
import torch

from softmax_topk_cases import crafted_rows

U24 = 2.0 ** -24


def reference(z: torch.Tensor, V: int):
    """(pbar64 [N,K], slack [N,K]) of fp32 logits z [N*V,K]."""
    M, K = z.shape
    z64 = z.double()
    p64 = torch.softmax(z64, dim=1)
    dist = (z64 - z64.amax(dim=1, keepdim=True)).abs()
    one_row = torch.where(p64 > 0, p64 * (2.0 * dist + 32.0) * U24, torch.zeros_like(p64))  # 0 * inf under -inf
    pbar = p64.view(M // V, V, K).mean(1)
    return pbar, one_row.view(M // V, V, K).mean(1) + (V + 1) * U24 * pbar + 2.0 ** -120


def stable_order(probs: torch.Tensor, k: int) -> torch.Tensor:
    """The k best columns of fp32 rows by value descending, equal values to the lower index, a NaN as -inf."""
    key = torch.where(probs != probs, torch.full_like(probs, float("-inf")), probs)
    return torch.sort(key, dim=1, descending=True, stable=True).indices[:, :k].to(torch.int32)


def assert_views(idx, prob, probs, z, V, k, what=""):
    """idx / prob / probs (any device) are the view-averaging head's answer (return_probs) for the fp32 logits z."""
    z, idx, prob, probs = z.cpu(), idx.cpu(), prob.cpu(), probs.cpu()
    N, K = z.shape[0] // V, z.shape[1]
    assert idx.dtype == torch.int32 and prob.dtype == torch.float32 and probs.dtype == torch.float32
    assert tuple(idx.shape) == tuple(prob.shape) == (N, k) and tuple(probs.shape) == (N, K)
    pbar, slack = reference(z, V)
    err = (probs.double() - pbar).abs()
    worst = (err / slack).max().item() if err.numel() else 0.0
    print(f"{what}: worst |pbar - pbar64| / bound = {worst:.3f}")
    assert (err <= slack).all(), f"{what}: mean probability off by {worst:.3f} x the bound"
    assert_order(idx, prob, probs, k, what)


def assert_order(idx, prob, probs, k, what=""):
    """The two checks that need no reference, so they hold for a row with a NaN too: idx is the stable descending
    order of the returned fp32 means (a NaN as -inf), and prob is probs at idx, bit for bit."""
    idx, prob, probs = idx.cpu(), prob.cpu(), probs.cpu()
    want = stable_order(probs, k)
    bad = (idx != want).any(dim=1).nonzero().flatten()
    assert bad.numel() == 0, (f"{what}: indices are not the stable order of the returned means in images "
                              f"{bad[:5].tolist()}: {idx[bad[0]].tolist()} != {want[bad[0]].tolist()}")
    picked = probs.gather(1, idx.long()).contiguous()
    assert torch.equal(prob.contiguous().view(torch.int32), picked.view(torch.int32)), f"{what}: prob is not probs at idx"


def one_hot_votes(K: int = 50, hot: float = 30.0):
    """Ten views of one image, each all but certain of one class: five for class 7, three for 3, two for 11, in
    mixed order. The means are 0.5, 0.3 and 0.2 up to exp(-30) K: apart by far more than any bound above."""
    votes = [7, 3, 7, 11, 7, 3, 7, 11, 3, 7]
    z = torch.zeros(len(votes), K)
    for v, c in enumerate(votes):
        z[v, c] = hot
    return z, [7, 3, 11]


def confident_minority(K: int = 50):
    """Ten views of one image: in nine, class 4 leads with 0.3 before class 9 with 0.25 (the rest shared evenly); the
    tenth is certain of class 9. Class 4 wins nine of ten views, but the means are 0.27 against 0.325: 9 before 4."""
    p = torch.full((K,), 0.45 / (K - 2), dtype=torch.float64)
    p[4], p[9] = 0.3, 0.25
    z = p.log().float().repeat(10, 1)
    z[9] = 0.0
    z[9, 9] = 50.0
    return z, [9, 4]


def repeated_crafted(K: int, V: int) -> dict:
    """The rows of softmax_topk_cases.crafted_rows that stress the softmax itself, each as one image of V equal
    views: the mean of equal rows is that row's softmax again."""
    rows = crafted_rows(K)
    return {name: rows[name].repeat(V, 1) for name in ("all_equal", "minus_inf_entries", "big_offset", "denormal")}
