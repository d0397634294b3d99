"""Shared by the evaluation head's tests (test_softmax_eval_cpu.py, test_softmax_eval_gpu.py): the fp64 reference, the
bounds on the loss, the labels and the crafted rows. Nothing here comes from what a kernel returns: the tests print the
worst ratio of an error to its bound before they assert.

RANK is exact. It is the position of the label y in the stable descending sort (a NaN as -inf, equal values to the
lower index) of the score row the head itself ranks:
* without views the fp32 logits, compared as their fp64 values (softmax_topk_cases.reference's sort);
* with views the fp32 mean row pbar that softmax_topk_views returns with return_probs for the same rows on the same
  device (as softmax_topk_views_cases.assert_order does: the order of fp64 means is not the order of fp32 means).
PRED is the first class of that sort.

LOSS WITHOUT VIEWS. The head computes nll = logf(S) - (z[y] - m) in fp32, m = max(z), S = sum_c expf(z[c] - m). The
reference is nll64 = logsumexp(z64) - z64[y]; write d = z[y] - m <= 0 and L = log(S64) <= ln K, so nll64 = L - d.
Absolute errors, in units of u = 2^-24:
* d = z[y] - m rounds once: |d| u.
* S carries the relative allowance of softmax_topk_cases.py's sum, (32 + ln K) u: 32 u is that file's (the exp, the
  K-term sum, K <= 2^16); the rounding of every exponent's argument z[c] - m is |z[c] - m| u relative on its term, so
  sum_c p_c |z[c] - m| u relative on S. With -ln p_c = |z[c] - m| + L that weight is H(p) - L, the entropy of p less
  L: at most ln K. A relative error e of S is an absolute error e of log S.
* logf is within 2 ulp of its result, a value <= ln K: 2 ulp <= 2 ln K 2^-23 = 4 ln K u.
* the final subtraction rounds once: |nll| u <= (ln K + |d|) u.
Sum: (32 + 6 ln K + 2 |d|) u. The bound the tests hold is
    |nll - nll64| <= (40 + 8 ln max(K, 2) + 2 |d|) 2^-24,
the same terms with the constants rounded up (8 u and 2 ln K u of headroom for the second-order products of the terms
above and for K = 1, where ln K = 0 would leave logf(1) - 0 no room at all). A -inf label logit gives nll64 = +inf:
there nll must be non-finite, and nowhere else.

LOSS WITH VIEWS. nll = -logf(pbar[y]) on the fp32 mean, against nll64 = -log(pbar64[y]):
* pbar[y] is within slack[y] of pbar64[y] (softmax_topk_views_cases.reference), so the logarithm's argument is off by
  slack[y] / pbar64[y] relative; -log turns a relative error e into e + e^2 / 2 + ..., inside 1.01 e for e < 2^-6,
  and slack / pbar64 is below 2^-10 wherever pbar64[y] >= 2^-100 (that file's own remark on e);
* logf is within 2 ulp of a value |nll64|: 4 |nll64| u; the 4 u cover a result near zero (pbar[y] next to 1, where
  the ulp of the argument, not of the result, sets the error: 1 ulp of pbar <= 2 u, twice over).
    |nll - nll64| <= 1.01 slack[y] / pbar64[y] + (4 |nll64| + 4) 2^-24    where pbar64[y] >= 2^-100.
Below 2^-100 the fp32 mean has lost its relative accuracy (or is zero): only nll >= 68 is required (-ln 2^-100 = 69.3;
+inf is allowed).

LABELS. At least half of every case's labels must be held to a bound, or the case checks little: with random labels
the V = 1, K = 1000 case of random_rows leaves 2 of 6 under it (a 1e4 logit pushes every other class below 2^-100).
So even images take the reference's top class as the label and odd images a seeded random class; assert_eval checks
the count."""
import math

import torch

from softmax_topk_cases import crafted_rows
from softmax_topk_views_cases import reference as views_reference

U24 = 2.0 ** -24
NLL_CAP = 1024.0
INT_MIN = -2 ** 31


def score64(z: torch.Tensor, V: int) -> torch.Tensor:
    """The fp64 score row per image of fp32 logits z: the logits (V == 0) or the mean softmax row."""
    return z.double() if V == 0 else views_reference(z, V)[0]


def labels_for(z: torch.Tensor, V: int, seed: int) -> torch.Tensor:
    """int32 [N]: even images the reference's top class (stable: the lowest index among equals), odd images a seeded
    random class."""
    s = score64(z, V)
    s = torch.where(s != s, torch.full_like(s, float("-inf")), s)
    top = torch.sort(s, dim=1, descending=True, stable=True).indices[:, 0]
    g = torch.Generator().manual_seed(seed)
    rnd = torch.randint(s.shape[1], (s.shape[0],), generator=g)
    return torch.where(torch.arange(s.shape[0]) % 2 == 0, top, rnd).to(torch.int32)


def order_of(score: torch.Tensor) -> torch.Tensor:
    """The stable descending order [N,K] of score rows (fp32 or fp64), a NaN as -inf."""
    key = torch.where(score != score, torch.full_like(score, float("-inf")), score)
    return torch.sort(key, dim=1, descending=True, stable=True).indices


def rank_and_pred(score: torch.Tensor, y: torch.Tensor):
    """(rank int32 [N], pred int32 [N]) of the labels y under order_of(score); rank -1 for a label outside the row."""
    K = score.shape[1]
    order = order_of(score)
    valid = (y >= 0) & (y < K)
    pos = (order == y.long().clamp(0, K - 1)[:, None]).int().argmax(dim=1)
    return torch.where(valid, pos, torch.full_like(pos, -1)).to(torch.int32), order[:, 0].to(torch.int32)


def assert_eval(rank, nll, pred, z, y, V, probs=None, what="", min_bounded=0.5):
    """rank / nll / pred (any device) are the evaluation head's answer for the fp32 logits z ([N * max(V, 1), K]) and the
    labels y. With views, probs is the fp32 mean row of softmax_topk_views(return_probs) for the same rows."""
    z, y = z.cpu(), y.cpu()
    rank, nll, pred = rank.cpu(), nll.cpu(), pred.cpu()
    K = z.shape[1]
    N = z.shape[0] // max(V, 1)
    assert rank.dtype == torch.int32 and nll.dtype == torch.float32 and pred.dtype == torch.int32
    assert tuple(rank.shape) == tuple(nll.shape) == tuple(pred.shape) == (N,)
    score = z.double() if V == 0 else probs.cpu()
    want_rank, want_pred = rank_and_pred(score, y)
    assert torch.equal(pred, want_pred), f"{what}: pred {pred.tolist()[:8]} != {want_pred.tolist()[:8]}"
    assert torch.equal(rank, want_rank), f"{what}: rank {rank.tolist()[:8]} != {want_rank.tolist()[:8]}"
    valid = (y >= 0) & (y < K)
    assert (nll[~valid] == 0).all(), f"{what}: an ignored image has a loss"
    if not bool(valid.any()):
        return
    yv = y[valid].long()[:, None]
    got = nll[valid].double()
    if V == 0:
        z64 = z.double()[valid]
        nll64 = torch.logsumexp(z64, dim=1) - z64.gather(1, yv)[:, 0]
        d = (z64.gather(1, yv)[:, 0] - z64.amax(dim=1)).abs()
        bounded = torch.isfinite(nll64)
        bound = (40.0 + 8.0 * math.log(max(K, 2)) + 2.0 * d) * U24
        loose = ~bounded
        assert not torch.isfinite(got[loose]).any(), f"{what}: a -inf label logit must give a non-finite loss"
    else:
        pbar, slack = views_reference(z, V)
        py = pbar[valid].gather(1, yv)[:, 0]
        nll64 = -torch.log(py)
        bounded = py >= 2.0 ** -100
        bound = 1.01 * slack[valid].gather(1, yv)[:, 0] / py + (4.0 * nll64.abs() + 4.0) * U24
        loose = ~bounded
        assert (got[loose] >= 68.0).all(), f"{what}: a label below 2^-100 must give a loss of at least 68"
    assert torch.isfinite(got[bounded]).all(), f"{what}: a non-finite loss where the reference's is finite"
    err = (got[bounded] - nll64[bounded]).abs()
    worst = (err / bound[bounded]).max().item() if err.numel() else 0.0
    print(f"{what}: worst |nll - nll64| / bound = {worst:.3f} ({int(bounded.sum())} of {int(valid.sum())} labels bounded)")
    assert (err <= bound[bounded]).all(), f"{what}: loss off by {worst:.3f} x the bound"
    assert int(bounded.sum()) >= min_bounded * int(valid.sum()), f"{what}: too few labels are held to the bound"


def nll_q32(x: float) -> int:
    """eval_nll_q32 (anx/ops.hpp) in Python integers: x is the exact value of the fp32 loss."""
    c = NLL_CAP if not x < NLL_CAP else max(x, 0.0)
    return int(c * 2.0 ** 32 + 0.5)  # exact in fp64: 24 significant bits below 2^43, and a half


def expected_stats(rank, nll, k: int) -> list:
    """[count, top1, topk, nll_q32] in Python integers from the returned rank and the returned loss's bits."""
    rank, nll = rank.cpu().tolist(), nll.cpu().double().tolist()
    out = [0, 0, 0, 0]
    for r, x in zip(rank, nll):
        if r < 0:
            continue
        out[0] += 1
        out[1] += r == 0
        out[2] += r < k
        out[3] += nll_q32(x)
    return out


def expected_confusion(y, pred, K: int) -> torch.Tensor:
    y, pred = y.cpu().long(), pred.cpu().long()
    valid = (y >= 0) & (y < K)
    return torch.bincount(y[valid] * K + pred[valid], minlength=K * K).view(K, K).to(torch.int32)


def crafted_eval_rows(K: int):
    """(z [R,K], y [R], names): rows of softmax_topk_cases.crafted_rows paired with the labels that go wrong under a
    sloppy rank: ties with the label's value before and after the label's index (all_equal, equal_maxima), signed
    zeros (a bit-pattern comparison splits them), -inf entries as the label (a non-finite loss) and beside it."""
    rows = crafted_rows(K)
    picks = [("all_equal", 0), ("all_equal", K // 2), ("all_equal", K - 1),
             ("ramp_up", 0), ("ramp_up", K - 1), ("max_first", 0), ("max_last", K - 1),
             ("equal_maxima", min(64, K - 1)), ("equal_maxima", min(255, K - 1)), ("equal_maxima", K // 3),
             ("signed_zeros", 0), ("signed_zeros", min(1, K - 1)), ("signed_zeros", min(2, K - 1)),
             ("signed_zeros", min(3, K - 1)), ("big_offset", K // 2),
             ("minus_inf_entries", K // 2), ("minus_inf_entries", min(1, K - 1)), ("minus_inf_entries", min(6, K - 1)),
             ("minus_inf_entries", 0), ("denormal", K // 2), ("denormal", 0)]
    z = torch.stack([rows[name] for name, _ in picks])
    y = torch.tensor([c for _, c in picks], dtype=torch.int32)
    return z, y, [f"{name}@{c}" for name, c in picks]


def special_value_rows(K: int):
    """(z [R,K], y [R]): rows whose softmax is NaN or that hold nothing but ties, each with the labels 0, K // 2 and
    K - 1: a lone +inf at an index > 0, all -inf, a NaN at index 0, all equal. No fp64 bound applies to them; what they
    check is that the evaluation head's first round and count give the order of the other heads' rounds."""
    g = torch.Generator().manual_seed(K)
    lone_inf = torch.randn(K, generator=g)
    lone_inf[K // 2] = float("inf")
    nan_first = torch.randn(K, generator=g)
    nan_first[0] = float("nan")
    rows = [lone_inf, torch.full((K,), float("-inf")), nan_first, torch.full((K,), -2.5)]
    labels = (0, K // 2, K - 1)
    z = torch.stack([r for r in rows for _ in labels])
    return z, torch.tensor([c for _ in rows for c in labels], dtype=torch.int32)


def assert_rank_in_head(rank, pred, y, idx, what=""):
    """pred is the head's first class, and rank the label's position in the head's indices idx [N,k] (with k == K every
    label has one; a label the head did not return must rank at k or later)."""
    rank, pred, y, idx = rank.cpu().tolist(), pred.cpu().tolist(), y.cpu().tolist(), idx.cpu().tolist()
    for i, row in enumerate(idx):
        assert pred[i] == row[0], f"{what}: image {i}: pred {pred[i]} is not the head's first class {row[0]}"
        if y[i] in row:
            assert rank[i] == row.index(y[i]), f"{what}: image {i}: rank {rank[i]}, the head has the label at {row.index(y[i])}"
        else:
            assert rank[i] >= len(row), f"{what}: image {i}: rank {rank[i]} < {len(row)}, but the head did not return the label"
