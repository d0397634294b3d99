"""Shared by the classifier-head tests (test_softmax_topk_cpu.py, test_softmax_topk_gpu.py): the fp64 reference, the
probability bound, and the rows that exercise the selection rule.

The bound on a returned probability p against p64 = torch.softmax(z.double()) is
    |p - p64| <= p64 * (2 |z - m| + 32) * 2^-24 + 2^-120,   m = max(z):
2 |z - m| * 2^-24 covers the rounding of the difference and of the exponent's argument, which exp carries over one to
one; 32 * 2^-24 the exp, the K-term sum (K <= 2^16) and the division; 2^-120 values that flush to zero."""
import torch

U24 = 2.0 ** -24
K_SIZES = (1, 2, 63, 64, 65, 255, 256, 257, 1000, 1001, 4099)


def reference(z: torch.Tensor, k: int):
    """(indices [M,k] int32, p64 [M,k], slack [M,k]) of fp32 logits z [M,K]: the stable descending sort of the fp64
    values (ties, the -0.0 / +0.0 pair included, go to the lower index) and the fp64 softmax with its allowance."""
    z64 = z.double()
    order = torch.sort(z64, dim=1, descending=True, stable=True).indices[:, :k]
    p64 = torch.softmax(z64, dim=1).gather(1, order)
    dist = (z64.gather(1, order) - z64.amax(dim=1, keepdim=True)).abs()
    rel = torch.where(p64 > 0, p64 * (2.0 * dist + 32.0) * U24, torch.zeros_like(p64))  # 0 * inf under a -inf logit
    return order.to(torch.int32), p64, rel + 2.0 ** -120


def assert_head(idx, prob, z, k, what=""):
    """idx / prob (any device) are the head's answer for the fp32 logits z (any device)."""
    want, p64, slack = reference(z.cpu(), k)
    idx, prob = idx.cpu(), prob.cpu()
    assert idx.dtype == torch.int32 and prob.dtype == torch.float32
    assert tuple(idx.shape) == tuple(prob.shape) == (z.shape[0], k)
    bad = (idx != want).any(dim=1).nonzero().flatten()
    assert bad.numel() == 0, f"{what}: indices differ in rows {bad[:5].tolist()}: {idx[bad[0]].tolist()} != {want[bad[0]].tolist()}"
    err = (prob.double() - p64).abs()
    worst = (err / slack).max().item() if err.numel() else 0.0
    print(f"{what}: worst |p - p64| / bound = {worst:.3f}")
    assert (err <= slack).all(), f"{what}: probability off by {worst:.3f} x the bound"


def random_rows(M: int, K: int, seed: int) -> torch.Tensor:
    """Rows of spread 1, 5 and 30 (cycling), one 1e4 entry in every third row (it overflows without the max
    subtraction), and a few exact ties."""
    g = torch.Generator().manual_seed(seed)
    z = torch.randn(M, K, generator=g) * torch.tensor([1.0, 5.0, 30.0])[torch.arange(M) % 3, None]
    for m in range(0, M, 3):
        z[m, int(torch.randint(K, (1,), generator=g))] = 1e4
    if K >= 4:
        for m in range(1, M, 2):  # two ties with the row's maximum, at random places
            j = torch.randint(K, (2,), generator=g)
            z[m, j] = z[m].max()
    return z


def crafted_rows(K: int) -> dict:
    """Named rows of K logits that go wrong under a sloppy selection rule or softmax."""
    g = torch.Generator().manual_seed(K)
    rows = {"all_equal": torch.full((K,), 0.75), "ramp_up": torch.arange(K, dtype=torch.float32) * 0.01 - 3.0}
    for name, at in (("max_first", 0), ("max_last", K - 1)):
        r = torch.randn(K, generator=g)
        r[at] = 9.0
        rows[name] = r
    r = torch.randn(K, generator=g).clamp(max=2.0)
    for at in (63, 64, 255, 256):  # equal maxima straddling lanes and waves
        if at < K:
            r[at] = 3.5
    rows["equal_maxima"] = r
    r = torch.full((K,), -1.0)
    r[::2] = 0.0
    r[1::4] = -0.0  # -0.0 before and after +0.0 entries: a bit-pattern comparison puts them last
    rows["signed_zeros"] = r
    rows["big_offset"] = 1e4 + torch.randn(K, generator=g)
    r = torch.randn(K, generator=g)
    r[::3] = -1e30
    r[1::5] = float("-inf")
    r[K // 2] = 1.0  # a finite maximum whatever the strides above hit
    rows["minus_inf_entries"] = r
    rows["denormal"] = torch.randn(K, generator=g) * 1e-40
    return rows
