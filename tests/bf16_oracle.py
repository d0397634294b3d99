"""Per-element fp64 oracle of the bf16 full-AlexNet layers (test_bf16_oracle_cpu.py shows on the host that it
passes a correct emulation and fails subtly wrong ones; test_full_alexnet_oracle_gpu.py holds the engine to it).

The model of a layer: inputs and weights are bf16 values, the bias is fp32, products are exact, accumulation is
fp32 in some order, the bias is added in fp32, ReLU, one round-to-nearest-even to bf16 (FC8: no rounding, fp32
out). For an output element, in fp64:

    ref = sum x*w + b        T = sum |x|*|w| + |b|        A = C_ACC * T        U = 2^-8 (bf16 unit roundoff)

    bf16 layers:  |got - act(ref)| <= A + U * (|act(ref)| + A)     (act is 1-Lipschitz, then one rounding)
    FC8:          |got - ref|      <= A

for EVERY element: no share of violations is allowed and no element is left out.

C_ACC = 2e-6: a direct fp32 sum is ~1e-7 of sum |x*w| in this project (test_winograd_numerics_gpu.py); a host
emulation (bf16 operands, fp32 matmul in BLAS order and in 64-wide K tiles, K = 432 .. 9216) has a worst value of
5e-8 * T. 2e-6 is 40x that and 50x below one mean product of FC6 (T / 9216): with one product of K dropped the same
sums violate the bound on 13-21 % of the elements. The constant is not tuned to the GPU.

Pools are exact. Pool1 fused into Conv1 (the 55x55 map never leaves the kernel): max is monotone, so the pooled
value lies in [maxpool(lo), maxpool(hi)] of the unfused per-element bounds. Pool2 + LRN: the max is exact, the LRN
runs in fp32 on v_log / v_exp and rounds once: |got - ref| <= (U + LRN_RTOL) * |ref|, LRN_RTOL = 1e-5 being 10x the
rtol the fp32 suite holds the same instruction sequence to (test_lrn_and_fused_pool_lrn)."""
import torch
import torch.nn.functional as F

C_ACC = 2e-6
U = 2.0 ** -8
LRN_RTOL = 1e-5


def nchw(t):
    return t.permute(0, 3, 1, 2)


def nhwc(t):
    return t.permute(0, 2, 3, 1)


def quant(t):
    """Round to bf16 (nearest even), as fp64."""
    return t.to(torch.bfloat16).double()


def conv_ref(x, w, b, stride=1, groups=1):
    """x: NHWC of bf16 values, padding already in it; w: KCFF fp32 (rounded to bf16 here); b: fp32.
    -> (ref, T), NHWC fp64."""
    xd, wq, bd = nchw(x.double()), quant(w), b.double()
    ref = F.conv2d(xd, wq, bd, stride=stride, groups=groups)
    T = F.conv2d(xd.abs(), wq.abs(), bd.abs(), stride=stride, groups=groups)
    return nhwc(ref), nhwc(T)


def fc_ref(x, w, b):
    """x: [M, K] of bf16 values; w: [out, K] fp32 (rounded to bf16 here); b: fp32. -> (ref, T), [M, out] fp64."""
    xd, wq, bd = x.double(), quant(w), b.double()
    return xd @ wq.T + bd, xd.abs() @ wq.abs().T + bd.abs()


def bf16_bound(ref, T, relu=True):
    """(want, tol) of a layer that stores bf16."""
    want = F.relu(ref) if relu else ref
    A = C_ACC * T
    return want, A + U * (want.abs() + A)


def f32_bound(ref, T):
    """(want, tol) of FC8: fp32 out, no rounding."""
    return ref, C_ACC * T


def worst(got, want, tol):
    """(number of elements outside the bound, max |got - want| / tol). Where tol is 0 (an all-zero sum) any
    difference counts as infinite."""
    err = (got.double() - want).abs()
    ratio = torch.where(err > 0, err / tol, torch.zeros_like(err))
    return int((err > tol).sum().item()), float(ratio.max().item())


def assert_within(got, want, tol, what):
    """Every element inside its bound; returns max |got - want| / tol."""
    assert got.shape == want.shape, (what, tuple(got.shape), tuple(want.shape))
    bad, ratio = worst(got, want, tol)
    if bad:
        err = (got.double() - want).abs()
        idx = torch.nonzero(err > tol)[:8].tolist()
        raise AssertionError(f"{what}: {bad} of {err.numel()} elements outside the bound, worst {ratio:.3g} x; "
                             f"first at {idx}")
    return ratio


def maxpool(x, f=3, s=2):
    """NHWC max pool (exact in every float type)."""
    return nhwc(F.max_pool2d(nchw(x), f, s))


def assert_pool_bracket(got, want, tol, what):
    """Pool fused behind a bf16 layer whose map is not stored: got in [maxpool(want - tol), maxpool(want + tol)].
    Returns the worst distance from the bracket's middle in half-widths (<= 1 inside)."""
    lo, hi = maxpool(want - tol), maxpool(want + tol)
    g = got.double()
    assert g.shape == lo.shape, (what, tuple(g.shape), tuple(lo.shape))
    out = (g < lo) | (g > hi)
    if out.any():
        raise AssertionError(f"{what}: {int(out.sum())} of {g.numel()} pooled elements outside the bracket; "
                             f"first at {torch.nonzero(out)[:8].tolist()}")
    mid, half = (hi + lo) / 2, (hi - lo) / 2
    d = (g - mid).abs()
    return float(torch.where(d > 0, d / half, torch.zeros_like(d)).max().item())


def lrn_bound(pooled, mode="div_n", size=5, alpha=1e-4, beta=0.75, k=2.0):
    """pooled: NHWC bf16 values (the exact max pool of conv2). -> (want, tol) of the stored bf16 LRN output.
    div_n: x / (k + alpha / size * sum x^2)^beta; raw: alpha undivided."""
    x = nchw(pooled.double())
    a = alpha if mode == "div_n" else alpha * size  # local_response_norm divides alpha by size itself
    want = nhwc(F.local_response_norm(x, size, alpha=a, beta=beta, k=k))
    return want, (U + LRN_RTOL) * want.abs()
