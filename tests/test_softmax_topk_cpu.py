"""The classifier head without a GPU: the host definition (cpu::softmax_topk through anx.ops.softmax_topk on CPU
tensors) against torch in fp64, the slab order against a torch fp32 loop bit for bit, and the plumbing (C ABI
symbols, argument errors with the function's name, the knob). The device tests (test_softmax_topk_gpu.py) compare
the kernel with this definition."""
import ctypes as C

import pytest
import torch

from anx import _native as nat
from anx.ops import softmax_topk
from anx.utils.tuning import KNOBS, default_knob, knob_value
from softmax_topk_cases import K_SIZES, assert_head, crafted_rows, random_rows, reference

BOUND_SIZES = (1, 2, 63, 64, 65, 257, 1000, 4099)


def test_stable_sort_is_the_tie_rule():
    z = torch.tensor([[1.0, 3.0, 3.0, -0.0, 0.0, 3.0, 2.0]])
    assert torch.sort(z.double(), dim=1, descending=True, stable=True).indices.tolist() == [[1, 2, 5, 6, 0, 3, 4]]
    idx, prob = softmax_topk(z, 7)
    assert idx.tolist() == [[1, 2, 5, 6, 0, 3, 4]]
    assert_head(idx, prob, z, 7, "tie row")


@pytest.mark.parametrize("K", sorted(set(K_SIZES) | set(BOUND_SIZES)))
def test_random_rows_against_fp64(K):
    z = random_rows(7, K, seed=K)
    for k in sorted({1, min(K, 5), min(K, 16)}):
        idx, prob = softmax_topk(z, k)
        assert_head(idx, prob, z, k, f"K={K} k={k}")


@pytest.mark.parametrize("K", (1, 2, 65, 257, 1000))
def test_crafted_rows(K):
    rows = crafted_rows(K)
    z = torch.stack(list(rows.values()))
    k = min(K, 16)
    idx, prob = softmax_topk(z, k)
    assert_head(idx, prob, z, k, f"crafted K={K}")
    names = list(rows)
    assert idx[names.index("all_equal")].tolist() == list(range(k))
    assert torch.allclose(prob[names.index("all_equal")].double(), torch.full((k,), 1.0 / K, dtype=torch.float64),
                          rtol=32 * 2.0 ** -24, atol=0)
    assert idx[names.index("max_first"), 0] == 0 and idx[names.index("max_last"), 0] == K - 1
    if K > 256:
        assert idx[names.index("equal_maxima"), :4].tolist() == [63, 64, 255, 256]


@pytest.mark.parametrize("ksplit", (1, 2, 7))
@pytest.mark.parametrize("with_bias", (True, False))
def test_slab_order_bit_for_bit(ksplit, with_bias):
    M, K = 5, 257
    g = torch.Generator().manual_seed(ksplit)
    ws = torch.randn(ksplit, M, K, generator=g) * torch.logspace(-3, 3, ksplit)[:, None, None]  # order matters
    bias = torch.randn(K, generator=g) if with_bias else None
    v = bias.expand(M, K).clone() if with_bias else ws[0].clone()
    for s in range(0 if with_bias else 1, ksplit):
        v = v + ws[s]
    idx, prob, z = softmax_topk(None, 5, slabs=ws, bias=bias, return_logits=True)
    assert torch.equal(z.view(torch.int32), v.view(torch.int32))
    # the answer depends only on the bits of z
    idx2, prob2 = softmax_topk(v, 5)
    assert torch.equal(idx, idx2) and torch.equal(prob.view(torch.int32), prob2.view(torch.int32))
    assert_head(idx, prob, v, 5, f"ksplit={ksplit}")


def test_logits_pass_through_with_their_bits():
    z = torch.tensor([[-0.0, 0.0, -0.0, 1e-42, float("-inf")]])
    idx, prob, out = softmax_topk(z, 3, return_logits=True)
    assert torch.equal(out.view(torch.int32), z.view(torch.int32))
    assert idx.tolist() == [[3, 0, 1]]  # the denormal, then the zeros of either sign by index


@pytest.mark.parametrize("row", ("nan", "all_minus_inf", "plus_inf"))
def test_bad_rows_still_give_distinct_indices(row):
    K, k = 100, 16
    z = random_rows(3, K, seed=3)
    if row == "nan":
        z[1, ::7] = float("nan")
    elif row == "all_minus_inf":
        z[1] = float("-inf")
    else:
        z[1, 40] = float("inf")
    idx, prob = softmax_topk(z, k)
    got = idx[1].tolist()
    assert len(set(got)) == k and all(0 <= i < K for i in got)
    keep = torch.tensor([0, 2])
    assert_head(idx[keep], prob[keep], z[keep], k, f"neighbours of the {row} row")


def test_python_argument_checks():
    z = torch.zeros(2, 20)
    for bad in (0, 17, 21):
        with pytest.raises(ValueError):
            softmax_topk(z, bad)
    with pytest.raises(ValueError):
        softmax_topk(torch.zeros(2, 3), 4)
    with pytest.raises(ValueError):
        softmax_topk(z, 5, slabs=torch.zeros(1, 2, 20))
    with pytest.raises(ValueError):
        softmax_topk(z.double(), 5)
    i, p = softmax_topk(torch.zeros(0, 20), 5)
    assert tuple(i.shape) == tuple(p.shape) == (0, 5)


# ---- plumbing

def test_abi_version_5():
    assert nat.lib().anx_abi_version() >= 5


def test_symbols_exported_and_declared():
    for lib, sigs, names in ((nat.lib(), nat._SIGS, ("anx_softmax_topk", "anx_cpu_softmax_topk")),
                             (nat.bf16(), nat._BF16_SIGS,
                              ("anx_full_run", "anx_full_last_head"))):
        for name in names:
            assert name in sigs, name
            fn = getattr(lib, name)  # AttributeError: the library does not export it
            assert fn.argtypes == sigs[name][1] and fn.restype is sigs[name][0]


def test_rejected_arguments_name_the_function():
    lib = nat.lib()
    z = torch.zeros(2, 20)
    idx = torch.zeros(2, 16, dtype=torch.int32)
    prob = torch.zeros(2, 16)
    ok = dict(src=z.data_ptr(), ksplit=1, stride=40, bias=None, M=2, K=20, k=5, idx=idx.data_ptr(), prob=prob.data_ptr())
    cases = {"k = 0": dict(k=0), "k = 17": dict(k=17), "k > K": dict(K=4, k=5), "null idx": dict(idx=None),
             "null prob": dict(prob=None), "null src": dict(src=None), "K = 0": dict(K=0, k=1)}
    for what, change in cases.items():
        a = {**ok, **change}
        args = (a["src"], a["ksplit"], a["stride"], a["bias"], a["M"], a["K"], a["k"], a["idx"], a["prob"], None)
        for name, full in (("anx_cpu_softmax_topk", args), ("anx_softmax_topk", args + (None,))):
            assert getattr(lib, name)(*full) != 0, (name, what)
            assert name in lib.anx_last_error().decode(), (name, what)
    assert lib.anx_cpu_softmax_topk(ok["src"], 1, 40, None, 2, 20, 5, ok["idx"], ok["prob"], None) == 0
    assert lib.anx_cpu_softmax_topk(None, 1, 0, None, 0, 20, 5, None, None, None) == 0  # no rows: nothing to do


def test_null_engine_is_an_error_with_a_message():
    lib = nat.bf16()
    buf = C.create_string_buffer(32)
    for name, args in (("anx_full_run", (None, C.byref(nat.FullCallC(rows=1, k=5)), None)),  # with head, floats
                       ("anx_full_run", (None, C.byref(nat.FullCallC(rows=1, k=5, u8=1)), None)),  # with head, bytes
                       ("anx_full_last_head", (None, buf, len(buf)))):
        assert getattr(lib, name)(*args) != 0, name
        msg = nat.lib().anx_last_error().decode()
        assert name in msg and "no engine" in msg, (name, msg)


def test_bf16_head_knob():
    assert "bf16_head" in KNOBS
    assert knob_value("bf16_head", True) == 1 and knob_value("bf16_head", 0) == 0
    with pytest.raises(ValueError):
        knob_value("bf16_head", 2)
    assert default_knob("bf16_head") in (0, 1)


def test_reference_helper_on_a_known_row():
    idx, p64, slack = reference(torch.tensor([[0.0, 1.0, 1.0]]), 2)
    assert idx.tolist() == [[1, 2]] and abs(p64[0, 0].item() - 1.0 / (2.0 + 2.718281828459045 ** -1)) < 1e-15
    assert (slack > 0).all()
