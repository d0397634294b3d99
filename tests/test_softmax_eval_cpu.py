"""The evaluation head without a GPU: the host definition (cpu::softmax_eval through anx.ops.softmax_eval on CPU
tensors) against softmax_eval_cases.py's fp64 reference and bounds, slabs against logits bit for bit, ignored labels,
the counters against an exact recomputation in Python integers, and the plumbing: the C ABI's symbols and every
refusal of anx_full_run that the evaluation head adds (they need no engine, so a null one reaches them)."""
import ctypes as C

import pytest
import torch

from anx import _native as nat
from anx.ops import eval_summary, softmax_eval, softmax_topk, softmax_topk_views
from softmax_eval_cases import (INT_MIN, assert_eval, assert_rank_in_head, crafted_eval_rows, expected_confusion,
                                expected_stats, labels_for, nll_q32, special_value_rows)
from softmax_topk_cases import K_SIZES, random_rows

V_SIZES = (None, 1, 2, 10, 32)


def bits(t):
    return t.contiguous().view(torch.int32)


def probs_of(z, V):
    return softmax_topk_views(z, V, 1, return_probs=True)[2] if V else None


@pytest.mark.parametrize("V", V_SIZES, ids=lambda v: f"V{v}")
@pytest.mark.parametrize("K", K_SIZES)
def test_random_rows_against_fp64(K, V):
    N, v = 6, V or 0
    z = random_rows(N * max(v, 1), K, seed=3000 * v + K)
    y = labels_for(z, v, seed=K + v)
    rank, nll, pred = softmax_eval(z, y, min(K, 5), views=V)
    assert_eval(rank, nll, pred, z, y, v, probs_of(z, V), f"K={K} V={V}")
    if V is None:  # the same first class and the same order as the head of the same rows
        idx, _ = softmax_topk(z, min(K, 16))
    else:
        idx, _ = softmax_topk_views(z, V, min(K, 16))
    assert torch.equal(pred, idx[:, 0])
    for i in range(N):
        r = int(rank[i])
        assert (int(idx[i, r]) == int(y[i])) if r < idx.shape[1] else (int(y[i]) not in idx[i].tolist())


@pytest.mark.parametrize("V", (None, 1, 3), ids=lambda v: f"V{v}")
@pytest.mark.parametrize("K", (1, 2, 5, 65, 257, 1000))
def test_crafted_rows(K, V):
    z1, y, names = crafted_eval_rows(K)
    v = V or 0
    z = z1.repeat_interleave(max(v, 1), dim=0)  # with views: every image V equal views, the mean is the row's softmax
    rank, nll, pred = softmax_eval(z, y, 1, views=V)
    assert_eval(rank, nll, pred, z, y, v, probs_of(z, V), f"crafted K={K} V={V}")
    at = {n: i for i, n in enumerate(names)}
    assert rank[at[f"all_equal@{K // 2}"]] == K // 2 and rank[at[f"all_equal@{K - 1}"]] == K - 1  # ties before the label
    assert rank[at["all_equal@0"]] == 0 and pred[at["all_equal@0"]] == 0                          # ties after it
    if V is None:
        if K > 256:
            assert rank[at["equal_maxima@64"]] == 1 and rank[at["equal_maxima@255"]] == 2
        if K >= 4:  # [0, -0, 0, -1, ...]: the zeros of either sign tie and go by index
            assert [int(rank[at[f"signed_zeros@{c}"]]) for c in (0, 1, 2)] == [0, 1, 2]
            assert not torch.isfinite(nll[at["minus_inf_entries@1"]]) and nll[at["minus_inf_entries@1"]] > 0
            assert torch.isfinite(nll[at["minus_inf_entries@0"]])  # -1e30: far down, but finite
    z1, y = special_value_rows(K)  # the first round on +inf, -inf, NaN and ties: the other heads' order
    z = z1.repeat_interleave(max(v, 1), dim=0)
    rank, _, pred = softmax_eval(z, y, 1, views=V)
    idx = softmax_topk(z, min(K, 16))[0] if V is None else softmax_topk_views(z, V, min(K, 16))[0]
    assert_rank_in_head(rank, pred, y, idx, f"special values K={K} V={V}")
    if V is None:  # by logit: the lone +inf at K // 2 wins, a row of -inf goes by index
        assert pred.tolist()[:6] == [K // 2] * 3 + [0] * 3


@pytest.mark.parametrize("V", (None, 2), ids=lambda v: f"V{v}")
@pytest.mark.parametrize("ksplit", (1, 3))
@pytest.mark.parametrize("with_bias", (True, False))
def test_slabs_equal_logits_bit_for_bit(ksplit, with_bias, V):
    N, K = 5, 257
    M = N * (V or 1)
    g = torch.Generator().manual_seed(ksplit)
    ws = torch.randn(ksplit, M, K, generator=g) * torch.logspace(-3, 3, ksplit)[:, None, None]  # order matters
    bias = torch.randn(K, generator=g) if with_bias else None
    v = bias.expand(M, K).clone() if with_bias else ws[0].clone()
    for s in range(0 if with_bias else 1, ksplit):
        v = v + ws[s]
    y = labels_for(v, V or 0, seed=ksplit)
    a = softmax_eval(None, y, 5, views=V, slabs=ws, bias=bias, return_logits=True)
    b = softmax_eval(v, y, 5, views=V, return_logits=True)
    assert torch.equal(bits(a[3]), bits(v)) and torch.equal(bits(b[3]), bits(v))
    for p, q in zip(a[:3], b[:3]):
        assert torch.equal(bits(p), bits(q))
    assert_eval(*a[:3], v, y, V or 0, probs_of(v, V), f"ksplit={ksplit} bias={with_bias} V={V}")


@pytest.mark.parametrize("V", (None, 2), ids=lambda v: f"V{v}")
def test_ignored_labels_count_nothing(V):
    K, N = 20, 6
    z = random_rows(N * (V or 1), K, seed=7)
    y = labels_for(z, V or 0, seed=1)
    y[1], y[2], y[4] = -1, K, INT_MIN
    stats = torch.zeros(4, dtype=torch.int64)
    conf = torch.zeros(K, K, dtype=torch.int32)
    rank, nll, pred = softmax_eval(z, y, 5, views=V, stats=stats, confusion=conf)
    assert_eval(rank, nll, pred, z, y, V or 0, probs_of(z, V), f"ignored V={V}")
    assert rank[[1, 2, 4]].tolist() == [-1, -1, -1] and nll[[1, 2, 4]].tolist() == [0.0, 0.0, 0.0]
    idx = softmax_topk(z, 1)[0] if V is None else softmax_topk_views(z, V, 1)[0]
    assert torch.equal(pred, idx[:, 0])  # the argmax is still written
    assert stats[0] == 3 and int(conf.sum()) == 3
    all_ignored = torch.full((N,), -1, dtype=torch.int32)
    before = (stats.clone(), conf.clone())
    rank, nll, _ = softmax_eval(z, all_ignored, 5, views=V, stats=stats, confusion=conf)
    assert (rank == -1).all() and (nll == 0).all()
    assert torch.equal(stats, before[0]) and torch.equal(conf, before[1])


@pytest.mark.parametrize("V", (None, 10), ids=lambda v: f"V{v}")
def test_stats_and_confusion_are_exact_and_accumulate(V):
    K, N, k = 37, 9, 5
    stats = torch.zeros(4, dtype=torch.int64)
    conf = torch.zeros(K, K, dtype=torch.int32)
    want, want_conf = [0, 0, 0, 0], torch.zeros(K, K, dtype=torch.int32)
    for call in range(2):
        z = random_rows(N * (V or 1), K, seed=50 + call)
        y = labels_for(z, V or 0, seed=call)
        y[3] = -1
        rank, nll, pred = softmax_eval(z, y, k, views=V, stats=stats, confusion=conf)
        want = [a + b for a, b in zip(want, expected_stats(rank, nll, k))]
        want_conf += expected_confusion(y, pred, K)
        assert stats.tolist() == want, f"call {call}"
        assert torch.equal(conf, want_conf), f"call {call}"
    assert want[0] == 16 and want[1] >= 8  # the even images are labelled with the top class
    s = eval_summary(stats, k)
    assert s["count"] == 16 and s["k"] == k and s["top1_error"] == 1.0 - want[1] / 16
    assert s["topk_error"] == 1.0 - want[2] / 16 and s["loss"] == want[3] / 2.0 ** 32 / 16


def test_loss_fixed_point():
    assert nll_q32(0.0) == 0 and nll_q32(1.0) == 2 ** 32 and nll_q32(float("inf")) == 2 ** 42
    assert nll_q32(float("nan")) == 2 ** 42 and nll_q32(2000.0) == 2 ** 42 and nll_q32(-1e-8) == 0
    # a -inf label logit counts as the cap; the counters take it
    z = torch.tensor([[0.0, float("-inf"), 1.0]])
    stats = torch.zeros(4, dtype=torch.int64)
    rank, nll, _ = softmax_eval(z, torch.tensor([1], dtype=torch.int32), 1, stats=stats)
    assert nll[0] == float("inf") and rank[0] == 2 and stats.tolist() == [1, 0, 0, 2 ** 42]
    assert eval_summary(stats, 1)["loss"] == 1024.0
    assert all(v != v for v in (eval_summary(torch.zeros(4, dtype=torch.int64), 5)[n] for n in ("loss", "top1_error")))


def test_python_argument_checks():
    z = torch.zeros(4, 20)
    y = torch.zeros(4, dtype=torch.int32)
    for bad_k in (0, 17, 21):
        with pytest.raises(ValueError):
            softmax_eval(z, y, bad_k)
    bad = [dict(labels=None), dict(labels=y.long()), dict(labels=y[:3]), dict(labels=torch.zeros(8, dtype=torch.int32)[::2]),
           dict(views=0), dict(views=3), dict(views=33), dict(views=True), dict(stats=torch.zeros(4, dtype=torch.int32)),
           dict(stats=torch.zeros(5, dtype=torch.int64)), dict(confusion=torch.zeros(20, 20, dtype=torch.int64)),
           dict(confusion=torch.zeros(20, 19, dtype=torch.int32)), dict(out=(y, y)),
           dict(out=(y.clone(), torch.zeros(4, dtype=torch.float64), y.clone())),
           dict(out=(torch.zeros(5, dtype=torch.int32), torch.zeros(4), y.clone()))]
    for change in bad:
        with pytest.raises(ValueError):
            softmax_eval(**{**dict(logits=z, labels=y, k=5), **change})
    with pytest.raises(ValueError):
        softmax_eval(z, y, 5, views=2)  # labels are per image: 2 images of 2 views take 2
    with pytest.raises(ValueError):
        softmax_eval(z, y, 5, slabs=torch.zeros(1, 4, 20))
    out = (torch.full((4,), 9, dtype=torch.int32), torch.full((4,), 9.0), torch.full((4,), 9, dtype=torch.int32))
    got = softmax_eval(z, y, 5, out=out)
    assert all(a is b for a, b in zip(got, out)) and got[0].tolist() == [0] * 4 and got[2].tolist() == [0] * 4
    r, n, p = softmax_eval(torch.zeros(0, 20), torch.zeros(0, dtype=torch.int32), 5)
    assert tuple(r.shape) == tuple(n.shape) == tuple(p.shape) == (0,)
    with pytest.raises(ValueError):
        eval_summary(torch.zeros(4, dtype=torch.int32), 5)


# ---- plumbing

def test_abi_version_9():
    assert nat.lib().anx_abi_version() >= 9


def test_symbols_exported_and_declared():
    lib = nat.lib()
    for name in ("anx_softmax_eval", "anx_cpu_softmax_eval"):
        assert name in nat._SIGS, name
        fn = getattr(lib, name)  # AttributeError: the library does not export it
        assert fn.argtypes == nat._SIGS[name][1] and fn.restype is nat._SIGS[name][0]
    names = [f[0] for f in nat.FullCallC._fields_]
    assert names[-6:] == ["labels", "rank", "nll", "pred", "stats", "confusion"]
    blank = nat.FullCallC(rows=1)
    assert all(getattr(blank, n) is None for n in names[-6:])  # the new fields default to null


def test_rejected_arguments_name_the_function():
    lib = nat.lib()
    z = torch.zeros(2, 20)
    y = torch.zeros(2, dtype=torch.int32)
    ok = dict(src=z.data_ptr(), ksplit=1, N=2, V=0, K=20, k=5, labels=y.data_ptr())
    cases = {"k = 0": dict(k=0), "k = 17": dict(k=17), "k > K": dict(K=4, k=5), "null labels": dict(labels=None),
             "null src": dict(src=None), "K = 0": dict(K=0, k=1), "V = -1": dict(V=-1), "V = 33": dict(V=33),
             "ksplit = 0": dict(ksplit=0), "N = -1": dict(N=-1)}
    for what, change in cases.items():
        a = {**ok, **change}
        args = (a["src"], a["ksplit"], 40, None, a["N"], a["V"], a["K"], a["k"], a["labels"], None, None, None, None, None,
                None)
        for name, full in (("anx_cpu_softmax_eval", args), ("anx_softmax_eval", args + (None,))):
            assert getattr(lib, name)(*full) != 0, (name, what)
            assert name in lib.anx_last_error().decode(), (name, what)
    # the device limits are refused before anything is launched (no GPU here: a launch would fail differently)
    for V, K in ((0, 15361), (2, 7681)):
        assert lib.anx_softmax_eval(ok["src"], 1, 0, None, 2, V, K, 5, ok["labels"], None, None, None, None, None, None,
                                    None) != 0
        assert "classes" in lib.anx_last_error().decode()
    assert lib.anx_cpu_softmax_eval(ok["src"], 1, 40, None, 2, 0, 20, 5, ok["labels"], None, None, None, None, None, None) == 0
    assert lib.anx_cpu_softmax_eval(None, 1, 0, None, 0, 0, 20, 5, None, None, None, None, None, None, None) == 0  # no rows


def test_full_run_refusals_of_the_evaluation_head():
    """What the evaluation head's fields rule out among themselves is refused before the engine is looked at, so a null
    engine reaches every reason; a well-formed evaluation call then gets as far as "no engine"."""
    lib, err = nat.bf16(), lambda: nat.lib().anx_last_error().decode()
    p = C.addressof(C.create_string_buffer(64))  # any non-null address: nothing dereferences it
    ev = dict(rows=1, k=5, labels=p, rank=p)
    cases = (("idx with labels", {**ev, "idx": p}, "one head"),
             ("prob with labels", {**ev, "prob": p}, "one head"),
             ("idx and prob with labels", {**ev, "idx": p, "prob": p}, "one head"),
             ("labels with no output", dict(rows=1, k=5, labels=p), "no output (rank, nll, pred, stats, confusion)"),
             ("k = 0", {**ev, "k": 0}, "k > 0"),
             *((f"{name} without labels", {"rows": 1, "k": 5, name: p}, "go with labels")
               for name in ("rank", "nll", "pred", "stats", "confusion")))
    for what, fields, reason in cases:
        assert lib.anx_full_run(None, C.byref(nat.FullCallC(**fields)), None) != 0, what
        assert err().startswith("anx_full_run: ") and reason in err() and "no engine" not in err(), (what, err())
    for name in ("rank", "nll", "pred", "stats", "confusion"):  # each output alone makes the call well-formed
        assert lib.anx_full_run(None, C.byref(nat.FullCallC(rows=1, k=5, labels=p, **{name: p})), None) != 0
        assert "no engine" in err(), (name, err())
    for delta in (-8, 8):  # the size check stays exact, and comes first
        c = nat.FullCallC(**ev)
        c.size = C.sizeof(nat.FullCallC) + delta
        assert lib.anx_full_run(None, C.byref(c), None) != 0
        assert "size" in err() and "no engine" not in err(), err()
    assert C.sizeof(nat.FullCallC) == 112
    # a call without the new fields is refused as it was
    assert lib.anx_full_run(None, C.byref(nat.FullCallC(rows=1, k=5)), None) != 0
    assert "no engine" in err()
