"""The bf16 full-AlexNet engine against the per-element fp64 oracle of bf16_oracle.py: every layer is fed the
engine's own input tap, and EVERY checked output element must lie inside |got - act(ref)| <= A + U * (|act(ref)| + A),
A = 2e-6 * (sum |x||w| + |b|) (FC8, fp32: |got - ref| <= A). Pools must be bit-exact, pool2 + LRN within
(U + 1e-5) * |ref|, pool1 fused into Conv1 inside [maxpool(lo), maxpool(hi)].

Weights are He-uniform with biases ~ N(0, 0.1^2) that are not bf16-representable (the engine keeps them fp32) and,
in every layer, two channels with a large negative bias that ReLU clips whole. Images are randn * 3. Each case
prints AlexNetFull.last_path() and asserts the route it is there for: the benchmark's batches (one Conv1 workgroup
per image with pool1 in its epilogue, a second FC M tile at 257), the register-staged and LDS-DMA kernels, every
Conv1 segment count, FC8 at class counts that leave the wide-tile and the split-K paths.

Measured on an MI355X, FC8's fp32 logits (the accumulation error alone, no rounding), max |got - ref| / T:
4.9e-8 at N = 257 (wide-tile, K in 8 slices), 7.4e-8 at N = 256 (16 slices), 4.9e-8 at N = 37 (register-staged
and LDS-DMA alike, 16 slices), 2.7e-8 / 4.4e-8 / 4.4e-8 at 10 / 12 / 1000 classes: 27x below C_ACC = 2e-6 and 7x
below the 5e-7 above which the figure would be a finding to explain. The bf16 layers reach 0.97-0.99 of their
bound, which is the rounding term: round-to-nearest-even attains U / (1 + U) of the value."""
import pytest
import torch

from anx.models.alexnet_full import AlexNetFull, init_full_weights
from bf16_oracle import (C_ACC, assert_pool_bracket, assert_within, bf16_bound, conv_ref, f32_bound, fc_ref, lrn_bound,
                         maxpool, worst)

LAYERS = ("conv1", "conv2", "conv3", "conv4", "conv5", "fc6", "fc7", "fc8")
GEMMS = LAYERS[1:]


def oracle_weights(seed, classes=1000, groups2=1):
    w = init_full_weights(seed, classes, groups2)
    g = torch.Generator().manual_seed(1000 + seed)
    for name in LAYERS:
        b = torch.randn(w["b_" + name].shape, generator=g) * 0.1
        b.view(torch.int32).bitwise_or_(1)  # low mantissa bit set: no bias is a bf16 value
        b[1] = -100.0 - 2.0 ** -10  # ReLU clips these channels whole (the second one lies in Conv2's group 1)
        b[-3] = -100.0 - 2.0 ** -10
        assert (b.to(torch.bfloat16).float() != b).all()
        w["b_" + name] = b
    return w


def images(N, seed, cuda):
    return (torch.randn(N, 227, 227, 3, generator=torch.Generator().manual_seed(seed)) * 3).to(cuda)


def run(m, x):
    """Forward -> (logits, the ten bf16 taps, last_path)."""
    N = x.shape[0]
    logits = m(x).clone()
    taps = [m.tap(i, N) for i in range(10)]
    torch.cuda.synchronize()
    return logits, taps, m.last_path()


def check_front(m, x, taps, path, imgs, ratios):
    """Conv1 and pool1 (convolution on images `imgs`, the pool on all)."""
    w = {k: v.to(x.device) for k, v in m.weights.items()}
    idx = torch.tensor(sorted(imgs), device=x.device)
    ref, T = conv_ref(x[idx].to(torch.bfloat16), w["w_conv1"], w["b_conv1"], stride=4)
    want, tol = bf16_bound(ref, T)
    assert (taps[1][:, :2] == 0).all() and (taps[1][:, -2:] == 0).all()
    assert (taps[1][:, :, :2] == 0).all() and (taps[1][:, :, -2:] == 0).all()
    inner = taps[1][:, 2:-2, 2:-2]
    if path["conv1"]["form"] == "ring_f32_pool":  # tap 0 is not written
        ratios["conv1+pool1"] = assert_pool_bracket(inner[idx], want, tol, "conv1+pool1")
    else:
        ratios["conv1"] = assert_within(taps[0][idx], want, tol, "conv1")
        assert torch.equal(inner.float(), maxpool(taps[0].float())), "pool1"


def check_engine(m, x, logits, taps, path, imgs):
    """Every layer of one forward. Convolutions on images `imgs`, pools, LRN and FC6-8 on all.
    -> {layer: max |got - want| / bound}, and FC8's max |got - ref| / T."""
    N = x.shape[0]
    w = {k: v.to(x.device) for k, v in m.weights.items()}
    idx = torch.tensor(sorted(imgs), device=x.device)
    r = {}
    check_front(m, x, taps, path, imgs, r)

    def conv(name, src, got, groups=1):
        ref, T = conv_ref(src[idx], w["w_" + name], w["b_" + name], groups=groups)
        r[name] = assert_within(got[idx], *bf16_bound(ref, T), name)

    conv("conv2", taps[1], taps[2], groups=m.groups2)
    want, tol = lrn_bound(maxpool(taps[2].float()), m.lrn_mode)
    r["pool2+lrn"] = assert_within(taps[3][:, 1:-1, 1:-1], want, tol, "pool2+lrn")
    for t in (3, 4, 5):  # the zero borders of the padded windows
        assert (taps[t][:, 0] == 0).all() and (taps[t][:, -1] == 0).all(), t
        assert (taps[t][:, :, 0] == 0).all() and (taps[t][:, :, -1] == 0).all(), t
    conv("conv3", taps[3], taps[4][:, 1:-1, 1:-1])
    conv("conv4", taps[4], taps[5][:, 1:-1, 1:-1])
    conv("conv5", taps[5], taps[6])
    assert torch.equal(taps[7].float(), maxpool(taps[6].float()).reshape(N, -1)), "pool5"
    for name, src, got in (("fc6", taps[7], taps[8]), ("fc7", taps[8], taps[9])):
        ref, T = fc_ref(src, w["w_" + name], w["b_" + name])
        r[name] = assert_within(got, *bf16_bound(ref, T), name)
    r["fc8"], acc = check_fc8(w, taps[9], logits)
    return r, acc


def check_fc8(w, fc7, logits):
    ref, T = fc_ref(fc7, w["w_fc8"], w["b_fc8"])
    acc = ((logits.double() - ref).abs() / T).max().item()
    print(f"fc8 accumulation: max |got - ref| / T = {acc:.3e} (bound C_ACC = {C_ACC:.0e})")
    return assert_within(logits, *f32_bound(ref, T), "fc8"), acc


def report(case, path, ratios, acc=None):
    print(f"\n[{case}] last_path: {path}")
    print(f"[{case}] max |got - want| / bound: " + ", ".join(f"{k} {v:.3f}" for k, v in ratios.items())
          + (f"; fc8 |got - ref| / T {acc:.3e}" if acc is not None else ""))


def kernels(path, names=GEMMS):
    return [path[n]["kernel"] for n in names]


@pytest.mark.gpu
def test_n257_default_route(cuda):
    """N = 257: the smallest batch with one Conv1 workgroup per image (pool1 in its epilogue, tap 0 not written)
    AND a second 256-row FC M tile, which holds one row (slab stride M * Kg). Default knobs, ungrouped Conv2."""
    N = 257
    m = AlexNetFull(oracle_weights(41), device=cuda, max_batch=N)
    x = images(N, 41, cuda)
    logits, taps, path = run(m, x)
    ratios, acc = check_engine(m, x, logits, taps, path, {0, 1, 127, 128, 255, 256})
    report("a: N=257", path, ratios, acc)
    assert path["conv1"] == {"form": "ring_f32_pool", "segs": 1}
    assert kernels(path) == ["big"] * 7
    assert path["fc6"]["splitk"] > 1 and path["fc7"]["splitk"] > 1
    m.close()


@pytest.mark.gpu
def test_n256_grouped_raw_lrn(cuda):
    """The benchmark's batch with Conv2 in two groups (the bias offset g * Kg of the wide-tile epilogue) and the
    undivided LRN scale."""
    N = 256
    m = AlexNetFull(oracle_weights(42, groups2=2), device=cuda, max_batch=N, groups2=2, lrn_mode="raw")
    x = images(N, 42, cuda)
    logits, taps, path = run(m, x)
    ratios, acc = check_engine(m, x, logits, taps, path, {0, 128, 255})
    report("b: N=256 groups2=2 raw", path, ratios, acc)
    assert path["conv1"] == {"form": "ring_f32_pool", "segs": 1}
    assert kernels(path) == ["big"] * 7
    assert path["fc6"]["splitk"] > 1 and path["fc7"]["splitk"] > 1
    m.close()


@pytest.mark.gpu
def test_n37_register_staged_and_lds_dma_kernels(cuda):
    """The register-staged kernel (the bitwise tests' reference) and the LDS-DMA ring with 2 and 3 slots against
    fp64 themselves, at a batch with partial M tiles everywhere. Layers of fewer than 256 * 128 * 128 outputs
    (conv3-5 here) take the 64x64 register-staged tiles under every bf16_glds."""
    N = 37
    m = AlexNetFull(oracle_weights(43), device=cuda, max_batch=N, knobs={"bf16_glds": 0, "bf16_big": -2})
    x = images(N, 43, cuda)
    for glds in (0, 2, 3):
        m.set_knob("bf16_glds", glds)
        logits, taps, path = run(m, x)
        ratios, acc = check_engine(m, x, logits, taps, path, {0, 18, 36})
        report(f"c: N=37 bf16_glds={glds}", path, ratios, acc)
        assert path["conv1"] == {"form": "ring_f32", "segs": 7}
        assert "big" not in kernels(path)
        if glds == 0:
            assert kernels(path) == ["staged"] * 7
        else:
            for name in ("conv2", "fc6", "fc7", "fc8"):
                assert (path[name]["kernel"], path[name]["id"]) == ("glds", glds), name
        assert path["fc6"]["splitk"] > 1
    m.close()


@pytest.mark.gpu
def test_conv1_every_segment_count(cuda):
    """Conv1's row-band kernel splits an image's 14 row tiles over min(7, ceil(CUs / N)) workgroups, each of which
    re-stages its first rows: 2, 3, 5, 6 and 7 segments (256 CUs) against the oracle on the first, the middle and
    the last image, then 3 segments of the polyphase-input ring. One segment: the N >= 256 cases."""
    m = AlexNetFull(oracle_weights(44), device=cuda, max_batch=128, knobs={"bf16_pool1": 0})
    for N, segs, conv1 in ((128, 2, 2), (86, 3, 2), (52, 5, 2), (43, 6, 2), (40, 7, 2), (1, 7, 2), (86, 3, 1)):
        m.set_knob("bf16_conv1", conv1)
        x = images(N, 100 * conv1 + N, cuda)  # other images every time: a forward that wrote nothing would show
        m(x)
        taps = [m.tap(0, N), m.tap(1, N)]
        torch.cuda.synchronize()
        path = m.last_path()
        ratios = {}
        check_front(m, x, taps, path, {0, N // 2, N - 1}, ratios)
        report(f"d: N={N} bf16_conv1={conv1}", path["conv1"], ratios)
        assert path["conv1"] == {"form": "ring_f32" if conv1 == 2 else "ring", "segs": segs}
    m.close()


@pytest.mark.gpu
@pytest.mark.parametrize("classes", [10, 12, 1000])
def test_fc8_class_counts(cuda, classes):
    """FC8 at class counts that leave the wide-tile path (classes % 8) and split-K with it (classes % 4), with
    biases, against the oracle fed tap 9."""
    N = 5
    m = AlexNetFull(oracle_weights(45, classes=classes), classes=classes, device=cuda, max_batch=N)
    x = images(N, 45, cuda)
    logits, taps, path = run(m, x)
    ratio, acc = check_fc8({k: v.to(cuda) for k, v in m.weights.items()}, taps[9], logits)
    report(f"e: classes={classes}", path["fc8"], {"fc8": ratio}, acc)
    fc8 = path["fc8"]
    if classes == 1000:
        assert fc8["kernel"] == "big"
    elif classes == 12:
        assert fc8["kernel"] in ("glds", "staged") and fc8["splitk"] > 1
    else:
        assert fc8["kernel"] in ("glds", "staged") and fc8["splitk"] == 1
    m.close()


@pytest.mark.gpu
def test_oracle_notices_wrong_biases_through_the_engine(cuda):
    """The control of the cases above: the same check fails an engine whose FC8 bias was rounded to bf16 (what the
    earlier per-layer oracle modelled), and one whose FC7 and Conv3 biases are each channel's neighbour's."""
    N = 5
    good = oracle_weights(46)
    fed = dict(good)
    fed["b_fc8"] = good["b_fc8"].to(torch.bfloat16).float()
    fed["b_fc7"] = good["b_fc7"].roll(1)
    fed["b_conv3"] = good["b_conv3"].roll(1)
    m = AlexNetFull(fed, device=cuda, max_batch=N)
    x = images(N, 46, cuda)
    logits, taps, _ = run(m, x)
    w = {k: v.to(cuda) for k, v in good.items()}
    with pytest.raises(AssertionError, match="fc8"):
        check_fc8(w, taps[9], logits)
    for name, src, got in (("fc7", taps[8], taps[9]), ("conv3", taps[3], taps[4][:, 1:-1, 1:-1])):
        ref, T = (fc_ref if name == "fc7" else conv_ref)(src, w["w_" + name], w["b_" + name])
        assert worst(got, *bf16_bound(ref, T))[0] > 0, name
    check_fc8({k: v.to(cuda) for k, v in fed.items()}, taps[9], logits)  # and passes with the biases the engine had
    m.close()


@pytest.mark.gpu
def test_last_path_of_a_new_engine_is_null(cuda):
    m = AlexNetFull(seed=1, device=cuda, max_batch=1)
    assert m.last_path() == dict.fromkeys(LAYERS)
    m.close()


def test_oracle_weights_have_unrepresentable_and_clipping_biases():
    w = oracle_weights(3, classes=10, groups2=2)
    for name in LAYERS:
        b = w["b_" + name]
        assert (b.to(torch.bfloat16).float() != b).all() and b[1] < -99 and b[-3] < -99
        assert 0.05 < b[(b > -99)].std() < 0.2
    assert worst(torch.zeros(1), torch.zeros(1, dtype=torch.float64), torch.zeros(1, dtype=torch.float64)) == (0, 0.0)
