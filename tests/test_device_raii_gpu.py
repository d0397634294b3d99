"""Lifetimes of the device owners (csrc/include/anx/device.hpp) seen through anx_device_live: every engine and
runtime returns the process to the counters it found, whether it is closed after use or its constructor (or a
forward) fails half way at any one of its device allocations.

The failures come from anx_device_fail_alloc: the armed allocation returns hipErrorOutOfMemory without calling
HIP, so no device error is involved and nothing is launched with a bad pointer. ``live`` is the first three
counters (buffers, bytes, streams + events) after a device synchronisation; torch's own allocator does not go
through them, so tensors may stay alive across the reads.
"""
import ctypes as C

import pytest
import torch

from anx import _native as nat
from anx.models.alexnet_blocks import AlexNetBlocks
from anx.models.alexnet_full import AlexNetFull, init_full_weights

pytestmark = pytest.mark.gpu

H = W = 35  # the smallest size of tests/geometry_cases.py


def counters():
    torch.cuda.synchronize()
    out = (C.c_size_t * 4)()
    nat.call("anx_device_live", out)
    return tuple(out)


def live():
    return counters()[:3]


def arm(k):
    nat.call("anx_device_fail_alloc", k)


@pytest.fixture(autouse=True)
def disarmed():
    arm(0)
    yield
    arm(0)


def blocks_model():
    return AlexNetBlocks(init="rand", seed=3, device="cuda", H=H, W=W, max_batch=16)


def images(n, seed):
    g = torch.Generator().manual_seed(seed)
    return torch.randint(0, 256, (n, H, W, 3), dtype=torch.uint8, generator=g).cuda()


@pytest.fixture(scope="module")
def full_weights():
    return init_full_weights(5, 10)


def full_model(w):
    return AlexNetFull(w, classes=10, max_batch=2, device=torch.device("cuda", 0))


def full_images(n, seed):
    g = torch.Generator().manual_seed(seed)
    return torch.randint(0, 256, (n, 227, 227, 3), dtype=torch.uint8, generator=g).cuda()


def sweep(build, base):
    """Every allocation of one successful build() fails once: each time build() raises through the C ABI's status
    code and the counters are back at ``base``. Returns the number of allocations."""
    before = counters()[3]
    m = build()
    K = counters()[3] - before
    m.close()
    assert K > 0 and live() == base
    for k in range(1, K + 1):
        arm(k)
        with pytest.raises(nat.NativeError):
            build()
        arm(0)
        assert live() == base, k
    return K


def test_blocks_engine_lifetime(cuda):
    base = live()
    m = blocks_model()
    assert all(a > b for a, b in zip(live()[:2], base[:2]))  # buffers and bytes; the engine owns no stream
    xb = images(16, 1)
    m(m.decode_u8(xb))                 # both Winograd paths
    m(xb)                              # the decode workspace
    during = live()
    m.set_knob("conv2_tile", 3)        # transformed weights and workspace replaced
    m.set_knob("conv2_algo", "direct")
    m(m.decode_u8(xb))                 # the direct path's pack
    m(m.decode_u8(xb[:2]))             # another pack variant
    assert all(a > b for a, b in zip(during[:2], base[:2])) and all(a > b for a, b in zip(live()[:2], base[:2]))
    m.close()
    assert live() == base


def test_full_engine_lifetime(cuda, full_weights):
    base = live()
    m = full_model(full_weights)
    assert all(a > b for a, b in zip(live()[:2], base[:2]))
    xb = full_images(3, 2)
    m(m.decode_u8(xb[:2]))
    m.set_knob("bf16_u8", 0)
    m(xb[:2])                          # the decode workspace
    assert m.last_input() == "u8_decode"
    m(m.decode_u8(xb))                 # 3 images: the engine is rebuilt for the larger batch
    assert all(a > b for a, b in zip(live()[:2], base[:2]))
    m.close()
    assert live() == base


def test_blocks_constructor_failure_sweep(cuda):
    base = live()
    x = images(16, 3)
    m = blocks_model()
    want = m(m.decode_u8(x)).clone()
    m.close()
    sweep(blocks_model, base)
    m = blocks_model()
    got = m(m.decode_u8(x))
    assert torch.equal(got, want)
    m.close()
    assert live() == base


def test_full_constructor_failure_sweep(cuda, full_weights):
    base = live()
    x = full_images(2, 4)
    m = full_model(full_weights)
    want = m(m.decode_u8(x)).clone()
    m.close()
    sweep(lambda: full_model(full_weights), base)
    m = full_model(full_weights)
    assert torch.equal(m(m.decode_u8(x)), want)
    m.close()
    assert live() == base


def test_blocks_failure_inside_forward(cuda):
    base = live()
    m = blocks_model()
    m(m.decode_u8(images(16, 5)))
    xb = images(2, 6)
    before = live()
    arm(1)  # the first allocation inside the call: the decode workspace (or a re-pack)
    with pytest.raises(nat.NativeError):
        m(xb)
    arm(0)
    assert live() == before
    y = m(xb).clone()
    assert torch.equal(y, m(m.decode_u8(xb)))
    m.close()
    assert live() == base


@pytest.mark.parametrize("k", [1, 2])  # the two allocations of Conv2's first pack
def test_full_failure_inside_forward(cuda, full_weights, k):
    base = live()
    x = full_images(2, 7)
    ref = full_model(full_weights)
    xf = ref.decode_u8(x)
    want = ref(xf).clone()
    ref.close()
    m = full_model(full_weights)
    before = live()
    arm(k)
    with pytest.raises(nat.NativeError):
        m(xf)
    arm(0)
    assert live() == before  # the layer kept what it had: nothing
    assert torch.equal(m(xf), want)
    m.close()
    assert live() == base


def _one_rank_env(monkeypatch):
    for k, v in (("RANK", "0"), ("WORLD_SIZE", "1"), ("LOCAL_RANK", "0"), ("LOCAL_WORLD_SIZE", "1")):
        monkeypatch.setenv(k, v)


def _runtime(kind, weights):
    from anx.config import blocks
    from anx.parallel.workloads import NativeV4, NativeV5
    kw = {"pipeline": 1, "poison": True} if kind == "v5" else {}
    return (NativeV5 if kind == "v5" else NativeV4)(6, weights, specs=blocks("raw", 1), timeout_s=60, **kw)


@pytest.mark.parametrize("kind", ["v5", "v4"])
def test_runtime_lifetime_one_rank(cuda, monkeypatch, kind):
    from anx.utils.init import init_input
    _one_rank_env(monkeypatch)
    w = AlexNetBlocks(init="rand", seed=9, device="cpu", lrn_mode="raw").weights
    base = live()
    rt = _runtime(kind, w)
    assert all(a > b for a, b in zip(live(), base))  # buffers, bytes, and its streams and events
    rt.fill(init_input(6, "rand", seed=9))
    rt.step()
    rt.sync()
    rt.close()
    assert live() == base


def test_v5_constructor_failure_sweep_one_rank(cuda, monkeypatch):
    _one_rank_env(monkeypatch)
    w = AlexNetBlocks(init="rand", seed=9, device="cpu", lrn_mode="raw").weights
    base = live()
    sweep(lambda: _runtime("v5", w), base)
    assert live() == base
