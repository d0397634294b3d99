"""The fp32 engine at image sizes other than 227x227, default knobs (the production kernel selection).

The fused chain (one-kernel Conv1 with pool1 in its epilogue -> merged Conv2 input transform -> F(4x4,5x5) GEMM
with pool2 in its epilogue -> LRN merge) hands partial maxima between kernels through side buffers, indexed by
the image's tile grids. The sizes of geometry_cases.py walk those grids: Conv1 tile remainders, even maps (a
pool drops the last row / column), Conv2 4x4 tile remainders, grids where one workgroup spans several images,
and both sides of every eligibility limit. Every case asserts AlexNetBlocks.last_path(), so none can pass on a
fallback it did not name."""
import math

import pytest
import torch

from anx.models.alexnet_blocks import AlexNetBlocks
from anx.models.reference import blocks_forward_all
from anx.parallel.plan import OVERLAP, make_plan
from anx.utils.init import init_input

from geometry_cases import FALLBACK_SIZES, FULL, FUSED_SIZES, MIDDLE, N_SMALL, N_SWEEP, SMALL_SIZES, UNFUSED

pytestmark = pytest.mark.gpu

# what an engine with one fusion knob off launches, by what the default knobs launch there
VARIANTS = {
    "conv1_pool": {"FULL": MIDDLE, "MIDDLE": MIDDLE, "UNFUSED": UNFUSED},  # pool2's epilogue runs behind pool1's only
    "conv2_pool": {"FULL": {**FULL, "pool2": "kernel"}, "MIDDLE": MIDDLE, "UNFUSED": UNFUSED},
    "fuse_pool1": {"FULL": UNFUSED, "MIDDLE": UNFUSED, "UNFUSED": UNFUSED},
}
PATHS = {"FULL": FULL, "MIDDLE": MIDDLE, "UNFUSED": UNFUSED}
NAME_OF = lambda path: next(k for k, v in PATHS.items() if v == path)  # noqa: E731

CASES = ([(hw, N_SWEEP, "FULL") for hw in FUSED_SIZES] + [(hw, N_SMALL, "FULL") for hw in SMALL_SIZES] +
         [(hw, N_SWEEP, NAME_OF(p)) for hw, p in FALLBACK_SIZES.items()])
CASES.sort(key=lambda c: (c[0][0] * c[0][1], c[1]))  # smallest first


@pytest.mark.parametrize("hw,N,path", CASES, ids=[f"{h}x{w}-n{n}" for (h, w), n, _ in CASES])
def test_engine_geometry(cuda, hw, N, path):
    """(a) the output against the fp64 oracle of every image at the suite's tolerance; (b) bit identity with
    engines that have one fusion off each (max is exact in any order: the project's contract); (c) a second
    forward into a NaN-filled output, so every pixel is shown to be rewritten. Each engine's path is asserted."""
    H, W = hw
    x = init_input(N, "rand", seed=3, H=H, W=W).to(cuda)
    mk = lambda kn: AlexNetBlocks(device=cuda, init="rand", seed=3, max_batch=N, H=H, W=W, knobs=kn)  # noqa: E731
    m = mk({})
    y = m(x)
    assert m.last_path() == PATHS[path]
    ref = blocks_forward_all(x, m.weights, m.b1, m.b2, device=cuda)
    torch.testing.assert_close(y.cpu().double(), ref, rtol=2e-5, atol=2e-6)
    for knob, expect in VARIANTS.items():
        v = mk({knob: 0})
        assert torch.equal(v(x), y), knob
        assert v.last_path() == expect[path], knob
    y2 = torch.full_like(y, float("nan"))
    m(x, out=y2)
    assert torch.equal(y2, y)
    assert m.last_path() == PATHS[path]


def test_last_path_before_forward_and_under_capture(cuda):
    """A new engine has launched nothing; the record is host state, readable while a stream capture is open."""
    H, W, N = 51, 83, N_SWEEP
    m = AlexNetBlocks(device=cuda, init="rand", seed=3, max_batch=N, H=H, W=W)
    assert m.last_path() == dict.fromkeys(("conv1", "pool1", "conv2", "pool2"))
    x = init_input(N, "rand", seed=3, H=H, W=W).to(cuda)
    ref = m(x).clone()
    y = torch.full_like(ref, float("nan"))
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        m(x, out=y)
    torch.cuda.current_stream().wait_stream(s)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        m(x, out=y)
        assert m.last_path() == FULL
    y.fill_(float("nan"))
    g.replay()
    torch.cuda.synchronize()
    assert torch.equal(y, ref)


def test_engine_geometry_randn_he(cuda):
    """131x179 with randn inputs and He-normal weights (as test_full_blocks_randn_he_vs_oracle, at its bound):
    sign-mixed pre-ReLU maps make the pooled maxima depend on which pixels a window holds."""
    H, W, N = 131, 179, N_SWEEP
    torch.manual_seed(5)
    ws = {"w1": torch.randn(96, 3, 11, 11) * math.sqrt(2.0 / 363), "b1": torch.randn(96) * 0.1,
          "w2": torch.randn(256, 96, 5, 5) * math.sqrt(2.0 / 2400), "b2": torch.randn(256) * 0.1}
    x = torch.randn(N, H, W, 3)
    m = AlexNetBlocks(ws, device=cuda, max_batch=N, H=H, W=W)
    y = m(x.to(cuda))
    assert m.last_path() == FULL
    ref = blocks_forward_all(x, m.weights, m.b1, m.b2, device=cuda)
    err = (y.cpu().double() - ref).abs().max().item()
    print(f"131x179 randn/He: max abs err {err:.3e}, bound {1e-5 * ref.abs().max().item():.3e}")
    assert err <= 1e-5 * ref.abs().max().item()
    plain = AlexNetBlocks(ws, device=cuda, max_batch=N, H=H, W=W, knobs={"conv1_pool": 0, "conv2_pool": 0, "fuse_pool1": 0})
    assert torch.equal(plain(x.to(cuda)), y)
    assert plain.last_path() == UNFUSED


@pytest.mark.parametrize("np_", [2, 3])
def test_row_tiles_other_width(cuda, np_):
    """Overlap row tiles of a 131x179 image (pool1 inside the Conv2 input transform, pool_wino_in_kernel, at a
    21-column map; both convs forced to Winograd as in the 227x227 row-tile tests, since a tile of 9 images is
    below the Auto crossover): concatenated, against the whole-image forward and the oracle."""
    H, W, N = 131, 179, N_SWEEP
    kn = {"conv1_algo": "winograd", "conv2_algo": "winograd"}
    x = init_input(N, "rand", seed=3, H=H, W=W).to(cuda)
    m = AlexNetBlocks(device=cuda, init="rand", seed=3, max_batch=N, H=H, W=W, knobs=kn)
    whole = m(x).clone()
    assert m.last_path() == FULL
    parts = []
    for t in make_plan(H, W, np_, OVERLAP).tiles:
        assert not t.out.empty
        parts.append(m.tile_forward(x[:, t.inp.lo:t.inp.hi].contiguous(), t))
        assert m.last_path() == MIDDLE
    y = torch.cat(parts, dim=1)
    # a row tile starts its Winograd tiles at its own first row: same values to rounding, not the same bits
    torch.testing.assert_close(y, whole, rtol=2e-5, atol=2e-6)
    ref = blocks_forward_all(x, m.weights, m.b1, m.b2, device=cuda)
    torch.testing.assert_close(y.cpu().double(), ref, rtol=2e-5, atol=2e-6)


def test_lanes_other_size(cuda):
    """115x147, 32 images on two stream lanes of 16: each lane's engine takes the fused chain, the result is
    bitwise the one-lane forward and matches the oracle."""
    H, W, N = 115, 147, 32
    x = init_input(N, "rand", seed=3, H=H, W=W).to(cuda)
    one = AlexNetBlocks(device=cuda, init="rand", seed=3, max_batch=N, H=H, W=W)
    two = AlexNetBlocks(one.weights, device=cuda, max_batch=N, H=H, W=W, lanes=2)
    ref = one(x).clone()
    y = torch.full_like(ref, float("nan"))
    two(x, out=y)
    torch.cuda.synchronize()
    assert two.lane_count() == 2 and two.last_path() == FULL and two.last_path(lane=1) == FULL
    assert one.last_path() == FULL
    assert torch.equal(y, ref)
    oracle = blocks_forward_all(x, one.weights, one.b1, one.b2, device=cuda)
    torch.testing.assert_close(y.cpu().double(), oracle, rtol=2e-5, atol=2e-6)
