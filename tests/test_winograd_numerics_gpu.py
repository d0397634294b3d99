"""fp32 Winograd kernels at realistic dynamic range (randn activations, He-init weights), with the
error bounded relative to the sum of absolute products Σ|x·w| of each output — the scale of fp32
accumulation error itself (a direct fp32 conv sits at ~1e-7 of it). The reference-init tests (inputs
U[0,0.1), weights ±0.01) exercise a narrow range only; these pin the transforms' cancellation error.
Also: the exact bench.py step (stream lanes) against the fp64 oracle, images of every lane."""
import math

import pytest
import torch

from anx import _native as nat
from anx.models.alexnet_blocks import AlexNetBlocks
from anx.models.reference import blocks_forward, blocks_forward_all, conv2d_nhwc

pytestmark = pytest.mark.gpu
# Bounds relative to Σ|x·w| per output. F(3x3,5x5) (Conv2) interpolates at 7 points (0, ±1, ±2, ±1/2)
# and F(3x3,3x3) (Conv1 polyphase) at 5, so the transforms cancel more for Conv2. MI355X run: Conv2
# max 1.8-2.6e-6 (mean 8e-8), Conv1 max 1.0-1.3e-6 (mean 4.4e-8). A broken transform or fold is >=1e-3.
# F(4x4,5x5) (8 points, {0, +-1, +-2, +-1/2, inf}) sits ~1.3x above F(3,5) in tools/winograd_numerics.py.
BOUND_CONV2 = 1e-5
BOUND_CONV1 = 4e-6


def _rel_to_terms(y, x, w, b, S, P, groups=1):
    ref = conv2d_nhwc(x.double(), w.double(), b.double(), S, P, groups)
    terms = conv2d_nhwc(x.double().abs(), w.double().abs(), b.double().abs(), S, P, groups)
    rel = (y.double() - ref).abs() / (terms + 1e-30)
    print(f"error / sum|x*w|: max {rel.max().item():.3e} mean {rel.mean().item():.3e}")
    return rel.max().item()


@pytest.mark.parametrize("N,groups,tile", [(12, 1, 3), (12, 2, 3), (9, 1, 3), (128, 1, 3), (140, 2, 3), (12, 1, 4),
                                          (9, 1, 4), (128, 1, 4), (141, 1, 4)])
def test_conv2_winograd_randn_he(cuda, N, groups, tile):
    """Conv2 (31x31 padded window, 96 -> 256, 5x5): randn inputs, He-normal weights; Winograd F(3x3,5x5)
    and F(4x4,5x5) (wino_gemm16.hpp: 16x16x4 MFMAs, 4x4 output tiles with a clipped last row/column)."""
    torch.manual_seed(21 + N)
    C, K = 96, 256
    x = torch.randn(N, 31, 31, C, device=cuda)
    x[:, :2] = 0
    x[:, -2:] = 0
    x[:, :, :2] = 0
    x[:, :, -2:] = 0  # the zero border of the conv2 window
    w = torch.randn(K, C // groups, 5, 5) * math.sqrt(2.0 / (C // groups * 25))
    b = torch.randn(K, device=cuda) * 0.1
    y = torch.full((N, 27, 27, K), float("nan"), device=cuda)
    nat.call("anx_conv2_wino_tile", x.data_ptr(), N, 31, 31, C, w.contiguous().data_ptr(), K, groups, b.data_ptr(),
             y.data_ptr(), 0, nat.stream_ptr(cuda), tile)
    assert torch.isfinite(y).all()
    assert _rel_to_terms(y, x, w.to(cuda), b, 1, 0, groups) < BOUND_CONV2


WINDOWS = [(7, 7), (8, 9), (12, 13), (13, 14), (14, 31), (31, 20)]  # (Hq, Wq): outputs (Hq - 4) x (Wq - 4)
WINDOW_CASES = [(hq, wq, n, g, t) for hq, wq in WINDOWS for n in ((9, 40) if hq <= 8 else (9,))
                for g, t in ((1, 3), (2, 3), (1, 4))]


@pytest.mark.parametrize("Hq,Wq,N,groups,tile", WINDOW_CASES)
def test_conv2_winograd_randn_he_windows(cuda, Hq, Wq, N, groups, tile):
    """test_conv2_winograd_randn_he at other Conv2 windows (it only ever runs 31x31, i.e. a last tile with 3
    valid rows and columns on F(4x4,5x5) and none partial on F(3x3,5x5)): outputs 3x3 (one tile), 4x5, 8x9
    (4x4 remainders 0 / 1), 9x10 (1 / 2), 10x27 and 27x16 (2 / 3, 3 / 0), non-square; 9 images, and 40 for the two
    smallest (several images per 32- or 64-tile workgroup). Same zero border, error measure and bound: the
    transforms are the 31x31 ones. Every output pixel must be written (the map starts as NaN).
    MI355X run, max error / sum|x*w| per window (F(3,5) groups 1, groups 2, F(4,5)), means 0.8-1.7e-7:
    7x7 2.3e-6 2.5e-6 2.7e-6 (40 images 2.4e-6 3.0e-6 2.9e-6); 8x9 1.0e-6 1.1e-6 2.4e-6 (40 images 1.2e-6 1.1e-6
    3.6e-6); 12x13 1.5e-6 1.3e-6 5.0e-6; 13x14 1.8e-6 1.6e-6 2.1e-6; 14x31 2.0e-6 2.2e-6 2.5e-6; 31x20 1.5e-6
    2.2e-6 2.9e-6. The largest, 5.0e-6, is half the bound."""
    torch.manual_seed(21 + N + 100 * Hq + Wq)
    C, K = 96, 256
    x = torch.randn(N, Hq, Wq, C, device=cuda)
    x[:, :2] = 0
    x[:, -2:] = 0
    x[:, :, :2] = 0
    x[:, :, -2:] = 0  # the zero border of the conv2 window
    w = torch.randn(K, C // groups, 5, 5) * math.sqrt(2.0 / (C // groups * 25))
    b = torch.randn(K, device=cuda) * 0.1
    y = torch.full((N, Hq - 4, Wq - 4, K), float("nan"), device=cuda)
    nat.call("anx_conv2_wino_tile", x.data_ptr(), N, Hq, Wq, C, w.contiguous().data_ptr(), K, groups, b.data_ptr(),
             y.data_ptr(), 0, nat.stream_ptr(cuda), tile)
    assert torch.isfinite(y).all()
    assert _rel_to_terms(y, x, w.to(cuda), b, 1, 0, groups) < BOUND_CONV2


@pytest.mark.parametrize("C,K,groups,tile", [(64, 256, 1, 3), (96, 200, 1, 4), (96, 256, 2, 4), (96, 256, 1, 5)])
def test_conv2_winograd_refuses_other_shapes(cuda, C, K, groups, tile):
    """A shape the Winograd entry has no kernel for is an error, and the output is left untouched."""
    x = torch.zeros(2, 12, 13, C, device=cuda)
    w = torch.zeros(K, C // groups, 5, 5)
    b = torch.zeros(K, device=cuda)
    y = torch.full((2, 8, 9, K), float("nan"), device=cuda)
    with pytest.raises(nat.NativeError):
        nat.call("anx_conv2_wino_tile", x.data_ptr(), 2, 12, 13, C, w.contiguous().data_ptr(), K, groups, b.data_ptr(),
                 y.data_ptr(), 0, nat.stream_ptr(cuda), tile)
    torch.cuda.synchronize()
    assert torch.isnan(y).all()


@pytest.mark.parametrize("N", [5, 70])
def test_conv1_polyphase_winograd_randn_he(cuda, N):
    """Conv1 (227x227x3, 11x11/4, 96 filters) on the polyphase Winograd path: randn inputs."""
    torch.manual_seed(31 + N)
    x = torch.randn(N, 227, 227, 3, device=cuda)
    w = torch.randn(96, 3, 11, 11) * math.sqrt(2.0 / (3 * 121))
    b = torch.randn(96, device=cuda) * 0.1
    y = torch.full((N, 55, 55, 96), float("nan"), device=cuda)
    nat.call("anx_conv1_wino", x.data_ptr(), N, 227, 227, w.contiguous().data_ptr(), 96, 11, b.data_ptr(),
             y.data_ptr(), 0, nat.stream_ptr(cuda))
    assert torch.isfinite(y).all()
    assert _rel_to_terms(y, x, w.to(cuda), b, 4, 0) < BOUND_CONV1


@pytest.mark.parametrize("tile", [3, 4])
def test_full_blocks_randn_he_vs_oracle(cuda, tile):
    """The whole Blocks 1-2 engine (both Winograd convs, pools, LRN) at randn/He scale, Conv2 on either
    Winograd tile (Knobs::conv2_tile)."""
    torch.manual_seed(5)
    w1 = torch.randn(96, 3, 11, 11) * math.sqrt(2.0 / 363)
    w2 = torch.randn(256, 96, 5, 5) * math.sqrt(2.0 / 2400)
    ws = {"w1": w1, "b1": torch.randn(96) * 0.1, "w2": w2, "b2": torch.randn(256) * 0.1}
    m = AlexNetBlocks(ws, device=cuda, max_batch=24, knobs={"conv2_tile": tile})
    assert m.get_knob("conv2_tile") == tile
    x = torch.randn(24, 227, 227, 3)
    y = m(x.to(cuda)).cpu().double()
    ref = blocks_forward(x, m.weights, m.b1, m.b2)
    assert (y - ref).abs().max().item() <= 1e-5 * ref.abs().max().item()


def test_bench_step_vs_oracle(cuda):
    """bench.py's default step: 128 images as 2 stream lanes of 64 (one engine per HIP stream),
    checked against the fp64 oracle on images from both lanes including the first and last."""
    B = 128
    m = AlexNetBlocks(init="rand", seed=1234, device=cuda, max_batch=B, lanes=2)
    g = torch.Generator(device=cuda)
    g.manual_seed(1234)
    x = torch.rand((B, 227, 227, 3), device=cuda, generator=g) * 0.1
    y = m(x)
    ref = blocks_forward_all(x, m.weights, m.b1, m.b2, device=cuda)  # all 128 images, fp64
    err = (y.cpu().double() - ref).abs().amax(dim=(1, 2, 3)) / ref.abs().amax(dim=(1, 2, 3))
    assert err.max().item() <= 1e-5, (err.argmax().item(), err.max().item())
    # the second lane's half is bitwise what one engine computes for it alone
    solo = AlexNetBlocks(init="rand", seed=1234, device=cuda, max_batch=B // 2)
    assert torch.equal(solo(x[B // 2:].contiguous()), y[B // 2:])
