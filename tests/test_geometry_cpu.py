"""The geometry sweep's list of image sizes (geometry_cases.py), kept honest without a GPU: every size is a valid
network input whose dims and tile grids are the ones the table states, the host engine matches the fp64 oracle
there, the list covers every remainder / parity / limit class it claims, and at the batch sizes the GPU sweep
uses the side-buffer hand-offs (straddling pool windows) really occur.

The straddle predicates used here are Python mirrors of pool1_straddles / pool2_straddles
(csrc/include/anx/ops.hpp:154-189), in geometry_cases.py."""
import pytest
import torch

from anx.config import blocks_dims
from anx.models.alexnet_blocks import AlexNetBlocks
from anx.models.reference import blocks_forward
from anx.parallel.plan import full_plan
from anx.utils.init import init_input

from geometry_cases import (ALL_SIZES, FALLBACK_SIZES, FUSED_SIZES, N_SMALL, N_SWEEP, SMALL_SIZES, launch_grids,
                            straddle_counts)

ceil_div = lambda a, b: -(-a // b)  # noqa: E731


@pytest.mark.parametrize("hw", ALL_SIZES, ids=lambda hw: f"{hw[0]}x{hw[1]}")
def test_host_engine_vs_oracle(hw):
    """The host engine (plain serial fp32) against the fp64 oracle at the suite's tolerance, 2 images."""
    H, W = hw
    m = AlexNetBlocks(device="cpu", init="rand", seed=3, H=H, W=W)
    x = init_input(2, "rand", seed=3, H=H, W=W)
    y = m(x)
    d = blocks_dims(H, W)
    assert tuple(y.shape) == (2, d.Hp2, d.Wp2, 256)
    torch.testing.assert_close(y.double(), blocks_forward(x, m.weights, m.b1, m.b2), rtol=2e-5, atol=2e-6)


@pytest.mark.parametrize("hw", list(FUSED_SIZES), ids=lambda hw: f"{hw[0]}x{hw[1]}")
def test_table_dims(hw):
    """blocks_dims and the tile grids against the table's numbers; the grids of the whole-image launch (which
    holds only the rows its output needs) are the maps' own."""
    (H1, W1), (Hp1, Wp1), (Hp2, Wp2), g1, g2 = FUSED_SIZES[hw]
    d = blocks_dims(*hw)
    assert (d.H1, d.W1, d.Hp1, d.Wp1, d.Hp2, d.Wp2) == (H1, W1, Hp1, Wp1, Hp2, Wp2)
    assert (d.H2, d.W2) == (Hp1, Wp1)  # Conv2 is 5x5, stride 1, padding 2
    assert g1 == (ceil_div(H1, 3), ceil_div(W1, 3)) and g2 == (ceil_div(Hp1, 4), ceil_div(Wp1, 4))
    assert launch_grids(*hw) == (g1, g2)
    t = full_plan(*hw)
    assert t.p1.lo == 0 and t.p1.size == Hp1 and t.c1.lo == 0 and t.c1.size == 2 * Hp1 + 1
    # inside the fused chain's limits: the window in the band transforms' LDS, the Conv1 epilogue's pixel decode
    # and its look-back over a window's tiles
    assert Wp1 + 4 <= 31 and Hp1 <= 32 and Wp1 <= 32 and g1[1] + 1 <= 20


def test_class_coverage():
    """What the list must cover between its sizes."""
    dims = [blocks_dims(*hw) for hw in FUSED_SIZES]
    for axis in ("H1", "W1"):
        assert {getattr(d, axis) % 3 for d in dims} == {0, 1, 2}
        assert {getattr(d, axis) % 2 for d in dims} == {0, 1}  # an even map: the pool drops its last row / column
    for axis in ("Hp1", "Wp1"):
        assert {getattr(d, axis) % 4 for d in dims} == {0, 1, 2, 3}  # Conv2 4x4 tile remainders
    assert {d.Hp2 % 2 for d in dims} == {0, 1} and {d.Wp2 % 2 for d in dims} == {0, 1}
    grids2 = [FUSED_SIZES[hw][4] for hw in FUSED_SIZES]
    assert (1, 1) in grids2 and any(g[0] == 1 and g[1] > 1 for g in grids2) and max(grids2) >= (8, 6)
    # several images per Conv2 workgroup, and per Conv1 workgroup
    assert any(g[0] * g[1] == 1 for g in grids2) and any(g[0] * g[1] <= 16 for g in (FUSED_SIZES[hw][3] for hw in FUSED_SIZES))
    # both sides of every limit: on it ...
    assert any(d.Wp1 + 4 == 31 for d in dims)           # window width (wq = 31)
    assert any(d.Hp1 == 32 for d in dims)               # pixel decode
    assert any(ceil_div(d.W1, 3) == 19 for d in dims)   # the widest Conv1 grid a 31-column window allows
    assert any(d.Wp1 + 4 == 31 and d.Hp1 == 32 and ceil_div(d.W1, 3) == 19 for d in dims)  # all at once
    # ... and the first size past it
    past = [blocks_dims(*hw) for hw in FALLBACK_SIZES]
    assert any(d.Wp1 + 4 == 32 for d in past) and any(d.Hp1 == 33 and d.Wp1 + 4 <= 31 for d in past)
    assert any(ceil_div(d.W1, 3) == 20 for d in past) and any(ceil_div(d.W1, 3) == 21 for d in past)
    assert set(SMALL_SIZES) <= set(FUSED_SIZES) and max(SMALL_SIZES) == (99, 63)


def test_last_path_is_gpu_only():
    """The launch record belongs to the GPU engine: the host engine has one path and says so."""
    m = AlexNetBlocks(device="cpu", init="rand", seed=3, H=35, W=35)
    with pytest.raises(ValueError):
        m.last_path()


def test_side_buffers_are_exercised():
    """At the batch sizes the sweep runs, every size with more than one Conv1 tile per image has pool1 windows
    that straddle two Conv1 workgroups (partial maxima through the p1 side buffer), and at least five sizes have
    pool2 windows that straddle two Conv2 GEMM workgroups (through p2)."""
    with_p2 = []
    for hw in FUSED_SIZES:
        for N in [N_SWEEP] + ([N_SMALL] if hw in SMALL_SIZES else []):
            s1, n1, s2, n2 = straddle_counts(*hw, N)
            g1 = FUSED_SIZES[hw][3]
            assert g1[0] * g1[1] > 1 and 0 < s1 < n1, (hw, N, s1, n1)
            assert s2 < n2
            if s2 and N == N_SWEEP:
                with_p2.append(hw)
    assert len(with_p2) >= 5, with_p2
    # two counts taken by hand from the predicate
    assert straddle_counts(51, 83, 9)[2:] == (5, 72)
    assert straddle_counts(267, 234, 9)[2:] == (195, 1755)
