"""Byte (uint8) image input on the host: the decode definition and the host engine's byte entry points.

A byte b of channel c means fmaf(float(b), scale[c], offset[c]), one fused multiply-add in fp32. The host decode
(anx_cpu_decode_u8) is the reference the device tests compare against bit for bit; here it is checked against
fp64 arithmetic, and AlexNetBlocks(device="cpu") fed bytes against the same model fed the decoded floats."""
import pytest
import torch

from anx.models.alexnet_blocks import AlexNetBlocks, norm_scale_offset
from anx.ops import decode_u8
from anx.parallel.plan import OVERLAP, make_plan
from anx.utils.tuning import KNOBS, knob_value

MEAN, STD = (123.7, 116.3, 103.5), (58.4, 57.1, 57.4)
COUNTS = [1, 15, 16, 17, 9 * 35 * 35 * 3]


def _bytes(n, off, seed=0):
    """n bytes starting `off` bytes into a larger buffer (a slice keeps the storage: the address is base + off)."""
    g = torch.Generator().manual_seed(seed)
    return torch.randint(0, 256, (n + 8,), dtype=torch.uint8, generator=g)[off:off + n]


@pytest.mark.parametrize("off", [0, 1, 3])
@pytest.mark.parametrize("n", COUNTS)
def test_cpu_decode_matches_fp64(n, off):
    """Within one fp32 rounding of b * scale + offset computed in fp64 (torch.addcmul). For these values the fp64
    result is exact (an 8-bit byte times a 24-bit scale plus a 24-bit offset of similar magnitude needs under 40
    bits), so a correctly rounded fmaf is in fact its nearest float: asserted too. A multiply rounded on its own
    before the add misses that for some of the 256 x 3 (byte, channel) pairs, all of which the large case holds."""
    x = _bytes(n, off)
    assert x.data_ptr() == x._base.data_ptr() + off
    scale, offset = norm_scale_offset((MEAN, STD), 3)
    y = decode_u8(x, scale, offset)
    assert y.dtype == torch.float32 and y.shape == x.shape
    ch = torch.arange(n) % 3
    exact = torch.addcmul(offset.double()[ch], x.double(), scale.double()[ch])
    near = exact.float()
    lo = torch.nextafter(near, torch.full_like(y, -float("inf")))
    hi = torch.nextafter(near, torch.full_like(y, float("inf")))
    assert bool(((y >= lo) & (y <= hi)).all())
    assert torch.equal(y, near)


@pytest.mark.parametrize("off", [0, 1, 3])
@pytest.mark.parametrize("n", COUNTS)
def test_cpu_decode_identity_exact(n, off):
    x = _bytes(n, off, seed=1)
    assert torch.equal(decode_u8(x, [1.0], [0.0]), x.float())


def test_decode_default_and_shape():
    x = _bytes(2 * 5 * 7 * 3, 1).view(2, 5, 7, 3)
    y = decode_u8(x)
    s = torch.tensor(1.0 / 255.0, dtype=torch.float64).float()
    assert y.shape == x.shape and torch.equal(y, x.float() * s)  # offset 0: the fmaf is one rounded multiply
    with pytest.raises(ValueError):
        decode_u8(x.float())
    with pytest.raises(ValueError):
        decode_u8(x, [1.0, 2.0], [0.0])


def _u8_images(N, H, W, seed=3):
    g = torch.Generator().manual_seed(seed)
    return torch.randint(0, 256, (N, H, W, 3), dtype=torch.uint8, generator=g)


@pytest.mark.parametrize("hw", [(35, 35), (39, 47)])
def test_cpu_model_u8_equals_decoded(hw):
    H, W = hw
    N = 2
    m = AlexNetBlocks(device="cpu", init="rand", seed=3, H=H, W=W, max_batch=N, input_norm=(MEAN, STD))
    x = _u8_images(N, H, W)
    xf = m.decode_u8(x)
    assert torch.equal(xf, decode_u8(x, *norm_scale_offset((MEAN, STD), 3)))
    assert xf.min() < 0 < xf.max()  # a non-zero mean: padding with offset[c] instead of 0 would show
    y = m(x)
    assert torch.equal(y, m(xf))
    assert y.abs().max() > 0
    for t in make_plan(H, W, 2, OVERLAP).tiles:
        if t.out.empty:
            continue
        a = m.tile_forward(x[:, t.inp.lo:t.inp.hi].contiguous(), t)
        b = m.tile_forward(xf[:, t.inp.lo:t.inp.hi].contiguous(), t)
        assert torch.equal(a, b)
    # stage1 / stage2 on bytes
    t = make_plan(H, W, 1, OVERLAP).tiles[0]
    m.stage1(x[:, t.inp.lo:t.inp.hi].contiguous(), t)  # 39 rows: the whole-image tile reads the 35 it needs
    assert torch.equal(m.stage2(N, t), y)
    # the default meaning, and a change of it, reach the engine
    m.set_input_norm()
    assert torch.equal(m(x), m(decode_u8(x)))
    assert not torch.equal(m(x), y)


def test_input_norm_validation():
    mk = lambda nm: AlexNetBlocks(device="cpu", H=35, W=35, input_norm=nm)  # noqa: E731
    for bad in [(MEAN, (1.0, 0.0, 1.0)), (MEAN, (1.0, -2.0, 1.0)), ((1.0, 2.0), STD), (MEAN, (1.0, 2.0)),
                ((float("nan"), 0.0, 0.0), STD), (MEAN, (float("inf"), 1.0, 1.0)), (MEAN,), "ab", (MEAN, 1e-42),
                (("a", "b", "c"), STD)]:
        with pytest.raises(ValueError):
            mk(bad)
    m = mk((100.0, 50.0))  # scalars broadcast over the channels
    scale, offset = norm_scale_offset((100.0, 50.0), 3)
    assert torch.equal(scale, torch.full((3,), 0.02)) and torch.equal(offset, torch.full((3,), -2.0))
    with pytest.raises(ValueError):
        m.set_input_norm(mean=1.0)
    with pytest.raises(ValueError):
        m.set_input_norm(MEAN, (0.0, 1.0, 1.0))
    # fp64 then one rounding
    s, o = norm_scale_offset((MEAN, STD), 3)
    assert torch.equal(s, (1.0 / torch.tensor(STD, dtype=torch.float64)).float())
    assert torch.equal(o, (-torch.tensor(MEAN, dtype=torch.float64) / torch.tensor(STD, dtype=torch.float64)).float())


def test_other_dtypes_rejected():
    m = AlexNetBlocks(device="cpu", H=35, W=35)
    for dt in (torch.float64, torch.int8, torch.float16, torch.int32):
        with pytest.raises(ValueError):
            m(torch.zeros(1, 35, 35, 3, dtype=dt))
    with pytest.raises(ValueError):
        m(torch.zeros(1, 35, 3, 35, dtype=torch.uint8).permute(0, 1, 3, 2))  # not contiguous


def test_conv1_u8_knob_known():
    assert "conv1_u8" in KNOBS
    assert knob_value("conv1_u8", True) == 1 and knob_value("conv1_u8", 0) == 0
    from anx.utils.tuning import default_knob
    assert default_knob("conv1_u8") in (0, 1)


def test_abi_version_bumped():
    from anx import _native as nat
    assert nat.lib().anx_abi_version() >= 2
