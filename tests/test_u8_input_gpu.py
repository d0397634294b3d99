"""Byte (uint8) image input on the device.

A byte b of channel c means fmaf(float(b), scale[c], offset[c]) in fp32. Three implementations of that one
expression exist (the host decode, the device decode kernel, the byte loader of the one-kernel Conv1) and every
arithmetic step after it is the fp32 engine's, so the checks here are bit identities: device decode == host
decode, and engine(bytes) == engine(decoded floats) on every route. Only the oracle checks carry a tolerance,
the suite's own. Shapes are the smallest that reach each hazard of the byte loader: odd row lengths (35, 55
columns: pairs and images at odd addresses), an even one, workgroups spanning images (40 images of 9 tiles),
the last byte of the buffer (the last image is black but for its last pixel), a non-zero offset (padding must
decode to 0, not to offset[c]), all four kernel forms, and the fallback that decodes into the workspace."""
import pytest
import torch

from anx.models.alexnet_blocks import AlexNetBlocks, norm_scale_offset
from anx.models.reference import blocks_forward_all
from anx.ops import decode_u8
from anx.parallel.plan import OVERLAP, full_plan, make_plan

from geometry_cases import FALLBACK_SIZES, FULL, FUSED_SIZES, MIDDLE, N_SMALL, N_SWEEP, UNFUSED

pytestmark = pytest.mark.gpu

MEAN, STD = (123.7, 116.3, 103.5), (58.4, 57.1, 57.4)
NORM = (MEAN, STD)
TENTH = (0.0, 2550.0)  # scale = 0.1 / 255: the decoded image lies in the suite's own [0, 0.1) input range
EVEN = (35, 38)        # an even width: rows of 114 bytes (asserted below to take the fused chain)
assert (35, 35) in FUSED_SIZES and (67, 55) in FUSED_SIZES and FALLBACK_SIZES[(227, 235)] == UNFUSED


def images(N, H, W, seed=3):
    """Seeded random bytes; the last image black except its last pixel: the buffer's last bytes matter."""
    g = torch.Generator().manual_seed(seed)
    x = torch.randint(0, 256, (N, H, W, 3), dtype=torch.uint8, generator=g)
    x[-1] = 0
    x[-1, -1, -1, :] = 255
    return x


# ---------------------------------------------------------------------------------------------- 1. the decode
@pytest.mark.parametrize("off", [0, 1, 3])
@pytest.mark.parametrize("n", [1, 15, 16, 17, 9 * 35 * 35 * 3])
def test_device_decode_equals_host_decode(cuda, n, off):
    g = torch.Generator().manual_seed(n + off)
    buf = torch.randint(0, 256, (n + 8,), dtype=torch.uint8, generator=g)
    scale, offset = norm_scale_offset(NORM, 3)
    host = decode_u8(buf[off:off + n], scale, offset)
    dev_buf = buf.to(cuda)
    xs = dev_buf[off:off + n]
    assert xs.data_ptr() == dev_buf.data_ptr() + off
    out = decode_u8(xs, scale, offset)
    assert out.dtype == torch.float32 and torch.equal(out.cpu(), host)
    assert torch.equal(decode_u8(xs, [1.0], [0.0]).cpu(), buf[off:off + n].float())


def test_device_decode_grid_stride(cuda):
    """More 16-byte units than the capped grid has threads (4096 x 256): the body loop takes a second trip; an
    odd start and a tail with it."""
    n = 4096 * 256 * 16 + 16 * 5 + 7
    g = torch.Generator().manual_seed(1)
    buf = torch.randint(0, 256, (n + 8,), dtype=torch.uint8, generator=g)
    scale, offset = norm_scale_offset(NORM, 3)
    host = decode_u8(buf[3:3 + n], scale, offset)
    assert torch.equal(decode_u8(buf.to(cuda)[3:3 + n], scale, offset).cpu(), host)


# ------------------------------------------------------------------- 2. + 3. bytes == decoded floats, per size
def _check_size(cuda, H, W, N, path, oracle):
    x = images(N, H, W).to(cuda)
    mk = lambda kn, nm=NORM: AlexNetBlocks(device=cuda, init="rand", seed=3, max_batch=N, H=H, W=W, knobs=kn,  # noqa: E731
                                          input_norm=nm)
    m = mk({"conv1_u8": 1})
    assert m.last_input() is None
    xf = m.decode_u8(x)
    assert torch.equal(xf.cpu(), decode_u8(x.cpu(), *norm_scale_offset(NORM, 3)))
    yf = m(xf).clone()
    assert m.last_input() == "f32" and m.last_path() == path
    y = m(x)
    assert m.last_input() == "u8_fused" and m.last_path() == path
    assert torch.equal(y, yf)
    for kn in ({"conv1_u8": 0}, {}):  # the decode route, also the default
        m0 = mk(kn)
        assert torch.equal(m0(x), yf)
        assert m0.last_input() == "u8_decode" and m0.last_path() == path
    # a second forward into a NaN-filled output: every pixel is rewritten
    y2 = torch.full_like(yf, float("nan"))
    m(x, out=y2)
    assert torch.equal(y2, yf)
    if oracle:
        # sign-mixed inputs (mean / std): the bound of test_engine_geometry_randn_he
        ref = blocks_forward_all(xf.cpu(), m.weights, m.b1, m.b2, device=cuda)
        err = (y.cpu().double() - ref).abs().max().item()
        print(f"{H}x{W} n{N} mean/std: max abs err {err:.3e}, bound {1e-5 * ref.abs().max().item():.3e}")
        assert err <= 1e-5 * ref.abs().max().item()
        # [0, 0.1) inputs: the suite's tolerance
        t = mk({"conv1_u8": 1}, TENTH)
        xt = t.decode_u8(x)
        assert 0 <= xt.min() and xt.max() < 0.1001
        yt = t(x)
        assert t.last_input() == "u8_fused" and torch.equal(yt, t(xt))
        ref = blocks_forward_all(xt.cpu(), t.weights, t.b1, t.b2, device=cuda)
        torch.testing.assert_close(yt.cpu().double(), ref, rtol=2e-5, atol=2e-6)
    return m, x, y


SIZES = [((35, 35), N_SWEEP, FULL, True), ((35, 35), N_SMALL, FULL, False), ((67, 55), N_SWEEP, FULL, False),
         (EVEN, N_SWEEP, FULL, False), ((227, 227), N_SWEEP, FULL, True), ((227, 235), N_SWEEP, UNFUSED, False)]


@pytest.mark.parametrize("hw,N,path,oracle", SIZES, ids=[f"{h}x{w}-n{n}" for (h, w), n, _, _ in SIZES])
def test_u8_equals_decoded_f32(cuda, hw, N, path, oracle):
    m, x, y = _check_size(cuda, hw[0], hw[1], N, path, oracle)
    if hw == (35, 35):
        # the last pixel of the last image (the buffer's last three bytes) reaches the output at this size
        xb = x.clone()
        xb[-1] = 0
        yb = m(xb)
        assert torch.equal(yb[:-1], y[:-1]) and not torch.equal(yb[-1], y[-1])


# ------------------------------------------------------------------------ 4. the four one-kernel instantiations
@pytest.mark.parametrize("kn,path", [({"conv1_fused": 1}, FULL), ({"conv1_fused": 2}, FULL), ({"conv1_fused": 3}, FULL),
                                     ({"conv1_pool": 0}, MIDDLE)],
                         ids=["shared_ring", "wave_ring", "u_in_registers", "no_pool"])
def test_u8_every_one_kernel_form(cuda, kn, path):
    H, W, N = 35, 35, N_SWEEP
    x = images(N, H, W).to(cuda)
    m = AlexNetBlocks(device=cuda, init="rand", seed=3, max_batch=N, H=H, W=W, knobs={**kn, "conv1_u8": 1}, input_norm=NORM)
    yf = m(m.decode_u8(x)).clone()
    assert m.last_input() == "f32" and m.last_path() == path
    assert torch.equal(m(x), yf)
    assert m.last_input() == "u8_fused" and m.last_path() == path


def test_u8_other_conv1_routes_decode_first(cuda):
    """Where Conv1 is not the one-kernel form the bytes go through the decode kernel: the band + GEMM Winograd
    form, the implicit GEMM below the Auto crossover, the direct oracle engine."""
    H, W = 35, 35
    for N, kw, conv1 in [(N_SWEEP, {"knobs": {"conv1_fused": 0}}, "wino"), (2, {}, "mfma"), (2, {"impl": "direct"}, "direct")]:
        x = images(N, H, W).to(cuda)
        m = AlexNetBlocks(device=cuda, init="rand", seed=3, max_batch=N, H=H, W=W, input_norm=NORM, **kw)
        yf = m(m.decode_u8(x)).clone()
        assert torch.equal(m(x), yf), conv1
        assert m.last_input() == "u8_decode" and m.last_path()["conv1"] == conv1


# ------------------------------------------------------------------------------------------ 5. every entry point
def test_u8_lanes_and_async(cuda):
    H, W, N = 115, 147, 32
    x = images(N, H, W).to(cuda)
    kn = {"conv1_u8": 1}
    one = AlexNetBlocks(device=cuda, init="rand", seed=3, max_batch=N, H=H, W=W, input_norm=NORM, knobs=kn)
    two = AlexNetBlocks(one.weights, device=cuda, max_batch=N, H=H, W=W, lanes=2, input_norm=NORM, knobs=kn)
    ref = one(x).clone()
    assert one.last_input() == "u8_fused" and one.last_path() == FULL
    assert torch.equal(ref, one(one.decode_u8(x)))
    y = torch.full_like(ref, float("nan"))
    two(x, out=y)
    torch.cuda.synchronize()
    assert two.lane_count() == 2 and two.last_input() == "u8_fused" and two.last_input(lane=1) == "u8_fused"
    assert two.last_path() == FULL and two.last_path(lane=1) == FULL
    assert torch.equal(y, ref)
    y.fill_(float("nan"))
    two.forward_async(x, y)
    two.join()
    torch.cuda.synchronize()
    assert torch.equal(y, ref)
    # a change of the normalisation reaches the side lane
    two.set_input_norm()
    one.set_input_norm()
    assert torch.equal(two(x), one(x))
    assert not torch.equal(one(x), ref)


def test_u8_row_tiles(cuda):
    H, W, N = 131, 179, N_SWEEP
    kn = {"conv1_algo": "winograd", "conv2_algo": "winograd", "conv1_u8": 1}
    x = images(N, H, W).to(cuda)
    m = AlexNetBlocks(device=cuda, init="rand", seed=3, max_batch=N, H=H, W=W, knobs=kn, input_norm=NORM)
    xf = m.decode_u8(x)
    for t in make_plan(H, W, 2, OVERLAP).tiles:
        assert not t.out.empty
        a = m.tile_forward(xf[:, t.inp.lo:t.inp.hi].contiguous(), t).clone()
        assert m.last_input() == "f32" and m.last_path() == MIDDLE
        b = m.tile_forward(x[:, t.inp.lo:t.inp.hi].contiguous(), t)
        assert m.last_input() == "u8_fused" and m.last_path() == MIDDLE
        assert torch.equal(a, b)


def test_u8_stage1_stage2(cuda):
    H, W, N = 67, 55, N_SWEEP
    x = images(N, H, W).to(cuda)
    m = AlexNetBlocks(device=cuda, init="rand", seed=3, max_batch=N, H=H, W=W, input_norm=NORM, knobs={"conv1_u8": 1})
    t = full_plan(H, W, m.b1, m.b2)
    rows = slice(t.inp.lo, t.inp.hi)
    m.stage1(m.decode_u8(x)[:, rows].contiguous(), t)
    assert m.last_input() == "f32"
    yf = m.stage2(N, t).clone()
    m.stage1(x[:, rows].contiguous(), t)
    assert m.last_input() == "u8_fused" and m.last_path() == UNFUSED
    assert torch.equal(m.stage2(N, t), yf)
    assert torch.equal(m(x), yf)  # the fused chain computes the same bits (the project's contract)


# ------------------------------------------------------------------------------------------- 6. stream capture
@pytest.mark.parametrize("conv1_u8", [1, 0])
def test_u8_under_capture(cuda, conv1_u8):
    """After one warm-up forward (it allocates the decode workspace where one is needed) a captured forward
    replays to the same bits; the input record is host state, readable while the capture is open."""
    H, W, N = 51, 83, N_SWEEP
    m = AlexNetBlocks(device=cuda, init="rand", seed=3, max_batch=N, H=H, W=W, input_norm=NORM, knobs={"conv1_u8": conv1_u8})
    x = images(N, H, W).to(cuda)
    ref = m(x).clone()
    assert torch.equal(ref, m(m.decode_u8(x)))
    y = torch.full_like(ref, float("nan"))
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        m(x, out=y)
    torch.cuda.current_stream().wait_stream(s)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        m(x, out=y)
        assert m.last_input() == ("u8_fused" if conv1_u8 else "u8_decode") and m.last_path() == FULL
    y.fill_(float("nan"))
    g.replay()
    torch.cuda.synchronize()
    assert torch.equal(y, ref)
