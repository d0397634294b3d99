"""Byte (uint8) image input of the bf16 full-AlexNet engine.

A byte b of channel c means fmaf(float(b), scale[c], offset[c]) in fp32, and that value then takes the float
path's own fp32 -> bf16 conversion. So every check here is a bit identity: logits and taps of a byte forward equal
(torch.equal) those of the SAME model's float forward of decode_u8(bytes), on both byte routes ("u8_ring": the
row-band Conv1 loads the bytes; "u8_decode": decode kernel into a workspace, then the float path), every Conv1
form, every segment count of the ring, with pool1 in its epilogue, from any start address, on lanes and under
stream capture. The one tolerance is bf16_oracle's own, on Conv1 + pool1 of the byte ring at N = 256.

Between the float and the byte forward a forward of other images runs and the byte forward writes into a
NaN-filled output: the taps are engine buffers that keep their content, and equal bits must not be left-overs.

Images are seeded random bytes; the last image is black except its last pixel, set to 255, so the buffer's last
bytes matter. Weights carry nonzero, not bf16-representable biases (as test_full_alexnet_oracle_gpu.py's)."""
import functools

import pytest
import torch

from anx.models.alexnet_full import AlexNetFull, init_full_weights
from bf16_oracle import assert_pool_bracket, bf16_bound, conv_ref

pytestmark = pytest.mark.gpu

NORM = ((123.7, 116.3, 103.5), (58.4, 57.1, 57.4))
IMAGE = 227 * 227 * 3  # 154,587 bytes: odd, so image i of a byte tensor starts at an odd address when i is odd
LAYERS = ("conv1", "conv2", "conv3", "conv4", "conv5", "fc6", "fc7", "fc8")
FLOAT_FORM = {2: "ring_f32", 1: "ring", 0: "tiles"}
MAX_BATCH = 257


@functools.lru_cache(maxsize=None)
def weights():
    w = init_full_weights(47)
    g = torch.Generator().manual_seed(1047)
    for name in LAYERS:
        b = torch.randn(w["b_" + name].shape, generator=g) * 0.1
        b.view(torch.int32).bitwise_or_(1)  # low mantissa bit set: no bias is a bf16 value
        w["b_" + name] = b
    return w


def images(N, seed=3):
    g = torch.Generator().manual_seed(seed)
    x = torch.randint(0, 256, (N, 227, 227, 3), dtype=torch.uint8, generator=g)
    x[-1] = 0
    x[-1, -1, -1, :] = 255
    return x


@pytest.fixture(scope="module")
def shared(cuda):
    m = AlexNetFull(weights(), device=cuda, max_batch=MAX_BATCH)
    yield m
    m.close()


def configure(m, norm=None, **knobs):
    """Every knob these tests touch, each time: a shared model carries nothing over from the test before."""
    for k, v in {"bf16_conv1": 2, "bf16_pool1": 1, "bf16_u8": 1, **knobs}.items():
        m.set_knob(k, v)
    if norm is None:
        m.set_input_norm()
    else:
        m.set_input_norm(*norm)


def float_then_bytes(m, x, taps=(0, 1)):
    """-> (float run, byte run), each (logits, [taps], last_path()["conv1"], last_input())."""
    N = x.shape[0]

    def grab(y):
        t = [m.tap(i, N) for i in taps]
        torch.cuda.synchronize()
        return y, t, m.last_path()["conv1"], m.last_input()

    xf = m.decode_u8(x)
    assert xf.dtype == torch.float32 and xf.shape == x.shape
    f = grab(m(xf).clone())
    m(torch.full_like(xf, 0.5))  # other images: the taps no longer hold the float run's values
    y = torch.full((N, m.classes), float("nan"), device=x.device)
    m(x, out=y)
    return f, grab(y)


def assert_same(f, b, what=""):
    assert not torch.isnan(b[0]).any(), what
    assert torch.equal(b[0], f[0]), f"logits {what}"
    for i, (tf, tb) in enumerate(zip(f[1], b[1])):
        assert torch.equal(tb, tf), f"tap #{i} {what}"


# ------------------------------------------------------------------------------- 1. every route at a small batch
def test_fresh_model_has_no_input_record(cuda):
    m = AlexNetFull(seed=1, device=cuda, max_batch=1)
    assert m.last_input() is None
    m.close()


@pytest.mark.parametrize("norm", [None, NORM], ids=["default", "mean_std"])
@pytest.mark.parametrize("u8", [1, 0])
@pytest.mark.parametrize("conv1", [2, 1, 0])
def test_every_route_small_batch(cuda, shared, conv1, u8, norm):
    m, N = shared, 3
    configure(m, norm, bf16_conv1=conv1, bf16_u8=u8, bf16_pool1=0)
    x = images(N).to(cuda)
    f, b = float_then_bytes(m, x)
    assert f[3] == "f32" and f[2]["form"] == FLOAT_FORM[conv1]
    ring = conv1 == 2 and u8 == 1
    assert b[3] == ("u8_ring" if ring else "u8_decode")
    assert b[2] == ({"form": "ring_u8", "segs": f[2]["segs"]} if ring else f[2])
    if conv1:
        assert f[2]["segs"] > 1  # a few images: each one's row tiles split over several workgroups
    assert_same(f, b, f"bf16_conv1={conv1} bf16_u8={u8}")
    if norm is not None:
        xf = m.decode_u8(x)
        assert xf.min() < 0 < xf.max()  # a nonzero offset: padding decoded to offset[c] instead of 0 would show


# --------------------------------------------------------------------------- 2. segment counts of the byte ring
def test_byte_ring_every_segment_count(cuda, shared):
    m = shared
    configure(m, NORM, bf16_pool1=0, bf16_u8=1)
    seen = set()
    for N in (128, 86, 52, 43, 40, 1):
        x = images(N, seed=N).to(cuda)
        f, b = float_then_bytes(m, x)
        assert f[3] == "f32" and f[2]["form"] == "ring_f32"
        assert b[3] == "u8_ring" and b[2]["form"] == "ring_u8"
        assert b[2]["segs"] == f[2]["segs"]
        print(f"N={N}: segs {b[2]['segs']}")
        seen.add(b[2]["segs"])
        assert_same(f, b, f"N={N} segs={b[2]['segs']}")
    assert len(seen) >= 4, seen


# ------------------------------------------------------------------------------------ 3. pool1 in the epilogue
@pytest.mark.parametrize("N", [256, 257])
def test_byte_ring_pool1_epilogue(cuda, shared, N):
    m = shared
    configure(m, NORM, bf16_u8=1)
    x = images(N, seed=N).to(cuda)
    f, b = float_then_bytes(m, x, taps=(1,))
    assert f[3] == "f32" and f[2] == {"form": "ring_f32_pool", "segs": 1}
    assert b[3] == "u8_ring" and b[2] == {"form": "ring_u8_pool", "segs": 1}
    assert_same(f, b, f"N={N}")
    y2 = torch.full_like(f[0], float("nan"))  # a second forward rewrites every logit
    m(x, out=y2)
    assert torch.equal(y2, f[0])
    if N == 256:  # independent of the float path: the fp64 oracle on the decoded image, its own bounds
        idx = torch.tensor([0, 128, 255], device=cuda)
        w = {k: v.to(cuda) for k, v in m.weights.items()}
        ref, T = conv_ref(m.decode_u8(x[idx]).to(torch.bfloat16), w["w_conv1"], w["b_conv1"], stride=4)
        want, tol = bf16_bound(ref, T)
        inner = b[1][0][:, 2:-2, 2:-2]
        ratio = assert_pool_bracket(inner[idx], want, tol, "conv1+pool1 (bytes)")
        print(f"conv1+pool1 from bytes: worst distance from the bracket's middle {ratio:.3f} half-widths")


# ------------------------------------------------------------ 4. any address, and the end of the allocation
@pytest.mark.parametrize("off", [0, 1, 2, 3])
def test_any_start_address_and_allocation_end(cuda, shared, off):
    m = shared
    n = 2 * IMAGE
    buf = torch.full((off + n + 16,), 255, dtype=torch.uint8, device=cuda)
    assert buf.data_ptr() % 4 == 0
    x = buf[off:off + n].view(2, 227, 227, 3)
    x.copy_(images(2, seed=10 + off))
    assert x.data_ptr() & 3 == off and x.is_contiguous()
    assert (buf[:off] == 255).all() and (buf[off + n:] == 255).all()
    for u8 in (1, 0):
        configure(m, NORM, bf16_u8=u8)
        f, b = float_then_bytes(m, x)  # the decoded tensor is a fresh allocation without such neighbours
        assert f[3] == "f32" and f[2]["form"] == "ring_f32"
        assert b[3] == ("u8_ring" if u8 else "u8_decode")
        assert b[2]["form"] == ("ring_u8" if u8 else "ring_f32") and b[2]["segs"] == f[2]["segs"]
        assert_same(f, b, f"off={off} bf16_u8={u8}")


# ------------------------------------------------------------------------------- 5. set_input_norm takes effect
def test_set_input_norm_takes_effect(cuda, shared):
    m = shared
    configure(m, None)
    x = images(2).to(cuda)
    y0 = m(x).clone()
    assert torch.equal(y0, m(m.decode_u8(x)))
    m.set_input_norm(*NORM)
    y1 = m(x).clone()
    assert m.last_input() == "u8_ring" and m.last_path()["conv1"]["form"] == "ring_u8"
    assert torch.equal(y1, m(m.decode_u8(x))) and not torch.equal(y1, y0)
    m.set_input_norm()
    y2 = m(x).clone()
    assert m.last_input() == "u8_ring" and m.last_path()["conv1"]["form"] == "ring_u8"
    assert torch.equal(y2, m(m.decode_u8(x))) and torch.equal(y2, y0) and not torch.equal(y2, y1)


# ----------------------------------------------------------------------------------------------------- 6. lanes
@pytest.mark.parametrize("N,off", [(5, 1), (5, 0), (6, 0)])
def test_lanes(cuda, shared, N, off):
    """Lane 1 takes images N // 2 .. N - 1. At N = 5 that is image 2 (an even offset), so the tensor itself starts
    one byte into its buffer there (off = 1: both lanes at odd addresses); at N = 6 lane 1 starts at image 3, an
    odd address in an aligned tensor."""
    one = shared
    configure(one, NORM)
    buf = torch.zeros(off + N * IMAGE, dtype=torch.uint8, device=cuda)
    x = buf[off:].view(N, 227, 227, 3)
    x.copy_(images(N, seed=N))
    two = AlexNetFull(weights(), device=cuda, max_batch=N, lanes=2, input_norm=NORM)
    lo = two.lane_bounds(N)[1]
    if (N, off) != (5, 0):
        assert x[lo:].data_ptr() % 2 == 1
    ref = one(x).clone()
    assert one.last_input() == "u8_ring" and one.last_path()["conv1"]["form"] == "ring_u8"
    assert torch.equal(ref, one(one.decode_u8(x)))
    y = torch.full_like(ref, float("nan"))
    two(x, out=y)
    torch.cuda.synchronize()
    assert two.last_input() == "u8_ring" and two.last_input(1) == "u8_ring"
    assert two.last_path(1)["conv1"]["form"] == "ring_u8"
    assert torch.equal(y, ref)
    y.fill_(float("nan"))
    two.forward_async(x, y)
    two.join()
    torch.cuda.synchronize()
    assert torch.equal(y, ref)
    # a change of the normalisation and of the route reaches the side lane
    two.set_input_norm()
    two.set_knob("bf16_u8", 0)
    one.set_input_norm()
    y.fill_(float("nan"))
    two(x, out=y)
    torch.cuda.synchronize()
    assert two.last_input(1) == "u8_decode" and two.last_path(1)["conv1"]["form"] == "ring_f32"
    assert torch.equal(y, one(x)) and not torch.equal(y, ref)
    two.close()


# -------------------------------------------------------------------------------------------- 7. stream capture
@pytest.mark.parametrize("u8", [1, 0])
def test_bytes_under_capture(cuda, u8):
    """After one warm-up forward (it allocates the decode workspace where one is needed) a captured forward
    replays to the same bits; the input record is host state, readable while the capture is open."""
    N = 2
    m = AlexNetFull(weights(), device=cuda, max_batch=N, input_norm=NORM, knobs={"bf16_u8": u8})
    x = images(N).to(cuda)
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
        assert m.last_input() == ("u8_ring" if u8 else "u8_decode")
        assert m.last_path()["conv1"]["form"] == ("ring_u8" if u8 else "ring_f32")
    y.fill_(float("nan"))
    g.replay()
    torch.cuda.synchronize()
    assert torch.equal(y, ref)
    m.close()


# ------------------------------------------------------------------------------------------------ 8. validation
def test_validation(cuda, shared):
    m = shared
    configure(m)
    ok = torch.zeros(1, 227, 227, 3, dtype=torch.uint8, device=cuda)
    with pytest.raises(ValueError):
        m(ok.to(torch.int8))
    with pytest.raises(ValueError):
        m(ok.cpu())
    with pytest.raises(ValueError):
        m(torch.zeros(1, 227, 3, 227, dtype=torch.uint8, device=cuda))
    with pytest.raises(ValueError):
        m(torch.zeros(1, 227, 3, 227, dtype=torch.uint8, device=cuda).permute(0, 1, 3, 2))  # not contiguous
    with pytest.raises(ValueError):
        m(ok, out=torch.zeros(1, m.classes, dtype=torch.float64, device=cuda))
    with pytest.raises(ValueError):
        m.set_input_norm(mean=1.0)
    with pytest.raises(ValueError):
        m.set_input_norm(NORM[0], (1.0, 0.0, 1.0))
    y = m(ok)  # and the model still runs, with the meaning it had
    assert m.last_input() == "u8_ring" and torch.equal(y, m(m.decode_u8(ok)))
