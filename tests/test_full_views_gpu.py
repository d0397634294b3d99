"""AlexNetFull.classify(views=V) and classify_images(views="ten"): the view-averaging head on top of the bf16
full-AlexNet forward.

Every check is a bit identity against the same model: classify(x, k, views=V) equals
anx.ops.softmax_topk_views(forward(x), V, k) (the kernel test_softmax_topk_views_gpu.py holds to fp64) on both head
routes (knob bf16_head: 1 = the view kernel reduces FC8's split-K slabs itself, 0 = the reduce writes the logits
first), for float and byte input; two lanes equal one lane wherever their forwards do, and never cut an image;
classify_images(views="ten") equals classify of the ten crops made by hand; views=None is the call as it was.
Weights carry nonzero biases that are no bf16 values; outputs are pre-filled (-1 / NaN) so equal bits are never
left-overs."""
import functools

import pytest
import torch

from anx.models.alexnet_full import AlexNetFull, init_full_weights
from anx.ops import resize_crop_u8, softmax_topk_views, ten_crop_boxes

pytestmark = pytest.mark.gpu

LAYERS = ("conv1", "conv2", "conv3", "conv4", "conv5", "fc6", "fc7", "fc8")
MAX_ROWS = 260


@functools.lru_cache(maxsize=None)
def weights():
    w = init_full_weights(71)
    g = torch.Generator().manual_seed(1071)
    for name in LAYERS:
        b = torch.randn(w["b_" + name].shape, generator=g) * 0.1
        b.view(torch.int32).bitwise_or_(1)  # low mantissa bit set: no bias is a bf16 value
        w["b_" + name] = b
    return w


def rows(n, dtype, seed=17):
    g = torch.Generator().manual_seed(seed + n)
    if dtype == torch.uint8:
        return torch.randint(0, 256, (n, 227, 227, 3), dtype=torch.uint8, generator=g)
    return torch.randn(n, 227, 227, 3, generator=g) * 3


@pytest.fixture(scope="module")
def models(cuda):
    made = {}

    def get(lanes=1):
        if lanes not in made:
            made[lanes] = AlexNetFull(weights(), device=cuda, max_batch=MAX_ROWS, lanes=lanes)
        return made[lanes]

    yield get
    for m in made.values():
        m.close()


def bits(t):
    return t.contiguous().view(torch.int32)


def fresh(N, k, cuda):
    return torch.full((N, k), -1, dtype=torch.int32, device=cuda), torch.full((N, k), float("nan"), device=cuda)


def assert_same_head(got, want, what):
    assert torch.equal(got[0], want[0]), f"indices {what}"
    assert torch.equal(bits(got[1]), bits(want[1])), f"probabilities {what}"


@pytest.mark.parametrize("dtype", [torch.float32, torch.uint8], ids=["float", "bytes"])
@pytest.mark.parametrize("N,V", [(2, 10), (26, 10)])
def test_classify_views_is_the_view_head_of_forward(cuda, models, N, V, dtype):
    m = models()
    m.set_knob("bf16_head", 1)
    x = rows(N * V, dtype).to(cuda)
    y = m(x).clone()
    path = m.last_path()
    # 260 rows are one image per workgroup of the ring Conv1, which then has pool1 in its epilogue; 20 are not
    form = ("ring_u8" if dtype == torch.uint8 else "ring_f32") + ("_pool" if N * V >= 260 else "")
    assert path["conv1"]["form"] == form, path
    k = 5
    want = softmax_topk_views(y, V, k)
    for head, route in ((1, "slabs"), (0, "logits")):
        m.set_knob("bf16_head", head)
        m(x[:V])  # a plain forward in between: nothing may be a left-over
        assert m.last_head() is None
        out = fresh(N, k, cuda)
        got = m.classify(x, k, views=V, out=out)
        torch.cuda.synchronize()
        what = f"N={N} V={V} {dtype} bf16_head={head}"
        assert m.last_head() == route, what
        assert m.last_path() == path, what
        assert got[0] is out[0] and got[1] is out[1] and tuple(got[0].shape) == (N, k)
        assert_same_head(got, want, what)
        gi, gp, gz = m.classify(x, k, views=V, return_logits=True)
        assert m.last_head() == route, what
        assert tuple(gz.shape) == (N * V, 1000) and torch.equal(bits(gz), bits(y)), f"logits {what}"
        assert_same_head((gi, gp), want, f"with logits {what}")
    m.set_knob("bf16_head", 1)
    assert torch.equal(bits(m(x)), bits(y)), "forward after classify"


def test_lanes_split_on_image_boundaries(cuda, models):
    one, two = models(1), models(2)
    N, V, k = 3, 10, 5
    for dtype in (torch.float32, torch.uint8):
        x = rows(N * V, dtype, seed=29).to(cuda)
        bounds = two.lane_bounds(N)
        assert bounds == [0, 1, 3]  # images: the lanes run rows 0 .. 10 and 10 .. 30
        y1 = one(x).clone()
        y2 = torch.cat([one(x[lo * V:hi * V]).clone() for lo, hi in zip(bounds, bounds[1:])])  # what each lane computes
        want = one.classify(x, k, views=V)
        got = two.classify(x, k, views=V, out=fresh(N, k, cuda))
        torch.cuda.synchronize()
        assert two.last_head() == "slabs" and two.last_head(1) == "slabs"
        # whole images per lane: each lane's answer is the view head of its own rows' logits
        assert_same_head(got, softmax_topk_views(y2, V, k), f"two lanes {dtype}")
        print(f"{dtype}: forward logits of one launch of 30 rows equal those of 10 + 20: {torch.equal(bits(y1), bits(y2))}")
        assert_same_head(got, want, f"two lanes against one {dtype}")
        out = fresh(N, k, cuda)
        ret = two.classify_async(x, out[0], out[1], k, views=V)
        two.join()
        torch.cuda.synchronize()
        assert ret[0] is out[0] and ret[1] is out[1]
        assert_same_head(out, got, f"classify_async + join {dtype}")


def test_ten_views_of_images(cuda, models):
    m = models()
    g = torch.Generator().manual_seed(41)
    images = [torch.randint(0, 256, (H, W, 3), dtype=torch.uint8, generator=g).to(cuda)
              for H, W in ((375, 500), (256, 256), (227, 300))]
    boxes, flips, source = [], [], []
    for i, im in enumerate(images):
        b, f = ten_crop_boxes(im.shape[0], im.shape[1])
        boxes, flips, source = boxes + b, flips + f, source + [i] * 10
    x = resize_crop_u8(images, 227, boxes=boxes, flips=flips, source=source)
    assert tuple(x.shape) == (30, 227, 227, 3)
    want = m.classify(x, 5, views=10, return_logits=True)
    got = m.classify_images(images, 5, views="ten", return_logits=True)
    torch.cuda.synchronize()
    assert tuple(got[0].shape) == (3, 5) and tuple(got[2].shape) == (30, 1000)
    assert_same_head(got, want, "ten views")
    assert torch.equal(bits(got[2]), bits(want[2]))
    assert m.last_input() == "u8_ring" and m.last_head() == "slabs"
    assert_same_head(m.classify_images(images, 5, views="ten"), want, "ten views, no logits")
    # the defaults are the calls as they were
    plain = resize_crop_u8(images)
    assert_same_head(m.classify_images(images, 5), m.classify(plain, 5), "views=None")
    assert_same_head(m.classify_images(images, 5, views=None), m.classify(plain, 5, views=None), "views=None, named")
    with pytest.raises(ValueError):
        m.classify_images(images, 5, views="five")


def test_views_are_validated(cuda, models):
    m = models()
    x = rows(30, torch.uint8).to(cuda)
    for bad in (33, 0, 4, 2.0, True, "ten"):
        with pytest.raises(ValueError):
            m.classify(x, 5, views=bad)
    with pytest.raises(ValueError):
        m.classify(x, 5, views=10, out=fresh(30, 5, cuda))  # outputs are per image
    with pytest.raises(ValueError):
        m.classify_async(x, *fresh(3, 5, cuda), 5, views=7)
    assert m.classify(x, 5, views=30)[0].shape == (1, 5)
