"""AlexNetFull.evaluate / evaluate_async / evaluate_images: the evaluation head on top of the bf16 full-AlexNet forward.

Every check is a bit identity against the same model: evaluate(x, y, k, views=V) equals
anx.ops.softmax_eval(forward(x), y, k, views=V) (the kernel test_softmax_eval_gpu.py holds to fp64) on both head routes
(knob bf16_head: 1 = the head kernel reduces FC8's split-K slabs itself, 0 = the reduce writes the logits first), for
float and byte input, with and without views; two lanes add into the same counters; launch chunks advance the
per-image arrays and share the counters; evaluate_images(views="ten") equals evaluate of the ten crops made by hand.
Weights carry nonzero biases that are no bf16 values (test_full_views_gpu.py's); outputs are pre-filled so equal bits
are never left-overs."""
import functools

import pytest
import torch

from anx.models.alexnet_full import AlexNetFull, init_full_weights
from anx.ops import eval_summary, resize_crop_u8, softmax_eval, softmax_topk, ten_crop_boxes
from softmax_eval_cases import expected_confusion, expected_stats, labels_for

pytestmark = pytest.mark.gpu

LAYERS = ("conv1", "conv2", "conv3", "conv4", "conv5", "fc6", "fc7", "fc8")
MAX_ROWS = 260
CLASSES = 1000


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

    def get(lanes=1, max_batch=MAX_ROWS):
        if (lanes, max_batch) not in made:
            made[lanes, max_batch] = AlexNetFull(weights(), device=cuda, max_batch=max_batch, lanes=lanes)
        return made[lanes, max_batch]

    yield get
    for m in made.values():
        m.close()


def bits(t):
    return t.contiguous().view(torch.int32)


def same(a, b):
    return all(torch.equal(bits(p), bits(q)) for p, q in zip(a, b))


def fresh(N, cuda):
    return (torch.full((N,), -9, dtype=torch.int32, device=cuda), torch.full((N,), float("nan"), device=cuda),
            torch.full((N,), -9, dtype=torch.int32, device=cuda))


def counters(cuda):
    return torch.zeros(4, dtype=torch.int64, device=cuda), torch.zeros(CLASSES, CLASSES, dtype=torch.int32, device=cuda)


def labels_of(y, V, seed, cuda):
    """Labels for the logits y: even images the top class, odd images random, the last image ignored if there are many."""
    lab = labels_for(y.cpu(), V or 0, seed)
    if lab.shape[0] > 4:
        lab[-1] = -1
    return lab.to(cuda)


@pytest.mark.parametrize("dtype", [torch.float32, torch.uint8], ids=["float", "bytes"])
@pytest.mark.parametrize("N,V", [(2, None), (26, None), (2, 10), (26, 10)])
def test_evaluate_is_the_evaluation_head_of_forward(cuda, models, N, V, dtype):
    m = models()
    m.set_knob("bf16_head", 1)
    x = rows(N * (V or 1), dtype).to(cuda)
    y = m(x).clone()
    path = m.last_path()
    k = 5
    lab = labels_of(y, V, N, cuda)
    ws, wc = counters(cuda)
    want = softmax_eval(y, lab, k, views=V, stats=ws, confusion=wc)
    ci, cp = m.classify(x, k, views=V)
    ci, cp = ci.clone(), cp.clone()
    for head, route in ((1, "slabs"), (0, "logits")):
        m.set_knob("bf16_head", head)
        m(x[:V or 1])  # a plain forward in between: nothing may be a left-over
        assert m.last_head() is None
        out = fresh(N, cuda)
        stats, conf = counters(cuda)
        got = m.evaluate(x, lab, k, views=V, stats=stats, confusion=conf, out=out)
        torch.cuda.synchronize()
        what = f"N={N} V={V} {dtype} bf16_head={head}"
        assert m.last_head() == route, what
        assert m.last_path() == path, what
        assert all(a is b for a, b in zip(got, out)) and tuple(got[0].shape) == (N,)
        assert same(got, want), what
        assert torch.equal(stats, ws) and torch.equal(conf, wc), what
        assert stats.tolist() == expected_stats(got[0], got[1], k), what
        assert torch.equal(conf.cpu(), expected_confusion(lab, got[2], CLASSES)), what
        assert torch.equal(got[2], ci[:, 0]), f"pred is not classify's first class: {what}"
        # without outputs and counters given: allocated, and the same
        assert same(m.evaluate(x, lab, k, views=V), want), f"allocated outputs {what}"
        s = eval_summary(stats, k)
        assert s["count"] == int((lab >= 0).sum()) and 0.0 <= s["topk_error"] <= s["top1_error"] <= 0.5
    m.set_knob("bf16_head", 1)
    assert torch.equal(bits(m(x)), bits(y)), "forward after evaluate"
    assert same(m.classify(x, k, views=V), (ci, cp)), "classify after evaluate"


@pytest.mark.parametrize("N,V", [(5, None), (3, 10)])
def test_two_lanes_add_into_the_same_counters(cuda, models, N, V):
    one, two = models(1), models(2)
    v, k = V or 1, 5
    for dtype in (torch.float32, torch.uint8):
        x = rows(N * v, dtype, seed=29).to(cuda)
        bounds = two.lane_bounds(N)
        y1 = one(x).clone()
        y2 = torch.cat([one(x[lo * v:hi * v]).clone() for lo, hi in zip(bounds, bounds[1:])])  # what each lane computes
        lab = labels_of(y1, V, 3, cuda)
        s1, c1 = counters(cuda)
        want = one.evaluate(x, lab, k, views=V, stats=s1, confusion=c1)
        s2, c2 = counters(cuda)
        got = two.evaluate(x, lab, k, views=V, stats=s2, confusion=c2, out=fresh(N, cuda))
        torch.cuda.synchronize()
        assert two.last_head() == "slabs" and two.last_head(1) == "slabs"
        # whole images per lane: each lane's answer is the evaluation head of its own rows' logits
        assert same(got, softmax_eval(y2, lab, k, views=V)), f"two lanes {dtype}"
        assert s2.tolist() == expected_stats(got[0], got[1], k), f"both lanes' images are counted {dtype}"
        assert torch.equal(c2.cpu(), expected_confusion(lab, got[2], CLASSES))
        agree = torch.equal(bits(y1), bits(y2))
        print(f"{dtype}: forward logits of one launch equal those of the lanes' launches: {agree}")
        if agree:
            assert same(got, want) and torch.equal(s2, s1) and torch.equal(c2, c1), f"two lanes against one {dtype}"
        out = fresh(N, cuda)
        s3, c3 = counters(cuda)
        ret = two.evaluate_async(x, lab, k, views=V, stats=s3, confusion=c3, out=out)
        two.join()
        torch.cuda.synchronize()
        assert all(a is b for a, b in zip(ret, out))
        assert same(out, got) and torch.equal(s3, s2) and torch.equal(c3, c2), f"evaluate_async + join {dtype}"


def test_launch_chunks_advance_the_outputs_and_share_the_counters(cuda, models):
    """An engine of 4 images is handed 10 rows (views = 2: 5 images, launch chunks of 2 images) through _launch, which
    does not grow it. Per-image outputs and counters equal one softmax_eval call on the chunks' logits."""
    m = models(1, 4)
    V, k = 2, 5
    x = rows(10, torch.uint8, seed=5).to(cuda)
    y = torch.cat([m(x[lo:lo + 4]).clone() for lo in (0, 4, 8)])
    lab = labels_of(y, V, 11, cuda)
    ws, wc = counters(cuda)
    want = softmax_eval(y, lab, k, views=V, stats=ws, confusion=wc)
    stats, conf = counters(cuda)
    head = m._check_eval(x, lab, k, V, stats, conf, fresh(5, cuda))
    assert m._cap == 4
    m._launch(x, None, head, None, False)
    torch.cuda.synchronize()
    assert m._cap == 4 and m.last_head() == "slabs"
    assert same((head.rank, head.nll, head.pred), want)
    assert torch.equal(stats, ws) and torch.equal(conf, wc) and int(stats[0]) == 4  # the last image is ignored


def test_evaluate_images_ten_views(cuda, models):
    m = models()
    g = torch.Generator().manual_seed(41)
    images = [torch.randint(0, 256, (H, W, 3), dtype=torch.uint8, generator=g).to(cuda)
              for H, W in ((375, 500), (256, 256), (227, 300))]
    boxes, flips, source = [], [], []
    for i, im in enumerate(images):
        b, f = ten_crop_boxes(im.shape[0], im.shape[1])
        boxes, flips, source = boxes + b, flips + f, source + [i] * 10
    x = resize_crop_u8(images, 227, boxes=boxes, flips=flips, source=source)
    first = m.classify(x, 5, views=10)[0][:, 0].clone()
    lab = torch.stack([first[0], (first[1] + 1) % CLASSES, first[2]]).to(torch.int32)
    ws, wc = counters(cuda)
    want = m.evaluate(x, lab, 5, views=10, stats=ws, confusion=wc)
    stats, conf = counters(cuda)
    got = m.evaluate_images(images, lab, 5, views="ten", stats=stats, confusion=conf)
    torch.cuda.synchronize()
    assert m.last_input() == "u8_ring" and m.last_head() == "slabs"
    assert same(got, want) and torch.equal(stats, ws) and torch.equal(conf, wc)
    assert got[0][0] == 0 and got[0][2] == 0 and got[0][1] > 0 and stats[:2].tolist() == [3, 2]
    # views=None: the centre crop, ranked by logit
    plain = resize_crop_u8(images)
    assert same(m.evaluate_images(images, lab, 5), m.evaluate(plain, lab, 5))
    assert same(m.evaluate(plain, lab, 5), softmax_eval(m(plain), lab, 5))
    assert torch.equal(m.evaluate(plain, lab, 5)[2], softmax_topk(m(plain), 1)[0][:, 0])
    with pytest.raises(ValueError):
        m.evaluate_images(images, lab, 5, views="five")


def test_arguments_are_validated(cuda, models):
    m = models()
    x = rows(20, torch.uint8).to(cuda)
    lab = torch.zeros(20, dtype=torch.int32, device=cuda)
    bad = [dict(labels=lab.long()), dict(labels=lab.float()), dict(labels=lab[:19]), dict(labels=lab.cpu()),
           dict(labels=torch.zeros(40, dtype=torch.int32, device=cuda)[::2]), dict(labels=None), dict(k=0), dict(k=17),
           dict(k=2.0), dict(views=3), dict(views=33), dict(views="ten"),
           dict(views=10),  # labels are per image: 2 images take 2 labels
           dict(stats=torch.zeros(4, dtype=torch.int32, device=cuda)), dict(stats=torch.zeros(4, dtype=torch.int64)),
           dict(confusion=torch.zeros(CLASSES, CLASSES, dtype=torch.int64, device=cuda)),
           dict(confusion=torch.zeros(CLASSES, 10, dtype=torch.int32, device=cuda)),
           dict(out=fresh(19, cuda)), dict(out=fresh(20, cuda)[:2]),
           dict(out=(lab.clone(), lab.clone(), lab.clone()))]
    for change in bad:
        with pytest.raises(ValueError):
            m.evaluate(**{**dict(x=x, labels=lab, k=5), **change})
    with pytest.raises(ValueError):
        m.evaluate(x.cpu(), lab, 5)
    with pytest.raises(ValueError):
        m.evaluate_async(x, lab[:3], 5)
    r, n, p = m.evaluate(x, lab[:2].contiguous(), 5, views=10)
    assert tuple(r.shape) == tuple(n.shape) == tuple(p.shape) == (2,)
