"""anx_full_run, the one C entry of the bf16 full model, driven raw (everything else goes through AlexNetFull).

On one tiny engine (10 classes, 4 images): every malformed call is refused with a message that names the entry
before anything is launched (last_input() stays None), and one well-formed call of each kind (forward on floats,
forward on bytes with mark, classify, classify over views) gives the bits of the Python API on a second engine with
the same weights."""
import ctypes as C

import pytest
import torch

from anx import _native as nat
from anx.models.alexnet_full import AlexNetFull, init_full_weights

pytestmark = pytest.mark.gpu

CLASSES, ROWS = 10, 4


@pytest.fixture(scope="module")
def engines(cuda):
    w = init_full_weights(83, classes=CLASSES)
    w["b_fc8"] = torch.linspace(-0.5, 0.5, CLASSES)
    raw, api = (AlexNetFull(w, classes=CLASSES, device=cuda, max_batch=ROWS) for _ in range(2))
    yield raw, api
    raw.close()
    api.close()


def test_malformed_calls_launch_nothing_then_each_kind_matches_the_python_api(cuda, engines):
    raw, api = engines
    g = torch.Generator().manual_seed(83)
    xf = (torch.randn(ROWS, 227, 227, 3, generator=g) * 3).to(cuda)
    xu = torch.randint(0, 256, (ROWS, 227, 227, 3), dtype=torch.uint8, generator=g).to(cuda)
    z = torch.full((ROWS, CLASSES), float("nan"), device=cuda)
    idx = torch.full((ROWS, 32), -1, dtype=torch.int32, device=cuda)  # room for the k no call may have
    prob = torch.full((ROWS, 32), float("nan"), device=cuda)
    stream = nat.stream_ptr(cuda)
    X, Z, I, P = xf.data_ptr(), z.data_ptr(), idx.data_ptr(), prob.data_ptr()

    def run(**fields):
        nat.call("anx_full_run", raw._h, C.byref(nat.FullCallC(**fields)), stream)

    assert raw.last_input() is None  # a fresh engine
    head = dict(x=X, rows=ROWS, idx=I, prob=P)
    malformed = {
        "k = 17": dict(head, k=17),
        "k = 11 of 10 classes": dict(head, k=11),
        "k = 0 with idx": dict(x=X, rows=ROWS, logits=Z, idx=I),
        "k = 0 with views": dict(x=X, rows=ROWS, logits=Z, views=2),
        "k = 5 without prob": dict(x=X, rows=ROWS, k=5, idx=I),
        "rows = 4 without x": dict(rows=ROWS, logits=Z),
        "k = 0 without logits": dict(x=X, rows=ROWS),
        "views = 33": dict(head, k=5, views=33),
        "3 rows of 2 views": dict(head, k=5, rows=3, views=2),
        "5 views in a chunk of 4": dict(head, k=5, rows=0, views=5),  # no rows: the chunk is the call's only flaw
        "rows = -1": dict(x=X, rows=-1, logits=Z),
    }
    for what, fields in malformed.items():
        with pytest.raises(nat.NativeError, match="anx_full_run"):
            run(**fields)
        assert raw.last_input() is None, what  # nothing was launched
    torch.cuda.synchronize()
    assert torch.isnan(z).all() and (idx == -1).all() and torch.isnan(prob).all()  # and nothing written

    def bits(t):
        return t.contiguous().view(torch.int32)

    # forward on floats
    run(x=X, rows=ROWS, logits=Z)
    torch.cuda.synchronize()
    assert raw.last_input() == "f32" and raw.last_head() is None
    assert torch.equal(bits(z), bits(api.forward(xf)))
    # forward on bytes with mark; the mark can then be waited for
    z.fill_(float("nan"))
    run(x=xu.data_ptr(), u8=1, rows=ROWS, logits=Z, mark=1)
    nat.call("anx_full_wait_mark", raw._h, stream)
    torch.cuda.synchronize()
    want = api.forward(xu)
    assert raw.last_input() == api.last_input() and torch.equal(bits(z), bits(want))
    # classify, k = 3, no logits taken
    k = 3
    i3, p3 = idx[:, :k].contiguous(), prob[:, :k].contiguous()
    run(x=X, rows=ROWS, k=k, idx=i3.data_ptr(), prob=p3.data_ptr())
    torch.cuda.synchronize()
    wi, wp = api.classify(xf, k)
    assert raw.last_head() == api.last_head() is not None
    assert torch.equal(i3, wi) and torch.equal(bits(p3), bits(wp))
    # views: 4 rows are 2 images of 2 views; with the logits
    iv = torch.full((2, k), -1, dtype=torch.int32, device=cuda)
    pv = torch.full((2, k), float("nan"), device=cuda)
    z.fill_(float("nan"))
    run(x=X, rows=ROWS, views=2, k=k, idx=iv.data_ptr(), prob=pv.data_ptr(), logits=Z)
    torch.cuda.synchronize()
    wi, wp, wz = api.classify(xf, k, views=2, return_logits=True)
    assert raw.last_head() == api.last_head() is not None
    assert torch.equal(iv, wi) and torch.equal(bits(pv), bits(wp)) and torch.equal(bits(z), bits(wz))
