"""AlexNetFull.forward_images / classify_images: byte images of any size in front of the bf16 full AlexNet.

Every check is a bit identity against the same model's byte path: forward_images(images) equals
forward(anx.ops.resize_crop_u8(images)) and classify_images equals classify of the same (indices, probabilities,
logits), on one lane and two, with and without input_norm. The resize kernel itself is held to the host definition by
test_resize_crop_gpu.py. Each model starts at max_batch 4 and sees 3 images first, then 17, so the second call grows
the byte workspace (and the engine). classes = 10 keeps the models small."""
import functools

import pytest
import torch

from anx.models.alexnet_full import AlexNetFull, init_full_weights
from anx.ops import resize_crop_u8

pytestmark = pytest.mark.gpu

SIZES = [(375, 500), (256, 256), (40, 37)]
NORM = ((123.7, 116.3, 103.5), (58.4, 57.1, 57.4))


@functools.lru_cache(maxsize=None)
def weights():
    return init_full_weights(61, classes=10)


def mixed_images(n, dev, seed):
    g = torch.Generator().manual_seed(seed)
    return [torch.randint(0, 256, (*SIZES[i % 3], 3), dtype=torch.uint8, generator=g).to(dev) for i in range(n)]


def bits(t):
    return t.cpu().contiguous().view(torch.int32)


def check(m, imgs, resize=256):
    x = resize_crop_u8(imgs, 227, resize)
    assert x.shape == (len(imgs), 227, 227, 3)
    want = m.forward(x)
    y = torch.full_like(want, float("nan"))
    got = m.forward_images(imgs, out=y, resize=resize)
    assert got is y and torch.equal(bits(got), bits(want))
    assert m.last_input() == "u8_ring"
    wi, wp, wz = m.classify(x, 5, return_logits=True)
    gi, gp, gz = m.classify_images(imgs, 5, resize=resize, return_logits=True)
    assert torch.equal(gi.cpu(), wi.cpu()) and torch.equal(bits(gp), bits(wp)) and torch.equal(bits(gz), bits(wz))
    assert torch.equal(bits(gz), bits(want))
    gi2, gp2 = m.classify_images(imgs, 3, resize=resize)
    assert torch.equal(gi2.cpu(), wi.cpu()[:, :3]) and torch.equal(bits(gp2), bits(wp)[:, :3])
    assert m.last_input() == "u8_ring" and m.last_head() is not None


@pytest.mark.parametrize("lanes", [1, 2])
def test_images_equal_the_byte_path(cuda, lanes):
    m = AlexNetFull(weights(), classes=10, device=cuda, max_batch=4, lanes=lanes)
    try:
        check(m, mixed_images(3, cuda, 1))
        check(m, mixed_images(17, cuda, 2))  # more than the first call: the workspace grows
        check(m, mixed_images(3, cuda, 3), resize=None)  # whole images, after the large batch
        m.set_input_norm(*NORM)
        check(m, mixed_images(17, cuda, 4))
        # one [N,H,W,3] tensor instead of a list
        x = torch.stack(mixed_images(9, cuda, 5)[::3])
        assert torch.equal(bits(m.forward_images(x)), bits(m.forward_images(list(x.unbind(0)))))
        with pytest.raises(ValueError):
            m.forward_images([im.cpu() for im in mixed_images(2, cuda, 6)])
    finally:
        m.close()


def test_input_norm_from_the_constructor(cuda):
    m = AlexNetFull(weights(), classes=10, device=cuda, max_batch=4, input_norm=NORM)
    plain = AlexNetFull(weights(), classes=10, device=cuda, max_batch=4)
    try:
        imgs = mixed_images(3, cuda, 7)
        check(m, imgs)
        assert not torch.equal(bits(m.forward_images(imgs)), bits(plain.forward_images(imgs)))  # the norm is applied
    finally:
        m.close()
        plain.close()
