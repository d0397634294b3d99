"""The resize + crop kernel (resize_crop_u8.hip through anx.ops.resize_crop_u8 on CUDA tensors) against the host
definition (the same op on CPU tensors): equal BIT FOR BIT, since both compute the same integers. Every case of
resize_crop_cases.py (1-pixel images, 34 taps, OW = 1, the widest box and output), batches of images of different
sizes in one launch, sources with a pitch from every byte alignment, and an output off the 16-B grid."""
import pytest
import torch

from anx.ops import center_box, resize_crop_u8
from resize_crop_cases import CASES, geometry, host_result, image, make_image

pytestmark = pytest.mark.gpu

MIXED = [(40, 37), (64, 48), (256, 256), (229, 700), (5, 9)]


@pytest.mark.parametrize("name,fill", CASES)
def test_case_equals_host(cuda, name, fill):
    _, ohw, box = geometry(name)
    got = resize_crop_u8([image(name, fill).to(cuda)], size=ohw, boxes=[box])
    assert got.is_cuda and got.dtype == torch.uint8
    assert torch.equal(got[0].cpu(), host_result(name, fill))


def test_257_images_of_five_sizes_in_one_launch(cuda):
    pool = [make_image(h, w, "random", 50 + i) for i, (h, w) in enumerate(MIXED * 2)]  # two images per size
    want = resize_crop_u8(pool)  # host, default centre boxes
    dev = [p.to(cuda) for p in pool]
    got = resize_crop_u8([dev[i % len(dev)] for i in range(257)]).cpu()
    assert got.shape == (257, 227, 227, 3)
    for i in range(257):  # an image's bytes do not depend on its position in the batch or on its neighbours
        assert torch.equal(got[i], want[i % len(pool)]), i


def test_three_images_to_12x7(cuda):
    imgs = [make_image(h, w, "checker", 70 + i) for i, (h, w) in enumerate([(5, 9), (64, 48), (40, 37)])]
    boxes = [center_box(*im.shape[:2], resize=None) for im in imgs]  # 64 x 48 -> 12 x 7 is 5.3x / 6.9x
    want = resize_crop_u8(imgs, size=(12, 7), boxes=boxes)
    got = resize_crop_u8([im.to(cuda) for im in imgs], size=(12, 7), boxes=boxes)
    assert torch.equal(got.cpu(), want)


def test_column_slices_from_every_byte_alignment(cuda):
    H, W = 75, 100
    big = make_image(H, 3 * W, "random", 90)
    bigd = big.to(cuda)
    seen = set()
    for c0 in (0, 1, 2, 3, 5, 16, 21):
        view = bigd[:, c0:c0 + W]  # pitch 9 W bytes, base 3 c0 bytes into a 16-B aligned allocation
        assert not view.is_contiguous() and view.stride(0) == 9 * W
        seen.add(view.data_ptr() % 4)
        want = resize_crop_u8([big[:, c0:c0 + W].contiguous()], size=(40, 33), resize=None)
        assert torch.equal(resize_crop_u8([view], size=(40, 33), resize=None).cpu(), want), c0
    assert seen == {0, 1, 2, 3}
    # several such slices, plus a compact image, in one launch
    views = [bigd[:, c0:c0 + W] for c0 in (1, 2, 3, 7)] + [bigd]
    want = resize_crop_u8([v.cpu().contiguous() for v in views], size=64, resize=None)
    assert torch.equal(resize_crop_u8(views, size=64, resize=None).cpu(), want)


def test_output_one_byte_off_a_16_byte_boundary(cuda):
    imgs = [make_image(h, w, "random", 95 + i) for i, (h, w) in enumerate([(64, 48), (40, 37), (256, 256)])]
    want = resize_crop_u8(imgs)
    n = want.numel()
    buf = torch.full((n + 32,), 0xA5, dtype=torch.uint8, device=cuda)
    assert buf.data_ptr() % 16 == 0
    out = buf[1:1 + n].view(want.shape)
    got = resize_crop_u8([im.to(cuda) for im in imgs], out=out)
    assert got.data_ptr() == buf.data_ptr() + 1
    assert torch.equal(got.cpu(), want)
    assert int(buf[0]) == 0xA5 and bool((buf[1 + n:] == 0xA5).all())  # nothing written around it
    # and short odd output rows (OW = 7: 21-byte rows) from 3 bytes off the grid
    want = resize_crop_u8(imgs, size=(12, 7))
    out = buf[3:3 + want.numel()].view(want.shape)
    buf.fill_(0x5A)
    assert torch.equal(resize_crop_u8([im.to(cuda) for im in imgs], size=(12, 7), out=out).cpu(), want)
    assert bool((buf[:3] == 0x5A).all()) and bool((buf[3 + want.numel():] == 0x5A).all())


def test_list_and_tensor_input_agree(cuda):
    x = torch.stack([make_image(61, 83, "random", 120 + i) for i in range(5)])
    want = resize_crop_u8(x)
    xd = x.to(cuda)
    a = resize_crop_u8(list(xd.unbind(0)))
    b = resize_crop_u8(xd)
    assert torch.equal(a, b) and torch.equal(a.cpu(), want)
    assert resize_crop_u8([], size=5).shape == (0, 5, 5, 3)
