"""Mirrored outputs and shared sources of anx.ops.resize_crop_u8 on the gfx950 kernel: the batches of
resize_flip_cases.py (every kernel instantiation, both tap forms, out at byte offsets 1 and 15, mixed flags), the
flipped bytes against the host definition's, sources with repeats, and null flags against the old entry point."""
import numpy as np
import pytest
import torch

from anx import _native as nat
from anx import ops
from anx.ops import resize_crop_u8, ten_crop_boxes
from resize_flip_cases import FLIPS, OH, OWS, SCALES, batch, check_batch

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("scale", SCALES)
@pytest.mark.parametrize("OW", OWS)
def test_flipped_outputs_are_the_mirror_image(cuda, OW, scale):
    check_batch(resize_crop_u8, OW, scale, cuda)


@pytest.mark.parametrize("OW,scale", [(86, 1.47), (257, 16.0)])
def test_flipped_bytes_equal_the_host_definition(cuda, OW, scale):
    images, boxes = batch(OW, scale)
    want = resize_crop_u8(images, (OH, OW), boxes=boxes, flips=list(FLIPS))
    got = resize_crop_u8([im.to(cuda) for im in images], (OH, OW), boxes=boxes, flips=list(FLIPS))
    assert torch.equal(got.cpu(), want)


def test_source_with_repeats_equals_repeated_images(cuda):
    images, boxes = batch(85, 1.47)
    images = [im.to(cuda) for im in images]
    source = [2, 0, 0, 1, 2, 2]
    flips = [False, True, False, True, True, False]
    per_output = [boxes[s] for s in source]
    want = resize_crop_u8([images[s] for s in source], (OH, 85), boxes=per_output, flips=flips)
    got = resize_crop_u8(images, (OH, 85), boxes=per_output, flips=flips, source=source)
    assert got.shape == (6, OH, 85, 3) and torch.equal(got, want)


def test_ten_views_of_one_image(cuda):
    g = torch.Generator().manual_seed(3)
    im = torch.randint(0, 256, (375, 500, 3), dtype=torch.uint8, generator=g)
    boxes, flips = ten_crop_boxes(375, 500)
    want = resize_crop_u8([im], 227, boxes=boxes, flips=flips, source=[0] * 10)
    got = resize_crop_u8([im.to(cuda)], 227, boxes=boxes, flips=flips, source=[0] * 10)
    assert torch.equal(got.cpu(), want)
    assert torch.equal(got[5:], torch.flip(got[:5], dims=[2]))


def test_null_flags_are_the_old_entry_point(cuda):
    images, boxes = batch(227, 1.47)
    images = [im.to(cuda) for im in images]
    geo, _ = ops._image_geometry(images)
    host = torch.from_numpy(ops._image_descs(geo, OH, 227, 256, boxes).view(np.uint8))
    want = resize_crop_u8(images, (OH, 227), boxes=boxes)  # flips=None: anx_resize_crop_u8
    got = torch.full_like(want, 0xAA)
    ddev = host.to(cuda)
    with torch.cuda.device(cuda):
        nat.call("anx_resize_crop_u8_flip", ddev.data_ptr(), host.data_ptr(), None, None, len(images),
                 got.data_ptr(), OH, 227, nat.stream_ptr(cuda))
    torch.cuda.synchronize()
    assert torch.equal(got, want)
