"""Mirrored outputs and shared sources of anx.ops.resize_crop_u8 on the host definition (CPU tensors), the ten-crop
boxes, and the C ABI's flag checks. resize_flip_cases.py holds the batches; test_resize_flip_gpu.py runs the same
on the kernel."""
import numpy as np
import pytest
import torch

from anx import _native as nat
from anx import ops
from anx.ops import center_box, resize_crop_u8, ten_crop_boxes
from resize_flip_cases import OH, OWS, SCALES, batch, check_batch

CPU = torch.device("cpu")


@pytest.mark.parametrize("scale", SCALES)
@pytest.mark.parametrize("OW", OWS)
def test_flipped_outputs_are_the_mirror_image(OW, scale):
    check_batch(resize_crop_u8, OW, scale, CPU)


def test_source_with_repeats_equals_repeated_images():
    images, boxes = batch(85, 1.47)
    source = [2, 0, 0, 1, 2, 2]
    flips = [False, True, False, True, True, False]
    per_output = [boxes[s] for s in source]
    want = resize_crop_u8([images[s] for s in source], (OH, 85), boxes=per_output, flips=flips)
    got = resize_crop_u8(images, (OH, 85), boxes=per_output, flips=flips, source=source)
    assert got.shape == (6, OH, 85, 3) and torch.equal(got, want)
    # default boxes are per output too (center_box of each output's source), and an empty source is no output
    assert torch.equal(resize_crop_u8(images, 9, source=source), resize_crop_u8([images[s] for s in source], 9))
    assert resize_crop_u8(images, 9, source=[]).shape == (0, 9, 9, 3)
    one = torch.stack([images[0], images[0]])  # a [N,H,W,3] tensor as the source set
    assert torch.equal(resize_crop_u8(one, 9, source=[1, 1, 0]), resize_crop_u8(one[[1, 1, 0]], 9))


def test_null_flags_are_the_old_entry_point():
    images, boxes = batch(227, 1.47)
    geo, _ = ops._image_geometry(images)
    desc = torch.from_numpy(ops._image_descs(geo, OH, 227, 256, boxes).view(np.uint8))
    want = resize_crop_u8(images, (OH, 227), boxes=boxes)  # flips=None: anx_cpu_resize_crop_u8
    got = torch.full_like(want, 0xAA)
    nat.call("anx_cpu_resize_crop_u8_flip", desc.data_ptr(), None, len(images), got.data_ptr(), OH, 227)
    assert torch.equal(got, want)


def test_python_argument_checks():
    images, boxes = batch(2, 1.0)
    for bad in (dict(flips=[True, False]), dict(flips=[1, 0, 1]), dict(flips=[True, False, None]),
                dict(flips=torch.tensor([1, 0, 1])), dict(flips=np.array([1, 0, 1])), dict(flips=True),
                dict(flips=torch.tensor([[True, False, True]])),
                dict(source=[0, 1, 3]), dict(source=[0, -1, 1]), dict(source=[0, 1]), dict(source=[0.5, 1, 2]),
                dict(source=[0, 1, 2, 2]), dict(source=[0, 0, 0, 0], flips=[True] * 3)):
        with pytest.raises(ValueError):
            resize_crop_u8(images, (OH, 2), boxes=boxes, **bad)
    ok = resize_crop_u8(images, (OH, 2), boxes=boxes, flips=np.array([True, False, True]), source=[0, 1, 2])
    assert ok.shape == (3, OH, 2, 3)


TEN = {(375, 500): (333, [(0, 0), (0, 334), (84, 0), (84, 334), (42, 167)]),
       (256, 256): (227, [(0, 0), (0, 58), (58, 0), (58, 58), (29, 29)]),
       (227, 300): (201, [(0, 0), (0, 198), (52, 0), (52, 198), (26, 99)])}


@pytest.mark.parametrize("hw", sorted(TEN))
def test_ten_crop_boxes(hw):
    H, W = hw
    b, origins = TEN[hw]
    boxes, flips = ten_crop_boxes(H, W)
    assert center_box(H, W)[2:] == (b, b)
    assert boxes == [(y, x, b, b) for y, x in origins] * 2
    assert flips == [False] * 5 + [True] * 5
    assert boxes[4] == center_box(H, W)
    # every box passes the op's own checks, and the mirrored five are the mirror images of the first five
    g = torch.Generator().manual_seed(H)
    im = torch.randint(0, 256, (H, W, 3), dtype=torch.uint8, generator=g)
    out = resize_crop_u8([im], 227, boxes=boxes, flips=flips, source=[0] * 10)
    assert torch.equal(out[5:], torch.flip(out[:5], dims=[2]))
    assert torch.equal(out[4], resize_crop_u8([im], 227)[0])


def test_ten_crop_boxes_of_the_whole_image():
    boxes, flips = ten_crop_boxes(40, 37, resize=None)
    assert boxes == [(0, 0, 40, 37)] * 10 and flips == [False] * 5 + [True] * 5
    im = torch.arange(40 * 37 * 3, dtype=torch.int64).remainder(251).to(torch.uint8).view(40, 37, 3)
    assert resize_crop_u8([im], 8, boxes=boxes, flips=flips, source=[0] * 10).shape == (10, 8, 8, 3)


def test_abi_refuses_half_a_flag_pair():
    """The device entry point takes the flags as a device copy plus the caller's host copy: one without the other is
    refused before any pointer is read or anything is launched (so this needs no GPU)."""
    lib = nat.lib()
    assert lib.anx_abi_version() >= 7
    images, boxes = batch(2, 1.0)
    geo, _ = ops._image_geometry(images)
    desc = torch.from_numpy(ops._image_descs(geo, OH, 2, 256, boxes).view(np.uint8))
    flags = torch.ones(3, dtype=torch.uint8)
    out = torch.zeros(3, OH, 2, 3, dtype=torch.uint8)
    for dev_copy, host_copy in ((flags.data_ptr(), None), (None, flags.data_ptr())):
        assert lib.anx_resize_crop_u8_flip(desc.data_ptr(), desc.data_ptr(), dev_copy, host_copy, 3, out.data_ptr(), OH, 2,
                                           None) != 0
        assert "anx_resize_crop_u8_flip" in lib.anx_last_error().decode()
    assert not out.any()
    for name in ("anx_resize_crop_u8_flip", "anx_cpu_resize_crop_u8_flip"):
        fn = getattr(lib, name)
        assert fn.argtypes == nat._SIGS[name][1] and fn.restype is nat._SIGS[name][0]
