"""Shared by test_resize_flip_cpu.py and test_resize_flip_gpu.py: the batches that the mirrored outputs of
anx.ops.resize_crop_u8 are checked on, and the check itself. A flipped output must equal torch.flip(unflipped,
dims=[2]) byte for byte, so no oracle is needed here: the unflipped bytes are held to theirs by the resize tests.

Output widths cover 1 to 6 elements per thread of the kernel (3 OW / 256 rounded up: 1, 1, 1, 2, 3, 4 and 6; 4 runs the 6-element kernel), both
band heights (16 rows up to 3 elements per thread, 8 above) and odd and even widths; OH = 20 gives every launch a
full band and a partial one. Scales 1 and 1.47 keep the tap rows in registers, 16 takes the LDS taps."""
import functools

import torch

OWS = (1, 2, 85, 86, 227, 257, 512)
SCALES = (1.0, 1.47, 16.0)
OH = 20
FLIPS = (True, False, True)


@functools.lru_cache(maxsize=None)
def batch(OW: int, scale: float):
    """(images, boxes): three images a little larger than their boxes (odd half-pixel origins), one size each."""
    g = torch.Generator().manual_seed(int(100 * scale) + OW)
    bh, bw = max(1, round(scale * OH)), max(1, round(scale * OW))
    images, boxes = [], []
    for i in range(len(FLIPS)):
        H, W = bh + 2 + i, bw + 3 + 2 * i
        images.append(torch.randint(0, 256, (H, W, 3), dtype=torch.uint8, generator=g))
        boxes.append((1 + i, 3 + 2 * i, bh, bw))
    return images, boxes


def sliced_out(n: int, OW: int, offset: int, dev) -> torch.Tensor:
    """A contiguous uint8 [n, OH, OW, 3] view that starts `offset` bytes into its (0xAA-filled) storage."""
    numel = n * OH * OW * 3
    flat = torch.full((numel + 32,), 0xAA, dtype=torch.uint8, device=dev)
    return flat[offset:offset + numel].view(n, OH, OW, 3)


def check_batch(resize_crop_u8, OW: int, scale: float, dev):
    images, boxes = batch(OW, scale)
    images = [im.to(dev) for im in images]
    plain = resize_crop_u8(images, (OH, OW), boxes=boxes)
    want = torch.stack([torch.flip(p, dims=[1]) if f else p for p, f in zip(plain, FLIPS)])
    assert not torch.equal(want, plain) or OW == 1
    got = resize_crop_u8(images, (OH, OW), boxes=boxes, flips=list(FLIPS))
    assert torch.equal(got, want), f"mixed batch OW={OW} scale={scale}"
    all_flipped = resize_crop_u8(images, (OH, OW), boxes=boxes, flips=[True] * len(images))
    assert torch.equal(all_flipped, torch.flip(plain, dims=[2])), f"all flipped OW={OW} scale={scale}"
    none = resize_crop_u8(images, (OH, OW), boxes=boxes, flips=[False] * len(images))
    assert torch.equal(none, plain), f"all-false flags OW={OW} scale={scale}"
    for offset in (1, 15):
        out = sliced_out(len(images), OW, offset, dev)
        assert out.data_ptr() % 16 == (out._base.data_ptr() + offset) % 16
        ret = resize_crop_u8(images, (OH, OW), boxes=boxes, flips=torch.tensor(FLIPS), out=out)
        assert ret is out and torch.equal(out, want), f"out at byte {offset} OW={OW} scale={scale}"
        base = out._base
        assert (base[:offset] == 0xAA).all() and (base[offset + out.numel():] == 0xAA).all(), "wrote outside out"
