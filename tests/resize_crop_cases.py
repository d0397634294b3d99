"""Shared cases and the fp64 oracle of the antialiased resize + crop (anx.ops.resize_crop_u8).

The oracle is written here from the real-valued formula, independently of the C++ and without fixed point: per axis
a dense weight matrix ``w[o][j] = t_j / T`` with ``t_j = max(0, S - |D_j|)`` over the source pixels INSIDE THE IMAGE
(``S = 2 max(b, n_out)``, ``D_j = 2 n_out j + n_out - c2``, ``c2 = n_out o0h + (2o + 1) b``; box origin ``o0h`` in half
pixels), and ``ref = Wy @ image @ Wx^T`` per channel in fp64. Inputs and references are computed once per case and
shared by every test (``functools.lru_cache``); tests must not modify them."""
import functools

import numpy as np
import torch

# name, (H, W), (OH, OW), box (y0h, x0h, bh, bw) or None = the whole image
SHAPES = [
    ("256x256", (256, 256), (227, 227), None),
    ("375x500", (375, 500), (227, 227), None),
    ("40x37_up", (40, 37), (227, 227), None),
    ("227_identity", (227, 227), (227, 227), None),
    ("1000x701", (1000, 701), (227, 227), None),
    ("229x3000_s13", (229, 3000), (227, 227), None),
    ("8x3632_s16", (8, 3632), (227, 227), None),
    ("5x9_to_12x7", (5, 9), (12, 7), None),
    ("64x48_to_7x5", (64, 48), (7, 5), None),
    ("1x1_to_3x2", (1, 1), (3, 2), None),
    ("300_box16_to_1x1", (300, 300), (1, 1), (200, 301, 16, 16)),
    # boxes: center_box results (half-pixel origins), and a box touching each image edge
    ("375x500_center", (375, 500), (227, 227), (42, 167, 333, 333)),
    ("256x256_center", (256, 256), (227, 227), (29, 29, 227, 227)),
    ("edge_top_left", (90, 120), (31, 45), (0, 0, 50, 77)),
    ("edge_bottom_right", (90, 120), (31, 45), (2 * 90 - 2 * 61, 2 * 120 - 2 * 33, 61, 33)),
    ("edge_half_pixel", (90, 120), (31, 45), (1, 2 * 120 - 2 * 100 - 1, 89, 100)),
    # the widest accepted output and box: 512 columns from 8192 (16x), the kernel's largest LDS footprint
    ("24x8200_to_3x512", (24, 8200), (3, 512), (0, 9, 24, 8192)),
]
CASES = [(name, fill) for name, *_ in SHAPES for fill in ("random", "checker")]
_BY_NAME = {s[0]: s for s in SHAPES}


def geometry(name):
    """(H, W), (OH, OW), box of a case (the whole image when the table says None)."""
    _, hw, ohw, box = _BY_NAME[name]
    return hw, ohw, box if box is not None else (0, 0, hw[0], hw[1])


def make_image(H, W, fill, seed):
    g = torch.Generator().manual_seed(seed)
    if fill == "random":
        return torch.randint(0, 256, (H, W, 3), dtype=torch.uint8, generator=g)
    return (torch.randint(0, 2, (H, W, 3), dtype=torch.uint8, generator=g) * 255).contiguous()  # 0 / 255 at random


@functools.lru_cache(maxsize=None)
def image(name, fill):
    (H, W), _, _ = geometry(name)
    return make_image(H, W, fill, 1000 + sorted(_BY_NAME).index(name))


def axis_weights(n_in, n_out, o0h, b):
    """fp64 [n_out, n_in] weights t_j / T of one axis, and the largest number of taps of any output."""
    o = np.arange(n_out, dtype=np.float64)[:, None]
    j = np.arange(n_in, dtype=np.float64)[None, :]
    S = 2.0 * max(b, n_out)
    c2 = n_out * o0h + (2 * o + 1) * b
    t = np.maximum(0.0, S - np.abs(2 * n_out * j + n_out - c2))
    return t / t.sum(axis=1, keepdims=True), int((t > 0).sum(axis=1).max())


def oracle(img, out_hw, box):
    """fp64 [OH, OW, 3] resample of a uint8 [H, W, 3] tensor's box, and (n_y, n_x), the largest tap counts."""
    H, W = img.shape[:2]
    y0h, x0h, bh, bw = box
    wy, ny = axis_weights(H, out_hw[0], y0h, bh)
    wx, nx = axis_weights(W, out_hw[1], x0h, bw)
    x = img.numpy().astype(np.float64)
    ref = np.einsum("oy,yxc,px->opc", wy, x, wx, optimize=True)
    return ref, (ny, nx)


@functools.lru_cache(maxsize=None)
def reference(name, fill):
    """(fp64 reference, (n_y, n_x)) of a case; shared, read-only."""
    _, ohw, box = geometry(name)
    ref, taps = oracle(image(name, fill), ohw, box)
    ref.setflags(write=False)
    return ref, taps


def scale(name):
    _, (OH, OW), (_, _, bh, bw) = geometry(name)
    return max(bh / OH, bw / OW)


@functools.lru_cache(maxsize=None)
def host_result(name, fill):
    """uint8 [OH, OW, 3] of the host definition (CPU tensors): what the GPU kernel must equal bit for bit."""
    from anx.ops import resize_crop_u8
    _, ohw, box = geometry(name)
    return resize_crop_u8([image(name, fill)], size=ohw, boxes=[box])[0]
