"""The host definition of the antialiased resize + crop (cpu::resize_crop_u8 through anx.ops.resize_crop_u8 on CPU
tensors) against the fp64 oracle of resize_crop_cases.py, which is first tied to torch's own antialiased bilinear
interpolation.

The bound on |out - ref| is derived, not measured: the final rounding loses at most 0.5; each floor of a tap weight
loses less than one unit of 2^-15 and the remainder lands on one tap, so the weights of an axis with n taps are off by
less than 2 (n - 1) / 2^15 in total, on bytes of at most 255; the 16-bit intermediate is rounded to 2^-8 of a byte, at
most 2^-9 off, which the 2^-8 term covers with room to spare. Besides the bound, at least 90 % of the elements of every
case of scale <= 4.5 must equal rint(ref); where the reference is an exact k + 0.5 (both neighbours equally near:
rint takes the even one, the definition rounds half up) either neighbour counts."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import anx._native as nat
from anx.ops import center_box, resize_crop_u8
from resize_crop_cases import CASES, SHAPES, geometry, host_result, image, make_image, oracle, reference, scale


@pytest.mark.parametrize("hw,ohw", [((256, 256), (227, 227)), ((375, 500), (227, 227)), ((40, 37), (227, 227)),
                                    ((229, 700), (227, 227)), ((64, 48), (7, 5)), ((5, 9), (12, 7)),
                                    ((300, 130), (23, 10)), ((1, 1), (3, 2))])
def test_oracle_is_torch_antialiased_bilinear(hw, ohw):
    img = make_image(*hw, "random", 7)
    ref, _ = oracle(img, ohw, (0, 0, *hw))
    x = img.double().permute(2, 0, 1)[None]
    t = F.interpolate(x, size=ohw, mode="bilinear", antialias=True, align_corners=False)[0].permute(1, 2, 0).numpy()
    err = np.abs(ref - t).max()
    print(f"{hw} -> {ohw}: oracle vs F.interpolate fp64 max |diff| {err:.3e}")
    assert err <= 1e-9


@pytest.mark.parametrize("name,fill", CASES)
def test_host_vs_oracle(name, fill):
    ref, (ny, nx) = reference(name, fill)
    got = host_result(name, fill).numpy().astype(np.float64)
    assert got.shape == ref.shape
    bound = 0.5 + 255.0 * 2.0 * ((nx - 1) + (ny - 1)) / 2 ** 15 + 2.0 ** -8
    err = np.abs(got - ref).max()
    # An exact tie (reference k + 0.5, e.g. the mean of 2 x 2 bytes under a half-pixel shift at scale 1) has two
    # nearest integers: rint picks the even one by convention, the definition rounds half up. Either counts.
    tie = np.abs(ref - np.floor(ref) - 0.5) < 1e-9
    same = float(((got == np.rint(ref)) | (tie & (np.abs(got - ref) < 0.5 + 1e-9))).mean())
    print(f"{name}/{fill}: taps ({ny}, {nx}) scale {scale(name):.2f} max |out - ref| {err:.4f} (bound {bound:.4f}), "
          f"equal to rint(ref) {100 * same:.2f} %")
    assert err <= bound
    if scale(name) <= 4.5:
        assert same >= 0.90


def test_identity_is_bit_exact():
    for fill in ("random", "checker"):
        assert torch.equal(host_result("227_identity", fill), image("227_identity", fill))


def test_center_box():
    assert center_box(375, 500) == (42, 167, 333, 333)
    assert center_box(256, 256) == (29, 29, 227, 227)
    assert center_box(375, 500, resize=None) == (0, 0, 375, 500)
    assert center_box(40, 37) == (7, 4, 33, 33)
    assert center_box(3, 1000, resize=256, size=227) == (0, 997, 3, 3)  # b clipped to the shorter side
    assert center_box(2, 2, resize=256, size=1) == (1, 1, 1, 1)          # b at least 1
    # the default boxes of the op are center_box's
    img = image("375x500_center", "random")
    assert torch.equal(resize_crop_u8([img])[0], host_result("375x500_center", "random"))


@pytest.mark.parametrize("v", [0, 1, 127, 255])
def test_constant_image_stays_constant(v):
    """The weights of every output sum to exactly 2^15 in both passes."""
    for (name, hw, ohw, _box) in SHAPES:
        if hw[0] * hw[1] > 400 * 600:
            continue
        _, _, box = geometry(name)
        out = resize_crop_u8([torch.full((*hw, 3), v, dtype=torch.uint8)], size=ohw, boxes=[box])
        assert out.shape == (1, *ohw, 3) and bool((out == v).all()), name


def test_pitch_and_odd_address():
    H, W = 61, 45
    big = make_image(H, 3 * W, "random", 11)
    compact = big[:, W + 1:2 * W + 1].contiguous()
    want = resize_crop_u8([compact], size=(31, 20), resize=None)
    view = big[:, W + 1:2 * W + 1]  # pitch 9 W bytes, base 3 (W + 1) bytes in: an even address
    assert not view.is_contiguous()
    assert torch.equal(resize_crop_u8([view], size=(31, 20), resize=None), want)
    flat = torch.zeros(H * W * 3 + 5, dtype=torch.uint8)
    for off in (1, 2, 3):  # the same bytes from odd (and every other) byte addresses
        odd = flat[off:off + H * W * 3].view(H, W, 3)
        odd.copy_(compact)
        assert odd.data_ptr() % 4 == (flat.data_ptr() + off) % 4
        assert torch.equal(resize_crop_u8([odd], size=(31, 20), resize=None), want)


def test_list_tensor_empty_and_out():
    x = torch.stack([make_image(40, 37, "random", s) for s in range(3)])
    a = resize_crop_u8(list(x.unbind(0)), size=(12, 7))
    b = resize_crop_u8(x, size=(12, 7))
    assert a.shape == (3, 12, 7, 3) and torch.equal(a, b)
    buf = torch.zeros(3 * 12 * 7 * 3 + 1, dtype=torch.uint8)
    o = buf[1:].view(3, 12, 7, 3)
    assert resize_crop_u8(x, size=(12, 7), out=o) is o and torch.equal(o, a) and buf[0] == 0
    e = resize_crop_u8([], size=9)
    assert e.shape == (0, 9, 9, 3) and e.dtype == torch.uint8


def test_limits_raise_value_error():
    img = make_image(64, 48, "random", 3)
    for box in ((0, 0, 65, 48), (1, 0, 64, 48), (0, 2, 64, 48), (-1, 0, 10, 10), (0, 0, 0, 10), (0, 0, 10, 0)):
        with pytest.raises(ValueError):
            resize_crop_u8([img], size=32, boxes=[box])
    with pytest.raises(ValueError):  # b > 16 n_out
        resize_crop_u8([img], size=(3, 32), resize=None)
    resize_crop_u8([img], size=(4, 3), resize=None)  # exactly 16x passes
    for size in (513, (227, 513), 0, (0, 5)):
        with pytest.raises(ValueError):
            resize_crop_u8([img], size=size)
    with pytest.raises(ValueError):
        resize_crop_u8([img.float()])
    with pytest.raises(ValueError):
        resize_crop_u8([img.permute(1, 0, 2)])  # rows not contiguous
    with pytest.raises(ValueError):
        resize_crop_u8([img[:, :, :2]])
    with pytest.raises(ValueError):
        resize_crop_u8([img], boxes=[])
    with pytest.raises(ValueError):
        resize_crop_u8([img], out=torch.empty((1, 227, 227, 3)))
    with pytest.raises(ValueError):  # mixed devices
        resize_crop_u8([img, img.to("meta")])


def test_native_entries_check_limits_themselves():
    """The C ABI refuses a bad descriptor before touching memory (Python's own checks are bypassed here)."""
    import ctypes as C
    from anx.ops import _IMAGE_DESC
    assert nat.lib().anx_abi_version() >= 6
    img = make_image(64, 48, "random", 3)
    out = torch.full((1, 8, 8, 3), 7, dtype=torch.uint8)
    good = (img.data_ptr(), 64, 48, 144, 0, 0, 64, 48)
    bad = [(img.data_ptr(), 64, 48, 144, 0, 0, 65, 48), (img.data_ptr(), 64, 48, 143, 0, 0, 64, 48),
           (0, 64, 48, 144, 0, 0, 64, 48), (img.data_ptr(), 64, 48, 144, 2, 0, 64, 48),
           (img.data_ptr(), 20000, 48, 144, 0, 0, 64, 48), (img.data_ptr(), 64, 48, 144, 0, 0, 64, 0)]
    for d, (oh, ow) in [(b, (8, 8)) for b in bad] + [(good, (3, 8)), (good, (8, 2)), (good, (513, 8)), (good, (8, 0))]:
        desc = np.zeros(1, dtype=_IMAGE_DESC)
        desc[0] = d
        rc = nat.lib().anx_cpu_resize_crop_u8(C.c_void_p(desc.ctypes.data), 1, C.c_void_p(out.data_ptr()), oh, ow)
        assert rc != 0 and nat.lib().anx_last_error(), (d, oh, ow)
        # the device entry validates its host copy first: no launch, so this needs no GPU
        rc = nat.lib().anx_resize_crop_u8(C.c_void_p(desc.ctypes.data), C.c_void_p(desc.ctypes.data), 1,
                                          C.c_void_p(out.data_ptr()), oh, ow, None)
        assert rc != 0, (d, oh, ow)
    assert bool((out == 7).all())
    for name in ("anx_resize_crop_u8", "anx_cpu_resize_crop_u8"):
        assert name in nat._SIGS and getattr(nat.lib(), name).argtypes == nat._SIGS[name][1]
