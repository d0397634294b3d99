"""Per-layer operators on torch tensors (NHWC fp32), each one native kernel.

GPU tensors run the libanx HIP kernels on torch's current stream; CPU tensors run libanx's C++ host
reference kernels. There is no eager-PyTorch path (the torch oracle is anx.models.reference).
These are the standalone, testable layer ops of SURVEY §7.1 item 3. They match the reference's
per-layer kernels:

* convKernel / serialConvLayer  (v3_cuda_only/src/layers_cuda.cu:20-46, v1_serial/src/layers_serial.cpp:37-81)
* reluKernel                    (layers_cuda.cu:56-62)
* poolKernel                    (layers_cuda.cu:78-104)
* lrnKernel                     (layers_cuda.cu:118-152; alpha mode: ``div_n`` V1/V2, ``raw`` V3/V4)

How the GPU versions differ:

* ``conv2d`` is the MFMA implicit GEMM: packed weights are cached per (weight tensor, version, plan).
  The cache entry holds a reference to the weight tensor, so its storage (and address) cannot be
  reused by another tensor while the entry exists; in-place edits through ``w.data`` do not bump
  ``w._version`` — call :func:`clear_cache` after them. ``impl="direct"`` selects the
  one-thread-per-output oracle kernel.
* ``maxpool`` uses float4 channels.
* ``maxpool_lrn`` is the fused pool+LRN kernel.
* ``conv2d`` can write into a channel slice of a preallocated output (``out`` / ``c_off``), which
  is how the filter-parallel strategy assembles its shards.
"""
from __future__ import annotations

import ctypes as C

import numpy as np
import torch
import torch.nn.functional as F

from .. import _native as nat
from ..config import conv_out_dim, pool_out_dim

__all__ = ["conv2d", "relu", "maxpool", "lrn", "maxpool_lrn", "decode_u8", "softmax_topk", "resize_crop_u8",
           "center_box", "ten_crop_boxes", "softmax_topk_views", "softmax_eval", "eval_summary", "clear_cache"]

_LRN_MODES = {"div_n": 0, "raw": 1}
_pack_cache: dict = {}


def clear_cache() -> None:
    _pack_cache.clear()


def _check(x: torch.Tensor, name: str) -> None:
    if x.dtype != torch.float32 or not x.is_contiguous():
        raise ValueError(f"{name}: expected a contiguous float32 tensor")


def _packed(w: torch.Tensor, plan, sizes: tuple[int, int], dev: torch.device):
    key = (w.data_ptr(), w._version, tuple(w.shape), w.stride(), str(w.device), tuple(plan), str(dev))
    hit = _pack_cache.get(key)
    if hit is not None and hit[0] is w:
        return hit[1], hit[2]
    wc = w.detach().to("cpu", torch.float32).contiguous()
    packed = torch.empty(sizes[0], dtype=torch.float32)
    koff = torch.empty(sizes[1], dtype=torch.int32)
    nat.call("anx_conv_pack", plan, C.c_void_p(wc.data_ptr()), C.c_void_p(packed.data_ptr()),
             C.c_void_p(koff.data_ptr()))
    if len(_pack_cache) > 64:
        _pack_cache.clear()
    # keep `w` alive with the entry: a freed temporary's address could otherwise be handed to the
    # next temporary of the same shape (e.g. equal-size filter shards) and hit this entry
    hit = (w, packed.to(dev), koff.to(dev))
    _pack_cache[key] = hit
    return hit[1], hit[2]


def conv2d(x: torch.Tensor, w: torch.Tensor, b: torch.Tensor | None = None, stride: int = 1, pad: int = 0,
           groups: int = 1, relu: bool = False, impl: str = "mfma", out: torch.Tensor | None = None,
           c_off: int = 0) -> torch.Tensor:
    """x [N,H,W,C], w [K,C/groups,F,F] (KCFF), b [K] -> [N,Ho,Wo,K] (or into out[..., c_off:c_off+K])."""
    _check(x, "conv2d")
    N, H, W, Cin = x.shape
    K, Cg, Fh, Fw = w.shape
    if Fh != Fw or Cg * groups != Cin or K % groups:
        raise ValueError("conv2d: bad weight shape")
    Ho, Wo = conv_out_dim(H, Fh, stride, pad), conv_out_dim(W, Fw, stride, pad)
    if out is None:
        out = torch.empty((N, Ho, Wo, K), device=x.device, dtype=torch.float32)
        c_off = 0
    if out.shape[:3] != (N, Ho, Wo) or c_off + K > out.shape[3]:
        raise ValueError("conv2d: out has the wrong shape")
    _check(out, "conv2d out")
    bias = (b if b is not None else torch.zeros(K, device=x.device)).to(x.device, torch.float32).contiguous()
    if not x.is_cuda:
        if c_off or out.shape[3] != K:
            tmp = torch.empty((N, Ho, Wo, K), dtype=torch.float32)
            conv2d(x, w, bias, stride, pad, groups, relu, impl, tmp)
            out[..., c_off:c_off + K] = tmp
            return out
        wc = w.detach().float().contiguous()
        nat.call("anx_cpu_conv2d", nat.ptr(x), nat.ptr(wc), nat.ptr(bias), nat.ptr(out), N, H, W, Cin, K, Fh,
                 stride, pad, groups, int(relu))
        return out
    s = nat.stream_ptr(x.device)
    if impl == "direct":
        if c_off or out.shape[3] != K:
            raise ValueError("conv2d: impl='direct' writes whole outputs only")
        wd = w.detach().to(x.device, torch.float32).contiguous()
        nat.call("anx_conv2d_direct", nat.ptr(x), nat.ptr(wd), nat.ptr(bias), nat.ptr(out), N, H, W, Cin, K, Fh,
                 stride, pad, groups, int(relu), s)
        return out
    xp = F.pad(x, (0, 0, pad, pad, pad, pad)).contiguous() if pad else x
    plan = (C.c_int * 16)()
    sz, kz = C.c_size_t(), C.c_size_t()
    nat.call("anx_conv_plan", N, H + 2 * pad, W + 2 * pad, Cin, K, Fh, stride, groups, plan, C.byref(sz), C.byref(kz))
    packed, koff = _packed(w, plan, (sz.value, kz.value), x.device)
    nat.call("anx_conv2d_mfma", plan, nat.ptr(xp), nat.ptr(packed), nat.ptr(koff), nat.ptr(bias), nat.ptr(out),
             Ho, Wo, out.shape[3], 0, 0, c_off, int(relu), s)
    return out


def decode_u8(x: torch.Tensor, scale=None, offset=None) -> torch.Tensor:
    """Byte image -> float32, the meaning of byte input everywhere in the package: element i (flat index) becomes
    ``fmaf(float(x[i]), scale[i % C], offset[i % C])``, one fused multiply-add in fp32, with C the number of
    scale values (default: ``scale = 1/255`` and ``offset = 0`` for each of the ``x.shape[-1]`` channels).
    ``x`` is a contiguous uint8 tensor that may start at any byte of its storage (a slice); the result has its
    shape. The reference has no byte input."""
    if x.dtype != torch.uint8 or not x.is_contiguous():
        raise ValueError("decode_u8: expected a contiguous uint8 tensor")
    Cn = x.shape[-1] if x.dim() > 1 else 1
    sc = torch.full((Cn,), 1.0 / 255.0, dtype=torch.float64) if scale is None else torch.as_tensor(scale, dtype=torch.float64).reshape(-1)
    of = torch.zeros_like(sc) if offset is None else torch.as_tensor(offset, dtype=torch.float64).reshape(-1)
    if sc.numel() != of.numel() or sc.numel() < 1 or (x.is_cuda and sc.numel() > 16):
        raise ValueError("decode_u8: scale and offset need the same number of values (1 to 16 on the GPU)")
    sc, of = sc.to("cpu", torch.float32).contiguous(), of.to("cpu", torch.float32).contiguous()
    y = torch.empty(x.shape, device=x.device, dtype=torch.float32)
    if x.numel() == 0:
        return y
    if x.is_cuda:
        nat.call("anx_decode_u8", x.data_ptr(), y.data_ptr(), x.numel(), sc.numel(), sc.data_ptr(), of.data_ptr(),
                 nat.stream_ptr(x.device))
    else:
        nat.call("anx_cpu_decode_u8", x.data_ptr(), y.data_ptr(), x.numel(), sc.numel(), sc.data_ptr(), of.data_ptr())
    return y


RESIZE_MAX_IN, RESIZE_MAX_OUT, RESIZE_MAX_SCALE = 16384, 512, 16  # kResizeMax* (anx/resize_taps.hpp)
_IMAGE_DESC = np.dtype([("ptr", "<u8"), ("H", "<i4"), ("W", "<i4"), ("pitch", "<i8"), ("y0h", "<i4"), ("x0h", "<i4"),
                        ("bh", "<i4"), ("bw", "<i4")])  # anx::ImageDesc / anx_image_desc: 40 bytes


def _size2(size) -> tuple[int, int]:
    oh, ow = (size, size) if isinstance(size, int) else tuple(size)
    return int(oh), int(ow)


def center_box(H: int, W: int, resize: int | None = 256, size=227) -> tuple[int, int, int, int]:
    """The usual "shorter side to ``resize``, centre crop ``size``" box of an ``H x W`` image, in the image's own
    pixels, as :func:`resize_crop_u8` takes it: ``(y0h, x0h, bh, bw)`` with the origin in HALF pixels (so a centred
    crop of odd slack is exact). ``b = max(1, round(size * min(H, W) / resize))`` (halves round up), clipped to
    ``min(H, W)``; ``y0h = H - bh``, ``x0h = W - bw``. ``size`` ``(OH, OW)`` gives a box of that aspect.
    ``resize=None``: the whole image, ``(0, 0, H, W)``."""
    if resize is None:
        return (0, 0, int(H), int(W))
    m = min(H, W)
    bh, bw = (min(m, max(1, (2 * s * m + resize) // (2 * resize))) for s in _size2(size))
    return (int(H - bh), int(W - bw), int(bh), int(bw))


def _image_geometry(images):
    """int64 [n, 4] rows (data pointer, H, W, row pitch in bytes) of a list of uint8 [H,W,3] tensors or one
    [N,H,W,3] tensor, and their device (None for an empty list); layouts the kernels cannot read raise."""
    bad_layout = "resize_crop_u8: the last two dims of an image must be contiguous, rows >= 3W bytes apart"
    if isinstance(images, torch.Tensor):
        if images.dim() != 4 or images.dtype != torch.uint8 or images.shape[3] != 3:
            raise ValueError("resize_crop_u8: a tensor of images must be uint8 [N,H,W,3]")
        N, H, W, _ = images.shape
        st = images.stride()
        pitch = st[1] if H > 1 else max(st[1], 3 * W)
        if (W > 1 and st[2] != 3) or st[3] != 1 or pitch < 3 * W or (N > 1 and st[0] < 0):
            raise ValueError(bad_layout)
        geo = np.empty((N, 4), dtype=np.int64)
        geo[:, 0] = images.data_ptr() + np.arange(N, dtype=np.int64) * st[0]
        geo[:, 1:] = (H, W, pitch)
        return geo, images.device
    rows, dev = [], None
    for im in images:
        if not isinstance(im, torch.Tensor) or im.dtype != torch.uint8 or im.dim() != 3 or im.shape[2] != 3:
            raise ValueError("resize_crop_u8: every image must be a uint8 [H,W,3] tensor")
        if dev is None:
            dev = im.device
        elif im.device != dev:
            raise ValueError("resize_crop_u8: all images must be on one device")
        H, W, _ = im.shape
        st = im.stride()
        pitch = st[0] if H > 1 else max(st[0], 3 * W)
        if (W > 1 and st[1] != 3) or st[2] != 1 or pitch < 3 * W:
            raise ValueError(bad_layout)
        rows.append((im.data_ptr(), H, W, pitch))
    return np.array(rows, dtype=np.int64).reshape(len(rows), 4), dev


def _image_descs(geo, OH: int, OW: int, resize, boxes):
    """The anx::ImageDesc array of images ``geo`` (:func:`_image_geometry`) with ``boxes`` (default
    :func:`center_box`), every limit of the operation checked: a miss is a ValueError naming the image."""
    n = geo.shape[0]
    H, W = geo[:, 1], geo[:, 2]
    if n and not (H.min() >= 1 and W.min() >= 1 and H.max() <= RESIZE_MAX_IN and W.max() <= RESIZE_MAX_IN):
        raise ValueError(f"resize_crop_u8: image sizes must be 1 .. {RESIZE_MAX_IN}")
    if boxes is None:
        if resize is None:
            box = np.stack([np.zeros_like(H), np.zeros_like(H), H, W], axis=1)
        else:  # center_box, for all images at once
            m = np.minimum(H, W)
            bh, bw = (np.minimum(m, np.maximum(1, (2 * s * m + resize) // (2 * resize))) for s in (OH, OW))
            box = np.stack([H - bh, W - bw, bh, bw], axis=1)
    else:
        try:
            box = np.array([[int(v) for v in b] for b in boxes], dtype=np.int64).reshape(len(boxes), 4)
        except (TypeError, ValueError) as e:
            raise ValueError("resize_crop_u8: a box is four integers (y0h, x0h, bh, bw)") from e
        if box.shape[0] != n:
            raise ValueError("resize_crop_u8: one box per image")
    y0h, x0h, bh, bw = box.T
    outside = (bh < 1) | (bw < 1) | (y0h < 0) | (x0h < 0) | (y0h + 2 * bh > 2 * H) | (x0h + 2 * bw > 2 * W)
    if outside.any():
        i = int(np.argmax(outside))
        raise ValueError(f"resize_crop_u8: box {tuple(int(v) for v in box[i])} (half-pixel origin) is not inside image "
                         f"{i} of {(int(H[i]), int(W[i]))}")
    big = (bh > RESIZE_MAX_SCALE * OH) | (bw > RESIZE_MAX_SCALE * OW)
    if big.any():
        i = int(np.argmax(big))
        raise ValueError(f"resize_crop_u8: box {(int(bh[i]), int(bw[i]))} of image {i} is more than {RESIZE_MAX_SCALE} "
                         f"times the output {(OH, OW)}")
    desc = np.zeros(n, dtype=_IMAGE_DESC)
    for k, col in zip(("ptr", "H", "W", "pitch"), geo.T):
        desc[k] = col
    for k, col in zip(("y0h", "x0h", "bh", "bw"), box.T):
        desc[k] = col
    return desc


def ten_crop_boxes(H: int, W: int, resize: int | None = 256, size=227):
    """The ten views of an ``H x W`` image that AlexNet's evaluation protocol takes, as ``(boxes, flips)`` for
    :func:`resize_crop_u8`, ten of each: the four corner crops and the centre crop, then the same five mirrored.
    All ten share the scale of ``center_box(H, W, resize, size)`` (its ``bh x bw``); the origins in half pixels are
    ``(0, 0)``, ``(0, 2 (W - bw))``, ``(2 (H - bh), 0)``, ``(2 (H - bh), 2 (W - bw))`` and the centre
    ``(H - bh, W - bw)``. ``resize=None`` makes the box the whole image, so the five origins coincide."""
    _, _, bh, bw = center_box(H, W, resize, size)
    y1, x1 = 2 * (int(H) - bh), 2 * (int(W) - bw)
    five = [(0, 0, bh, bw), (0, x1, bh, bw), (y1, 0, bh, bw), (y1, x1, bh, bw), (y1 // 2, x1 // 2, bh, bw)]
    return five + five, [False] * 5 + [True] * 5


def _flip_flags(flips, n: int) -> np.ndarray:
    """``flips`` of :func:`resize_crop_u8` as ``n`` flag bytes; anything but ``n`` booleans raises."""
    if isinstance(flips, torch.Tensor):
        if flips.dtype != torch.bool or flips.dim() != 1:
            raise ValueError("resize_crop_u8: flips must be booleans, one per output")
        flips = flips.cpu().numpy()
    elif isinstance(flips, np.ndarray):
        if flips.dtype != np.bool_ or flips.ndim != 1:
            raise ValueError("resize_crop_u8: flips must be booleans, one per output")
    else:
        try:
            flips = list(flips)
        except TypeError as e:
            raise ValueError("resize_crop_u8: flips must be booleans, one per output") from e
        if not all(isinstance(f, (bool, np.bool_)) for f in flips):
            raise ValueError("resize_crop_u8: flips must be booleans, one per output")
        flips = np.array(flips, dtype=np.bool_)
    if flips.shape[0] != n:
        raise ValueError(f"resize_crop_u8: one flip per output: {flips.shape[0]} for {n} outputs")
    return np.ascontiguousarray(flips).astype(np.uint8)


def resize_crop_u8(images, size=227, resize: int | None = 256, boxes=None, out: torch.Tensor | None = None,
                   flips=None, source=None) -> torch.Tensor:
    """Byte images of any size -> ``uint8 [N, OH, OW, 3]``: each image's box resampled onto the output with torch /
    PIL's antialiased bilinear (triangle) filter, in fixed point, one native kernel for the whole batch.

    ``flips``: one boolean per output; a flipped output is the unflipped one with its columns reversed,
    ``out[oy][OW-1-ox][c]`` (default: none, today's call). ``source``: ``source[i]`` is the index of the image that
    output ``i`` is cut from (default: output ``i`` from image ``i``); ``boxes`` and ``flips`` are then per output and
    the result has ``len(source)`` outputs, so several views share one source image without repeating tensors.

    ``images``: a list of ``uint8 [H,W,3]`` tensors (each its own size) or one ``[N,H,W,3]`` tensor, all on one
    device; the last two dims contiguous, the row stride free (a column slice of a bigger image is fine).
    ``size``: ``OH = OW`` or ``(OH, OW)``, 1 to 512. ``boxes``: one ``(y0h, x0h, bh, bw)`` per image (origin in half
    pixels, size in pixels, inside the image, at most 16 times the output per axis); default
    :func:`center_box` ``(H, W, resize, size)``. ``out``: a contiguous ``uint8 [N,OH,OW,3]`` tensor on the images'
    device to write into (any byte offset). A missed limit is a ``ValueError``.

    The definition is the host function ``cpu::resize_crop_u8`` (CPU tensors run it): per axis 15-bit tap weights
    ``q`` summing to exactly 2^15 (``anx/resize_taps.hpp``), horizontal pass first into 16 bits,
    ``h = (sum q_x * src + 64) >> 7``, then ``out = (sum q_y * h + 2^22) >> 23``. GPU tensors run the gfx950 kernel
    on torch's current stream; it computes the same integers, so the bytes are equal. The descriptors (pointer,
    size, pitch, box per image) are built on the host, checked there natively, and copied to the device with the
    stream. The reference has no resampling stage."""
    OH, OW = _size2(size)
    if not (1 <= OH <= RESIZE_MAX_OUT and 1 <= OW <= RESIZE_MAX_OUT):
        raise ValueError(f"resize_crop_u8: output size must be 1 .. {RESIZE_MAX_OUT}, got {(OH, OW)}")
    geo, dev = _image_geometry(images)
    if source is not None:
        try:
            src = np.asarray(source.cpu() if isinstance(source, torch.Tensor) else source)
        except (TypeError, ValueError) as e:
            raise ValueError("resize_crop_u8: source must be image indices, one per output") from e
        if src.ndim != 1 or (src.size and src.dtype.kind not in "iu"):
            raise ValueError("resize_crop_u8: source must be image indices, one per output")
        src = src.astype(np.int64)
        if src.size and not (src.min() >= 0 and src.max() < geo.shape[0]):
            raise ValueError(f"resize_crop_u8: source indices must be 0 .. {geo.shape[0] - 1}")
        geo = geo[src]
    n = geo.shape[0]
    if dev is None:
        dev = out.device if out is not None else torch.device("cpu")
    desc = _image_descs(geo, OH, OW, resize, boxes)
    flags = _flip_flags(flips, n) if flips is not None else None
    shape = (n, OH, OW, 3)
    if out is None:
        out = torch.empty(shape, device=dev, dtype=torch.uint8)
    elif tuple(out.shape) != shape or out.dtype != torch.uint8 or not out.is_contiguous() or out.device != dev:
        raise ValueError(f"resize_crop_u8: out must be a contiguous uint8 {shape} tensor on {dev}, got "
                         f"{tuple(out.shape)} {out.dtype} on {out.device}")
    if n == 0:
        return out
    host = torch.from_numpy(desc.view(np.uint8))
    fhost = torch.from_numpy(flags) if flags is not None else None
    if dev.type == "cuda":
        with torch.cuda.device(dev):
            ddev = host.to(dev, non_blocking=True)  # on the current stream, ahead of the kernel
            if fhost is None:
                nat.call("anx_resize_crop_u8", ddev.data_ptr(), host.data_ptr(), n, out.data_ptr(), OH, OW,
                         nat.stream_ptr(dev))
            else:
                fdev = fhost.to(dev, non_blocking=True)
                nat.call("anx_resize_crop_u8_flip", ddev.data_ptr(), host.data_ptr(), fdev.data_ptr(),
                         fhost.data_ptr(), n, out.data_ptr(), OH, OW, nat.stream_ptr(dev))
    elif fhost is None:
        nat.call("anx_cpu_resize_crop_u8", host.data_ptr(), n, out.data_ptr(), OH, OW)
    else:
        nat.call("anx_cpu_resize_crop_u8_flip", host.data_ptr(), fhost.data_ptr(), n, out.data_ptr(), OH, OW)
    return out


MAX_TOPK = 16               # kMaxTopK (anx/ops.hpp)
MAX_VIEWS = 32              # kMaxViews (anx/ops.hpp)
VIEWS_MAX_CLASSES = 7680    # kSoftmaxViewsMaxK: two rows of the view-averaging head in LDS on the GPU
_HEAD_LDS_ROW = 15 * 1024   # kSoftmaxTopkLdsRow: a longer row is staged in the logits output on the GPU


def _head_views(fn: str, views, none_ok: bool) -> int:
    """``views`` of a head, checked: 1 .. 32, or None (returned as 0, the native side's "no views") where ``fn``
    takes that."""
    if views is None and none_ok:
        return 0
    if not isinstance(views, int) or isinstance(views, bool) or not 1 <= views <= MAX_VIEWS:
        what = "None or an integer" if none_ok else "an integer"
        raise ValueError(f"{fn}: views must be {what} 1 .. {MAX_VIEWS}, got {views!r}")
    return views


def _head_source(fn: str, rows: str, logits, slabs, bias, k):
    """What every head takes: ``logits`` ``[rows,K]`` or ``slabs`` ``[ksplit,rows,K]`` (+ ``bias`` ``[K]``) and ``k``,
    checked. Returns ``(src, head, M, K, k)``, ``head`` being the leading ``(src, ksplit, slab_stride, bias)``
    arguments of the native entries; ``fn`` and ``rows`` (how ``fn`` names the row count) go into the messages."""
    if (logits is None) == (slabs is None):
        raise ValueError(f"{fn}: give logits [{rows},K] or slabs [ksplit,{rows},K], not both")
    src = logits if slabs is None else slabs
    _check(src, fn)
    if slabs is None:
        if src.dim() != 2:
            raise ValueError(f"{fn}: logits must be [{rows},K]")
        if bias is not None:
            raise ValueError(f"{fn}: a bias goes with slabs")
        ksplit, (M, K) = 1, src.shape
    else:
        if src.dim() != 3 or src.shape[0] < 1:
            raise ValueError(f"{fn}: slabs must be [ksplit,{rows},K] with ksplit >= 1")
        ksplit, M, K = src.shape
    if K < 1 or not 1 <= int(k) <= min(K, MAX_TOPK):
        raise ValueError(f"{fn}: need 1 <= k <= min(K, {MAX_TOPK}), got k = {k} for K = {K}")
    if bias is not None:
        _check(bias, f"{fn} bias")
        if tuple(bias.shape) != (K,) or bias.device != src.device:
            raise ValueError(f"{fn}: bias must be [K] on the source's device")
    return src, (src.data_ptr(), ksplit, M * K, bias.data_ptr() if bias is not None else None), M, K, int(k)


def softmax_topk(logits: torch.Tensor | None = None, k: int = 5, *, slabs: torch.Tensor | None = None,
                 bias: torch.Tensor | None = None, return_logits: bool = False):
    """The classifier head: the ``k`` most likely classes of each row and their softmax probabilities, one native
    kernel. Returns ``(indices int32 [M,k], probs float32 [M,k])``, plus the ``[M,K]`` logits with ``return_logits``.

    The rows are ``logits`` ``[M,K]``, or the sum ``bias + slabs[0] + slabs[1] + ...`` of split-K partial sums
    ``slabs`` ``[ksplit,M,K]`` (fp32 adds in that order, the order of the bf16 engine's split-K reduce; ``bias``
    ``[K]`` is optional). Classes are ordered by value descending, then index ascending; values compare as floats, so
    ``-0.0`` and ``+0.0`` tie. ``p = exp(z - max) / sum(exp(z - max))`` in fp32. ``1 <= k <= min(K, 16)``. A row that
    holds a NaN or whose maximum is infinite still gets ``k`` distinct indices; its probabilities are unspecified.
    The host function ``cpu::softmax_topk`` (CPU tensors) is the definition the GPU kernel is tested against."""
    src, head, M, K, k = _head_source("softmax_topk", "M", logits, slabs, bias, k)
    idx = torch.empty((M, k), device=src.device, dtype=torch.int32)
    prob = torch.empty((M, k), device=src.device, dtype=torch.float32)
    z = None
    if return_logits or (src.is_cuda and K > _HEAD_LDS_ROW):
        z = torch.empty((M, K), device=src.device, dtype=torch.float32)
    if M:
        args = (*head, M, K, k, idx.data_ptr(), prob.data_ptr(), z.data_ptr() if z is not None else None)
        if src.is_cuda:
            nat.call("anx_softmax_topk", *args, nat.stream_ptr(src.device))
        else:
            nat.call("anx_cpu_softmax_topk", *args)
    return (idx, prob, z) if return_logits else (idx, prob)


def softmax_topk_views(logits: torch.Tensor | None = None, views: int | None = None, k: int = 5, *,
                       slabs: torch.Tensor | None = None, bias: torch.Tensor | None = None, return_probs: bool = False):
    """The view-averaging head: the rows are ``views`` consecutive views per image, ``[N * views, K]`` image-major
    (row ``i * views + v`` is view ``v`` of image ``i``), given as ``logits`` or as ``slabs`` ``[ksplit, N * views, K]``
    (+ ``bias``) exactly as :func:`softmax_topk` takes them. Per row ``p_v = exp(z - max) / sum(exp(z - max))`` in
    fp32 (:func:`softmax_topk`'s expressions); per image ``pbar = ((p_0 + p_1) + ... + p_{V-1}) / float(V)`` in fp32,
    adding in view order. Returns ``(indices int32 [N,k], probs float32 [N,k])``: the ``k`` classes of the largest
    ``pbar`` (descending, then index ascending) and ``pbar`` there; with ``return_probs`` also the whole ``[N,K]``
    ``pbar``. One native kernel; ``1 <= views <= 32``, ``1 <= k <= min(K, 16)``, and ``K <= 7680`` on the GPU.

    The ranking is by probability, not by logit. With ``views=1`` the probabilities are :func:`softmax_topk`'s bits,
    but classes whose probabilities underflow to the same value (zero, say) tie here and go to the lower index, where
    :func:`softmax_topk` still orders them by their logits. The host function ``cpu::softmax_topk_views`` (CPU
    tensors) is the definition; ``expf`` differs between host and device, so both are held to an fp64 softmax mean
    rather than to each other's bits."""
    views = _head_views("softmax_topk_views", views, none_ok=False)
    src, head, M, K, k = _head_source("softmax_topk_views", "N*V", logits, slabs, bias, k)
    if M % views:
        raise ValueError(f"softmax_topk_views: {M} rows are no whole number of images of {views} views")
    if src.is_cuda and K > VIEWS_MAX_CLASSES:
        raise ValueError(f"softmax_topk_views: at most {VIEWS_MAX_CLASSES} classes on the GPU, got {K}")
    N = M // views
    idx = torch.empty((N, k), device=src.device, dtype=torch.int32)
    prob = torch.empty((N, k), device=src.device, dtype=torch.float32)
    probs = torch.empty((N, K), device=src.device, dtype=torch.float32) if return_probs else None
    if N:
        args = (*head, N, views, K, k, idx.data_ptr(), prob.data_ptr(),
                probs.data_ptr() if probs is not None else None, None)
        if src.is_cuda:
            with torch.cuda.device(src.device):
                nat.call("anx_softmax_topk_views", *args, nat.stream_ptr(src.device))
        else:
            nat.call("anx_cpu_softmax_topk_views", *args)
    return (idx, prob, probs) if return_probs else (idx, prob)


EVAL_MAX_CLASSES = _HEAD_LDS_ROW  # kSoftmaxEvalMaxK: one row of the evaluation head in LDS on the GPU (views=None)
EVAL_STATS = 4               # kEvalStats: images, top-1 hits, top-k hits, loss in 2^-32 units
EVAL_NLL_CAP = 1024.0        # eval_nll_q32: a loss that is NaN or not below this counts as this


def _eval_buffer(fn: str, name: str, t, shape, dtype, device, fill=None) -> torch.Tensor:
    """An output of the evaluation head, checked as the kernels assume it (shape, dtype, contiguity, device), or made
    when not given (``fill`` None: uninitialised)."""
    if t is None:
        return (torch.empty(shape, device=device, dtype=dtype) if fill is None
                else torch.full(shape, fill, device=device, dtype=dtype))
    if (not isinstance(t, torch.Tensor) or tuple(t.shape) != tuple(shape) or t.dtype != dtype or not t.is_contiguous()
            or t.device != device):
        got = f"{tuple(t.shape)} {t.dtype} on {t.device}" if isinstance(t, torch.Tensor) else repr(t)
        raise ValueError(f"{fn}: {name} must be a contiguous {dtype} {tuple(shape)} tensor on {device}, got {got}")
    return t


def _eval_outputs(fn: str, N: int, K: int, device, labels, stats, confusion, out):
    """``labels``, ``stats``, ``confusion`` and ``out`` of the evaluation head, validated; returns ``(rank, nll,
    pred)`` (allocated when ``out`` is None)."""
    if labels is None:
        raise ValueError(f"{fn}: labels (int32 [{N}], one per image) are required")
    _eval_buffer(fn, "labels", labels, (N,), torch.int32, device)
    if stats is not None:
        _eval_buffer(fn, "stats", stats, (EVAL_STATS,), torch.int64, device)
    if confusion is not None:
        _eval_buffer(fn, "confusion", confusion, (K, K), torch.int32, device)
    out = tuple(out) if out is not None else (None, None, None)
    if len(out) != 3:
        raise ValueError(f"{fn}: out must be (rank, nll, pred)")
    return tuple(_eval_buffer(fn, name, t, (N,), dt, device)
                 for t, dt, name in zip(out, (torch.int32, torch.float32, torch.int32), ("rank", "nll", "pred")))


def softmax_eval(logits: torch.Tensor | None = None, labels: torch.Tensor | None = None, k: int = 5, *,
                 views: int | None = None, slabs: torch.Tensor | None = None, bias: torch.Tensor | None = None,
                 stats: torch.Tensor | None = None, confusion: torch.Tensor | None = None, out=None,
                 return_logits: bool = False):
    """The evaluation head: the rows held to ``labels`` (``int32 [N]``, one per image, on the rows' device), one native
    kernel. Returns ``(rank int32 [N], nll float32 [N], pred int32 [N])``, plus the reduced logits with
    ``return_logits``.

    The rows are ``logits`` or ``slabs`` (+ ``bias``) exactly as :func:`softmax_topk` takes them. ``views=None``: one
    row per image, the score row is the logits (:func:`softmax_topk`'s order). ``views=V`` (1 to 32): ``V``
    consecutive rows per image, the score row is the mean ``pbar`` of the views' softmax rows
    (:func:`softmax_topk_views`' expressions and order). Per image with label ``y``:

    * ``pred`` is the class that ranks first (value descending, then index ascending, a NaN as ``-inf``);
    * ``rank`` is the number of classes that rank before ``y``: ``rank < k`` exactly when ``y`` is among the ``k``
      classes the head of the same rows returns, and ``indices[i, rank[i]] == y`` there;
    * ``nll`` is ``logf(S) - (z[y] - max)`` with ``S = sum(expf(z - max))`` without views (finite where the
      probability underflows, ``+inf`` for a ``-inf`` label logit), and ``-logf(pbar[y])`` with views.

    A label outside ``0 .. K-1`` (the ``-1`` padding of a last batch) marks an ignored image: ``rank = -1``,
    ``nll = 0``, ``pred`` still written, nothing counted. Every other image adds into ``stats`` (``int64 [4]``, zeroed
    by the caller once, accumulated into: images, ``rank == 0``, ``rank < k``, and the loss in units of ``2^-32``, a
    NaN or anything not below 1024 counting as 1024; :func:`eval_summary` reads it) and into ``confusion`` (``int32
    [K,K]``, ``[y, pred] += 1``). These are integer sums, so the totals are the same bits whatever order images,
    streams and workgroups finish in. ``out``: ``(rank, nll, pred)`` tensors to write into. ``1 <= k <= min(K, 16)``;
    on the GPU ``K <= 15360`` without views and ``K <= 7680`` with views. Nothing here synchronises. The host function
    ``cpu::softmax_eval`` (CPU tensors) is the definition the GPU kernel is tested against."""
    fn = "softmax_eval"
    V = _head_views(fn, views, none_ok=True)
    src, head, M, K, k = _head_source(fn, "N*V" if V else "N", logits, slabs, bias, k)
    if V and M % V:
        raise ValueError(f"{fn}: {M} rows are no whole number of images of {V} views")
    most = VIEWS_MAX_CLASSES if V else EVAL_MAX_CLASSES
    if src.is_cuda and K > most:
        raise ValueError(f"{fn}: at most {most} classes on the GPU {'with' if V else 'without'} views, got {K}")
    N = M // V if V else M
    rank, nll, pred = _eval_outputs(fn, N, K, src.device, labels, stats, confusion, out)
    z = torch.empty((M, K), device=src.device, dtype=torch.float32) if return_logits else None
    if N:
        args = (*head, N, V, K, k, labels.data_ptr(), rank.data_ptr(), nll.data_ptr(), pred.data_ptr(),
                stats.data_ptr() if stats is not None else None,
                confusion.data_ptr() if confusion is not None else None, z.data_ptr() if z is not None else None)
        if src.is_cuda:
            with torch.cuda.device(src.device):
                nat.call("anx_softmax_eval", *args, nat.stream_ptr(src.device))
        else:
            nat.call("anx_cpu_softmax_eval", *args)
    return (rank, nll, pred, z) if return_logits else (rank, nll, pred)


def eval_summary(stats: torch.Tensor, k: int) -> dict:
    """The counters of :func:`softmax_eval` / ``AlexNetFull.evaluate`` as numbers: ``{"count", "top1_error",
    "topk_error", "loss", "k"}`` (the errors and the mean loss are NaN while nothing is counted). Copying the four
    counters to the host is the one place of an evaluation that waits for the device."""
    if not isinstance(stats, torch.Tensor) or tuple(stats.shape) != (EVAL_STATS,) or stats.dtype != torch.int64:
        raise ValueError(f"eval_summary: stats must be the int64 [{EVAL_STATS}] tensor of softmax_eval")
    count, top1, topk, nll_q32 = (int(v) & (2 ** 64 - 1) for v in stats.tolist())  # the kernel's counters are unsigned
    nan = float("nan")
    return {"count": count, "top1_error": 1.0 - top1 / count if count else nan,
            "topk_error": 1.0 - topk / count if count else nan,
            "loss": nll_q32 / 2.0 ** 32 / count if count else nan, "k": int(k)}


def relu(x: torch.Tensor, inplace: bool = False) -> torch.Tensor:
    _check(x, "relu")
    y = x if inplace else x.clone()
    if y.is_cuda:
        nat.call("anx_relu", nat.ptr(y), y.numel(), nat.stream_ptr(y.device))
    else:
        y.clamp_(min=0.0)  # host ReLU is part of anx_cpu_conv2d (relu=True); standalone it is one clamp
    return y


def maxpool(x: torch.Tensor, size: int = 3, stride: int = 2, impl: str = "vec4") -> torch.Tensor:
    _check(x, "maxpool")
    N, H, W, Cn = x.shape
    Ho, Wo = pool_out_dim(H, size, stride), pool_out_dim(W, size, stride)
    y = torch.empty((N, Ho, Wo, Cn), device=x.device, dtype=torch.float32)
    if not x.is_cuda:
        nat.call("anx_cpu_maxpool", nat.ptr(x), nat.ptr(y), N, H, W, Cn, size, stride)
    elif impl == "direct" or Cn % 4:
        nat.call("anx_maxpool_direct", nat.ptr(x), nat.ptr(y), N, H, W, Cn, size, stride, nat.stream_ptr(x.device))
    else:
        nat.call("anx_maxpool", nat.ptr(x), N, H, W, Cn, size, stride, nat.ptr(y), Ho, Wo, Cn, 0, 0, 0,
                 nat.stream_ptr(x.device))
    return y


def lrn(x: torch.Tensor, size: int = 5, alpha: float = 1e-4, beta: float = 0.75, k: float = 2.0,
        mode: str = "div_n") -> torch.Tensor:
    _check(x, "lrn")
    N, H, W, Cn = x.shape
    y = torch.empty_like(x)
    m = _LRN_MODES[mode]
    if x.is_cuda:
        nat.call("anx_lrn_direct", nat.ptr(x), nat.ptr(y), N, H, W, Cn, size, alpha, beta, k, m,
                 nat.stream_ptr(x.device))
    else:
        nat.call("anx_cpu_lrn", nat.ptr(x), nat.ptr(y), N, H, W, Cn, size, alpha, beta, k, m)
    return y


def maxpool_lrn(x: torch.Tensor, pool: int = 3, stride: int = 2, size: int = 5, alpha: float = 1e-4,
                beta: float = 0.75, k: float = 2.0, mode: str = "div_n") -> torch.Tensor:
    """Fused max-pool + LRN (one kernel on the GPU; pool then LRN on the host)."""
    _check(x, "maxpool_lrn")
    if not x.is_cuda or x.shape[3] % 4:
        return lrn(maxpool(x, pool, stride), size, alpha, beta, k, mode)
    N, H, W, Cn = x.shape
    y = torch.empty((N, pool_out_dim(H, pool, stride), pool_out_dim(W, pool, stride), Cn), device=x.device)
    nat.call("anx_maxpool_lrn", nat.ptr(x), nat.ptr(y), N, H, W, Cn, pool, stride, size, alpha, beta, k,
             _LRN_MODES[mode], nat.stream_ptr(x.device))
    return y
