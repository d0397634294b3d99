"""Full AlexNet (extension model family, BASELINE.json config "Full AlexNet Conv1-5 + FC6-8 bf16,
batch=2048"): the reference's Blocks 1-2 (Conv1-ReLU-Pool1-Conv2-ReLU-Pool2-LRN2) followed by the
AlexNet tail Conv3/4/5 (3x3, pad 1) + Pool5 + FC6/FC7/FC8, inference in bf16 with fp32 accumulation
on v_mfma_f32_32x32x16_bf16 (csrc/src/hip/conv_bf16.hip, csrc/src/full_engine.cpp).

The reference itself stops after Block 2; this family exists because the benchmark
configs name it. FC layers run on the same implicit-GEMM kernel as 1x1 convolutions.

Input is NHWC ``[N,227,227,3]`` on the device, contiguous: ``float32``, or ``torch.uint8`` byte images. A byte
``b`` of channel ``c`` means ``fmaf(float(b), scale[c], offset[c])`` in fp32 (:func:`anx.ops.decode_u8`), with
``scale = 1/255`` and ``offset = 0`` unless ``input_norm=(mean, std)`` (0-255 pixel units) sets ``scale = 1/std``,
``offset = -mean/std``; logits and taps equal those of the float forward of :meth:`AlexNetFull.decode_u8`, bit for
bit. With the default Conv1 (``bf16_conv1`` 2) and knob ``bf16_u8=1`` the row-band kernel loads the bytes itself
(``last_input() == "u8_ring"``, no float copy of the input on the device); everywhere else the launch chunk is
decoded into a workspace that the first such forward allocates (``"u8_decode"``: warm up once before capturing a
graph) and the float kernels run on it.

Byte images of any other size go through :meth:`AlexNetFull.forward_images` / :meth:`AlexNetFull.classify_images`:
one :func:`anx.ops.resize_crop_u8` launch (antialiased resize + centre crop, integer arithmetic) into a byte workspace
of the model, then the byte path above. ``classify_images(views="ten")`` is AlexNet's ten-view protocol (corner and
centre crops and their mirror images, one resize launch for all of them) on ``classify(views=10)``, whose head
kernel averages the views' softmax outputs on chip (:func:`anx.ops.softmax_topk_views`).

:meth:`AlexNetFull.evaluate` / :meth:`AlexNetFull.evaluate_images` hold the model to labels on the chip
(:func:`anx.ops.softmax_eval`): per image the rank of the true class, the loss and the prediction, and running device
counters that :func:`anx.ops.eval_summary` turns into top-1 / top-k error and mean loss once the set is through.
"""
from __future__ import annotations

import ctypes as C
from typing import NamedTuple

import numpy as np
import torch
import torch.nn.functional as F

from .. import _native as nat
from ..utils.init import STREAM_EXTRA, uniform
from ..utils.tuning import apply_knobs, knob_value
from .alexnet_blocks import norm_scale_offset
from .lanes import Lanes

LAYERS = ("conv1", "conv2", "conv3", "conv4", "conv5", "fc6", "fc7", "fc8")
FLOPS_PER_IMAGE = 2.0 * (55 * 55 * 96 * 363 + 27 * 27 * 256 * 2400 + 13 * 13 * 384 * 2304 + 13 * 13 * 384 * 3456 +
                         13 * 13 * 256 * 3456 + 9216 * 4096 + 4096 * 4096 + 4096 * 1000)


def weight_shapes(classes: int = 1000, groups2: int = 1):
    wn, bn = (C.c_size_t * 8)(), (C.c_size_t * 8)()
    nat.call("anx_full_weight_sizes", classes, groups2, wn, bn)
    conv = [(96, 3, 11, 11), (256, 96 // groups2, 5, 5), (384, 256, 3, 3), (384, 384, 3, 3), (256, 384, 3, 3)]
    fc = [(4096, 9216), (4096, 4096), (classes, 4096)]
    shapes = conv + fc
    assert [int(np.prod(s)) for s in shapes] == list(wn)
    return shapes, [int(b) for b in bn]


def init_full_weights(seed: int = 0, classes: int = 1000, groups2: int = 1) -> dict:
    """He-uniform weights from the counter-based RNG (deterministic on every rank), zero biases."""
    shapes, bsz = weight_shapes(classes, groups2)
    out = {}
    for i, (name, s) in enumerate(zip(LAYERS, shapes)):
        fan_in = int(np.prod(s[1:]))
        bound = float(np.sqrt(6.0 / fan_in))
        u = uniform(seed, STREAM_EXTRA + i, int(np.prod(s)))
        out["w_" + name] = torch.from_numpy(((u * 2 - 1) * bound).astype(np.float32).reshape(s))
        out["b_" + name] = torch.zeros(bsz[i])
    return out


class _Head(NamedTuple):
    """The classifier head of a call: ``indices`` / ``probs`` ``[N,k]`` outputs; ``views`` rows of ``x`` per image for
    the view-averaging head, 0 for one row per image ranked by logit (``views=1`` is not 0: it ranks by probability)."""
    k: int
    idx: torch.Tensor
    prob: torch.Tensor
    views: int = 0

    def part(self, lo: int, hi: int) -> "_Head":
        """The head of images ``lo .. hi`` (a lane's share)."""
        return self._replace(idx=self.idx[lo:hi], prob=self.prob[lo:hi])

    def describe(self, call) -> None:
        call.k, call.idx, call.prob, call.views = self.k, self.idx.data_ptr(), self.prob.data_ptr(), self.views


class _EvalHead(NamedTuple):
    """The evaluation head of a call: ``labels`` and the per-image outputs ``rank`` / ``nll`` / ``pred`` ``[N]``, the
    running counters ``stats`` and ``confusion`` (either may be None), ``k`` the top-k threshold; ``views`` as in
    :class:`_Head`."""
    k: int
    labels: torch.Tensor
    rank: torch.Tensor
    nll: torch.Tensor
    pred: torch.Tensor
    stats: torch.Tensor | None = None
    confusion: torch.Tensor | None = None
    views: int = 0

    def part(self, lo: int, hi: int) -> "_EvalHead":
        """The head of images ``lo .. hi`` (a lane's share): every lane adds into the same counters."""
        return self._replace(labels=self.labels[lo:hi], rank=self.rank[lo:hi], nll=self.nll[lo:hi], pred=self.pred[lo:hi])

    def describe(self, call) -> None:
        call.k, call.views = self.k, self.views
        call.labels, call.rank, call.nll, call.pred = (t.data_ptr() for t in (self.labels, self.rank, self.nll, self.pred))
        call.stats = self.stats.data_ptr() if self.stats is not None else None
        call.confusion = self.confusion.data_ptr() if self.confusion is not None else None


class AlexNetFull:
    def __init__(self, weights: dict | None = None, *, seed: int = 0, classes: int = 1000, device="cuda",
                 max_batch: int = 1, groups2: int = 1, lrn_mode: str = "div_n", knobs: dict | None = None,
                 lanes: int = 1, input_norm=None):
        self.classes, self.groups2, self.lrn_mode = classes, groups2, lrn_mode
        self.knobs = {k: knob_value(k, v) for k, v in (knobs or {}).items()}  # e.g. {"bf16_glds": 3}
        self.weights = {k: v.detach().to("cpu", torch.float32).contiguous()
                        for k, v in (weights or init_full_weights(seed, classes, groups2)).items()}
        self.device = torch.device(device)
        if self.device.type != "cuda":
            raise ValueError("the bf16 full-AlexNet engine is GPU-only (use reference_forward on the CPU)")
        self._h = None
        self._cap = 0
        self._img_ws, self._img_cap = None, 0  # byte workspace of forward_images / classify_images (lane 0's model)
        self.input_norm = input_norm
        self._norm = norm_scale_offset(input_norm, 3)
        if lanes < 1:
            raise ValueError("lanes must be >= 1")
        per_lane = -(-max(1, max_batch) // lanes)
        self._ensure(per_lane)  # lane 0's share; a forward of more images on lane 0 alone grows it
        # lanes > 1: the batch is split over engines on concurrent HIP streams (forked from / joined to
        # the caller's stream; anx.models.lanes defines the order), so one lane's partial last rounds overlap the
        # other's kernels. Measured slower at 256 images (281k vs 305k img/s: half-size launches of
        # the 1-workgroup-per-CU kernels quantize worse), 334k at 512 as 2 x 256
        # (profiles/r02_ab_full_lanes.txt)
        self._lanes: list[AlexNetFull] = []
        for _ in range(lanes - 1):
            self._lanes.append(AlexNetFull(self.weights, classes=classes, device=self.device, max_batch=per_lane,
                                           groups2=groups2, lrn_mode=lrn_mode, knobs=self.knobs,
                                           input_norm=input_norm))
        self._streams = Lanes(self.device, lanes, 1)  # any batch of at least one image per lane is split

    def _lane(self, i: int) -> "AlexNetFull":
        """The model whose engine runs lane ``i``: this one for lane 0, else a side lane's."""
        return self._lanes[i - 1] if i else self

    def _ensure(self, n):
        """Grow THIS engine to n images (the other lanes' engines are untouched)."""
        if self._h is not None and n <= self._cap:
            return
        if self._h is not None:
            torch.cuda.synchronize(self.device)
            nat.bf16().anx_full_destroy(self._h)
            self._h = None
        ws = (C.c_void_p * 8)(*[self.weights["w_" + k].data_ptr() for k in LAYERS])
        bs = (C.c_void_p * 8)(*[self.weights["b_" + k].data_ptr() for k in LAYERS])
        h = C.c_void_p()
        with torch.cuda.device(self.device):
            nat.call("anx_full_create", C.byref(h), ws, bs, self.classes, max(1, n), self.groups2,
                     0 if self.lrn_mode == "div_n" else 1)
        try:
            apply_knobs(h, self.knobs, full=True)
            nat.call("anx_full_set_input_norm", h, self._norm[0].data_ptr(), self._norm[1].data_ptr())
        except Exception:
            nat.bf16().anx_full_destroy(h)
            raise
        self._h, self._cap = h, max(1, n)

    def set_knob(self, name: str, value) -> None:
        v = knob_value(name, value)
        apply_knobs(self._h, {name: v}, full=True)
        self.knobs[name] = v
        for m in getattr(self, "_lanes", ()):
            m.set_knob(name, v)

    def set_input_norm(self, mean=None, std=None) -> None:
        """Meaning of byte input from now on (every lane): ``(mean, std)`` in 0-255 pixel units, a number or one
        per channel each; no arguments: back to ``byte / 255``."""
        if (mean is None) != (std is None):
            raise ValueError("set_input_norm takes both mean and std, or neither")
        norm = None if mean is None else (mean, std)
        self._norm = norm_scale_offset(norm, 3)
        self.input_norm = norm
        nat.call("anx_full_set_input_norm", self._h, self._norm[0].data_ptr(), self._norm[1].data_ptr())
        for m in getattr(self, "_lanes", ()):
            m.set_input_norm(mean, std)

    def decode_u8(self, x: torch.Tensor) -> torch.Tensor:
        """The float32 image this model's byte input means (:func:`anx.ops.decode_u8` with its scale / offset)."""
        from ..ops import decode_u8
        return decode_u8(x, self._norm[0], self._norm[1])

    def last_input(self, lane: int = 0) -> str | None:
        """How the last forward of this model's engine (``lane`` > 0: that side lane's) fed Conv1: ``"f32"`` (float
        input), ``"u8_ring"`` (the row-band Conv1 loaded the bytes), ``"u8_decode"`` (decode kernel, then the float
        path); ``None`` before the first. Recorded at the launch; reading it makes no device call."""
        return nat.read_str("anx_full_last_input", self._lane(lane)._h, 32)

    def close(self):
        for m in getattr(self, "_lanes", ()):
            m.close()
        if self._h is not None:
            torch.cuda.synchronize(self.device)
            nat.bf16().anx_full_destroy(self._h)
            self._h = None

    def __del__(self):  # pragma: no cover
        try:
            self.close()
        except Exception:
            pass

    def _check_x(self, x: torch.Tensor) -> None:
        if (x.dim() != 4 or tuple(x.shape[1:]) != (227, 227, 3) or x.dtype not in (torch.float32, torch.uint8)
                or not x.is_contiguous() or x.device != self.device):
            raise ValueError(f"expected contiguous fp32 (or uint8: byte images) NHWC [N,227,227,3] on {self.device}, got "
                             f"{tuple(x.shape)} {x.dtype} on {x.device}")

    def _check(self, x: torch.Tensor, out: torch.Tensor | None) -> torch.Tensor:
        """The engine reads x and writes out through raw pointers: both must be exactly what the
        kernels assume (shape, dtype, contiguity, device)."""
        self._check_x(x)
        shape = (x.shape[0], self.classes)
        if out is None:
            return torch.empty(shape, device=self.device)
        if (tuple(out.shape) != shape or out.dtype != torch.float32 or not out.is_contiguous()
                or out.device != self.device):
            raise ValueError(f"out must be a contiguous fp32 {shape} tensor on {self.device}, got "
                             f"{tuple(out.shape)} {out.dtype} on {out.device}")
        return out

    def forward(self, x: torch.Tensor, out: torch.Tensor | None = None) -> torch.Tensor:
        """x: [N,227,227,3] fp32 (or uint8: byte images) NHWC on the device -> logits [N, classes] fp32."""
        y = self._check(x, out)
        self._run(x, y, None)
        return y

    __call__ = forward

    def forward_async(self, x: torch.Tensor, out: torch.Tensor, on_lane=None, pre_lane=None) -> torch.Tensor:
        """Throughput form for repeated forwards on the same buffers (contract and hooks:
        :meth:`anx.models.lanes.Lanes.run_free`): lanes on their own streams, never joined per call; when all
        are idle they fork from the current stream and lane i starts at lane i-1's mid-forward mark
        (after Conv2 + Pool2/LRN), so they run half a forward apart. :meth:`join` before reading out."""
        out = self._check(x, out)
        self._run(x, out, None, True, pre_lane, on_lane)
        return out

    def _launch(self, x, z, head, stream, mark: bool) -> None:
        """This engine's one native call on images ``x`` (the only place that names the entry point): the forward
        into logits ``z``, or with a :class:`_Head` / :class:`_EvalHead` the call with that head (``z`` may be None).
        ``stream`` None: the current stream. ``mark``: record the mid-forward mark that ``anx_full_wait_mark`` waits for."""
        call = nat.FullCallC(x=x.data_ptr(), u8=int(x.dtype == torch.uint8), rows=x.shape[0],
                             logits=z.data_ptr() if z is not None else None, mark=int(mark))
        if head is not None:
            head.describe(call)
        nat.call("anx_full_run", self._h, C.byref(call), stream if stream is not None else nat.stream_ptr(self.device))

    def _run(self, x, z, head, free: bool = False, pre_lane=None, on_lane=None) -> None:
        """:meth:`_launch` of every lane's slice through :mod:`anx.models.lanes`: forked and joined within the
        call, or (``free``) left running on the lanes' streams until :meth:`join`. A head with views splits on image
        boundaries: the lanes divide the ``N`` images, and image ``i`` is rows ``i V .. (i + 1) V`` of ``x`` and
        ``z``."""
        V = (head.views if head is not None else 0) or 1

        def run(i, lo, hi, st=None, lead=False):
            eng = self._lane(i)
            eng._ensure((hi - lo) * V)
            eng._launch(x[lo * V:hi * V], z[lo * V:hi * V] if z is not None else None,
                        head.part(lo, hi) if head is not None else None,
                        st.cuda_stream if st is not None else None, lead)
            if lead:
                return lambda s: nat.call("anx_full_wait_mark", eng._h, s.cuda_stream)

        if free:
            # growing an engine may synchronise the device: before its lane's waits, not between them and the call
            self._streams.run_free(x.shape[0] // V, run, pre_lane, on_lane,
                                   prepare=lambda i, lo, hi: self._lane(i)._ensure((hi - lo) * V))
        else:
            self._streams.run_joined(x.shape[0] // V, run)

    def _check_views(self, x, views) -> int:
        """``views`` of :meth:`classify` as the head takes it: 0 for None, else the rows per image of ``x``."""
        from ..ops import MAX_VIEWS, VIEWS_MAX_CLASSES
        if views is None:
            return 0
        if not isinstance(views, int) or isinstance(views, bool) or not 1 <= views <= MAX_VIEWS:
            raise ValueError(f"views must be None or an integer 1 .. {MAX_VIEWS}, got {views!r}")
        if x.shape[0] % views:
            raise ValueError(f"{x.shape[0]} rows are no whole number of images of {views} views")
        if self.classes > VIEWS_MAX_CLASSES:
            raise ValueError(f"the view-averaging head takes at most {VIEWS_MAX_CLASSES} classes")
        return views

    def _check_head(self, x, k, idx, prob, views=0) -> _Head:
        """classify's head: ``k`` checked, the outputs validated like ``out`` in :meth:`_check`, allocated when not
        given."""
        from ..ops import MAX_TOPK
        kmax = min(self.classes, MAX_TOPK)
        if not isinstance(k, int) or isinstance(k, bool) or not 1 <= k <= kmax:
            raise ValueError(f"k must be an integer with 1 <= k <= min(classes, {MAX_TOPK}) = {kmax}, got {k!r}")
        shape = (x.shape[0] // (views or 1), k)
        outs = []
        for t, dt, name in ((idx, torch.int32, "indices"), (prob, torch.float32, "probabilities")):
            if t is None:
                t = torch.empty(shape, device=self.device, dtype=dt)
            elif tuple(t.shape) != shape or t.dtype != dt or not t.is_contiguous() or t.device != self.device:
                raise ValueError(f"{name} must be a contiguous {dt} {shape} tensor on {self.device}, got "
                                 f"{tuple(t.shape)} {t.dtype} on {t.device}")
            outs.append(t)
        return _Head(k, *outs, views)

    def classify(self, x: torch.Tensor, k: int = 5, *, views: int | None = None, return_logits: bool = False, out=None):
        """x as in :meth:`forward` -> ``(indices [N,k] int32, probs [N,k] fp32)``: the ``k`` most likely classes of
        each image (logit descending, then class index ascending) and their softmax probabilities, equal bit for bit
        to ``anx.ops.softmax_topk(forward(x), k)``. ``return_logits`` appends the ``[N, classes]`` logits, the bits
        :meth:`forward` gives. ``out``: ``(indices, probs)`` or ``(indices, probs, logits)`` tensors to write into.
        Where FC8 ran split-K, the head kernel reduces the slabs itself (knob ``bf16_head``), so without
        ``return_logits`` the logits never reach device memory; :meth:`last_head` tells. Lanes as :meth:`forward`.

        ``views=V`` (1 to 32): ``x`` is ``[N * V,227,227,3]``, ``V`` consecutive views per image, and the outputs are
        ``[N,k]``: the ``k`` classes of the largest mean softmax probability over an image's views and that mean,
        equal bit for bit to ``anx.ops.softmax_topk_views(forward(x), V, k)``; the head kernel averages on chip, on
        FC8's slabs where there are any. Lanes split on image boundaries; ``return_logits`` gives
        ``[N * V, classes]``. ``views=None`` is the call without views."""
        out = tuple(out) if out is not None else ()
        if len(out) not in (0, 2, 3):
            raise ValueError("out must be (indices, probs) or (indices, probs, logits)")
        want_logits = return_logits or len(out) == 3
        self._check_x(x)
        views = self._check_views(x, views)
        z = self._check(x, out[2] if len(out) == 3 else None) if want_logits else None
        head = self._check_head(x, k, *(out[:2] if out else (None, None)), views)
        self._run(x, z, head)
        return (head.idx, head.prob, z) if want_logits else (head.idx, head.prob)

    def _preprocess(self, images, resize, views=None) -> torch.Tensor:
        """``images`` (as :func:`anx.ops.resize_crop_u8` takes them) -> ``uint8 [N,227,227,3]`` in the model-owned
        byte workspace, by one :func:`anx.ops.resize_crop_u8` launch on the current stream (``center_box`` boxes).
        ``views="ten"``: ``[10 N,227,227,3]``, each image's :func:`anx.ops.ten_crop_boxes` views, still one launch
        (every view names its source image, none is copied)."""
        from ..ops import resize_crop_u8, ten_crop_boxes
        if views not in (None, "ten"):
            raise ValueError(f'views must be None or "ten", got {views!r}')
        n = images.shape[0] if isinstance(images, torch.Tensor) else len(images)
        for im in ((images,) if isinstance(images, torch.Tensor) else images):
            if isinstance(im, torch.Tensor) and im.device != self.device:
                raise ValueError(f"expected images on {self.device}, got one on {im.device}")
        more = {}
        if views == "ten":
            boxes, flips, source = [], [], []
            for i in range(n):
                im = images[i]
                if not isinstance(im, torch.Tensor) or im.dim() != 3:
                    raise ValueError("every image must be a uint8 [H,W,3] tensor")
                b, f = ten_crop_boxes(im.shape[0], im.shape[1], resize, 227)
                boxes += b
                flips += f
                source += [i] * 10
            more = {"boxes": boxes, "flips": flips, "source": source}
            n *= 10
        if self._img_ws is None or n > self._img_cap:
            # the old workspace goes back to torch's allocator, which hands it out again in stream order
            self._img_cap = max(1, n)
            self._img_ws = torch.empty((self._img_cap, 227, 227, 3), device=self.device, dtype=torch.uint8)
        return resize_crop_u8(images, 227, resize, out=self._img_ws[:n], **more)

    def forward_images(self, images, out: torch.Tensor | None = None, resize: int | None = 256) -> torch.Tensor:
        """Byte images of any size -> logits ``[N, classes]``: ``images`` is a list of ``uint8 [H,W,3]`` tensors (each
        its own size) or one ``[N,H,W,3]`` tensor on the model's device. Each image is resized and centre-cropped to
        227 x 227 ("shorter side to ``resize``, centre crop 227": :func:`anx.ops.center_box`; ``resize=None``
        resamples the whole image) by :func:`anx.ops.resize_crop_u8`, one kernel for the batch, into a byte
        workspace the model owns; then the byte forward runs on it, so lanes, ``input_norm``, :meth:`last_input`
        (``"u8_ring"`` by default) and :meth:`last_head` mean what they mean for :meth:`forward`. The result equals
        ``forward(anx.ops.resize_crop_u8(images, 227, resize))`` bit for bit. The workspace grows to the largest
        batch seen, like the engine itself, and each call copies its image descriptors to the device: call once with
        the largest batch before capturing a graph, as for the ``"u8_decode"`` workspace."""
        return self.forward(self._preprocess(images, resize), out)

    def classify_images(self, images, k: int = 5, resize: int | None = 256, return_logits: bool = False, views=None):
        """:meth:`classify` of byte images of any size (``images``, ``resize`` and the workspace as in
        :meth:`forward_images`): equal bit for bit to ``classify(anx.ops.resize_crop_u8(images, 227, resize), k)``.

        ``views="ten"``: AlexNet's ten-view protocol. Each image's four corner crops, centre crop and their mirror
        images (:func:`anx.ops.ten_crop_boxes`, all at the centre crop's scale) are cut by one
        :func:`anx.ops.resize_crop_u8` launch of ``10 N`` outputs into the byte workspace, and
        ``classify(..., views=10)`` ranks the mean of the ten softmax outputs; ``return_logits`` gives
        ``[10 N, classes]``."""
        return self.classify(self._preprocess(images, resize, views), k, views=10 if views == "ten" else None,
                             return_logits=return_logits)

    def classify_async(self, x: torch.Tensor, idx_out: torch.Tensor, prob_out: torch.Tensor, k: int = 5, on_lane=None,
                       pre_lane=None, views: int | None = None):
        """:meth:`classify` in the throughput form of :meth:`forward_async` (same contract: free-running lanes on
        their own streams, lane i starting at lane i-1's mid-forward mark when all are idle, never joined per call):
        writes ``idx_out`` ``[N,k]`` int32 and ``prob_out`` ``[N,k]`` fp32. :meth:`join` before reading them.
        ``views`` as in :meth:`classify` (the hooks then get image bounds, not row bounds)."""
        self._check_x(x)
        head = self._check_head(x, k, idx_out, prob_out, self._check_views(x, views))
        self._run(x, None, head, True, pre_lane, on_lane)
        return head.idx, head.prob

    def _check_eval(self, x, labels, k, views, stats, confusion, out) -> _EvalHead:
        """evaluate's head: ``k`` and ``views`` checked as classify checks them, ``labels``, ``stats``, ``confusion``
        and ``out`` validated like ``out`` in :meth:`_check` (dtype, shape, contiguity, device), the per-image outputs
        allocated when not given."""
        from ..ops import EVAL_MAX_CLASSES, MAX_TOPK, _eval_outputs
        self._check_x(x)
        views = self._check_views(x, views)
        kmax = min(self.classes, MAX_TOPK)
        if not isinstance(k, int) or isinstance(k, bool) or not 1 <= k <= kmax:
            raise ValueError(f"k must be an integer with 1 <= k <= min(classes, {MAX_TOPK}) = {kmax}, got {k!r}")
        if not views and self.classes > EVAL_MAX_CLASSES:
            raise ValueError(f"the evaluation head takes at most {EVAL_MAX_CLASSES} classes without views")
        N = x.shape[0] // (views or 1)
        rank, nll, pred = _eval_outputs("evaluate", N, self.classes, self.device, labels, stats, confusion, out)
        return _EvalHead(k, labels, rank, nll, pred, stats, confusion, views)

    def evaluate(self, x: torch.Tensor, labels: torch.Tensor, k: int = 5, *, views: int | None = None,
                 stats: torch.Tensor | None = None, confusion: torch.Tensor | None = None, out=None):
        """x as in :meth:`forward`, held to ``labels`` (``int32 [N]`` on the model's device; with ``views`` one per
        image, not per row) -> ``(rank [N] int32, nll [N] fp32, pred [N] int32)``: the number of classes that rank
        before the true one, the negative log-likelihood and the top-1 prediction, equal bit for bit to
        ``anx.ops.softmax_eval(forward(x), labels, k, views=views)`` (which has the definitions). The evaluation head
        kernel runs where :meth:`classify`'s runs (on FC8's split-K slabs with knob ``bf16_head``; :meth:`last_head`
        tells), so the logits never reach device memory.

        ``stats`` (``int64 [4]``, zeroed once by the caller) and ``confusion`` (``int32 [classes, classes]``) are
        running device counters that every call adds into: images, top-1 hits, top-``k`` hits, the loss in fixed
        point, and ``[label, pred]`` counts. A label outside ``0 .. classes-1`` (``-1`` padding) leaves them alone.
        They are integer sums: lanes, launch chunks and workgroups may finish in any order and the totals are the
        same bits. Nothing here synchronises: run the whole validation set, then read
        ``anx.ops.eval_summary(stats, k)``. ``views`` and lanes as in :meth:`classify`; every lane adds into the
        same ``stats`` and ``confusion``. ``out``: ``(rank, nll, pred)`` tensors to write into."""
        head = self._check_eval(x, labels, k, views, stats, confusion, out)
        self._run(x, None, head)
        return head.rank, head.nll, head.pred

    def evaluate_async(self, x: torch.Tensor, labels: torch.Tensor, k: int = 5, *, views: int | None = None,
                       stats: torch.Tensor | None = None, confusion: torch.Tensor | None = None, out=None,
                       on_lane=None, pre_lane=None):
        """:meth:`evaluate` in the throughput form of :meth:`forward_async` (free-running lanes on their own streams,
        never joined per call). :meth:`join` before reading the outputs, ``stats`` or ``confusion``."""
        head = self._check_eval(x, labels, k, views, stats, confusion, out)
        self._run(x, None, head, True, pre_lane, on_lane)
        return head.rank, head.nll, head.pred

    def evaluate_images(self, images, labels: torch.Tensor, k: int = 5, resize: int | None = 256, views=None, *,
                        stats: torch.Tensor | None = None, confusion: torch.Tensor | None = None, out=None):
        """:meth:`evaluate` of byte images of any size (``images``, ``resize`` and the workspace as in
        :meth:`forward_images`). ``views="ten"`` is AlexNet's evaluation protocol end to end: the ten crops of
        :meth:`classify_images`, the forward, and top-1 / top-``k`` hits and the log loss of the averaged
        prediction, counted on the device."""
        return self.evaluate(self._preprocess(images, resize, views), labels, k, views=10 if views == "ten" else None,
                             stats=stats, confusion=confusion, out=out)

    def last_head(self, lane: int = 0) -> str | None:
        """What the head of the last call of this model's engine (``lane`` > 0: that side lane's) read: ``"slabs"``
        (it reduced FC8's split-K slabs itself), ``"logits"`` (logits FC8 or the split-K reduce wrote), ``None`` when
        that call was a plain forward. Recorded at the launch; reading it makes no device call."""
        return nat.read_str("anx_full_last_head", self._lane(lane)._h, 32)

    def lane_bounds(self, n: int) -> list[int]:
        """Image boundaries [0, ..., n] of the lanes :meth:`forward_async` runs ``n`` images on (the
        pipeline's per-lane gather segments; ScatterComputeGather's root shedding needs them)."""
        return self._streams.bounds(n)

    def join(self) -> None:
        """Make the current stream wait for every lane of :meth:`forward_async` / :meth:`classify_async`."""
        self._streams.join()

    TAPS = ((55, 55, 96), (31, 31, 96), (27, 27, 256), (15, 15, 256), (15, 15, 384), (15, 15, 384), (13, 13, 256),
            (9216,), (4096,), (4096,), (57, 57, 48))

    def tap(self, i: int, N: int) -> torch.Tensor:
        """bf16 activation ``i`` of the last forward (see FullEngine::tap): conv1, pool1 window,
        conv2, pool2+LRN window, conv3/conv4 windows, conv5, pool5, fc6, fc7; 10: the bf16
        polyphase (space-to-depth by 4) input of conv1. Tap 0 holds conv1 only when the forward
        wrote it: with pool1 fused into the Conv1 kernel (knob ``bf16_pool1``, one workgroup per
        image) the 55x55 map never leaves the kernel."""
        y = torch.empty((N, *self.TAPS[i]), device=self.device, dtype=torch.bfloat16)
        n = C.c_size_t()
        nat.call("anx_full_tap", self._h, i, N, y.data_ptr(), C.byref(n), nat.stream_ptr(self.device))
        return y

    def last_path(self, lane: int = 0) -> dict:
        """Which kernels the last forward of this model's engine launched (``lane`` > 0: that side lane's
        engine; of a chunked forward, the last chunk): ``{"conv1": {"form": "ring_f32_pool" | "ring_f32" |
        "ring" | "tiles" | "taps8", "segs": workgroups per image of the ring forms or None}, "conv2" ..
        "conv5", "fc6" .. "fc8": {"kernel": "big" | "glds" | "staged", "id": wide-tile config | LDS-DMA
        slots | tile variant, "splitk": K slices}}``, ``None`` for a layer that has not run. The engine
        records it where it launches, and reading it makes no device call."""
        import json
        return json.loads(nat.read_str("anx_full_last_path", self._lane(lane)._h, 1024))


def reference_forward(x: torch.Tensor, w: dict, groups2: int = 1, lrn_mode: str = "div_n",
                      dtype=torch.float32) -> torch.Tensor:
    """Plain PyTorch oracle (NHWC in, logits out) of the same topology."""
    h = x.permute(0, 3, 1, 2).to(dtype)
    g = lambda k: w[k].to(h.device, dtype)  # noqa: E731
    h = F.max_pool2d(F.relu(F.conv2d(h, g("w_conv1"), g("b_conv1"), stride=4)), 3, 2)
    h = F.max_pool2d(F.relu(F.conv2d(h, g("w_conv2"), g("b_conv2"), padding=2, groups=groups2)), 3, 2)
    a = 1e-4 if lrn_mode == "div_n" else 1e-4 * 5
    h = F.local_response_norm(h, 5, alpha=a, beta=0.75, k=2.0)
    h = F.relu(F.conv2d(h, g("w_conv3"), g("b_conv3"), padding=1))
    h = F.relu(F.conv2d(h, g("w_conv4"), g("b_conv4"), padding=1))
    h = F.max_pool2d(F.relu(F.conv2d(h, g("w_conv5"), g("b_conv5"), padding=1)), 3, 2)
    h = h.permute(0, 2, 3, 1).reshape(h.shape[0], -1)  # NHWC flatten (the engine's FC6 input order)
    h = F.relu(F.linear(h, g("w_fc6"), g("b_fc6")))
    h = F.relu(F.linear(h, g("w_fc7"), g("b_fc7")))
    return F.linear(h, g("w_fc8"), g("b_fc8"))
