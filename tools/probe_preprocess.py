#!/usr/bin/env python3
"""Probe: what the resize + crop kernel saves in front of the bf16 full AlexNet.

Two device-resident image sets, `--images` (256) byte images each: 375x500 (a typical photograph: the centre box is
333 x 333, scale 1.47) and 256x256 (box 227 x 227 at a half-pixel origin, scale 1). Each step ends with the top-k
answer on the device. Arms, interleaved in one process on one GPU:

  a  images      classify_images: one resize_crop_u8 launch into the model's byte workspace, then classify
  b  torch       what a caller had to do before: the images as one float NCHW tensor through
                 F.interpolate(mode="bilinear", antialias=True) to "shorter side 256", centre crop 227, round, clamp,
                 to NHWC bytes, then classify. The set is one [N,H,W,3] tensor, so torch resizes the whole batch in
                 one call: its best case (a list of images of different sizes needs a call per image).
  c  kernel      resize_crop_u8 alone into a preallocated output; its achieved GB/s over source-box bytes + output bytes
  d  classify    classify alone on bytes that are already 227 x 227, for scale

Before any timing the kernel is compared with torch's antialiased resize on the same geometry (16 whole images onto
227 x 227): two roundings of the same filter (fixed point / fp32), so they may differ by one level on a small share
of the bytes, which is reported, and nowhere by more. (The timed routes place the crop slightly differently: torch
resizes to an integer size and crops at an integer offset, center_box keeps the half pixel.) Then `--rounds`
rounds, each timing every arm once in turn (so drift and neighbours hit all arms alike): untimed warm-up steps, a
device synchronise, then `--steps` steps between two device events. One JSON line per (round, set, arm) and a summary
line per (set, arm) (median, min, max over the rounds) go to --out/probe.jsonl. Needs a GPU: there is no CPU fallback.

usage: tools/probe_preprocess.py [--images 256] [--rounds 7] [--out profiles/preprocess]
"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
os.environ["GPU_MAX_HW_QUEUES"] = os.environ.get("ANX_HW_QUEUES", "8")  # as bench.py; read at HIP's first call

import torch  # noqa: E402
import torch.nn.functional as F  # noqa: E402

import anx  # noqa: E402,F401
from anx.models.alexnet_full import AlexNetFull  # noqa: E402
from anx.ops import center_box, resize_crop_u8  # noqa: E402

MEAN, STD = (123.7, 116.3, 103.5), (58.4, 57.1, 57.4)
SETS = (("375x500", 375, 500), ("256x256", 256, 256))


def torch_preprocess(x, resize=256, size=227):
    """[N,H,W,3] bytes -> [N,size,size,3] bytes the torch way: shorter side to `resize`, centre crop, round, clamp."""
    _, H, W, _ = x.shape
    m = min(H, W)
    nh, nw = max(size, round(H * resize / m)), max(size, round(W * resize / m))
    f = F.interpolate(x.permute(0, 3, 1, 2).float(), size=(nh, nw), mode="bilinear", antialias=True, align_corners=False)
    t, l = (nh - size) // 2, (nw - size) // 2
    return f[:, :, t:t + size, l:l + size].round().clamp(0, 255).to(torch.uint8).permute(0, 2, 3, 1).contiguous()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--images", type=int, default=256)
    ap.add_argument("--k", type=int, default=5)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--steps", type=int, default=200, help="timed steps per round, set and arm")
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "preprocess"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("probe_preprocess needs a GPU")
    dev = torch.device("cuda", 0)
    B, k = a.images, a.k
    m = AlexNetFull(seed=1234, device=dev, max_batch=B, input_norm=(MEAN, STD))
    idx = torch.empty((B, k), dtype=torch.int32, device=dev)
    prob = torch.empty((B, k), device=dev)
    ready = torch.empty((B, 227, 227, 3), dtype=torch.uint8, device=dev)

    arms, agree = [], {}
    for name, H, W in SETS:
        x = torch.randint(0, 256, (B, H, W, 3), dtype=torch.uint8, generator=torch.Generator().manual_seed(H)).to(dev)
        imgs = list(x.unbind(0))
        _, _, bh, bw = center_box(H, W)
        nbytes = B * (bh * bw * 3 + 227 * 227 * 3)  # source-box bytes + output bytes of the kernel alone
        # same geometry on both routes (the whole image onto 227 x 227): two roundings of one filter
        ours = resize_crop_u8(imgs[:16], resize=None)
        f = F.interpolate(x[:16].permute(0, 3, 1, 2).float(), size=(227, 227), mode="bilinear", antialias=True,
                          align_corners=False)
        diff = (ours.int() - f.round().clamp(0, 255).permute(0, 2, 3, 1).int()).abs()
        torch.cuda.synchronize()
        agree[name] = {"max_abs_diff_vs_torch": int(diff.max()), "share_differing": round(float((diff > 0).float().mean()), 5)}
        if int(diff.max()) > 1:
            raise SystemExit(f"{name}: the kernel's bytes differ from torch's antialiased resize by more than one level")

        def images_arm(imgs=imgs):
            m.classify_images(imgs, k)

        def torch_arm(x=x):
            m.classify(torch_preprocess(x), k, out=(idx, prob))

        def kernel_arm(imgs=imgs):
            resize_crop_u8(imgs, out=ready)

        arms += [(name, "images", images_arm, 0), (name, "torch", torch_arm, 0), (name, "kernel", kernel_arm, nbytes)]

    def classify_arm():
        m.classify(ready, k, out=(idx, prob))
    arms.append(("227x227", "classify", classify_arm, 0))

    def run(step):
        for _ in range(a.warmup):
            step()
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(a.steps):
            step()
        e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1) / a.steps

    # a second of untimed work so the timed windows run at the loaded clock
    t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    t0.record()
    while True:
        for _ in range(100):
            classify_arm()
        t1.record()
        t1.synchronize()
        if t0.elapsed_time(t1) > 1000:
            break

    os.makedirs(a.out, exist_ok=True)
    per_arm = {(s, n): [] for s, n, *_ in arms}
    with open(os.path.join(a.out, "probe.jsonl"), "w") as f:
        def emit(rec):
            line = json.dumps(rec)
            print(line, flush=True)
            f.write(line + "\n")
            f.flush()
        emit({"agreement_with_torch": agree, "images": B, "k": k, "input": m.last_input(), "head": m.last_head()})
        for r in range(a.rounds):
            for s, n, step, _ in arms:
                ms = run(step)
                per_arm[s, n].append(ms)
                emit({"round": r, "set": s, "arm": n, "images": B, "steps": a.steps, "ms_per_step": round(ms, 4)})
        for s, n, _, nbytes in arms:
            v = per_arm[s, n]
            med = statistics.median(v)
            rec = {"summary": n, "set": s, "images": B, "rounds": a.rounds, "ms_median": round(med, 4),
                   "ms_min": round(min(v), 4), "ms_max": round(max(v), 4), "images_per_s_median": round(B / med * 1e3, 1),
                   "device": torch.cuda.get_device_name(0), "gpu_max_hw_queues": os.environ["GPU_MAX_HW_QUEUES"]}
            if nbytes:
                rec["bytes_per_step"] = nbytes
                rec["gb_per_s_median"] = round(nbytes / med / 1e6, 1)
            emit(rec)


if __name__ == "__main__":
    main()
