#!/usr/bin/env python3
"""Probe: ten views per image through the fused path against the same protocol assembled from torch kernels.

`--images` (256) device-resident byte images of 375x500 through AlexNetFull on one lane, ten views each (four corner
crops, the centre crop, their mirror images: anx.ops.ten_crop_boxes), each step ending with the top-k answer of the
mean of the ten softmax outputs on the device. Two arms, interleaved in one process on one GPU:

  a  fused   classify_images(views="ten"): one resize_crop_u8 launch of 10 N outputs into the model's byte workspace,
             the forward, and the view-averaging head (on FC8's split-K slabs where there are any): neither the
             [10 N, classes] logits nor the probabilities reach device memory
  b  torch   the same resize_crop_u8 call into a preallocated [10 N,227,227,3] tensor, forward, torch.softmax,
             view(N, 10, classes).mean(1), torch.topk: what a caller had to do before

Before any timing the two arms' class indices are compared wherever arm b's k-th and (k+1)-th mean probabilities
differ, and their probabilities to 1e-6. Then `--rounds` rounds, each timing every arm once in turn (so drift and
neighbours hit both arms alike): untimed warm-up steps, a device synchronise, then `--steps` steps between two device
events. One JSON line per (round, arm) and a summary line per arm (median, min, max over the rounds) go to
--out/probe.jsonl. Needs a GPU: there is no CPU fallback.

usage: tools/probe_multiview.py [--images 256] [--rounds 7] [--out profiles/multiview]
       tools/probe_multiview.py --images 8 --rounds 1     (a quick run)
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

import anx  # noqa: E402,F401
from anx.models.alexnet_full import AlexNetFull  # noqa: E402
from anx.ops import resize_crop_u8, ten_crop_boxes  # noqa: E402

MEAN, STD = (123.7, 116.3, 103.5), (58.4, 57.1, 57.4)
H, W, VIEWS = 375, 500, 10


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--images", type=int, default=256)
    ap.add_argument("--k", type=int, default=5)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--steps", type=int, default=30, help="timed steps per round and arm")
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "multiview"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("probe_multiview needs a GPU")
    dev = torch.device("cuda", 0)
    B, k = a.images, a.k
    rows = B * VIEWS

    m = AlexNetFull(seed=1234, device=dev, max_batch=rows, input_norm=(MEAN, STD))
    x = torch.randint(0, 256, (B, H, W, 3), dtype=torch.uint8, generator=torch.Generator().manual_seed(H)).to(dev)
    imgs = list(x.unbind(0))
    b, f = ten_crop_boxes(H, W)
    boxes, flips, source = b * B, f * B, [i for i in range(B) for _ in range(VIEWS)]
    crops = torch.empty((rows, 227, 227, 3), dtype=torch.uint8, device=dev)
    y = torch.empty((rows, m.classes), device=dev)
    out = {}

    def fused():
        out["fused"] = m.classify_images(imgs, k, views="ten")

    def torch_route():
        resize_crop_u8(imgs, 227, boxes=boxes, flips=flips, source=source, out=crops)
        m.forward(crops, y)
        p = torch.softmax(y, dim=1).view(B, VIEWS, m.classes).mean(1)
        out["torch"] = torch.topk(p, k, dim=1)

    arms = [("fused", fused), ("torch", torch_route)]

    # same results first
    fused()
    route = {"head": m.last_head(), "fc8": m.last_path()["fc8"], "conv1": m.last_path()["conv1"], "input": m.last_input()}
    torch_route()
    torch.cuda.synchronize()
    f_idx, f_prob = out["fused"]
    t_prob, t_idx = out["torch"]
    pbar = torch.softmax(y, dim=1).view(B, VIEWS, m.classes).mean(1)
    srt = torch.sort(pbar, dim=1, descending=True).values
    clear = (srt[:, :k] != srt[:, 1:k + 1]).all(dim=1)  # rows whose top k are not tied: one right answer
    if not torch.equal(f_idx[clear].long(), t_idx[clear]):
        raise SystemExit("class indices differ from the torch route's on rows without ties")
    worst = float((f_prob[clear] - t_prob[clear]).abs().max()) if bool(clear.any()) else 0.0
    if worst > 1e-6:
        raise SystemExit(f"mean probabilities differ from the torch route's by {worst:.3e}")

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
        for _ in range(3):
            m.forward(crops, y)
        t1.record()
        t1.synchronize()
        if t0.elapsed_time(t1) > 1000:
            break

    os.makedirs(a.out, exist_ok=True)
    per_arm = {name: [] for name, _ in arms}
    with open(os.path.join(a.out, "probe.jsonl"), "w") as fo:
        def emit(rec):
            line = json.dumps(rec)
            print(line, flush=True)
            fo.write(line + "\n")
            fo.flush()
        emit({"route": route, "rows_without_ties": int(clear.sum()), "max_prob_diff_vs_torch": worst, "images": B,
              "views": VIEWS, "k": k, "image_size": [H, W]})
        for r in range(a.rounds):
            for name, step in arms:
                ms = run(step)
                per_arm[name].append(ms)
                emit({"round": r, "arm": name, "images": B, "views": VIEWS, "steps": a.steps, "ms_per_step": round(ms, 4),
                      "images_per_s": round(B / ms * 1e3, 1)})
        for name, _ in arms:
            v = per_arm[name]
            med = statistics.median(v)
            emit({"summary": name, "images": B, "views": VIEWS, "k": k, "rounds": a.rounds, "ms_median": round(med, 4),
                  "ms_min": round(min(v), 4), "ms_max": round(max(v), 4), "images_per_s_median": round(B / med * 1e3, 1),
                  "device": torch.cuda.get_device_name(0), "gpu_max_hw_queues": os.environ["GPU_MAX_HW_QUEUES"]})


if __name__ == "__main__":
    main()
