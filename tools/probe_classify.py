#!/usr/bin/env python3
"""Probe: what the fused classifier head saves on the bf16 full AlexNet.

`--images` (256) byte images of 227x227x3 through AlexNetFull on one lane, each step ending with the top-k answer
(indices int32 and probabilities fp32, `--k` 5) in pinned host memory. Four arms interleaved in one process on one
GPU:

  a  torch_head   forward, torch.softmax, torch.topk, then the D2H of indices and probabilities (what a caller had
                  to do before classify existed)
  b  head_slabs   classify with bf16_head=1 (the head kernel reduces FC8's split-K slabs itself), the same D2H
  c  head_logits  classify with bf16_head=0 (the split-K reduce writes the logits, the head runs on them), same D2H
  d  logits_d2h   forward, then the D2H of the full logits: the copy a host-side top-k would need, for scale

Before any timing arms b and c are compared bit for bit with each other and with anx.ops.softmax_topk of arm a's
logits, and their class indices with torch.topk's wherever the k-th and (k+1)-th logits differ. Then `--rounds`
rounds, each timing every arm once in turn (so drift and neighbours hit all arms alike): untimed warm-up steps, a
device synchronise, then `--steps` steps between two device events. One JSON line per (round, arm) and a summary
line per arm (median, min, max over the rounds) go to --out/probe.jsonl. Needs a GPU: there is no CPU fallback.

usage: tools/probe_classify.py [--images 256] [--rounds 7] [--out profiles/classify_head]
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
from anx.ops import softmax_topk  # noqa: E402

MEAN, STD = (123.7, 116.3, 103.5), (58.4, 57.1, 57.4)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--images", type=int, default=256)
    ap.add_argument("--k", type=int, default=5)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--steps", type=int, default=500, help="timed steps per round and arm")
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "classify_head"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("probe_classify needs a GPU")
    dev = torch.device("cuda", 0)
    B, k = a.images, a.k

    m_t = AlexNetFull(seed=1234, device=dev, max_batch=B, input_norm=(MEAN, STD))
    m_s = AlexNetFull(m_t.weights, device=dev, max_batch=B, input_norm=(MEAN, STD), knobs={"bf16_head": 1})
    m_l = AlexNetFull(m_t.weights, device=dev, max_batch=B, input_norm=(MEAN, STD), knobs={"bf16_head": 0})
    x = torch.randint(0, 256, (B, 227, 227, 3), dtype=torch.uint8, generator=torch.Generator().manual_seed(1)).to(dev)
    y = torch.empty((B, m_t.classes), device=dev)
    idx = torch.empty((B, k), dtype=torch.int32, device=dev)
    prob = torch.empty((B, k), device=dev)
    h_idx = torch.empty((B, k), dtype=torch.int32).pin_memory()
    h_idx64 = torch.empty((B, k), dtype=torch.int64).pin_memory()  # torch.topk's index type
    h_prob = torch.empty((B, k)).pin_memory()
    h_y = torch.empty((B, m_t.classes)).pin_memory()

    def torch_head():
        m_t.forward(x, y)
        p, i = torch.topk(torch.softmax(y, dim=1), k, dim=1)
        h_idx64.copy_(i, non_blocking=True)
        h_prob.copy_(p, non_blocking=True)

    def head(m):
        def step():
            m.classify(x, k, out=(idx, prob))
            h_idx.copy_(idx, non_blocking=True)
            h_prob.copy_(prob, non_blocking=True)
        return step

    def logits_d2h():
        m_t.forward(x, y)
        h_y.copy_(y, non_blocking=True)

    arms = [("torch_head", torch_head, B * k * 12), ("head_slabs", head(m_s), B * k * 8),
            ("head_logits", head(m_l), B * k * 8), ("logits_d2h", logits_d2h, y.numel() * 4)]

    # same results first
    torch_head()
    torch.cuda.synchronize()
    want = softmax_topk(y, k)
    t_idx = h_idx64.clone()
    routes = {}
    for name, m in (("head_slabs", m_s), ("head_logits", m_l)):
        idx.fill_(-1)
        prob.fill_(float("nan"))
        head(m)()
        torch.cuda.synchronize()
        if not (torch.equal(idx, want[0]) and torch.equal(prob.view(torch.int32), want[1].view(torch.int32))):
            raise SystemExit(f"arm {name}: differs from softmax_topk of the forward's logits")
        routes[name] = {"head": m.last_head(), "fc8": m.last_path()["fc8"], "input": m.last_input()}
    srt = torch.sort(y, dim=1, descending=True).values
    clear = (srt[:, :k] != srt[:, 1:k + 1]).all(dim=1).cpu()  # rows whose top k are not tied: one right answer
    if not torch.equal(h_idx[clear].long(), t_idx[clear]):
        raise SystemExit("class indices differ from torch.topk's on rows without ties")
    assert routes["head_logits"]["head"] == "logits", routes

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
            m_t.forward(x, y)
        t1.record()
        t1.synchronize()
        if t0.elapsed_time(t1) > 1000:
            break

    os.makedirs(a.out, exist_ok=True)
    per_arm = {name: [] for name, *_ in arms}
    with open(os.path.join(a.out, "probe.jsonl"), "w") as f:
        def emit(rec):
            line = json.dumps(rec)
            print(line, flush=True)
            f.write(line + "\n")
            f.flush()
        emit({"routes": routes, "rows_without_ties": int(clear.sum()), "images": B, "k": k})
        for r in range(a.rounds):
            for name, step, d2h in arms:
                ms = run(step)
                per_arm[name].append(ms)
                emit({"round": r, "arm": name, "images": B, "steps": a.steps, "ms_per_step": round(ms, 4),
                      "images_per_s": round(B / ms * 1e3, 1), "d2h_bytes_per_step": d2h})
        for name, _, d2h in arms:
            v = per_arm[name]
            med = statistics.median(v)
            emit({"summary": name, "images": B, "k": k, "rounds": a.rounds, "ms_median": round(med, 4),
                  "ms_min": round(min(v), 4), "ms_max": round(max(v), 4), "images_per_s_median": round(B / med * 1e3, 1),
                  "d2h_bytes_per_step": d2h, "device": torch.cuda.get_device_name(0),
                  "gpu_max_hw_queues": os.environ["GPU_MAX_HW_QUEUES"]})


if __name__ == "__main__":
    main()
