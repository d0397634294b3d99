#!/usr/bin/env python3
"""Probe: what holding the bf16 full AlexNet to labels costs, on the chip and through torch.

`--images` (256) device-resident byte images of 227x227x3 and their labels through AlexNetFull on one lane, `--k` 5.
Three arms, interleaved in one process on one GPU; a timed window is `--steps` steps between two device events and
ends with the one synchronise an evaluation needs (the event's), no step waits for the device:

  a  evaluate   evaluate(x, labels, k) into device counters (stats int64 [4]): the evaluation head kernel on FC8's
                split-K slabs, per-image rank / loss / prediction and four integer atomics per image
  b  classify   classify(x, k): the classifier head on the same slabs. The floor: the same forward, a head that also
                ranks the k best classes but knows no labels. Nothing is accumulated.
  c  torch      forward into logits, then torch.log_softmax + nll_loss (sum) + topk + compare with the labels, added
                into device tensors: what a caller had to do before evaluate existed

Before any timing arm a's counters are compared with arm c's: images, top-1 hits and top-k hits exactly on batches
without ties at the k-th place, the loss sum to 1e-4 relative. Then `--rounds` rounds, each timing every arm once in
turn (so drift and neighbours hit all arms alike): untimed warm-up steps, a device synchronise, then the window. One
JSON line per (round, arm) and a summary line per arm (median, min, max over the rounds) go to --out/probe.jsonl.
Needs a GPU: there is no CPU fallback. Not covered: cold start with the new code object, and lanes > 1.

usage: tools/probe_evaluate.py [--images 256] [--rounds 7] [--out profiles/evaluate]
       tools/probe_evaluate.py --images 8 --rounds 1     (a quick run)
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
from anx.ops import eval_summary  # noqa: E402

MEAN, STD = (123.7, 116.3, 103.5), (58.4, 57.1, 57.4)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--images", type=int, default=256)
    ap.add_argument("--k", type=int, default=5)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--steps", type=int, default=500, help="timed steps per round and arm")
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "evaluate"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("probe_evaluate needs a GPU")
    dev = torch.device("cuda", 0)
    B, k = a.images, a.k

    m = AlexNetFull(seed=1234, device=dev, max_batch=B, input_norm=(MEAN, STD))
    x = torch.randint(0, 256, (B, 227, 227, 3), dtype=torch.uint8, generator=torch.Generator().manual_seed(1)).to(dev)
    y = torch.empty((B, m.classes), device=dev)
    # labels: the model's own answer for every other image, a fixed class for the rest (hits and misses both occur)
    m.forward(x, y)
    labels = torch.where(torch.arange(B, device=dev) % 2 == 0, y.argmax(dim=1), torch.full((B,), 7, device=dev)).to(torch.int32)
    labels64 = labels.long()
    out = (torch.empty(B, dtype=torch.int32, device=dev), torch.empty(B, device=dev),
           torch.empty(B, dtype=torch.int32, device=dev))
    stats = torch.zeros(4, dtype=torch.int64, device=dev)
    idx = torch.empty((B, k), dtype=torch.int32, device=dev)
    prob = torch.empty((B, k), device=dev)
    t_count = torch.zeros((), dtype=torch.int64, device=dev)
    t_top1 = torch.zeros((), dtype=torch.int64, device=dev)
    t_topk = torch.zeros((), dtype=torch.int64, device=dev)
    t_loss = torch.zeros((), dtype=torch.float64, device=dev)

    def evaluate():
        m.evaluate(x, labels, k, stats=stats, out=out)

    def classify():
        m.classify(x, k, out=(idx, prob))

    def torch_route():
        m.forward(x, y)
        t_loss.add_(F.nll_loss(torch.log_softmax(y, dim=1), labels64, reduction="sum"))
        hit = torch.topk(y, k, dim=1).indices == labels64[:, None]
        t_top1.add_(hit[:, 0].sum())
        t_topk.add_(hit.any(dim=1).sum())
        t_count.add_(B)

    arms = [("evaluate", evaluate), ("classify", classify), ("torch", torch_route)]

    # same results first
    evaluate()
    route = {"head": m.last_head(), "fc8": m.last_path()["fc8"], "conv1": m.last_path()["conv1"], "input": m.last_input()}
    torch_route()
    torch.cuda.synchronize()
    srt = torch.sort(y, dim=1, descending=True).values
    ties = int((srt[:, k - 1] == srt[:, k]).sum()) + int((srt[:, 0] == srt[:, 1]).sum())
    got = [int(v) for v in stats.tolist()]
    want = [int(t_count), int(t_top1), int(t_topk)]
    if ties == 0 and got[:3] != want:
        raise SystemExit(f"counters {got[:3]} differ from the torch route's {want}")
    loss_a, loss_t = got[3] / 2.0 ** 32, float(t_loss)
    if abs(loss_a - loss_t) > 1e-4 * abs(loss_t):
        raise SystemExit(f"loss sum {loss_a} differs from the torch route's {loss_t}")
    first = eval_summary(stats, k)

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
            m.forward(x, y)
        t1.record()
        t1.synchronize()
        if t0.elapsed_time(t1) > 1000:
            break

    os.makedirs(a.out, exist_ok=True)
    per_arm = {name: [] for name, _ in arms}
    with open(os.path.join(a.out, "probe.jsonl"), "w") as f:
        def emit(rec):
            line = json.dumps(rec)
            print(line, flush=True)
            f.write(line + "\n")
            f.flush()
        emit({"route": route, "first_batch": first, "torch_first_batch": {"counts": want, "loss_sum": loss_t},
              "rows_tied_at_1_or_k": ties, "images": B, "k": k})
        for r in range(a.rounds):
            for name, step in arms:
                ms = run(step)
                per_arm[name].append(ms)
                emit({"round": r, "arm": name, "images": B, "steps": a.steps, "ms_per_step": round(ms, 4),
                      "images_per_s": round(B / ms * 1e3, 1)})
        for name, _ in arms:
            v = per_arm[name]
            med = statistics.median(v)
            emit({"summary": name, "images": B, "k": k, "rounds": a.rounds, "ms_median": round(med, 4),
                  "ms_min": round(min(v), 4), "ms_max": round(max(v), 4), "images_per_s_median": round(B / med * 1e3, 1),
                  "device": torch.cuda.get_device_name(0), "gpu_max_hw_queues": os.environ["GPU_MAX_HW_QUEUES"]})
        total = eval_summary(stats, k)  # every timed and warm-up step of arm a added the same batch: the same errors
        emit({"after_all_steps": total, "same_errors_as_first_batch": all(total[n] == first[n] for n in ("top1_error", "topk_error"))})


if __name__ == "__main__":
    main()
