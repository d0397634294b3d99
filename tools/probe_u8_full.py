#!/usr/bin/env python3
"""Probe: what byte (uint8) image input costs or saves on the bf16 full AlexNet.

`--images` (256) images of 227x227x3 through AlexNetFull on one lane (as `bench.py --model full`), five arms
interleaved in one process on one GPU:

  a  f32_device   device-resident float32 input
  b  u8_ring      device-resident uint8 input, bf16_u8=1 (the row-band Conv1 loads the bytes)
  c  u8_decode    device-resident uint8 input, bf16_u8=0 (decode kernel into a workspace, then the float kernel)
  d  f32_host     arm a fed from pinned host memory every step (upload on the forward's stream, then compute)
  e  u8_host      bytes fed from pinned host memory every step, into the model's default byte route

Before any timing every arm's logits are compared bit for bit with arm a's. Then `--rounds` rounds, each timing
every arm once in turn (so drift and neighbours hit all arms alike): untimed warm-up steps, a device synchronise,
then `steps` forwards between two device events. One JSON line per (round, arm) and a summary line per arm
(median, min, max over the rounds) go to --out/probe.jsonl. Needs a GPU: there is no CPU fallback, a time from
anything else would mean nothing.

usage: tools/probe_u8_full.py [--images 256] [--rounds 5] [--out profiles/bf16_u8_input]
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
from anx.utils.tuning import default_knob  # noqa: E402

MEAN, STD = (123.7, 116.3, 103.5), (58.4, 57.1, 57.4)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--images", type=int, default=256)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--steps-device", type=int, default=1000, help="timed steps per round, device-resident arms")
    ap.add_argument("--steps-host", type=int, default=200, help="timed steps per round, host-fed arms")
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--arms", default="", help="comma-separated arm names to run (default: all)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "bf16_u8_input"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("probe_u8_full needs a GPU")
    dev = torch.device("cuda", 0)
    B = a.images

    m_f = AlexNetFull(seed=1234, device=dev, max_batch=B, input_norm=(MEAN, STD))
    m_r = AlexNetFull(m_f.weights, device=dev, max_batch=B, input_norm=(MEAN, STD), knobs={"bf16_u8": 1})
    m_d = AlexNetFull(m_f.weights, device=dev, max_batch=B, input_norm=(MEAN, STD), knobs={"bf16_u8": 0})
    g = torch.Generator().manual_seed(1)
    xb_host = torch.randint(0, 256, (B, 227, 227, 3), dtype=torch.uint8, generator=g).pin_memory()
    xb = xb_host.to(dev)
    xf = m_f.decode_u8(xb)
    xf_host = xf.cpu().pin_memory()
    xf_stage, xb_stage = torch.empty_like(xf), torch.empty_like(xb)  # what the host-fed arms upload into
    y = torch.empty((B, m_f.classes), device=dev)

    def fed(host, stage):
        return lambda: stage.copy_(host, non_blocking=True)  # on the current stream, ahead of the forward

    arms = [("f32_device", m_f, xf, None, a.steps_device, 0),
            ("u8_ring", m_r, xb, None, a.steps_device, 0),
            ("u8_decode", m_d, xb, None, a.steps_device, 0),
            ("f32_host", m_f, xf_stage, fed(xf_host, xf_stage), a.steps_host, xf.numel() * 4),
            ("u8_host", m_f, xb_stage, fed(xb_host, xb_stage), a.steps_host, xb.numel())]
    want = {"u8_ring": "u8_ring", "u8_decode": "u8_decode",
            "u8_host": "u8_ring" if default_knob("bf16_u8") else "u8_decode"}

    def step(m, x, pre):
        if pre is not None:
            pre()
        m.forward(x, y)

    # same results first
    ref, routes = None, {}
    for name, m, x, pre, _, _ in arms:
        y.fill_(float("nan"))
        step(m, x, pre)
        torch.cuda.synchronize()
        if ref is None:
            ref = y.clone()
        elif not torch.equal(y, ref):
            raise SystemExit(f"arm {name}: logits differ from f32_device")
        if name in want:
            assert m.last_input() == want[name], (name, m.last_input())
        routes[name] = {"input": m.last_input(), "conv1": m.last_path()["conv1"]}
    if a.arms:
        arms = [arm for arm in arms if arm[0] in a.arms.split(",")]

    def run(m, x, pre, steps):
        for _ in range(a.warmup):
            step(m, x, pre)
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(steps):
            step(m, x, pre)
        e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1) / steps

    # a second of untimed work so the timed windows run at the loaded clock
    t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    t0.record()
    while True:
        run(m_f, xf, None, 100)
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
        emit({"routes": routes})
        for r in range(a.rounds):
            for name, m, x, pre, steps, h2d in arms:
                ms = run(m, x, pre, steps)
                per_arm[name].append(ms)
                emit({"round": r, "arm": name, "images": B, "steps": steps, "ms_per_step": round(ms, 4),
                      "images_per_s": round(B / ms * 1e3, 1), "h2d_bytes_per_step": h2d})
        for name, *_, h2d in arms:
            v = per_arm[name]
            med = statistics.median(v)
            emit({"summary": name, "images": B, "rounds": a.rounds, "ms_median": round(med, 4), "ms_min": round(min(v), 4),
                  "ms_max": round(max(v), 4), "images_per_s_median": round(B / med * 1e3, 1), "h2d_bytes_per_step": h2d,
                  "h2d_gb_per_s_if_copy_bound": round(h2d / med / 1e6, 2) if h2d else None,
                  "device": torch.cuda.get_device_name(0), "gpu_max_hw_queues": os.environ["GPU_MAX_HW_QUEUES"]})


if __name__ == "__main__":
    main()
