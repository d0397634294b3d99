#!/usr/bin/env python3
"""Probe: the resize + crop kernel alone, this tree against another build of the project (its parent commit, say).

The unflipped entry point `anx_resize_crop_u8` on the two image sets of tools/probe_preprocess.py (`--images` (256)
device-resident byte images of 375x500 and of 256x256, centre boxes onto 227x227). The descriptors are built once and
the loop calls the C ABI directly, so a step is bound by the kernel and not by the host's descriptor work (which is
what probe_preprocess.py's `kernel` arm times from Python): `--warmup` launches, a device synchronise, then `--steps`
launches between two device events. Before timing the output is compared with `anx.ops.resize_crop_u8`'s, and its
checksum is recorded so that two builds can be seen to write the same bytes.

`--other ROOT` names a second checkout with its own built libraries (`git worktree add ROOT <commit>` and its
build). Each of `--rounds` rounds then runs ROOT and this tree once each, in turn, each in a fresh process that
loads only its own tree's package and library: drift and neighbours hit both alike. Without `--other` only this
tree runs. One JSON line per (round, tree, set) and a summary line per (tree, set) (median, min, max over the
rounds) go to --out/resize_ab.jsonl. Needs a GPU: there is no CPU fallback.

usage: tools/probe_resize_ab.py --other ../parent [--rounds 7] [--out profiles/multiview]
"""
import argparse
import json
import os
import statistics
import subprocess
import sys

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SETS = (("375x500", 375, 500), ("256x256", 256, 256))


def child(a):
    """One round on the tree at a.root; prints one JSON line per set."""
    root = os.path.abspath(a.root)
    sys.path.insert(0, root)
    os.environ["GPU_MAX_HW_QUEUES"] = os.environ.get("ANX_HW_QUEUES", "8")  # as bench.py; read at HIP's first call
    import numpy as np
    import torch

    import anx  # noqa: F401
    from anx import _native as nat
    from anx import ops

    if not os.path.abspath(nat.LIB_PATH).startswith(root + os.sep):
        raise SystemExit(f"{nat.LIB_PATH} is not under {root}")
    if not torch.cuda.is_available():
        raise SystemExit("probe_resize_ab needs a GPU")
    dev = torch.device("cuda", 0)
    B = a.images
    for name, H, W in SETS:
        x = torch.randint(0, 256, (B, H, W, 3), dtype=torch.uint8, generator=torch.Generator().manual_seed(H)).to(dev)
        imgs = list(x.unbind(0))
        geo, _ = ops._image_geometry(imgs)
        host = torch.from_numpy(ops._image_descs(geo, 227, 227, 256, None).view(np.uint8))
        ddev = host.to(dev)
        out = torch.empty((B, 227, 227, 3), dtype=torch.uint8, device=dev)
        want = ops.resize_crop_u8(imgs)
        s = nat.stream_ptr(dev)

        def step():
            nat.call("anx_resize_crop_u8", ddev.data_ptr(), host.data_ptr(), B, out.data_ptr(), 227, 227, s)

        step()
        torch.cuda.synchronize()
        if not torch.equal(out, want):
            raise SystemExit(f"{name}: the entry point's bytes differ from anx.ops.resize_crop_u8's")
        for _ in range(a.warmup):
            step()
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(a.steps):
            step()
        e1.record()
        e1.synchronize()
        print(json.dumps({"round": a.round, "tree": a.tag, "abi": nat.lib().anx_abi_version(), "set": name, "images": B,
                          "steps": a.steps, "us_per_launch": round(e0.elapsed_time(e1) / a.steps * 1e3, 3),
                          "checksum": int(out.to(torch.int64).sum()), "device": torch.cuda.get_device_name(0),
                          "gpu_max_hw_queues": os.environ["GPU_MAX_HW_QUEUES"]}), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--other", default=None, help="root of a second built checkout to alternate with")
    ap.add_argument("--images", type=int, default=256)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--steps", type=int, default=2000, help="timed launches per round, tree and set")
    ap.add_argument("--warmup", type=int, default=200)
    ap.add_argument("--out", default=os.path.join(HERE, "profiles", "multiview"))
    ap.add_argument("--root", default=None, help=argparse.SUPPRESS)  # child mode: one round on this tree
    ap.add_argument("--tag", default="this", help=argparse.SUPPRESS)
    ap.add_argument("--round", type=int, default=0, help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.root is not None:
        child(a)
        return
    trees = ([("other", a.other)] if a.other else []) + [("this", HERE)]
    os.makedirs(a.out, exist_ok=True)
    rows = []
    with open(os.path.join(a.out, "resize_ab.jsonl"), "w") as f:
        def emit(rec):
            line = json.dumps(rec)
            print(line, flush=True)
            f.write(line + "\n")
            f.flush()
        for r in range(a.rounds):
            for tag, root in trees:
                # a fresh process per tree and round: this one never initialises the GPU
                p = subprocess.run([sys.executable, os.path.abspath(__file__), "--root", root, "--tag", tag, "--round",
                                    str(r), "--images", str(a.images), "--steps", str(a.steps), "--warmup", str(a.warmup)],
                                   capture_output=True, text=True, timeout=300)
                if p.returncode != 0:
                    raise SystemExit(f"round {r}, tree {tag}: exit {p.returncode}\n{p.stderr[-2000:]}")
                for line in p.stdout.splitlines():
                    if line.startswith("{"):
                        rows.append(json.loads(line))
                        emit(rows[-1])
        for tag, _ in trees:
            for name, *_ in SETS:
                v = [x["us_per_launch"] for x in rows if x["tree"] == tag and x["set"] == name]
                emit({"summary": tag, "set": name, "images": a.images, "rounds": a.rounds,
                      "us_median": round(statistics.median(v), 3), "us_min": min(v), "us_max": max(v)})


if __name__ == "__main__":
    main()
