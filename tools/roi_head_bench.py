"""What the ROI head costs next to the classification head it replaces (profiles/roi_head_mi355x.txt).

    python tools/roi_head_bench.py [--out FILE] [--batch 64] [--no-step]

Kernel level, on X3D-M's head tensors (batch x 432 x 16 x 7 x 7, bf16, K = 8 box slots, 7 x 7 bins, sampling ratio 0): x3d_roi_pool_fwd
against x3d_pool_fwd and x3d_roi_pool_bwd against x3d_relu_bn_bwd_reduce in its dpool form, the same conv5 tensor under both.  The
two siblings are the parent's kernels reading the same bytes.  Boxes: per clip 1..K random person-sized boxes of a 224^2 clip.
Step level: Trainer.step of X3D-M with DETECTION.ENABLE against the classification step, same clips.
Three alternating rounds in ONE process; device events around 50 launches (kernel level), host clock around a device synchronise
and 10 steps (step level).  A record, not a gate."""
import argparse
import os
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
ap = argparse.ArgumentParser()
ap.add_argument("--out", help="also write the lines to this file")
ap.add_argument("--batch", type=int, default=64)
ap.add_argument("--no-step", action="store_true", help="kernel level only")
args = ap.parse_args()
lines = []


def say(s):
    print(s, flush=True)
    lines.append(s)
    if args.out:
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


import x3d_tf_amd as x  # noqa: E402
from x3d_tf_amd import ops  # noqa: E402
from x3d_tf_amd.model import X3D  # noqa: E402
from x3d_tf_amd.train import Trainer  # noqa: E402

dev = torch.device("cuda:0")
say(f"device: {torch.cuda.get_device_name(0)}")
N, C, T, H, W, K, R = args.batch, 432, 16, 7, 7, 8, 7
g = torch.Generator(device=dev).manual_seed(1000)
c5 = torch.randn((N, C, T, H, W), generator=g, device=dev).to(torch.bfloat16)
ss = torch.stack([0.5 + torch.rand(C, generator=g, device=dev), 0.25 + torch.rand(C, generator=g, device=dev)], 1).contiguous()
cg = torch.Generator().manual_seed(1001)
ctr, half = 32 + 160 * torch.rand(N, K, 2, generator=cg), 20 + 60 * torch.rand(N, K, 2, generator=cg)
boxes = torch.cat([ctr - half, ctr + half], 2).clamp(0, 224).contiguous()
num_boxes = torch.randint(1, K + 1, (N,), generator=cg, dtype=torch.int32)
d_boxes, d_nb = boxes.to(dev), num_boxes.to(dev)
pooled_r, argmax = torch.empty(N * K, C, device=dev), torch.empty(N * K, C, dtype=torch.uint8, device=dev)
pooled_c = torch.empty(N, C, device=dev)
dp_r, dp_c = torch.randn(N * K, C, generator=g, device=dev), torch.randn(N, C, generator=g, device=dev)
g5, sums = torch.empty_like(c5), torch.zeros(C, 2, dtype=torch.float64, device=dev)

ARMS = [("x3d_pool_fwd", lambda: ops.pool_fwd(c5, ss, pooled_c)),
        ("x3d_roi_pool_fwd", lambda: ops.roi_pool_fwd(c5, ss, d_boxes, d_nb, pooled_r, argmax, R, 0, 1.0 / 32)),
        ("x3d_relu_bn_bwd_reduce (dpool)", lambda: ops.relu_bn_bwd_reduce(None, dp_c, c5, ss, g5, sums)),
        ("x3d_roi_pool_bwd", lambda: ops.roi_pool_bwd(dp_r, argmax, d_boxes, d_nb, c5, ss, g5, sums, R, 0, 1.0 / 32))]
say(f"kernel level: conv5 tensor {N} x {C} x {T} x {H} x {W} bf16 ({c5.numel() * 2 / 1e6:.1f} MB), K = {K} slots, {int(num_boxes.sum())} "
    f"boxes, R = {R}, sampling ratio 0; 50 launches between device events after 5 warm-up launches; three alternating rounds")
for rnd in range(3):
    us = {}
    for name, fn in ARMS:
        for _ in range(5):
            fn()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(50):
            fn()
        e1.record()
        torch.cuda.synchronize()
        us[name] = e0.elapsed_time(e1) * 1000.0 / 50
        say(f"round {rnd + 1}  {name:<32s} {us[name]:8.2f} us / launch")
    say(f"round {rnd + 1}  roi fwd / pool fwd = {us['x3d_roi_pool_fwd'] / us['x3d_pool_fwd']:.2f}   "
        f"roi bwd / reduce = {us['x3d_roi_pool_bwd'] / us['x3d_relu_bn_bwd_reduce (dpool)']:.2f}")

if not args.no_step:
    S = 224
    clips = torch.randn((N, T, S, S, 3), generator=g, device=dev, dtype=torch.float32).to(torch.bfloat16)
    one_view = ["TEST.NUM_SPATIAL_CROPS", 1, "TEST.NUM_TEMPORAL_VIEWS", 1]
    steps = {}
    for name, over, labels, kw in (
            ("classification step", one_view, torch.randint(0, 400, (N,), generator=cg).to(dev), {}),
            ("detection step", one_view + ["DETECTION.ENABLE", True, "DETECTION.MAX_BOXES", K],
             torch.randint(0, 400, (N, K), generator=cg).to(dev), dict(boxes=d_boxes, num_boxes=num_boxes))):
        cfg = x.get_config("M", over)
        model = X3D(cfg, dtype=torch.bfloat16, device=dev, seed=0)
        tr = Trainer(model, cfg)
        steps[name] = (lambda tr=tr, labels=labels, kw=kw, lr=cfg.TRAIN.WARMUP_LR: tr.step(clips, labels, lr, **kw))
        for _ in range(3):
            steps[name]()
    say(f"step level: X3D-M, {N} x {T} x {S}^2, bf16, SGD: Trainer.step, 10 timed steps after 3 warm-up steps, host clock around a "
        "device synchronise; three alternating rounds")
    for rnd in range(3):
        ms = {}
        for name, step in steps.items():
            step()
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(10):
                step()
            torch.cuda.synchronize()
            ms[name] = (time.perf_counter() - t0) * 100.0
            say(f"round {rnd + 1}  {name:<22s} {ms[name]:7.3f} ms / step")
        d = ms["detection step"] - ms["classification step"]
        say(f"round {rnd + 1}  detection - classification = {d:7.3f} ms ({100.0 * d / ms['classification step']:5.1f} %)")
