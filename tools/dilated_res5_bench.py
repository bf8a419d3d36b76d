"""What the dilated stride-1 res5 (NETWORK.RES5_DILATION = 2) costs (profiles/dilated_res5_mi355x.txt).

    python tools/dilated_res5_bench.py [--out FILE] [--batch 64] [--no-step]

Kernel level, on the tensors of X3D-M's dilated res5 `b` convs (batch x 432 x 16 x 14 x 14, bf16): x3d_dw3d_fwd_dil / x3d_dw3d_bwd_dil
with dilation = 2 against x3d_dw3d_fwd / x3d_dw3d_bwd on the same tensors -- the dense kernels are the sibling that moves
the same bytes -- with the achieved bytes per second of each (forward: x read, y written; backward: dv, braw, araw read, ga
written).
Step level: Trainer.step of X3D-M with the key at 2 against the key at 1, classification and detection (scale factor 16 / 32),
same clips and boxes.
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
from x3d_tf_amd import hip, ops  # noqa: E402
from x3d_tf_amd.model import X3D  # noqa: E402
from x3d_tf_amd.train import Trainer  # noqa: E402

dev = torch.device("cuda:0")
say(f"device: {torch.cuda.get_device_name(0)}")
N, C, T, H, W = args.batch, 432, 16, 14, 14
g = torch.Generator(device=dev).manual_seed(1000)
shape = (N, C, T, H, W)
araw, dv, braw = (torch.randn(shape, generator=g, device=dev).to(torch.bfloat16) for _ in range(3))
y, ga = torch.empty_like(araw), torch.empty_like(araw)
wt = (torch.randn((C, 3, 3, 3), generator=g, device=dev) * 0.3).contiguous()
ss = torch.stack([0.5 + torch.rand(C, generator=g, device=dev), 0.25 * torch.randn(C, generator=g, device=dev)], 1).contiguous()
coef = (torch.randn((N, C, 4), generator=g, device=dev) * 0.5).contiguous()
stats, pool = ops.stats_buffer(C, dev), torch.zeros(N, C, dtype=torch.float64, device=dev)      # (the library's replicated layout)
a_sums, dw = torch.zeros(C, 2, dtype=torch.float64, device=dev), torch.zeros(C, 27, device=dev)
code = hip.dtype_code(torch.bfloat16)


def fwd(d):
    return lambda: ops.dw3d_fwd(araw, wt, 1, y=y, in_ss=ss, in_act=1, stats=stats, pool=pool, dilation=d)


def bwd(d):
    return lambda: ops.dw3d_bwd(dv, braw, coef, araw, ss, wt.view(C, 27), ga, a_sums, dw, 1, dilation=d)


def names(d):
    f = hip.Dw3dFwdArgs(araw.data_ptr(), wt.data_ptr(), y.data_ptr(), ss.data_ptr(), 1, stats.data_ptr(), pool.data_ptr(), N, C, T, H, W,
                        1, code, None)
    b = hip.Dw3dBwdArgs(dv.data_ptr(), braw.data_ptr(), coef.data_ptr(), araw.data_ptr(), ss.data_ptr(), wt.data_ptr(), ga.data_ptr(),
                        a_sums.data_ptr(), dw.data_ptr(), N, C, T, H, W, 1, code)
    return hip.dw3d_kernel_name(hip.dilated(f, d)), hip.dw3d_kernel_name(hip.dilated(b, d))


tensor_mb = araw.numel() * 2 / 1e6
ARMS = [("fwd dense", fwd(0), 2), ("fwd dilation 2", fwd(2), 2), ("bwd dense", bwd(0), 4), ("bwd dilation 2", bwd(2), 4)]
say(f"kernel level: {N} x {C} x {T} x {H} x {W} bf16 ({tensor_mb:.1f} MB per tensor; forward moves 2 of them, backward 4); 50 launches "
    "between device events after 5 warm-up launches; three alternating rounds")
say(f"kernels: dense {names(0)[0]} / {names(0)[1]}; dilated {names(2)[0]} / {names(2)[1]}")
for rnd in range(3):
    us = {}
    for name, fn, tensors in ARMS:
        for _ in range(5):
            fn()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(50):
            fn()
        e1.record()
        torch.cuda.synchronize()
        us[name] = e0.elapsed_time(e1) * 1000.0 / 50
        say(f"round {rnd + 1}  {name:<16s} {us[name]:8.2f} us / launch   {tensors * tensor_mb / us[name]:6.2f} TB/s")
    say(f"round {rnd + 1}  fwd dilated / dense = {us['fwd dilation 2'] / us['fwd dense']:.2f}   "
        f"bwd dilated / dense = {us['bwd dilation 2'] / us['bwd dense']:.2f}")

if not args.no_step:
    S, K = 224, 8
    clips = torch.randn((N, T, S, S, 3), generator=g, device=dev, dtype=torch.float32).to(torch.bfloat16)
    cg = torch.Generator().manual_seed(1001)
    ctr, half = 32 + 160 * torch.rand(N, K, 2, generator=cg), 20 + 60 * torch.rand(N, K, 2, generator=cg)
    boxes = torch.cat([ctr - half, ctr + half], 2).clamp(0, 224).contiguous().to(dev)
    num_boxes = torch.randint(1, K + 1, (N,), generator=cg, dtype=torch.int32)
    one_view = ["TEST.NUM_SPATIAL_CROPS", 1, "TEST.NUM_TEMPORAL_VIEWS", 1]
    lab_c = torch.randint(0, 400, (N,), generator=cg).to(dev)
    lab_d = torch.randint(0, 400, (N, K), generator=cg).to(dev)
    steps = {}
    for name, over, labels, kw in (
            ("classification, key 1", one_view, lab_c, {}),
            ("classification, key 2", one_view + ["NETWORK.RES5_DILATION", 2], lab_c, {}),
            ("detection, key 1", one_view + ["DETECTION.ENABLE", True, "DETECTION.MAX_BOXES", K], lab_d, dict(boxes=boxes, num_boxes=num_boxes)),
            ("detection, key 2", one_view + ["DETECTION.ENABLE", True, "DETECTION.MAX_BOXES", K, "NETWORK.RES5_DILATION", 2,
                                             "DETECTION.SPATIAL_SCALE_FACTOR", 16], lab_d, dict(boxes=boxes, num_boxes=num_boxes))):
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
        for kind in ("classification", "detection"):
            d = ms[f"{kind}, key 2"] - ms[f"{kind}, key 1"]
            say(f"round {rnd + 1}  {kind}: key 2 - key 1 = {d:7.3f} ms ({100.0 * d / ms[f'{kind}, key 1']:5.1f} %)")
