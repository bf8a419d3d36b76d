"""What knowledge distillation costs a training step (profiles/distill_mi355x.txt).

    python tools/distill_bench.py [--out FILE] [--head-only]

Three measurements in ONE process on the MI355X, every pair of arms alternating:
  1. the KD head launch x3d_softmax_xent_kd (dense targets, alpha 0.5, T 2) at 64 x 400 next to x3d_softmax_xent_soft on the
     same logits and targets (HIP events, 200 launches after 20 warm-ups);
  2. `teacher.logits` of an X3D-M teacher at 64 x 16 x 224^2 in bf16 (HIP events, 10 calls after 3 warm-ups);
  3. the X3D-M student's Trainer.step with DISTILL off and on (that teacher, alpha 0.5, T 2), 10 timed steps after 3 warm-up
     steps, host clock around a device synchronise.
The expectation to hold the result against: the distilled step costs about one teacher forward (2.) more than the
feature-off step of the same round."""
import argparse
import os
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
ap = argparse.ArgumentParser()
ap.add_argument("--out", help="also write the lines to this file")
ap.add_argument("--head-only", action="store_true", help="measurement 1 alone (the run to put under rocprofv3 --kernel-trace "
                "--stats for the kernels' own times)")
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


def events(fn, warm, reps):
    """mean milliseconds per call of fn over `reps` calls after `warm` warm-ups (HIP events)"""
    for _ in range(warm):
        fn()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / reps


# ---- 1. the head launch -----------------------------------------------------------------------------------------------
N, M = 64, 400
g = torch.Generator(device=dev).manual_seed(1000)
z = torch.randn((N, M), generator=g, device=dev) * 2
t = torch.randn((N, M), generator=g, device=dev) * 3
y = torch.softmax(torch.randn((N, M), generator=g, device=dev), -1)
probs, rows, kd, dl = (torch.empty(N, M, device=dev), torch.empty(N, device=dev), torch.empty(N, device=dev),
                       torch.empty(N, M, device=dev))
heads = [("x3d_softmax_xent_soft", lambda: ops.softmax_xent_soft(z, y, probs, rows, dl, 1.0 / N)),
         ("x3d_softmax_xent_kd (targets, a 0.5, T 2)",
          lambda: ops.softmax_xent_kd(z, t, probs, targets=y, loss_rows=rows, kd_rows=kd, dlogits=dl, grad_scale=1.0 / N,
                                      alpha=0.5, temperature=2.0)),
         ("x3d_softmax_xent_kd (targets, a 0)",
          lambda: ops.softmax_xent_kd(z, None, probs, targets=y, loss_rows=rows, kd_rows=kd, dlogits=dl, grad_scale=1.0 / N,
                                      alpha=0.0, temperature=2.0))]
say(f"head launch at {N} x {M}, back-to-back launches through the ops wrappers (HIP events, 200 launches after 20 warm-ups): "
    "launch rate, not kernel time")
for rnd in range(3):
    for name, fn in heads:
        say(f"round {rnd + 1}  {name:<44s} {events(fn, 20, 200) * 1e3:8.2f} us / launch")

if args.head_only:
    sys.exit(0)

# ---- 2. and 3.: the teacher's forward and the student's step ----------------------------------------------------------
B, T, S = 64, 16, 224
clips = torch.randn((B, T, S, S, 3), generator=g, device=dev, dtype=torch.float32).to(torch.bfloat16)
labels = torch.randint(0, 400, (B,), generator=g, device=dev)
teacher = X3D(x.get_config("M"), dtype=torch.bfloat16, device=dev, seed=7)


def arm(over, **kw):
    cfg = x.get_config("M", over)
    torch.manual_seed(2000)
    model = X3D(cfg, dtype=torch.bfloat16, device=dev, seed=0)
    tr = Trainer(model, cfg, **kw)
    state0 = (model.flat_params.clone(), model.flat_velocity.clone())

    def step():
        model.flat_params.copy_(state0[0])
        model.flat_velocity.copy_(state0[1])
        return tr.step(clips, labels, cfg.TRAIN.WARMUP_LR)
    return step


arms = [("DISTILL off", arm(None)),
        ("DISTILL on (M teacher, a 0.5, T 2)", arm(["DISTILL.ENABLE", True, "DISTILL.ALPHA", 0.5, "DISTILL.TEMPERATURE", 2.0],
                                                   teacher=teacher))]
say(f"X3D-M, {B} x {T} x {S}^2, bf16: teacher.logits (HIP events, 10 calls after 3 warm-ups) and Trainer.step (10 timed steps "
    "after 3 warm-up steps, host clock around a device synchronise)")
for name, step in arms:
    for _ in range(3):
        step()
    torch.cuda.synchronize()
for rnd in range(3):
    fwd = events(lambda: teacher.logits(clips), 3 if rnd == 0 else 1, 10)
    say(f"round {rnd + 1}  {'teacher.logits':<36s} {fwd:7.3f} ms / call")
    ms = {}
    for name, step in arms:
        step()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(10):
            pl = step()
        torch.cuda.synchronize()
        ms[name] = (time.perf_counter() - t0) * 100.0
        extra = f"   kd rows mean {float(pl.kd_rows.double().mean()):.6f}" if pl.kd_rows is not None else ""
        say(f"round {rnd + 1}  {name:<36s} {ms[name]:7.3f} ms / step   loss rows mean {float(pl.loss_rows.double().mean()):.6f}{extra}")
    on, off = ms[arms[1][0]], ms[arms[0][0]]
    say(f"round {rnd + 1}  on - off = {on - off:6.3f} ms = {(on - off) / fwd:4.2f} teacher forwards ({100.0 * (on - off) / off:4.1f} % of the step)")
