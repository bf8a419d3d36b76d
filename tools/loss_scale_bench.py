"""What SOLVER.DEVICE_LOSS_SCALE does to an fp16 training step (profiles/loss_scale_mi355x.txt).

    python tools/loss_scale_bench.py [--out FILE]

X3D-M, 64 x 16 x 224^2, SGD, three arms in ONE process on the MI355X: float16 with the switch off (the host asks grads_finite()
in every step and waits for the answer), float16 with the switch on (the scaler lives on the device, the step reads nothing), and
bfloat16 (no loss scaling) for context.  Three alternating rounds of 10 timed Trainer.step after 3 warm-up steps per arm, host
clock around one device synchronise.  Before its warm-up each fp16 arm steps until its scale has settled (a step is applied,
not skipped), so that the timed steps of both are applied steps: a skipped step of the off arm launches no update at all and
would not be the same work.  The skipped steps of every round are printed; they should be 0.

The on arm is held against the off arm of the same round.  No speed-up is promised: on one GPU the off arm loses the host's
lead once per step and the on arm adds three small launches; what the switch removes is a stall every data-parallel rank takes
at the same place, which one GPU cannot show."""
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
args = ap.parse_args()
lines = []


def say(s):
    print(s, flush=True)
    lines.append(s)
    if args.out:
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


import x3d_tf_amd as x  # noqa: E402
from x3d_tf_amd.model import X3D  # noqa: E402
from x3d_tf_amd.train import Trainer  # noqa: E402

dev = torch.device("cuda:0")
say(f"device: {torch.cuda.get_device_name(0)}")
B, T, S = args.batch, 16, 224
g = torch.Generator(device=dev).manual_seed(1000)
clips32 = torch.randn((B, T, S, S, 3), generator=g, device=dev, dtype=torch.float32)
labels = torch.randint(0, 400, (B,), generator=g, device=dev)


def arm(over, dtype):
    """(step function, trainer) of one arm, settled and warmed up"""
    cfg = x.get_config("M", over)
    torch.manual_seed(2000)
    model = X3D(cfg, dtype=dtype, device=dev, seed=0)
    tr = Trainer(model, cfg)
    clips = clips32.to(dtype)
    state0 = (model.flat_params.clone(), model.flat_velocity.clone())

    def step():
        model.flat_params.copy_(state0[0])
        model.flat_velocity.copy_(state0[1])
        return tr.step(clips, labels, cfg.TRAIN.WARMUP_LR)

    settle = 0
    while tr.dynamic_scale and tr.opt_step == 0 and settle < 40:      # (reading opt_step synchronises: not timed)
        step()
        settle += 1
    for _ in range(3):
        step()
    torch.cuda.synchronize()
    return step, tr, settle


ARMS = [("fp16, DEVICE_LOSS_SCALE off", None, torch.float16),
        ("fp16, DEVICE_LOSS_SCALE on", ["SOLVER.DEVICE_LOSS_SCALE", True], torch.float16),
        ("bf16 (no loss scaling)", None, torch.bfloat16)]
say(f"X3D-M, {B} x {T} x {S}^2, SGD: Trainer.step, 10 timed steps after 3 warm-up steps, host clock around a device synchronise; "
    "three alternating rounds")
steps, trainers = {}, {}
for name, over, dtype in ARMS:
    steps[name], trainers[name], settle = arm(over, dtype)
    tr = trainers[name]
    say(f"{name:<30s} settled after {settle:2d} steps at loss scale {tr.loss_scale:g}, skipped so far {tr.skipped_steps}")
diffs = []
for rnd in range(3):
    ms = {}
    for name, _, _ in ARMS:
        step, tr = steps[name], trainers[name]
        step()
        torch.cuda.synchronize()
        skipped = tr.skipped_steps
        t0 = time.perf_counter()
        for _ in range(10):
            pl = step()
        torch.cuda.synchronize()
        ms[name] = (time.perf_counter() - t0) * 100.0
        say(f"round {rnd + 1}  {name:<30s} {ms[name]:7.3f} ms / step = {B / ms[name] * 1000.0:7.1f} clips/s   skipped steps "
            f"{tr.skipped_steps - skipped}   loss rows mean {float(pl.loss_rows.double().mean()):.6f}")
    d = ms[ARMS[1][0]] - ms[ARMS[0][0]]
    diffs.append(d)
    say(f"round {rnd + 1}  on - off = {d:7.3f} ms ({100.0 * d / ms[ARMS[0][0]]:5.2f} % of the off step)")
say(f"on - off over the rounds: min {min(diffs):.3f} ms, max {max(diffs):.3f} ms, spread {max(diffs) - min(diffs):.3f} ms")
