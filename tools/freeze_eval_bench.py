"""What SOLVER.FREEZE_EVAL saves a fine-tuning step (profiles/freeze_eval_mi355x.txt).

    python tools/freeze_eval_bench.py [--out FILE]

X3D-M, 64 x 16 x 224^2, bf16, SGD, five arms in ONE process on the MI355X: no FREEZE; FREEZE = [conv1/, stages/0/, stages/1/]
with FREEZE_EVAL off and on; FREEZE = [conv1/, stages/] with FREEZE_EVAL off and on.  Three alternating rounds of 10 timed
Trainer.step after 3 warm-up steps per arm, host clock around one device synchronise.  Per arm: ms per step, the device memory
the arm holds and its peak (torch.cuda.max_memory_allocated over building it and its warm-up steps, less what was allocated
before), and the number of launches in its forward and backward lists.  Each on arm is held against the off arm of the same
round.  The expectation: an on arm makes a strict subset of the off arm's backward launches and keeps fewer tensors, so it is
faster and smaller in every round."""
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
clips = torch.randn((B, T, S, S, 3), generator=g, device=dev, dtype=torch.float32).to(torch.bfloat16)
labels = torch.randint(0, 400, (B,), generator=g, device=dev)
GB = 1 << 30


def arm(over):
    """(step function, info) of one arm; the warm-up steps run here, so that the memory figures are the arm's own"""
    torch.cuda.synchronize()
    base = torch.cuda.memory_allocated(dev)
    torch.cuda.reset_peak_memory_stats(dev)
    cfg = x.get_config("M", over)
    torch.manual_seed(2000)
    model = X3D(cfg, dtype=torch.bfloat16, device=dev, seed=0)
    tr = Trainer(model, cfg)
    state0 = (model.flat_params.clone(), model.flat_velocity.clone())

    def step():
        model.flat_params.copy_(state0[0])
        model.flat_velocity.copy_(state0[1])
        return tr.step(clips, labels, cfg.TRAIN.WARMUP_LR)

    for _ in range(3):
        pl = step()
    torch.cuda.synchronize()
    info = dict(held=(torch.cuda.memory_allocated(dev) - base) / GB, peak=(torch.cuda.max_memory_allocated(dev) - base) / GB,
                fwd=len(pl.fwd), bwd=len(pl.bwd), k=model.frozen_prefix)
    return step, info


PART = ["conv1/", "stages/0/", "stages/1/"]
TRUNK = ["conv1/", "stages/"]
ARMS = [("no FREEZE", None),
        ("FREEZE stem + stages 0-1, FREEZE_EVAL off", ["SOLVER.FREEZE", PART]),
        ("FREEZE stem + stages 0-1, FREEZE_EVAL on", ["SOLVER.FREEZE", PART, "SOLVER.FREEZE_EVAL", True]),
        ("FREEZE stem + all stages, FREEZE_EVAL off", ["SOLVER.FREEZE", TRUNK]),
        ("FREEZE stem + all stages, FREEZE_EVAL on", ["SOLVER.FREEZE", TRUNK, "SOLVER.FREEZE_EVAL", True])]
say(f"X3D-M, {B} x {T} x {S}^2, bf16, SGD: Trainer.step, 10 timed steps after 3 warm-up steps, host clock around a device "
    "synchronise; three alternating rounds")
steps, infos = {}, {}
for name, over in ARMS:
    steps[name], infos[name] = arm(over)
    i = infos[name]
    say(f"{name:<44s} frozen prefix {i['k']:2d} units   launches fwd {i['fwd']:4d}  bwd {i['bwd']:4d}   "
        f"memory held {i['held']:6.2f} GiB  peak {i['peak']:6.2f} GiB")
for rnd in range(3):
    ms = {}
    for name, _ in ARMS:
        step = steps[name]
        step()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(10):
            pl = step()
        torch.cuda.synchronize()
        ms[name] = (time.perf_counter() - t0) * 100.0
        say(f"round {rnd + 1}  {name:<44s} {ms[name]:7.3f} ms / step   loss rows mean {float(pl.loss_rows.double().mean()):.6f}")
    for off, on in ((ARMS[1][0], ARMS[2][0]), (ARMS[3][0], ARMS[4][0])):
        d = ms[on] - ms[off]
        say(f"round {rnd + 1}  {on}: on - off = {d:7.3f} ms ({100.0 * d / ms[off]:5.1f} % of the off step), "
            f"memory held {infos[on]['held'] - infos[off]['held']:6.2f} GiB, launches bwd {infos[on]['bwd'] - infos[off]['bwd']:4d}")
