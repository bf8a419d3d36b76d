"""What SOLVER.FREEZE_BN costs or saves a training step.

    timeout -k 10 300 python tools/frozen_bn_bench.py --out profiles/frozen_bn_mi355x.txt

X3D-M, 64 x 16 x 224^2, bf16, SGD, two arms in ONE process on the MI355X: FREEZE_BN off (the step every plan records without
the key) and FREEZE_BN = [""] (every BatchNorm layer on its moving statistics).  Three alternating rounds of 10 timed
Trainer.step after 3 warm-up steps per arm, host clock around one device synchronise.  Per arm: ms per step and the number of
launches in its forward and backward lists (and of x3d_bn_finalize among them).  The on arm is held against the off arm of the
same round.  The expectation from the code: 84 finalize launches fewer and one batched coefficient launch more in the forward
list, no statistics atomics in the producers' epilogues, and a backward list with one x3d_bn_bwd_finalize launch more for every
layer whose table the off arm's consumers derive themselves (37: the frozen form is the launches', not the consumers')."""
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


def arm(over):
    """(step function, info) of one arm, after its warm-up steps"""
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
    names = [e[0] for e in pl.fwd]
    info = dict(fwd=len(pl.fwd), bwd=len(pl.bwd), fin=names.count("x3d_bn_finalize"), frozen=len(model.frozen_bn),
                acc=sum(1 for b in pl.bn_layers if b.stats is not None))
    return step, info


ARMS = [("FREEZE_BN off", None), ('FREEZE_BN = [""]', ["SOLVER.FREEZE_BN", [""]])]
say(f"X3D-M, {B} x {T} x {S}^2, bf16, SGD: Trainer.step, 10 timed steps after 3 warm-up steps, host clock around a device "
    "synchronise; three alternating rounds")
steps, infos = {}, {}
for name, over in ARMS:
    steps[name], infos[name] = arm(over)
    i = infos[name]
    say(f"{name:<18s} frozen layers {i['frozen']:3d}   launches fwd {i['fwd']:4d} (x3d_bn_finalize {i['fin']:3d})  bwd {i['bwd']:4d}   "
        f"statistics accumulators {i['acc']:3d}")
ms_all = {name: [] for name, _ in ARMS}
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
        ms_all[name].append(ms[name])
        say(f"round {rnd + 1}  {name:<18s} {ms[name]:7.3f} ms / step   loss rows mean {float(pl.loss_rows.double().mean()):.6f}")
    off, on = ARMS[0][0], ARMS[1][0]
    d = ms[on] - ms[off]
    say(f"round {rnd + 1}  on - off = {d:7.3f} ms ({100.0 * d / ms[off]:5.1f} % of the off step), launches fwd "
        f"{infos[on]['fwd'] - infos[off]['fwd']:4d}  bwd {infos[on]['bwd'] - infos[off]['bwd']:4d}")
spread = {name: max(v) - min(v) for name, v in ms_all.items()}
say("spread between rounds: " + ", ".join(f"{name} {s:.3f} ms" for name, s in spread.items()))
