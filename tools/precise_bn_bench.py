"""What a precise-BatchNorm batch costs on the device (writes profiles/precise_bn_mi355x.txt).

    python tools/precise_bn_bench.py [--out FILE] [--batch N]        (FILE defaults to profiles/precise_bn_mi355x.txt)

X3D-M 16 x 224 x 224, batch 64, bf16 -- the shape of bench.py -- HIP events around 10 calls after 2 warm-ups, the arms alternating
over 3 rounds in one process, best and all rounds:
  step       forward_backward + apply_sgd: the full training step a precise batch is to be compared with
  forward    model(clips, training=True): what update_bn_stats runs per batch
  accum      x3d_precise_bn_accum on that plan's table (84 layers, one launch), 100 launches per timing
  final      x3d_precise_bn_final, once per update_bn_stats call
  update     update_bn_stats over 4 batches, per batch: forward + accum + the share of the zeroing and of final"""
import argparse
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
ap = argparse.ArgumentParser()
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "precise_bn_mi355x.txt"), help="the lines are written here at the end")
ap.add_argument("--batch", type=int, default=64)
args = ap.parse_args()
lines = []


def say(s):
    print(s, flush=True)
    lines.append(s)


import x3d_tf_amd as x  # noqa: E402
from x3d_tf_amd import hip  # noqa: E402
from x3d_tf_amd.model import X3D  # noqa: E402
from x3d_tf_amd.precise_bn import update_bn_stats  # noqa: E402

assert torch.cuda.is_available(), "precise_bn_bench.py measures on the GPU: there is nothing to time without one"
dev = torch.device("cuda:0")
ROUNDS = 3


def timed(fn, warm=2, reps=10):
    """milliseconds per call of fn (which only enqueues launches)"""
    for _ in range(warm):
        fn()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(reps):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / reps


N, DT = args.batch, torch.bfloat16
torch.manual_seed(0)
clips = torch.randn(N, 16, 224, 224, 3, device=dev).to(DT)
labels = torch.randint(0, 400, (N,), device=dev)
m = X3D(x.get_config("M"), dtype=DT, device=dev, seed=0)
m.forward_backward(clips, labels)
pl = m._plan(N, 16, 224, 224, True)
table = pl.precise_bn_table()
lay = m.precise_bn_layout()
pooled = torch.zeros(lay.pooled_size, dtype=torch.float64, device=dev)
scratch = m.flat_params.clone()                 # final writes here: the model's own statistics stay what training left


def step():
    m.forward_backward(clips, labels)
    m.apply_sgd(0.0, 0.9)


arms = [
    ("step", step, 2, 10),
    ("forward", lambda: m(clips, training=True), 2, 10),
    ("accum", lambda: hip.call("x3d_precise_bn_accum", table.data_ptr(), len(lay.prefixes), pooled.data_ptr()), 5, 100),
    ("final", lambda: hip.call("x3d_precise_bn_final", table.data_ptr(), len(lay.prefixes), pooled.data_ptr(), scratch.data_ptr()), 5, 100),
]
got = {a[0]: [] for a in arms}
got["update"] = []
keep = m.moving_stats_flat().clone()
for _ in range(ROUNDS):
    for name, fn, warm, reps in arms:
        got[name].append(timed(fn, warm, reps))
    got["update"].append(timed(lambda: update_bn_stats(m, [clips] * 4, 4), 1, 3) / 4)
    m.moving_stats_flat().copy_(keep)
say(f"device: {torch.cuda.get_device_name(0)}; X3D-M 16 x 224 x 224, batch {N}, bf16; HIP events, {ROUNDS} alternating rounds")
say(f"{len(lay.prefixes)} BatchNorm layers, {sum(lay.channels)} channels, pooled buffer {lay.pooled_size} doubles")
for name in ("step", "forward", "update"):
    say(f"  {name:<8} best {min(got[name]):8.3f} ms   all {[round(v, 3) for v in got[name]]}")
for name in ("accum", "final"):
    say(f"  {name:<8} best {min(got[name]) * 1e3:8.1f} us   all {[round(v * 1e3, 1) for v in got[name]]}")
say(f"a precise batch (forward + accum) against a training step: {(min(got['forward']) + min(got['accum'])) / min(got['step']):.3f} x")

os.makedirs(os.path.dirname(args.out), exist_ok=True)
with open(args.out, "w") as f:
    f.write("\n".join(lines) + "\n")
