"""What the layer-wise optimizers cost on the device (writes profiles/layerwise_mi355x.txt).

    python tools/layerwise_bench.py [--out FILE]

At the X3D-M and X3D-XL trainable blocks WITH THEIR REAL SEGMENTS (tensor offsets and lengths from dry models, so the ~250
tiny BatchNorm tensors are in), HIP events around 50 calls after 10 warm-ups, the arms alternating over 3 rounds in one process:
    sgd_ex           x3d_sgd_nesterov_ex (no norm, no ema)      the yardstick: one flat range, 5 streams of 4n bytes + the mask
    seg_sumsq        x3d_seg_sumsq(w)                           1 stream, two launches (partials, per-segment sum)
    lars             x3d_lars                                   sums 2 streams (w, g) + q + apply 5 streams (w, v, g in; w, v out)
    adamw            x3d_adamw                                  7 streams (w, m, v, g in; w, m, v out), one launch
    lamb             x3d_lamb                                   first pass 6 streams (w, m, v, g in; m, v out) + q + apply 4 (w, m, v in; w out)
The buffers (15 - 60 MB) fit the 256 MiB Infinity Cache, so the GB/s are cache-resident rates, as they are in a train step."""
import argparse
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
ap = argparse.ArgumentParser()
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "layerwise_mi355x.txt"), help="the lines are written here at the end")
args = ap.parse_args()
lines = []


def say(s):
    print(s, flush=True)
    lines.append(s)


import x3d_tf_amd as x  # noqa: E402
from x3d_tf_amd import hip, ops  # noqa: E402
from x3d_tf_amd.model import X3D  # noqa: E402
from x3d_tf_amd.segments import SegTable  # noqa: E402

assert torch.cuda.is_available(), "layerwise_bench.py measures on the GPU: there is nothing to time without one"
dev = torch.device("cuda:0")
say(f"device: {torch.cuda.get_device_name(0)}; HIP events, 50 calls after 10 warm-ups, 3 alternating rounds, best and median")
WARM, REPS, ROUNDS = 10, 50, 3
LR, MOM, WD, GS = 0.1, 0.9, 5e-5, 1.0 / 1024.0


def timed(fn):
    """microseconds per call of fn (which only enqueues launches)"""
    for _ in range(WARM):
        fn()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(REPS):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) * 1e3 / REPS


for name in ("M", "XL"):
    dry = X3D(x.get_config(name), device="dry")
    n = dry.n_trainable_flat
    tb = SegTable(dry.segments).to(dev)
    small = sum(1 for s in dry.segments if s.length < hip.SEG_CHUNK)
    gen = torch.Generator(device=dev).manual_seed(1)
    w = torch.randn(n, device=dev, generator=gen)
    v = 0.1 * torch.randn(n, device=dev, generator=gen)
    v2 = v.abs() * 0.01
    g = 1024.0 * torch.randn(n, device=dev, generator=gen)
    mask = dry.l2_mask.to(dev)
    partials = torch.empty(2 * tb.nchunk, dtype=torch.float64, device=dev)
    q = torch.ones(tb.nseg, device=dev)
    out = torch.empty(tb.nseg, dtype=torch.float64, device=dev)
    arms = {
        "sgd_ex": (5, lambda: hip.call("x3d_sgd_nesterov_ex", w.data_ptr(), v.data_ptr(), g.data_ptr(), mask.data_ptr(), LR, MOM,
                                       WD, GS, None, 0.0, None, 0.0, n)),
        "seg_sumsq": (1, lambda: ops.seg_sumsq(w, tb, out, partials)),
        "lars": (7, lambda: ops.lars(w, v, g, tb, LR, MOM, WD, 0.001, 1e-8, False, GS, partials=partials, q=q)),
        "adamw": (7, lambda: ops.adamw(w, v, v2, g, tb, 1e-4, 3, decay=0.01, grad_scale=GS)),
        "lamb": (10, lambda: ops.lamb(w, v, v2, g, tb, 1e-4, 3, decay=0.01, grad_scale=GS, partials=partials, q=q)),
    }
    res = {k: [] for k in arms}
    for _ in range(ROUNDS):
        for k, (_, fn) in arms.items():
            res[k].append(timed(fn))
    say(f"X3D-{name}: {n} floats ({4 * n / 2 ** 20:.1f} MiB per stream), {tb.nseg} segments ({small} shorter than one chunk), "
        f"{tb.nchunk} chunks of <= {hip.SEG_CHUNK}")
    base = min(res["sgd_ex"])
    for k, (streams, _) in arms.items():
        best, med = min(res[k]), sorted(res[k])[len(res[k]) // 2]
        say(f"  {k:<10} best {best:8.1f} us  median {med:8.1f} us  {streams:2d} streams -> {streams * 4 * n / best / 1e3:7.1f} GB/s"
            f"   x{best / base:5.2f} of sgd_ex")
os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
with open(args.out, "w") as f:
    f.write("\n".join(lines) + "\n")
