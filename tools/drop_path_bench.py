"""What stochastic depth costs on the device (writes profiles/drop_path_mi355x.txt, which holds the run on an MI355X).

    python tools/drop_path_bench.py [--out FILE] [--no-step]          (FILE defaults to profiles/drop_path_mi355x.txt)

Kernels: x3d_tail_fwd_dp / x3d_tail_bwd_dp against x3d_tail_fwd / x3d_tail_bwd at a 56 x 56, a 14 x 14 and a 7 x 7 block shape
of X3D-M, batch 64, bf16, identity shortcut -- HIP events around 30 launches after 5 warm-ups, the arms alternating over 3 rounds
in one process.  Bytes: forward c_raw + shortcut in, y out (3 tensors; a dropped sample: 2); backward dy, y, c_raw in, g out
(4), the _dp form writes g_branch too (5; a dropped sample: 4).  "half": every second sample dropped.
Step: X3D-M batch 64 bf16 forward_backward at NETWORK.DROP_PATH_RATE 0.2 against 0 (device draws), alternating, 3 rounds of 10."""
import argparse
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
ap = argparse.ArgumentParser()
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "drop_path_mi355x.txt"), help="the lines are written here at the end")
ap.add_argument("--no-step", action="store_true", help="kernels only")
args = ap.parse_args()
lines = []


def say(s):
    print(s, flush=True)
    lines.append(s)


import x3d_tf_amd as x  # noqa: E402
from x3d_tf_amd import ops  # noqa: E402
from x3d_tf_amd.model import X3D  # noqa: E402

assert torch.cuda.is_available(), "drop_path_bench.py measures on the GPU: there is nothing to time without one"
dev = torch.device("cuda:0")
WARM, REPS, ROUNDS = 5, 30, 3
say(f"device: {torch.cuda.get_device_name(0)}; HIP events, {REPS} launches after {WARM} warm-ups, {ROUNDS} alternating rounds, best")


def timed(fn, warm=WARM, reps=REPS):
    """microseconds per call of fn (which only enqueues launches)"""
    for _ in range(warm):
        fn()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(reps):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) * 1e3 / reps


N, DT = 64, torch.bfloat16
for label, c, p in (("56 x 56 (24 ch, 16 frames)", 24, 16 * 56 * 56), ("14 x 14 (96 ch)", 96, 16 * 14 * 14), ("7 x 7 (192 ch)", 192, 16 * 7 * 7)):
    gen = torch.Generator(device=dev).manual_seed(1)
    mk = lambda: torch.randn(N, c, p, generator=gen, device=dev).to(DT)
    c_raw, sh, y, dy, gbr = mk(), mk(), mk(), mk(), mk()
    ss = torch.stack([torch.ones(c, device=dev), torch.zeros(c, device=dev)], 1).contiguous()
    sums = torch.zeros(c, 2, dtype=torch.float64, device=dev)
    all_kept = torch.full((N,), 1.25, device=dev)
    half = all_kept.clone()
    half[1::2] = 0.0
    tb = c_raw.numel() * 2            # bytes of one tensor
    arms = [
        ("x3d_tail_fwd", lambda: ops.tail_fwd(c_raw, ss, sh, None, y), 3 * tb),
        ("x3d_tail_fwd_dp all kept", lambda: ops.tail_fwd_dp(c_raw, ss, sh, None, all_kept, y), 3 * tb),
        ("x3d_tail_fwd_dp half", lambda: ops.tail_fwd_dp(c_raw, ss, sh, None, half, y), 2.5 * tb),
        ("x3d_tail_bwd", lambda: ops.tail_bwd(dy, y, c_raw, None, sums, None), 4 * tb),
        ("x3d_tail_bwd_dp all kept", lambda: ops.tail_bwd_dp(dy, gbr, y, c_raw, None, all_kept, sums, None), 5 * tb),
        ("x3d_tail_bwd_dp half", lambda: ops.tail_bwd_dp(dy, gbr, y, c_raw, None, half, sums, None), 4.5 * tb),
    ]
    got = {a[0]: [] for a in arms}
    for _ in range(ROUNDS):
        for name, fn, _b in arms:
            got[name].append(timed(fn))
    say(f"X3D-M batch {N} bf16, {label}: {tb / 1e6:.1f} MB per tensor")
    rate = {}
    for name, _fn, nbytes in arms:
        t = min(got[name])
        rate[name] = nbytes / t / 1e3
        say(f"  {name:<26} best {t:8.1f} us  {nbytes / 1e6:7.1f} MB  {rate[name]:7.1f} GB/s")
    say(f"  all kept against the plain kernel, bytes per second: forward {rate['x3d_tail_fwd_dp all kept'] / rate['x3d_tail_fwd']:.3f} x, "
        f"backward {rate['x3d_tail_bwd_dp all kept'] / rate['x3d_tail_bwd']:.3f} x")
    del c_raw, sh, y, dy, gbr

if not args.no_step:
    torch.manual_seed(0)
    clips = torch.randn(N, 16, 224, 224, 3, device=dev).to(DT)
    labels = torch.randint(0, 400, (N,), device=dev)
    ms = {}
    for r in (0.0, 0.2):
        m = X3D(x.get_config("M", ["NETWORK.DROP_PATH_RATE", r]), dtype=DT, device=dev, seed=0)
        m.forward_backward(clips, labels)
        ms[r] = m
    got = {r: [] for r in ms}
    for _ in range(ROUNDS):
        for r, m in ms.items():
            got[r].append(timed(lambda: m.forward_backward(clips, labels), warm=2, reps=10) / 1e3)
    for r, m in ms.items():
        pl = m._plans[(N, 16, 224, 224, True)]
        say(f"X3D-M batch {N} bf16 forward_backward, DROP_PATH_RATE {r}: best {min(got[r]):.2f} ms, all {[round(v, 2) for v in got[r]]}; "
            f"{len(pl.fwd)} + {len(pl.bwd)} launches, forward tails folded {sum(B.tail_fwd_folded for B in pl.blocks)}, "
            f"backward tails folded {sum(B.tail_folded for B in pl.blocks)}")
    say(f"rate 0.2 against rate 0: {min(got[0.2]) / min(got[0.0]):.3f} x")

with open(args.out, "w") as f:
    f.write("\n".join(lines) + "\n")
