"""What the solver step costs on the device (prints; --out FILE keeps the lines.  profiles/solver_mi355x.txt holds recorded runs).

    python tools/solver_bench.py [--out FILE] [--spread]

At the X3D-M and X3D-XL parameter counts (the flat trainable block, from dry models), HIP events around 50 launches after 10
warm-ups, the arms alternating over 10 rounds in one process:
    plain            x3d_sgd_nesterov                                 5 streams of 4n bytes (w, v, g in; w, v out)
    clip             x3d_grad_sumsq + x3d_sgd_nesterov_ex(norm)       6 streams (+ g once more)
    clip + ema       x3d_grad_sumsq + x3d_sgd_nesterov_ex(norm, ema)  8 streams (+ ema in and out)
    adam_ex          x3d_adam_ex(norm, ema)                           9 streams (w, m, v, g, ema in; w, m, v, ema out)
    ema_update       x3d_ema_update                                   3 streams
    grad_accum       x3d_grad_accum, first = 1 / 0                    2 / 3 streams
    seg_sumsq, lars, adamw, lamb                                      the layer-wise entry points with norm and ema over
                     SegTable(model.segments) of the dry model: 1 / 9 / 9 / 12 streams (tools/layerwise_bench.py: their
                     passes; + ema in and out)
(the l2 mask adds n bytes to each flat update).  The buffers (15 - 60 MB) fit the 256 MiB Infinity Cache, so the GB/s are
cache-resident rates, as they are in a train step, where the backward pass has just written the gradient.
--spread: also the run-to-run spread of the backward pass at the shapes of tests/test_solver_gpu.py (two twin models, same
seed, same batch, max |g_a - g_b| / max |g|), the figure the accumulation tests take their limit from."""
import argparse
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
ap = argparse.ArgumentParser()
ap.add_argument("--out", help="the lines are also written here at the end")
ap.add_argument("--spread", action="store_true", help="measure the backward's run-to-run spread at the test shapes too")
args = ap.parse_args()
lines = []


def say(s):
    print(s, flush=True)
    lines.append(s)


import x3d_tf_amd as x  # noqa: E402
from x3d_tf_amd import hip, ops  # noqa: E402
from x3d_tf_amd.model import X3D  # noqa: E402
from x3d_tf_amd.segments import SegTable  # noqa: E402

assert torch.cuda.is_available(), "solver_bench.py measures on the GPU: there is nothing to time without one"
dev = torch.device("cuda:0")
say(f"device: {torch.cuda.get_device_name(0)}; library {hip.LIB_PATH}")
say("HIP events, 50 launches after 10 warm-ups, 10 alternating rounds, best and median")
WARM, REPS, ROUNDS = 10, 50, 10
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
    gen = torch.Generator(device=dev).manual_seed(1)
    w = torch.randn(n, generator=gen, device=dev)
    v = torch.zeros(n, device=dev)
    g = torch.randn(n, generator=gen, device=dev) * 1024.0
    v2 = v.clone()
    ema = w.clone()
    acc = torch.zeros(n, device=dev)
    partials = torch.empty(2 * tb.nchunk, dtype=torch.float64, device=dev)
    q = torch.ones(tb.nseg, device=dev)
    seg_out = torch.empty(tb.nseg, dtype=torch.float64, device=dev)
    mask = (torch.rand(n, generator=gen, device=dev) < 0.9).to(torch.uint8)
    norm = torch.zeros(2, dtype=torch.float64, device=dev)
    scratch = torch.zeros(int(hip.load().x3d_grad_sumsq_scratch(n)), dtype=torch.float64, device=dev)
    p = [t.data_ptr() for t in (w, v, g, mask)]
    extras = dict(grad_scale=GS, norm=norm, max_norm=1.0, ema=ema, ema_decay=0.9999)

    def plain():
        hip.call("x3d_sgd_nesterov", *p, LR, MOM, WD, GS, n)

    def sumsq():
        ops.grad_sumsq(g, norm, scratch)

    def clip():
        sumsq()
        hip.call("x3d_sgd_nesterov_ex", *p, LR, MOM, WD, GS, norm.data_ptr(), 1.0, None, 0.0, n)

    def clip_ema():
        sumsq()
        hip.call("x3d_sgd_nesterov_ex", *p, LR, MOM, WD, GS, norm.data_ptr(), 1.0, ema.data_ptr(), 0.9999, n)

    def adam_ex():
        hip.call("x3d_adam_ex", p[0], p[1], v2.data_ptr(), p[2], p[3], 1e-3, 0.9, 0.999, 1e-7, WD, GS, 3, norm.data_ptr(), 1.0,
                 ema.data_ptr(), 0.9999, n)

    arms = [("plain: x3d_sgd_nesterov", plain, 5 * 4 * n + n), ("x3d_grad_sumsq alone", sumsq, 4 * n),
            ("clip: sumsq + _ex", clip, 6 * 4 * n + n), ("clip + ema: sumsq + _ex", clip_ema, 8 * 4 * n + n),
            ("x3d_adam_ex(norm, ema)", adam_ex, 9 * 4 * n + n),
            ("x3d_ema_update", lambda: ops.ema_update(ema, w, 0.9999), 3 * 4 * n),
            ("x3d_grad_accum first", lambda: ops.grad_accum(acc, g, first=True), 2 * 4 * n),
            ("x3d_grad_accum add", lambda: ops.grad_accum(acc, g), 3 * 4 * n),
            ("x3d_seg_sumsq", lambda: ops.seg_sumsq(g, tb, seg_out, partials), 4 * n),
            ("x3d_lars(norm, ema)", lambda: ops.lars(w, v, g, tb, LR, MOM, WD, 0.001, 1e-8, False, partials=partials, q=q,
                                                     **extras), 9 * 4 * n),
            ("x3d_adamw(norm, ema)", lambda: ops.adamw(w, v, v2, g, tb, 1e-4, 3, decay=0.01, **extras), 9 * 4 * n),
            ("x3d_lamb(norm, ema)", lambda: ops.lamb(w, v, v2, g, tb, 1e-4, 3, decay=0.01, partials=partials, q=q, **extras),
             12 * 4 * n)]
    got = {a[0]: [] for a in arms}
    for _ in range(ROUNDS):
        for label, fn, _b in arms:
            got[label].append(timed(fn))
    say(f"X3D-{name}: n_trainable_flat = {n} floats ({4 * n / 1e6:.1f} MB per stream)")
    base = min(got[arms[0][0]])
    for label, _fn, nbytes in arms:
        t = sorted(got[label])
        say(f"  {label:<28} best {t[0]:8.2f} us  median {t[len(t) // 2]:8.2f} us   {nbytes / 1e6:7.1f} MB   "
            f"{nbytes / t[0] / 1e3:6.2f} GB/s at best   {t[0] / base:5.2f} x plain")
    del w, v, v2, g, ema, acc, mask

if args.spread:
    # the shapes of the trainer tests in tests/test_solver_gpu.py: XS, 10 classes, no dropout, 2 clips of 4 x 32 x 32, fp32 storage
    cfg = x.get_config("XS", ["DATA.TEMP_DURATION", 4, "DATA.TRAIN_CROP_SIZE", 32, "NETWORK.NUM_CLASSES", 10,
                              "NETWORK.DROPOUT_RATE", 0.0])
    gen = torch.Generator().manual_seed(5)
    x2, y2 = torch.randn(2, 4, 32, 32, 3, generator=gen), torch.randint(0, 10, (2,), generator=gen)
    worst = 0.0
    for rep in range(3):
        gs = []
        for _ in range(2):
            m = X3D(cfg, dtype=torch.float32, device=dev, seed=1)
            m.forward_backward(x2.to(dev), y2.to(dev), global_batch=4)
            gs.append(m.flat_grads.clone())
        s = float((gs[0] - gs[1]).abs().max() / gs[0].abs().max())
        worst = max(worst, s)
        say(f"backward run-to-run spread, XS 2 x 4 x 32 x 32 fp32, pair {rep}: max |g_a - g_b| / max |g| = {s:.3e}")
    say(f"worst of the three pairs: {worst:.3e}")

if args.out:
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")
