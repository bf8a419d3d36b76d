"""What the solver step costs on the device (prints; --out FILE keeps the lines.  profiles/solver_mi355x.txt holds recorded runs).

    python tools/solver_bench.py [--out FILE] [--spread] [--finetune]

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
--finetune: INSTEAD of the arms above, the fine-tuning entry points at the X3D-M layout (profiles/finetune_mi355x.txt), each next
to the existing entry point of the same rule in the same run, arms alternating, 200 launches per window: x3d_seg_grad_sumsq
against x3d_grad_sumsq; x3d_sgd_pt / x3d_adam_pt against x3d_sgd_nesterov_ex / x3d_adam_ex (byte mask = the l2 flags);
x3d_lars_pt / x3d_adamw_pt / x3d_lamb_pt against x3d_lars / x3d_adamw / x3d_lamb -- all with norm and ema, nothing frozen and
every scale 1; then the step with the stem and the first two stages frozen and LAYER_DECAY 0.75 (seg_grad_sumsq + sgd_pt).
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
ap.add_argument("--finetune", action="store_true", help="the fine-tuning entry points next to their existing counterparts instead")
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
say(f"device: {torch.cuda.get_device_name(0)}; library {os.path.relpath(hip.LIB_PATH, ROOT)}")
WARM, REPS, ROUNDS = 10, 200 if args.finetune else 50, 10
say(f"HIP events, {REPS} launches after {WARM} warm-ups, {ROUNDS} alternating rounds, best and median")
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


def finetune_arms():
    """the _pt entry points next to the existing ones, X3D-M layout"""
    dry = X3D(x.get_config("M"), device="dry")
    n = dry.n_trainable_flat
    tb = SegTable(dry.segments).to(dev)
    gen = torch.Generator(device=dev).manual_seed(1)
    w = torch.randn(n, generator=gen, device=dev)
    v, v2 = torch.zeros(n, device=dev), torch.zeros(n, device=dev)
    g = torch.randn(n, generator=gen, device=dev) * 1024.0
    ema = w.clone()
    mask = dry.l2_mask.to(dev)
    ones = torch.ones(tb.nseg, device=dev)
    partials = torch.empty(2 * tb.nchunk, dtype=torch.float64, device=dev)
    q = torch.ones(tb.nseg, device=dev)
    norm = torch.zeros(2, dtype=torch.float64, device=dev)
    scratch = torch.zeros(int(hip.load().x3d_grad_sumsq_scratch(n)), dtype=torch.float64, device=dev)
    ops.grad_sumsq(g, norm, scratch)
    p = [t.data_ptr() for t in (w, v, g, mask)]
    ex = dict(grad_scale=GS, norm=norm, max_norm=1.0, ema=ema, ema_decay=0.9999)
    tail = (norm.data_ptr(), 1.0, ema.data_ptr(), 0.9999, n)
    dry.set_finetune(freeze=["conv1/", "stages/0/", "stages/1/"], layer_decay=0.75)
    ft = SegTable(dry.tuned_segments).to(dev)
    ft_scale = torch.tensor([dry.lr_scales[s.name] for s in dry.tuned_segments], device=dev)
    ft_n = sum(s.length for s in dry.tuned_segments)
    ft_q = torch.ones(ft.nseg, device=dev)

    def frozen_step():
        ops.seg_grad_sumsq(g, ft, norm, partials)
        ops.sgd_pt(w, v, g, ft, ft_scale, LR, MOM, WD, **ex)

    def full_step():
        ops.grad_sumsq(g, norm, scratch)
        hip.call("x3d_sgd_nesterov_ex", *p, LR, MOM, WD, GS, *tail)

    def full_pt_step():
        ops.seg_grad_sumsq(g, tb, norm, partials)
        ops.sgd_pt(w, v, g, tb, ones, LR, MOM, WD, **ex)

    pairs = [
        ("x3d_grad_sumsq", lambda: ops.grad_sumsq(g, norm, scratch),
         "x3d_seg_grad_sumsq", lambda: ops.seg_grad_sumsq(g, tb, norm, partials), 4 * n),
        ("x3d_sgd_nesterov_ex", lambda: hip.call("x3d_sgd_nesterov_ex", *p, LR, MOM, WD, GS, *tail),
         "x3d_sgd_pt", lambda: ops.sgd_pt(w, v, g, tb, ones, LR, MOM, WD, **ex), 7 * 4 * n),
        ("x3d_adam_ex", lambda: hip.call("x3d_adam_ex", p[0], p[1], v2.data_ptr(), p[2], p[3], 1e-4, 0.9, 0.999, 1e-7, WD, GS, 3,
                                         *tail),
         "x3d_adam_pt", lambda: ops.adam_pt(w, v, v2, g, tb, ones, 1e-4, 3, weight_decay=WD, **ex), 9 * 4 * n),
        ("x3d_lars", lambda: ops.lars(w, v, g, tb, LR, MOM, WD, 0.001, 1e-8, False, partials=partials, q=q, **ex),
         "x3d_lars_pt", lambda: ops.lars_pt(w, v, g, tb, ones, LR, MOM, WD, 0.001, 1e-8, False, partials=partials, q=q, **ex),
         9 * 4 * n),
        ("x3d_adamw", lambda: ops.adamw(w, v, v2, g, tb, 1e-4, 3, decay=0.01, **ex),
         "x3d_adamw_pt", lambda: ops.adamw_pt(w, v, v2, g, tb, ones, 1e-4, 3, decay=0.01, **ex), 9 * 4 * n),
        ("x3d_lamb", lambda: ops.lamb(w, v, v2, g, tb, 1e-4, 3, decay=0.01, partials=partials, q=q, **ex),
         "x3d_lamb_pt", lambda: ops.lamb_pt(w, v, v2, g, tb, ones, 1e-4, 3, decay=0.01, partials=partials, q=q, **ex),
         12 * 4 * n),
        ("step: sumsq + sgd_ex", full_step, "step: seg_grad_sumsq + sgd_pt", full_pt_step, 8 * 4 * n),
        ("step: sumsq + sgd_ex", full_step, "step, stem + 2 stages frozen", frozen_step, 8 * 4 * ft_n),
        ("x3d_lamb", lambda: ops.lamb(w, v, v2, g, tb, 1e-4, 3, decay=0.01, partials=partials, q=q, **ex),
         "x3d_lamb_pt, stem + 2 stages frozen",
         lambda: ops.lamb_pt(w, v, v2, g, ft, ft_scale, 1e-4, 3, decay=0.01, partials=partials, q=ft_q, **ex), 12 * 4 * ft_n),
    ]
    say(f"X3D-M: n_trainable_flat = {n} floats ({4 * n / 1e6:.1f} MB per stream), {tb.nseg} tensors in {tb.nchunk} chunks; "
        f"stem + stages 0, 1 frozen: {ft_n} floats in {ft.nseg} tensors, {ft.nchunk} chunks")
    say("all arms with norm (the clip is active) and ema; bytes and GB/s are those of the second arm, x = second / first at best")
    for old, f_old, new, f_new, nbytes in pairs:
        a, b = [], []
        for _ in range(ROUNDS):
            a.append(timed(f_old))
            b.append(timed(f_new))
        a.sort()
        b.sort()
        say(f"  {old:<22} best {a[0]:8.2f} us  median {a[len(a) // 2]:8.2f} us | {new:<36} best {b[0]:8.2f} us  median "
            f"{b[len(b) // 2]:8.2f} us   {nbytes / 1e6:6.1f} MB  {nbytes / b[0] / 1e3:7.2f} GB/s at best   {b[0] / a[0]:5.2f} x")


if args.finetune:
    finetune_arms()

for name in (() if args.finetune else ("M", "XL")):
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
