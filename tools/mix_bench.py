"""What mixup costs a training step, and what x3d_mix_clips reaches on its own (profiles/mix_mi355x.txt).

    python tools/mix_bench.py [--parent DIR] [--out FILE]

The headline step (X3D-M, 64 x 16 x 224^2, bf16) through Trainer.step with the feature off, with mixup on (PROB = 1,
SWITCH_PROB = 0) and -- with --parent DIR, the `x3d-tf_amd` package directory of a built checkout of another commit -- through
that commit's package, in ONE process, alternating twice; then x3d_mix_clips alone (HIP events, 20 launches after 5
warm-ups) with its bytes per second.  Compare the latter with the 1 : 1 arm of tools/micro/rw_mix on the same box."""
import argparse
import importlib.util
import os
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
ap = argparse.ArgumentParser()
ap.add_argument("--parent", help="x3d-tf_amd package directory of a built checkout to compare with")
ap.add_argument("--out", help="also write the lines to this file")
args = ap.parse_args()
OUT = args.out
lines = []


def say(s):
    print(s, flush=True)
    lines.append(s)
    if OUT:
        with open(OUT, "w") as f:
            f.write("\n".join(lines) + "\n")


def load_pkg(name, d):
    spec = importlib.util.spec_from_file_location(name, os.path.join(d, "__init__.py"), submodule_search_locations=[d])
    mod = importlib.util.module_from_spec(spec)
    sys.modules[name] = mod
    spec.loader.exec_module(mod)
    return mod


import x3d_tf_amd as cur  # noqa: E402
par = load_pkg("x3d_parent", os.path.abspath(args.parent)) if args.parent else None
dev = torch.device("cuda:0")
B, T, S = 64, 16, 224
g = torch.Generator(device=dev).manual_seed(1000)
clips = torch.randn((B, T, S, S, 3), generator=g, device=dev, dtype=torch.float32).to(torch.bfloat16)
labels = torch.randint(0, 400, (B,), generator=g, device=dev)


def arm(pkg, over):
    model_mod = importlib.import_module(pkg.__name__ + ".model")
    train_mod = importlib.import_module(pkg.__name__ + ".train")
    cfg = pkg.get_config("M", over)
    torch.manual_seed(2000)
    model = model_mod.X3D(cfg, dtype=torch.bfloat16, device=dev, seed=0)
    tr = train_mod.Trainer(model, cfg)
    state0 = (model.flat_params.clone(), model.flat_velocity.clone())

    def step():
        model.flat_params.copy_(state0[0])
        model.flat_velocity.copy_(state0[1])
        return tr.step(clips, labels, cfg.TRAIN.WARMUP_LR)
    return step


arms = [("feature off (this commit)", arm(cur, None))]
if par is not None:
    arms.append(("parent commit", arm(par, None)))
arms.append(("mixup on (PROB 1, SWITCH_PROB 0)", arm(cur, ["MIXUP.ENABLE", True, "MIXUP.PROB", 1.0, "MIXUP.SWITCH_PROB", 0.0])))
say(f"device: {torch.cuda.get_device_name(0)}; X3D-M, {B} x {T} x {S}^2, bf16, Trainer.step, 10 timed steps after 3 warm-up steps, "
    "host clock around a device synchronise")
for name, step in arms:
    for _ in range(3):
        step()
    torch.cuda.synchronize()
for rnd in range(2):
    for name, step in arms:
        step()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(10):
            pl = step()
        torch.cuda.synchronize()
        ms = (time.perf_counter() - t0) * 100.0
        say(f"round {rnd + 1}  {name:<36s} {ms:7.3f} ms / step   loss rows mean {float(pl.loss_rows.double().mean()):.6f}")

from x3d_tf_amd import ops  # noqa: E402
nbytes = clips.numel() * 2
buf = clips.clone()
box = (S // 4, S // 4 + S // 2, S // 4, S // 4 + S // 2)
for name, mode, lam, bx, moved in (("mixup, in place", "mixup", 0.3, (0, 0, 0, 0), 2 * nbytes),
                                   ("CutMix, quarter-frame box, in place", "cutmix", 0.75, box, 2 * nbytes // 4),
                                   ("mixup, out of place", "mixup", 0.3, (0, 0, 0, 0), 2 * nbytes)):
    out = buf if "in place" in name else torch.empty_like(buf)
    for _ in range(5):
        ops.mix_clips(buf, mode, lam, bx, out=out)
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(20):
        ops.mix_clips(buf, mode, lam, bx, out=out)
    e1.record()
    torch.cuda.synchronize()
    ms = e0.elapsed_time(e1) / 20
    say(f"x3d_mix_clips {name:<38s} {ms * 1e3:8.1f} us   {moved / 1e6:7.1f} MB read + written   {moved / ms / 1e9:6.2f} TB/s"
        "   (HIP events, 20 launches after 5 warm-ups)")
