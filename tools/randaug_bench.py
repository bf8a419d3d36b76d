"""What RandAugment costs beside the batched augmentation call it precedes (profiles/randaug_mi355x.txt).

    python tools/randaug_bench.py [--out FILE]

64 clips of 16 x 256 x 340 (the decoded size of the Kinetics records, T frames per clip as the device-decode reader hands
them over): x3d_randaug_clips with the ops of a seeded "rand-m7-n2-mstd0.5-inc1" and "rand-m7-n4-mstd0.5-inc1" draw, and
x3d_train_clips_aug (random-resized crop to 224, bf16) on the same batch as the yardstick.  HIP events around 10 calls after 3
warm-ups; tables uploaded once, outside the timed region.  Each measurement is a child process under its own `timeout`; the
first one that fails ends the run.  One pass over the batch is 267 MB read and 267 MB written."""
import argparse
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
STEPS = ("aug", "n2", "n4")
N, T, H, W, S = 64, 16, 256, 340, 224


def child(step):
    import numpy as np
    import torch
    import x3d_tf_amd as x
    from x3d_tf_amd import aug, hip, views
    from x3d_tf_amd.config import parse_aa_type
    dev = torch.device("cuda:0")
    g = torch.Generator(device=dev).manual_seed(7)
    videos = [torch.randint(0, 256, (T, H, W, 3), generator=g, device=dev, dtype=torch.uint8) for _ in range(N)]
    cfg = x.get_config("M", ["AUG.ENABLE", True, "AUG.CROP", "rrc", "DATA.TEMP_DURATION", T, "DATA.TRAIN_CROP_SIZE", S])
    lib = hip.load()
    rng = np.random.default_rng(0)
    if step == "aug":
        params = [aug.draw_aug_params(cfg, T, H, W, rng)._replace(start=0) for _ in range(N)]
        out = torch.empty((N, T, S, S, 3), dtype=torch.bfloat16, device=dev)

        def run():
            views.make_train_batch_aug(videos, cfg, params_list=params, out=out, rate=1)
        what = f"x3d_train_clips_aug (rrc -> {S}^2 bf16, tables uploaded per call)"
    else:
        spec = parse_aa_type(f"rand-m7-n{step[1:]}-mstd0.5-inc1")
        ra = [aug.draw_randaug(spec, H, W, rng) for _ in range(N)]
        clips, ops, xform, work_bytes, _ = views.randaug_tables([(T, H, W)] * N, [0] * N, ra, T, 1)
        work = torch.empty((work_bytes,), dtype=torch.uint8, device=dev)
        scratch = torch.empty((int(lib.x3d_randaug_scratch(N, T)),), dtype=torch.uint8, device=dev)
        addrs = torch.tensor([v.data_ptr() for v in videos], dtype=torch.int64, device=dev)
        dc, do, dx = (torch.from_numpy(a).to(dev) for a in (clips, ops, xform))
        fill = views.randaug_fill(cfg)

        def run():
            hip.call("x3d_randaug_clips", addrs.data_ptr(), dc.data_ptr(), do.data_ptr(), dx.data_ptr(), clips.ctypes.data,
                     ops.ctypes.data, xform.ctypes.data, work.data_ptr(), work.numel(), scratch.data_ptr(), N, T, 1,
                     int(ops.shape[1]), *fill)
        per_layer = [sum(1 for r in ra if r[l].name != "none") for l in range(spec.layers)]
        stat = [sum(1 for r in ra if r[l].name in ("AutoContrast", "Equalize", "Contrast")) for l in range(spec.layers)]
        what = (f"x3d_randaug_clips n = {spec.layers} (clips with an op per layer {per_layer}, of them with statistics {stat}, "
                f"work area {work_bytes / 1e6:.0f} MB)")
    for _ in range(3):
        run()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(10):
        run()
    e1.record()
    torch.cuda.synchronize()
    print(f"{what}: {e0.elapsed_time(e1) / 10:.3f} ms per call", flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--step", choices=STEPS)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "randaug_mi355x.txt"))
    args = ap.parse_args()
    if args.step:
        return child(args.step)
    lines = [f"{N} clips of {T} x {H} x {W} uint8 ({N * T * H * W * 3 / 1e6:.0f} MB per pass and direction); HIP events, 10 calls "
             "after 3 warm-ups, one process per line"]
    for step in STEPS:
        r = subprocess.run(["timeout", "-k", "10", "180", sys.executable, os.path.abspath(__file__), "--step", step],
                           capture_output=True, text=True)
        if r.returncode != 0:        # stop at the first failure: nothing more is started on the GPU
            print(r.stdout + r.stderr[-2000:], flush=True)
            print(f"step {step} failed with status {r.returncode}; stopping", flush=True)
            return r.returncode
        lines.append(r.stdout.strip().splitlines()[-1])
        print(lines[-1], flush=True)
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
