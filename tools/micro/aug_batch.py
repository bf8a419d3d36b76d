"""Times the construction of one training batch of 64 clips of 16 x 224 x 224 (bf16) from 256 x 340 videos, in one process:
  per-clip   64 x3d_train_clip launches (views.make_train_clip), what InputReader does without AUG.ENABLE
  batched    one views.make_train_batch_aug call: "jitter" rows with neutral colour; "rrc" without contrast (one launch);
             "rrc" with contrast (mean pass + apply pass)
Each configuration: warm-up calls, then --repeats timed groups of --inner calls between two events; the median group is
reported, with the write bandwidth of the 64 x 16 x 224 x 224 x 3 x 2 bytes the batch stores.  The host work of a call
(table build, one small upload) is inside the timed region: it is part of what replaces the 64 launches.

    python tools/micro/aug_batch.py [--out profiles/aug_mi355x.txt]"""
import argparse
import os
import statistics
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
import x3d_tf_amd as x                                  # noqa: E402
from x3d_tf_amd import aug, views                       # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--clips", type=int, default=64)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--repeats", type=int, default=15)
    ap.add_argument("--inner", type=int, default=3)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    n, t, s, f, h, w = a.clips, 16, 224, 32, 256, 340
    cfg = x.get_config("M", ["DATA.TEMP_DURATION", t, "DATA.TRAIN_CROP_SIZE", s, "DATA.FRAME_RATE", 2,
                             "DATA.TRAIN_JITTER_SCALES", [256, 320], "AUG.ENABLE", True])
    g = torch.Generator().manual_seed(0)
    base = torch.randint(0, 256, (4, f, h, w, 3), dtype=torch.uint8, generator=g).to(dev)
    videos = [base[i % 4].clone() for i in range(n)]                 # 64 separate allocations, 26 MB each
    gen = torch.Generator().manual_seed(1)
    dicts = [views.draw_train_params(f, h, w, cfg, gen) for _ in range(n)]
    rng = np.random.default_rng(2)
    jit = [aug.neutral_params("jitter", d["start"], d["jitter"], d["y0"], d["x0"], flip=True) for d in dicts]
    boxes = [aug.rrc_box(h, w, (0.08, 1.0), (0.75, 1.3333), rng)[0] for _ in range(n)]
    rrc = [aug.neutral_params("rrc", d["start"], box=b, flip=bool(i & 1))._replace(brightness=1.2, saturation=0.8)
           for i, (d, b) in enumerate(zip(dicts, boxes))]
    rrc_c = [p._replace(contrast=1.3) for p in rrc]
    out = torch.empty((n, t, s, s, 3), dtype=torch.bfloat16, device=dev)

    def per_clip():
        for i, (v, d) in enumerate(zip(videos, dicts)):
            views.make_train_clip(v, cfg, params=d, out=out[i])

    configs = [("per-clip: 64 x x3d_train_clip", per_clip),
               ("batched: jitter, neutral colour", lambda: views.make_train_batch_aug(videos, cfg, params_list=jit, out=out)),
               ("batched: rrc, no contrast", lambda: views.make_train_batch_aug(videos, cfg, params_list=rrc, out=out)),
               ("batched: rrc, contrast (mean pass)", lambda: views.make_train_batch_aug(videos, cfg, params_list=rrc_c, out=out))]
    nbytes = out.numel() * out.element_size()
    lines = [f"{torch.cuda.get_device_name(0)}; batch {n} x {t} x {s} x {s} x 3 bf16 = {nbytes / 1e6:.1f} MB stored, videos "
             f"{f} x {h} x {w}; median of {a.repeats} groups of {a.inner} calls after {a.warmup} warm-up calls"]
    for name, fn in configs:
        for _ in range(a.warmup):
            fn()
        torch.cuda.synchronize()
        times = []
        for _ in range(a.repeats):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(a.inner):
                fn()
            e1.record()
            e1.synchronize()
            times.append(e0.elapsed_time(e1) / a.inner)
        med = statistics.median(times)
        lines.append(f"{name:38s} {med:8.3f} ms  (min {min(times):.3f}, max {max(times):.3f})  {nbytes / med / 1e6:7.1f} GB/s written")
    text = "\n".join(lines)
    print(text)
    if a.out:
        with open(a.out, "w") as fh:
            fh.write(text + "\n")


if __name__ == "__main__":
    main()
