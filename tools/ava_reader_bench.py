"""Clips per second of the AVA reader (profiles/ava_reader_mi355x.txt).

    python tools/ava_reader_bench.py [--out FILE] [--batches 10] [--batch 16] [--workers 8]

A synthetic frame tree written into a temporary directory (4 videos of 120 frames, 256 x 340 JPEG, quality 90; a keyframe with
three boxes every second at 10 frames per second), read by `ava.AvaReader` in training mode with AUG.ENABLE -- X3D-M's clip shape,
16 x 224^2, DATA.FRAME_RATE 5, bf16 -- in both decode modes, next to `dataloader.InputReader(jpeg_decode="device")` on TFRecords of
the same frames (one record per video) at the same clip shape and batch.  Per arm a fresh reader, 2 warm-up batches, then the host
clock around `--batches` batches, ending in a device synchronisation; the arms alternate in ONE process over three rounds.  File
I/O and the host's JPEG decoder are part of what is measured: a record, not a gate."""
import argparse
import os
import sys
import tempfile
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
ap = argparse.ArgumentParser()
ap.add_argument("--out", help="also write the lines to this file")
ap.add_argument("--batches", type=int, default=10)
ap.add_argument("--batch", type=int, default=16)
ap.add_argument("--workers", type=int, default=8)
args = ap.parse_args()
lines = []


def say(s):
    print(s, flush=True)
    lines.append(s)
    if args.out:
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


import x3d_tf_amd as x  # noqa: E402
from x3d_tf_amd import ava, dataloader as DL  # noqa: E402

dev = torch.device("cuda:0")
H, W, F, FPS, VIDEOS = 256, 340, 120, 10, 4
K, C = 8, 80


def frame(v, i):
    rng = np.random.default_rng(1000 * v + i)
    yy, xx = np.mgrid[0:H, 0:W]
    base = np.sin(yy / 23.0 + 0.1 * i + v)[..., None] * 60 + np.cos(xx[..., None] / 31.0 + np.arange(3) + 0.05 * i) * 60 + 128
    return np.clip(base + rng.normal(0, 4, base.shape), 0, 255).astype(np.uint8)


def write_tree(root):
    """the frame tree, its frame list, a ground-truth box list and TFRecords of the same JPEG strings"""
    rows, boxes, records = [ava.FRAME_LIST_HEADER], [], []
    os.makedirs(os.path.join(root, "records"))
    for v in range(VIDEOS):
        name = f"video{v}"
        os.makedirs(os.path.join(root, "frames", name))
        jpegs = []
        for i in range(F):
            rel = os.path.join(name, f"{name}_{i + 1:06d}.jpg")
            jpegs.append(DL.encode_jpeg(frame(v, i)))
            with open(os.path.join(root, "frames", rel), "wb") as f:
                f.write(jpegs[-1])
            rows.append(f'{name} {v} {i} {rel} ""')
        for sec in range(900, 900 + F // FPS):
            for p in range(3):
                x1, y1 = 0.05 + 0.25 * p, 0.1 + 0.05 * p
                boxes.append(f"{name},{sec},{x1:.3f},{y1:.3f},{x1 + 0.3:.3f},{y1 + 0.7:.3f},{1 + (sec + 7 * p) % C},{p}")
        records.append(DL.make_sequence_example(None, [v, v + 1], encoded=jpegs))
    for k, rec in enumerate(records):
        DL.write_tfrecords(os.path.join(root, "records", f"part-{k}.tfrecord"), [rec])
    with open(os.path.join(root, "train.csv"), "w") as f:
        f.write("\n".join(rows) + "\n")
    with open(os.path.join(root, "train_gt.csv"), "w") as f:
        f.write("\n".join(boxes) + "\n")
    return os.path.join(root, "records", "part-*.tfrecord")


def rate(batches_iter, n_clips_of):
    """clips per second over args.batches batches after 2 warm-up batches"""
    try:
        for _ in range(2):
            next(batches_iter)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        clips = 0
        for _ in range(args.batches):
            clips += n_clips_of(next(batches_iter))
        torch.cuda.synchronize()
        return clips / (time.perf_counter() - t0)
    finally:
        batches_iter.close()


say(f"device: {torch.cuda.get_device_name(0)}")
with tempfile.TemporaryDirectory() as root:
    t0 = time.perf_counter()
    pattern = write_tree(root)
    cfg = x.get_config("M", ["TEST.NUM_SPATIAL_CROPS", 1, "TEST.NUM_TEMPORAL_VIEWS", 1, "DETECTION.ENABLE", True,
                             "DETECTION.MAX_BOXES", K, "NETWORK.NUM_CLASSES", C, "DATA.MULTI_LABEL", True, "AUG.ENABLE", True,
                             "AVA.FRAME_DIR", os.path.join(root, "frames"), "AVA.FRAME_LIST_DIR", root, "AVA.ANNOTATION_DIR", root,
                             "AVA.TRAIN_GT_BOX_LISTS", ["train_gt.csv"], "AVA.FPS", FPS, "AVA.VALID_SECS", [900, 900 + F // FPS - 1]])
    t, s = int(cfg.DATA.TEMP_DURATION), int(cfg.DATA.TRAIN_CROP_SIZE)
    say(f"{VIDEOS} videos of {F} frames, {H} x {W} JPEG, written in {time.perf_counter() - t0:.1f} s; clips {t} x {s}^2, "
        f"DATA.FRAME_RATE {int(cfg.DATA.FRAME_RATE)}, bf16, AUG.ENABLE ({cfg.AUG.CROP}), batch {args.batch}, {args.workers} workers, "
        f"prefetch 2; {args.batches} batches on the host clock after 2 warm-up batches; three alternating rounds")
    kw = dict(device=dev, seed=1, mixed_precision=True, dtype=torch.bfloat16, num_workers=args.workers)

    def ava_arm(mode):
        return rate(ava.AvaReader(cfg, True, jpeg_decode=mode, **kw)(args.batch), lambda b: int(b[0].shape[0]))

    def tfrecord_arm():
        return rate(DL.InputReader(cfg, True, True, jpeg_decode="device", **kw)(pattern, args.batch), lambda b: int(b[0].shape[0]))

    ARMS = [("AvaReader, jpeg_decode=host", lambda: ava_arm("host")), ("AvaReader, jpeg_decode=device", lambda: ava_arm("device")),
            ("InputReader (TFRecords), jpeg_decode=device", tfrecord_arm)]
    for rnd in range(3):
        for name, fn in ARMS:
            say(f"round {rnd + 1}  {name:<46s} {fn():9.1f} clips/s")
