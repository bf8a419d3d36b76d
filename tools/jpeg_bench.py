"""Throughput of the JPEG frame decode of the TFRecord input pipeline: device (jpeg.decode_jpeg_batch) against host
(dataloader.decode_jpeg on a thread pool), and InputReader clips/s in both jpeg_decode modes.

    python tools/jpeg_bench.py [--out FILE] [--threads 16] [--reader-batches 4]

Synthetic data made with make_sequence_example: 340x256 and 320x240 frames, 300 frames per video, quality 90 (4:2:0).
Every timed region ends with a synchronise (decode_jpeg_batch waits for its own stream; the reader hands over finished
batches and the consumer synchronises before the clock is read); the first batch / call of each row is warm-up."""
import argparse
import json
import os
import sys
import tempfile
import time
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import x3d_tf_amd as x  # noqa: E402
from x3d_tf_amd import dataloader as DL  # noqa: E402
from x3d_tf_amd.jpeg import decode_jpeg_batch  # noqa: E402

FRAMES = 300


def synth_video(h, w, seed, frames=FRAMES):
    """a moving textured scene with sensor-like noise: JPEG sizes of the order of real 340x256 Kinetics frames"""
    rng = np.random.default_rng(seed)
    yy, xx = np.mgrid[0:h, 0:w].astype(np.float32)
    out = np.empty((frames, h, w, 3), np.uint8)
    for t in range(frames):
        r = 128 + 60 * np.sin((xx + 2 * t) / 11.0 + seed) * np.cos(yy / 17.0)
        g = 128 + 50 * np.cos((yy - t) / 9.0 + seed) + 20 * ((xx // 24 + yy // 24 + t // 8) % 2)
        b = 110 + 70 * np.sin((xx + yy + 3 * t) / 23.0)
        img = np.stack([r, g, b], -1) + rng.normal(0, 7, (h, w, 3))
        out[t] = np.clip(img, 0, 255).astype(np.uint8)
    return out


def encode_frames(video, threads):
    with ThreadPoolExecutor(threads) as ex:
        return list(ex.map(DL.encode_jpeg, video))


def time_it(fn, reps):
    fn()                                     # warm-up
    t0 = time.perf_counter()
    for _ in range(reps):
        fn()
    return (time.perf_counter() - t0) / reps


def reader_rate(cfg, pattern, training, mode, batch, batches, threads, dev):
    r = DL.InputReader(cfg, training, True, device=dev, seed=0, num_workers=threads, jpeg_decode=mode,
                       mixed_precision=training, dtype=torch.bfloat16)
    it = r(pattern, batch)
    clips, _ = next(it)                      # warm-up batch (thread pools, allocator, first launches)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    n = 0
    for _ in range(batches):
        clips, _ = next(it)
        n += clips.shape[0]
    torch.cuda.synchronize()
    dt = time.perf_counter() - t0
    it.close()
    return n / dt, dt / batches


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None, help="also write the JSON lines here")
    ap.add_argument("--threads", type=int, default=16)
    ap.add_argument("--reader-batches", type=int, default=4)
    ap.add_argument("--videos", type=int, default=8, help="distinct synthetic videos per size")
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    rows = []

    def emit(**kw):
        rows.append(kw)
        print(json.dumps(kw), flush=True)

    t0 = time.perf_counter()
    enc = {}
    for (h, w) in [(256, 340), (240, 320)]:
        enc[(h, w)] = [encode_frames(synth_video(h, w, seed=17 * i + h), a.threads) for i in range(a.videos)]
    sizes = [len(j) for v in enc[(256, 340)] for j in v]
    emit(what="data", videos_per_size=a.videos, frames_per_video=FRAMES, mean_jpeg_bytes_340x256=float(np.mean(sizes)),
         encode_s=round(time.perf_counter() - t0, 1), device=torch.cuda.get_device_name(0))

    # -- frame decode: device vs host ------------------------------------------------------------------------------
    for (h, w), vids in enc.items():
        pool = [j for v in vids for j in v]
        for n in (256, 1024, 4096):
            frames = [pool[i % len(pool)] for i in range(n)]
            out = torch.empty((n, h, w, 3), dtype=torch.uint8, device=dev)
            dt = time_it(lambda: decode_jpeg_batch(frames, dev, out=out), reps=5 if n < 4096 else 3)
            emit(what="device_decode", frame=f"{w}x{h}", frames_per_batch=n, ms_per_batch=round(dt * 1e3, 2),
                 frames_per_s=round(n / dt))
        frames = pool[:2048]
        with ThreadPoolExecutor(a.threads) as ex:
            dt = time_it(lambda: list(ex.map(DL.decode_jpeg, frames)), reps=2)
        emit(what="host_decode", frame=f"{w}x{h}", threads=a.threads, frames=len(frames), frames_per_s=round(len(frames) / dt))

    # -- InputReader clips/s in both modes ----------------------------------------------------------------------------
    with tempfile.TemporaryDirectory() as tmp:
        recs = []
        for (h, w), vids in enc.items():
            for i, v in enumerate(vids):
                recs.append(DL.make_sequence_example(None, i % 400, encoded=v))
        DL.write_tfrecords(os.path.join(tmp, "part-0.tfrecord"), recs[0::2], level=1)
        DL.write_tfrecords(os.path.join(tmp, "part-1.tfrecord"), recs[1::2], level=1)
        pattern = os.path.join(tmp, "part-*.tfrecord")
        DL.write_tfrecords(os.path.join(tmp, "eval-0.tfrecord"), recs * 3, level=1)     # evaluation makes one pass
        m = x.get_config("M")
        s = x.get_config("S")
        for mode in ("host", "device"):
            rate, per = reader_rate(m, pattern, True, mode, 64, a.reader_batches, a.threads, dev)
            emit(what="reader", config="X3D-M train", batch=64, T=int(m.DATA.TEMP_DURATION), crop=int(m.DATA.TRAIN_CROP_SIZE),
                 mode=mode, clips_per_s=round(rate, 1), s_per_batch=round(per, 3))
        eb = int(s.TEST.BATCH_SIZE)
        for mode in ("host", "device"):
            rate, per = reader_rate(s, os.path.join(tmp, "eval-*.tfrecord"), False, mode, eb, a.reader_batches, a.threads, dev)
            views = int(s.TEST.NUM_TEMPORAL_VIEWS) * int(s.TEST.NUM_SPATIAL_CROPS)
            emit(what="reader", config="X3D-S eval", batch=eb, T=int(s.DATA.TEMP_DURATION), crop=int(s.DATA.TEST_CROP_SIZE),
                 views=views, mode=mode, clips_per_s=round(rate, 1), videos_per_s=round(rate / views, 2),
                 s_per_batch=round(per, 3))
    if a.out:
        with open(a.out, "w") as f:
            for r in rows:
                f.write(json.dumps(r) + "\n")


if __name__ == "__main__":
    main()
