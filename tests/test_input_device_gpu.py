"""InputReader(..., jpeg_decode="device") against the default host-decoding reader on the same TFRecords and seed:
identical training and evaluation batches and random draws, and a short Trainer.fit from device-decoded records."""
import os

import numpy as np
import pytest
import torch

from x3d_tf_amd import dataloader as DL

CLASSES = 10
OPTS = ["DATA.TEMP_DURATION", 4, "DATA.TRAIN_CROP_SIZE", 32, "DATA.TRAIN_JITTER_SCALES", [34, 40], "DATA.FRAME_RATE", 2,
        "DATA.TEST_CROP_SIZE", 32, "TEST.NUM_TEMPORAL_VIEWS", 2, "TEST.NUM_SPATIAL_CROPS", 3, "TEST.BATCH_SIZE", 2,
        "NETWORK.NUM_CLASSES", CLASSES, "TRAIN.BATCH_SIZE", 2, "TRAIN.DATASET_SIZE", 4, "TRAIN.EPOCHS", 1]


def _turbo():
    from PIL import features
    return bool(features.check_feature("libjpeg_turbo"))


pytestmark = pytest.mark.skipif(not _turbo(), reason="the device decoder reproduces libjpeg-turbo's decode; this Pillow "
                                                     "is not built on it")


def _cfg():
    import x3d_tf_amd as x
    return x.get_config("XS", OPTS)


def _video(h, w, f, seed):
    rng = np.random.default_rng(seed)
    yy, xx = np.mgrid[0:h, 0:w]
    base = np.sin(yy / 5.0 + seed)[..., None] * 60 + np.cos(xx[..., None] / 7.0 + np.arange(3)) * 60 + 128
    return np.stack([np.clip(base + 9 * t + rng.normal(0, 6, base.shape), 0, 255) for t in range(f)]).astype(np.uint8)


def _write(dirpath, n, seed, progressive_in=None):
    """n videos of 5-19 frames; sizes with partial MCUs; one video may carry a progressive frame (host fall-back)"""
    from PIL import Image
    import io
    os.makedirs(dirpath, exist_ok=True)
    rng = np.random.default_rng(seed)
    recs = []
    for i in range(n):
        h, w = [(41, 50), (40, 48), (37, 61)][i % 3]
        vid = _video(h, w, int(rng.integers(5, 20)), seed * 100 + i)
        jpegs = [DL.encode_jpeg(f) for f in vid]
        if i == progressive_in:
            buf = io.BytesIO()
            Image.fromarray(vid[1]).save(buf, "JPEG", quality=90, progressive=True)
            jpegs = [buf.getvalue()] * len(jpegs)
        recs.append(DL.make_sequence_example(None, int(rng.integers(0, CLASSES)), encoded=jpegs))
    for k in range(0, n, 3):
        DL.write_tfrecords(os.path.join(dirpath, f"part-{k // 3}.tfrecord"), recs[k:k + 3])
    return os.path.join(dirpath, "part-*.tfrecord")


def _compare(cfg, pattern, training, gpu, steps, mixed=False):
    kw = dict(device=gpu, seed=11, mixed_precision=mixed, dtype=torch.bfloat16)
    rh = DL.InputReader(cfg, training, True, **kw)
    rd = DL.InputReader(cfg, training, True, jpeg_decode="device", **kw)
    bs = cfg.TRAIN.BATCH_SIZE if training else cfg.TEST.BATCH_SIZE
    ih, idv = rh(pattern, bs), rd(pattern, bs)
    n = 0
    try:
        for (ch, lh), (cd, ld) in zip(ih, idv):
            assert ch.dtype == cd.dtype and ch.shape == cd.shape
            assert torch.equal(ch, cd), n
            assert torch.equal(lh, ld)
            assert rh.last_params == rd.last_params
            n += 1
            if n == steps:
                break
    finally:
        ih.close()
        idv.close()
    return n, rh.last_params


@pytest.mark.gpu
def test_training_batches_and_draws_equal_the_host_mode(gpu, tmp_path):
    cfg = _cfg()
    pattern = _write(str(tmp_path / "train"), 7, seed=3, progressive_in=4)
    n, last = _compare(cfg, pattern, True, gpu, steps=8)          # > one pass: the repeat and reshuffle are crossed
    assert n == 8 and len(last) == 2 and all("start" in p for p in last)
    n, _ = _compare(cfg, pattern, True, gpu, steps=3, mixed=True)
    assert n == 3


@pytest.mark.gpu
def test_evaluation_batches_equal_the_host_mode(gpu, tmp_path):
    cfg = _cfg()
    pattern = _write(str(tmp_path / "val"), 7, seed=5, progressive_in=2)
    n, last = _compare(cfg, pattern, False, gpu, steps=100)
    assert n == 3 and last == []                                   # 7 videos, batch 2: the seventh is dropped


@pytest.mark.gpu
def test_frames_of_different_sizes_fail_as_in_the_host_mode(gpu, tmp_path):
    cfg = _cfg()
    os.makedirs(tmp_path / "mixed")
    jpegs = [DL.encode_jpeg(f) for f in _video(40, 48, 6, 1)] + [DL.encode_jpeg(_video(41, 50, 1, 2)[0])]
    DL.write_tfrecords(str(tmp_path / "mixed" / "part-0.tfrecord"), [DL.make_sequence_example(None, 1, encoded=jpegs)] * 2)
    pattern = str(tmp_path / "mixed" / "part-*.tfrecord")
    for mode in ("host", "device"):
        it = DL.InputReader(cfg, False, True, device=gpu, jpeg_decode=mode)(pattern, 2)
        with pytest.raises(ValueError, match="same shape"):
            next(it)
        it.close()


@pytest.mark.gpu
def test_fit_from_device_decoded_records(gpu, tmp_path):
    from x3d_tf_amd.model import X3D
    from x3d_tf_amd.train import Trainer
    cfg = _cfg()
    pattern = _write(str(tmp_path / "train"), 4, seed=9)
    m = X3D(cfg, dtype=torch.float32, device=gpu, seed=1)
    tr = Trainer(m, cfg)
    ds = DL.InputReader(cfg, True, True, device=gpu, seed=3, jpeg_decode="device")(pattern, cfg.TRAIN.BATCH_SIZE)
    hist = tr.fit(ds, model_dir=str(tmp_path / "run"))
    ds.close()
    assert len(hist) == 1 and np.isfinite(hist).all()
    assert tr.opt_step == 2
