"""Trainer.fit as the reference's `model.fit(...)` runs it (train.py:102-152, utils.py:128-132): training metrics
counted on the device, validation after every epoch, step-based checkpoints and the --pretrained_ckpt start."""
import glob
import json
import os
import socket
import sys

import numpy as np
import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from x3d_tf_amd import dataloader as DL  # noqa: E402

CLASSES = 10
OPTS = ["DATA.TEMP_DURATION", 4, "DATA.TRAIN_CROP_SIZE", 32, "DATA.TRAIN_JITTER_SCALES", [34, 40], "DATA.FRAME_RATE", 1,
        "DATA.TEST_CROP_SIZE", 32, "TEST.NUM_TEMPORAL_VIEWS", 1, "TEST.NUM_SPATIAL_CROPS", 3, "TEST.BATCH_SIZE", 2,
        "NETWORK.NUM_CLASSES", CLASSES, "TRAIN.BATCH_SIZE", 2, "TRAIN.DATASET_SIZE", 4, "TRAIN.EPOCHS", 2]


def _cfg():
    import x3d_tf_amd as x
    return x.get_config("XS", OPTS)


def _write(dirpath, n, seed, per_file=2):
    """n smooth synthetic videos (JPEG-friendly, distinguishable) as TFRecords; returns the file pattern."""
    os.makedirs(dirpath, exist_ok=True)
    rng = np.random.default_rng(seed)
    vids = []
    for i in range(n):
        f = int(rng.integers(5, 9))
        yy, xx = np.mgrid[0:40, 0:48]
        base = np.sin(yy / 5.0 + i + seed)[..., None] * 60 + np.cos(xx[..., None] / 7.0 + np.arange(3) + i) * 60 + 128
        vid = np.stack([np.clip(base + 10 * t, 0, 255) for t in range(f)]).astype(np.uint8)
        vids.append((vid, int(rng.integers(0, CLASSES))))
    for k in range(0, n, per_file):
        DL.write_tfrecords(os.path.join(dirpath, f"part-{k // per_file}.tfrecord"),
                           [DL.make_sequence_example(v, lab) for v, lab in vids[k:k + per_file]])
    return os.path.join(dirpath, "part-*.tfrecord")


def _host_hits(probs, labels):
    """first-index argmax == label; tf.math.in_top_k(k=5): #{p_j > p_y} < 5 (fp64 on the host)"""
    p = probs.double().cpu().numpy()
    t1 = t5 = 0
    for row, y in zip(p, labels.cpu().numpy().astype(np.int64)):
        t1 += int(np.argmax(row) == y)
        t5 += int((row > row[y]).sum() < 5)
    return t1, t5


@pytest.mark.gpu
def test_fit_validates_counts_metrics_and_saves_by_step(gpu, tmp_path):
    from x3d_tf_amd.checkpoint import latest_checkpoint
    from x3d_tf_amd.evaluate import DeviceMetrics
    from x3d_tf_amd.model import X3D
    from x3d_tf_amd.train import Trainer
    cfg = _cfg()
    train_pattern = _write(str(tmp_path / "train"), 4, seed=4)
    val_pattern = _write(str(tmp_path / "val"), 5, seed=8)     # 5 videos, batch 2: two batches, the fifth is dropped
    run = str(tmp_path / "run")
    m = X3D(cfg, dtype=torch.float32, device=gpu, seed=1)
    tr = Trainer(m, cfg)
    seen = []

    def on_step(trainer, pl):
        seen.append((trainer.epoch, pl, pl.probs.clone(), pl.labels.clone()))

    def val():
        return DL.InputReader(cfg, False, True, device=gpu)(val_pattern, cfg.TEST.BATCH_SIZE)

    ds = DL.InputReader(cfg, True, True, device=gpu, seed=3)(train_pattern, cfg.TRAIN.BATCH_SIZE)
    hist = tr.fit(ds, model_dir=run, on_step=on_step, validation_data=val, save_freq=3)
    ds.close()
    h = tr.history
    assert set(h) == {"loss", "lr", "acc", "top_5_acc", "val_loss", "val_acc", "val_top_5_acc"}
    assert all(len(v) == 2 for v in h.values())
    assert h["loss"] == hist and all(np.isfinite(hist))
    assert tr.epoch == 2 and tr.opt_step == 4
    # the training plan survived both validations: the same object in every step of both epochs
    assert [e for e, *_ in seen] == [0, 0, 1, 1]
    assert all(pl is seen[0][1] for _, pl, _, _ in seen)
    # training metrics = an fp64 host recount of the steps' probabilities
    for e in range(2):
        t1 = t5 = 0
        for ep, _, probs, labels in seen:
            if ep == e:
                a, b = _host_hits(probs, labels)
                t1, t5 = t1 + a, t5 + b
        assert h["acc"][e] == t1 / 4 and h["top_5_acc"][e] == t5 / 4, (e, t1, t5)
    # validation of the last epoch = a fresh DeviceMetrics pass with the final weights
    dm = DeviceMetrics(m.regularization_loss())
    for clips, labels in val():
        dm.update(m(clips, training=False), labels)
    want = dm.result()
    assert want["videos"] == 4
    assert h["val_acc"][-1] == want["acc"] and h["val_top_5_acc"][-1] == want["top_5_acc"]
    assert abs(h["val_loss"][-1] - want["loss"]) < 1e-6
    assert 0.0 < h["val_loss"][0] and np.isfinite(h["val_loss"]).all()
    # save_freq=3 over 2 x 2 steps: one write, after global step 3 (epoch index 1) -> ckpt-2, nothing at epoch end
    assert sorted(os.path.basename(p) for p in glob.glob(os.path.join(run, "ckpt-*.index"))) == ["ckpt-2.index"]
    assert latest_checkpoint(run) == os.path.join(run, "ckpt-2")

    # --pretrained_ckpt (train.py:131-143)
    ref = Trainer(X3D(cfg, dtype=torch.float32, device=gpu, seed=7), cfg)
    assert ref.resume(run) == 2 and ref.opt_step == 3
    ckpt2 = ref.model.flat_params.clone()
    assert not torch.equal(ckpt2, m.flat_params)               # written after step 3, not the final weights
    other = str(tmp_path / "other")
    src = Trainer(X3D(cfg, dtype=torch.float32, device=gpu, seed=5), cfg)
    src.save_checkpoint(other, 7)
    for pre in (run, os.path.join(run, "ckpt-2")):             # a directory (its latest checkpoint) or a prefix
        t = Trainer(X3D(cfg, dtype=torch.float32, device=gpu, seed=9), cfg)
        t.epoch = 5
        assert t.resume(str(tmp_path / f"empty-{len(pre)}"), pretrained_ckpt=pre) == 0 and t.epoch == 0
        assert torch.equal(t.model.flat_params, ckpt2) and t.opt_step == 3
    t = Trainer(X3D(cfg, dtype=torch.float32, device=gpu, seed=9), cfg)
    assert t.resume(str(tmp_path / "empty-other"), pretrained_ckpt=other) == 0
    assert torch.equal(t.model.flat_params, src.model.flat_params)
    # a populated model_dir wins: pretrained_ckpt is ignored
    t = Trainer(X3D(cfg, dtype=torch.float32, device=gpu, seed=9), cfg)
    assert t.resume(run, pretrained_ckpt=other) == 2 and t.epoch == 2
    assert torch.equal(t.model.flat_params, ckpt2)
    os.makedirs(tmp_path / "no-ckpt")
    with pytest.raises(FileNotFoundError):
        Trainer(X3D(cfg, dtype=torch.float32, device=gpu, seed=9), cfg).resume(str(tmp_path / "empty-x"),
                                                                                 pretrained_ckpt=str(tmp_path / "no-ckpt"))


@pytest.mark.gpu
def test_fit_without_metrics_or_validation_keeps_loss_and_lr_only(gpu, tmp_path):
    from x3d_tf_amd.model import X3D
    from x3d_tf_amd.train import Trainer
    cfg = _cfg()
    train_pattern = _write(str(tmp_path / "train"), 4, seed=4)
    val_pattern = _write(str(tmp_path / "val"), 4, seed=8)
    m = X3D(cfg, dtype=torch.float32, device=gpu, seed=1)
    tr = Trainer(m, cfg)
    ds = DL.InputReader(cfg, True, True, device=gpu, seed=3)(train_pattern, cfg.TRAIN.BATCH_SIZE)
    hist = tr.fit(ds, epochs=1, metrics=())
    assert tr.history == {"loss": hist, "lr": [tr.history["lr"][0]]} and len(hist) == 1
    # one epoch left: a one-shot iterator is accepted; validation_steps=1 takes its first batch only
    one_shot = DL.InputReader(cfg, False, True, device=gpu)(val_pattern, cfg.TEST.BATCH_SIZE)
    tr.fit(ds, epochs=2, metrics=("acc",), validation_data=one_shot, validation_steps=1)
    ds.close()
    assert set(tr.history) == {"loss", "lr", "acc", "val_loss", "val_acc", "val_top_5_acc"}
    assert all(len(v) == 1 for v in tr.history.values())
    with pytest.raises(StopIteration):
        next(one_shot)                                          # closed after validation


# ---- two ranks on one GPU (gloo, as test_dist.py's Trainer test) ----------------------------------------------------
def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _rank_worker(rank, world, port, tmp):
    sys.path.insert(0, ROOT)
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world),
                      LOCAL_RANK=str(rank), X3D_DIST_BACKEND="gloo")
    from x3d_tf_amd import dist as xd
    from x3d_tf_amd.model import X3D
    from x3d_tf_amd.train import Trainer
    r, lr_, w = xd.init_process_group()
    dev = torch.device(f"cuda:{xd.local_device(lr_)}")
    torch.cuda.set_device(dev)
    cfg = _cfg()
    m = X3D(cfg, dtype=torch.float32, device=dev, seed=1 + rank)
    tr = Trainer(m, cfg)
    val_pattern = os.path.join(tmp, "val", "part-*.tfrecord")

    def val():
        return DL.InputReader(cfg, False, True, device=dev)(val_pattern, cfg.TEST.BATCH_SIZE)

    ds = DL.InputReader(cfg, True, True, device=dev, seed=3)(os.path.join(tmp, "train", "part-*.tfrecord"),
                                                                cfg.TRAIN.BATCH_SIZE)
    tr.fit(ds, epochs=1, validation_data=val)
    ds.close()
    videos = tr.validate(val())["videos"]
    with open(os.path.join(tmp, f"rank{rank}.json"), "w") as f:
        json.dump(dict(history=tr.history, videos=videos), f)
    dist.barrier()
    dist.destroy_process_group()


@pytest.mark.gpu
def test_fit_validation_two_ranks_on_gpu(gpu, tmp_path):
    """every rank validates its shard of the stream; the counters are summed once, so both ranks report the same history
    and the validation covers every video of the set (8 videos, global batch 2: four batches, one video per rank each)"""
    _write(str(tmp_path / "train"), 4, seed=4)
    _write(str(tmp_path / "val"), 8, seed=8)
    mp.spawn(_rank_worker, args=(2, _free_port(), str(tmp_path)), nprocs=2, join=True)
    r0 = json.load(open(tmp_path / "rank0.json"))
    r1 = json.load(open(tmp_path / "rank1.json"))
    assert r0["history"] == r1["history"]
    assert set(r0["history"]) == {"loss", "lr", "acc", "top_5_acc", "val_loss", "val_acc", "val_top_5_acc"}
    assert all(len(v) == 1 for v in r0["history"].values())
    assert r0["videos"] == r1["videos"] == 8
    assert np.isfinite(r0["history"]["val_loss"][0])
