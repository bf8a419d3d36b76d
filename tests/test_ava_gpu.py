"""The AVA input pipeline on the GPU: the host box maps (x3d_tf_amd/boxes.py) against the pixels the clip kernels produce, the
reader's two decode modes against each other, the launch structure of a training batch, and Trainer.fit / validate on AvaReader
batches with the frame-mAP held to tests/frame_map_ref.py.  The dataset is tests/test_ava.py's (written into tmp_path)."""
import math
import os
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import x3d_tf_amd as x  # noqa: E402
from tests import frame_map_ref as R  # noqa: E402
from tests import test_ava as A  # noqa: E402
from x3d_tf_amd import ava, boxes as B, hip, views  # noqa: E402
from x3d_tf_amd.aug import neutral_params  # noqa: E402

pytestmark = pytest.mark.gpu
T, S, K, CLASSES = A.T, A.S, A.K, A.CLASSES


# ---- 6. the boxes follow the pixels -----------------------------------------------------------------------------------------
def _video(gpu, h, w, rect):
    """T identical frames, 0 everywhere and 255 inside the integer source rectangle (x1, y1, x2, y2)"""
    v = torch.zeros((T, h, w, 3), dtype=torch.uint8)
    x1, y1, x2, y2 = rect
    v[:, y1:y2, x1:x2] = 255
    return v.to(gpu)


def _found_box(cfg, clip):
    """the clip un-normalised and thresholded at 128 -> (x1, y1, x2, y2) as pixel edges: the first and last column / row at or
    above the threshold (None when no pixel is); every frame and channel must show the same rectangle, its inside filled"""
    mean, std = torch.tensor(cfg.DATA.MEAN), torch.tensor(cfg.DATA.STD)
    px = (clip.float().cpu() * std + mean) * 255.0
    mask = px >= 128.0
    assert bool((mask == mask[0, :, :, :1]).all()), "the frames or channels of the clip differ"
    m = mask[0, :, :, 0]
    if not bool(m.any()):
        return None
    cols, rows = m.any(0).nonzero().flatten(), m.any(1).nonzero().flatten()
    x1, x2, y1, y2 = int(cols[0]), int(cols[-1]) + 1, int(rows[0]), int(rows[-1]) + 1
    # (a corner pixel holds the product of two edge weights and may stay below the threshold where each side alone passes)
    assert bool(m[y1 + 1:y2 - 1, x1 + 1:x2 - 1].all()), "the thresholded region is not a filled rectangle"
    return x1, y1, x2, y2


JIT = dict(jitter=36.0, y0=2, x0=10)                   # 48 x 64 -> 36 x 48, crop at (2, 10)
RRC = dict(crop="rrc", box=(6, 12, 30, 40))            # rows 6..36, columns 12..52 of the source
RECT = (20, 10, 44, 34)
# name, builder, (H, W), source rectangle, parameters, cut by the crop?
CASES = [
    ("jitter", "aug", (48, 64), RECT, neutral_params(**JIT), False),
    ("jitter-mirror", "aug", (48, 64), RECT, neutral_params(flip=True, **JIT), False),
    ("rrc", "aug", (48, 64), RECT, neutral_params(**RRC), False),
    ("rrc-mirror", "aug", (48, 64), RECT, neutral_params(flip=True, **RRC), False),
    ("train-clip", "train", (48, 64), RECT, dict(start=0, jitter=38.0, y0=3, x0=12, flip=True), False),
    ("eval-landscape", "eval", (48, 64), RECT, None, False),
    ("eval-portrait", "eval", (64, 48), (10, 20, 34, 44), None, False),
    ("cut-on-two-sides", "aug", (48, 64), (0, 0, 30, 20), neutral_params(**JIT), True),
    ("cut-on-two-sides-mirror", "aug", (48, 64), (0, 0, 30, 20), neutral_params(flip=True, **JIT), True),
]


def _map(kind, rect, h, w, params):
    b = np.array([rect], np.float64)
    if kind == "aug":
        return B.boxes_through_aug(b, h, w, params, S)
    if kind == "train":
        return B.boxes_through_train(b, h, w, params, S)
    return B.boxes_through_eval(b, h, w, S)


def _build(kind, cfg, video, params):
    if kind == "aug":
        return views.make_train_batch_aug([video], cfg, params_list=[params], rate=1)[0]
    if kind == "train":
        return views.make_train_clip(video, cfg, params=params, rate=1)
    return views.make_eval_views(video, cfg)[0]


@pytest.mark.parametrize("case", CASES, ids=lambda c: c[0])
def test_boxes_follow_the_pixels(gpu, case):
    """A video that is 255 inside an integer rectangle and 0 outside goes through the real clip builder; on each side the edge found
    in the output lies within 1.0 px of the mapped (and, where the crop cuts it, clamped) box.  An output pixel is inside iff the
    source coordinate of its centre is past the source edge (bilinear interpolation of a step crosses half at the edge), which puts
    the found edge within 0.5 px of the mapped one; the uint8 truncation and 128 against 127.5 move the crossing by well under the
    other 0.5 px at the scales used here (0.66 to 1.07 output pixels per source pixel)."""
    name, kind, (h, w), rect, params, cut = case
    cfg = x.get_config("XS", A.BASE)
    mapped = _map(kind, rect, h, w, params)
    packed, _, n, _ = B.clip_and_pack(mapped, None, S, K)
    # the map alone: the rectangle stays at least 3 output pixels wide, and it is cut exactly where the case says
    assert n == 1 and packed[0, 2] - packed[0, 0] >= 3 and packed[0, 3] - packed[0, 1] >= 3
    inside = bool((mapped >= 0).all() and (mapped <= S).all())
    assert inside != cut
    if cut:
        assert int((mapped[0] < 0).sum() + (mapped[0] > S).sum()) == 2
    clip = _build(kind, cfg, _video(gpu, h, w, rect), params)
    torch.cuda.synchronize()
    assert tuple(clip.shape) == (T, S, S, 3)
    found = _found_box(cfg, clip)
    want = np.clip(mapped[0], 0, S)
    print(f"{name}: mapped {mapped[0].tolist()} clamped {want.tolist()} found {found}")
    assert found is not None
    err = np.abs(np.array(found, np.float64) - want)
    assert (err <= 1.0).all(), f"{name}: edges {found} against the mapped box {want.tolist()}: off by {err.tolist()}"
    assert (np.abs(np.array(found, np.float64) - packed[0].astype(np.float64)) <= 1.0).all()


@pytest.mark.parametrize("flip", [False, True], ids=["plain", "mirror"])
def test_a_box_outside_the_crop_is_dropped(gpu, flip):
    """the rectangle lies right of the crop (left of it once mirrored): no pixel of the clip shows it, clip_and_pack drops the box
    and num_boxes says so -- next to a box that stays"""
    cfg = x.get_config("XS", A.BASE)
    h, w = 48, 64
    params = neutral_params(flip=flip, **JIT)
    outside, stays = (58, 30, 64, 46), RECT
    mapped = B.boxes_through_aug(np.array([outside, stays], np.float64), h, w, params, S)
    assert (mapped[0, 0] >= S) if not flip else (mapped[0, 2] <= 0)
    packed, labels, n, kept = B.clip_and_pack(mapped, np.array([[1, 0], [0, 1]], np.float32), S, K)
    assert n == 1 and kept.tolist() == [1] and labels[0].tolist() == [0.0, 1.0] and not packed[1:].any()
    clip = views.make_train_batch_aug([_video(gpu, h, w, outside)], cfg, params_list=[params], rate=1)[0]
    torch.cuda.synchronize()
    assert _found_box(cfg, clip) is None


# ---- 7. / 8. the reader's decode modes and its launches -----------------------------------------------------------------------
def _same(a, b):
    if a is None or b is None:
        return a is None and b is None
    return a.dtype == b.dtype and a.shape == b.shape and torch.equal(a.cpu(), b.cpu())


@pytest.mark.parametrize("aug", [True, False], ids=["aug", "plain"])
def test_decode_modes_agree(gpu, tmp_path, aug):
    cfg = A.make_cfg(tmp_path, "AUG.ENABLE", aug)
    for training, steps in ((True, 7), (False, 100)):
        kw = dict(device=gpu, seed=11, mixed_precision=True, dtype=torch.bfloat16)
        rh, rd = ava.AvaReader(cfg, training, **kw), ava.AvaReader(cfg, training, jpeg_decode="device", **kw)
        ih, idv = rh(2), rd(2)
        n = 0
        try:
            for bh, bd in zip(ih, idv):
                assert len(bh) == len(bd) == (4 if training else 7)
                assert bh[0].is_cuda and bh[0].dtype == torch.bfloat16 and tuple(bh[0].shape) == (2, T, S, S, 3)
                assert all(_same(u, v) for u, v in zip(bh, bd)), n
                assert rh.last_params == rd.last_params and len(rh.last_params) == (2 if training else 0)
                if training:
                    assert bh[1].is_cuda and bh[1].dtype == torch.float32 and tuple(bh[1].shape) == (2, K, CLASSES)
                assert not bh[2].is_cuda and bh[2].dtype == torch.float32 and not bh[3].is_cuda and bh[3].dtype == torch.int64
                n += 1
                if n == steps:
                    break
        finally:
            ih.close()
            idv.close()
        assert n == (7 if training else 4)                 # 7 > the 5 batches of a pass; evaluation: 8 keyframes, one pass


def test_one_decode_and_one_clip_call_per_training_batch(gpu, tmp_path, monkeypatch):
    from x3d_tf_amd import jpeg
    cfg = A.make_cfg(tmp_path)
    calls = {"decode": [], "lib": []}
    real_decode, real_call = jpeg.decode_jpeg_batch, hip.call

    def decode(frames, *a, **k):
        calls["decode"].append(len(frames))
        return real_decode(frames, *a, **k)

    def call(name, *a, **k):
        calls["lib"].append(name)
        return real_call(name, *a, **k)
    monkeypatch.setattr(jpeg, "decode_jpeg_batch", decode)
    monkeypatch.setattr(hip, "call", call)
    r = ava.AvaReader(cfg, True, device=gpu, seed=2, jpeg_decode="device")
    it = r._batches(2)
    for step in (1, 2):
        batch = next(it)
        torch.cuda.synchronize()
        assert tuple(batch[0].shape) == (2, T, S, S, 3)
        assert calls["decode"] == [2 * T] * step                           # every frame of the batch in one call
        assert calls["lib"].count("x3d_train_clips_aug") == step
        assert not any(name in ("x3d_train_clip", "x3d_eval_views", "x3d_randaug_clips") for name in calls["lib"])
    it.close()


# ---- 9. end to end ----------------------------------------------------------------------------------------------------------
def _want_frame_map(m, batches, unannotated=()):
    """tests/frame_map_ref.py on the probabilities read back from `m`; unannotated: (batch, clip) pairs whose ground truth is
    left out (num_gt = 0)"""
    tps, dets, ngt = [], [], np.zeros(CLASSES, np.int32)
    for i, (clips, _, bx, nb, gtb, gtl, ng) in enumerate(batches):
        ng = ng.clone()
        for b, c in unannotated:
            if b == i:
                ng[c] = 0
        p = m(clips, boxes=bx, num_boxes=nb).float().cpu().numpy().reshape(-1, CLASSES)
        tp, det, ngt = R.frame_match(p, bx.numpy(), nb.numpy(), gtb.numpy(), gtl.numpy(), ng.numpy(), 0.5, ngt=ngt)
        tps.append(tp)
        dets.append(det)
    ap, ntp = R.frame_ap(np.concatenate(tps), np.concatenate(dets), ngt)
    return R.frame_map(ap, ngt), ap, ngt, float((np.max(ntp) + 2) * 2.0 ** -52) + 2.0 ** -52


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float32], ids=["bf16", "fp32"])
def test_fit_and_validate_on_reader_batches(gpu, tmp_path, dtype):
    from x3d_tf_amd.model import X3D
    from x3d_tf_amd.params import init_params, randomize_bn_
    from x3d_tf_amd.train import Trainer
    cfg = A.make_cfg(tmp_path)
    m = X3D(cfg, dtype=dtype, device=gpu, seed=0)
    m.load_state_dict(randomize_bn_(init_params(x.build_arch(cfg), seed=3), seed=4))
    tr = Trainer(m, cfg)
    kw = dict(device=gpu, seed=7, mixed_precision=dtype != torch.float32, dtype=dtype, jpeg_decode="device")
    reader = ava.AvaReader(cfg, True, **kw)
    ds = reader(cfg.TRAIN.BATCH_SIZE)
    try:
        losses = tr.fit(ds, epochs=1, validation_data=lambda: ava.AvaReader(cfg, False, **kw)(cfg.TEST.BATCH_SIZE))
    finally:
        ds.close()
    assert tr.opt_step == 2 and len(losses) == 1 and math.isfinite(losses[0])
    assert {"loss", "lr", "mAP", "val_loss", "val_mAP", "val_frame_mAP"} <= set(tr.history)
    assert all(len(v) == 1 for v in tr.history.values()) and math.isfinite(tr.history["loss"][0])
    assert math.isfinite(tr.history["val_frame_mAP"][0])
    assert len(reader.last_params) == 2 and reader.stats["boxes_dropped"] == 2
    # validate on the reader's seven-item batches against the reference on the read-back probabilities and the reader's own boxes
    batches = list(ava.AvaReader(cfg, False, **kw)(cfg.TEST.BATCH_SIZE))
    assert len(batches) == 4 and all(len(b) == 7 and b[1] is None for b in batches)
    r = tr.validate(batches)
    want, ap, ngt, tol = _want_frame_map(m, batches)
    print(f"frame_mAP {r['frame_mAP']} vs {want} (tolerance {tol:.3e}); ap {ap.tolist()} ngt {ngt.tolist()}")
    assert math.isfinite(want) and abs(r["frame_mAP"] - want) <= tol
    assert abs(tr.history["val_frame_mAP"][0] - want) <= tol           # fit's validation read the same set with the same weights
    assert r["gt_boxes"] == sum(R.num_valid(b[4].numpy(), b[6].numpy()) for b in batches) == 9
    assert r["detections"] == sum(R.num_valid(b[2].numpy(), b[3].numpy()) for b in batches) == 12
    # vidA,904 -- ground truth, no proposal -- is in the set (batch 2, first clip) and its misses count: class 4 is annotated there
    # and at vidA,900, so with it the class has two boxes to find instead of one and its AP is half of what it is without
    assert int(batches[2][3][0]) == 0 and int(batches[2][6][0]) == 1 and int(batches[2][5][0, 0, 4]) == 1
    without, ap_wo, ngt_wo, _ = _want_frame_map(m, batches, unannotated=[(2, 0)])
    assert ngt[4] == 2 and ngt_wo[4] == 1 and ap_wo[4] > 0 and ap[4] == ap_wo[4] / 2 and want < without
