"""The AVA input pipeline on the host: the box maps of x3d_tf_amd/boxes.py against closed forms, clip_and_pack, the parsers and
keyframe arithmetic of x3d_tf_amd/ava.py, the reader's order, draws and shards (AvaReader.host_batches: everything of a batch but
its clips), and the refusals of config.ava_reader_check.  The dataset is written here: 48 x 64 JPEG frames and CSVs as strings.
tests/test_ava_gpu.py holds the maps to the pixels the clip kernels produce."""
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import x3d_tf_amd as x  # noqa: E402
from x3d_tf_amd import ava, boxes as B  # noqa: E402
from x3d_tf_amd.aug import neutral_params  # noqa: E402
from x3d_tf_amd.config import ava_reader_check, ava_settings  # noqa: E402

H, W, F = 48, 64, 12
T, S, K, CLASSES = 4, 32, 4, 7
VIDEOS = ("vidA", "vidB")
BASE = ["DATA.TEMP_DURATION", T, "DATA.FRAME_RATE", 2, "DATA.TRAIN_CROP_SIZE", S, "DATA.TEST_CROP_SIZE", S,
        "DATA.TRAIN_JITTER_SCALES", [34, 40], "TEST.NUM_SPATIAL_CROPS", 1, "TEST.NUM_TEMPORAL_VIEWS", 1, "TEST.BATCH_SIZE", 2,
        "NETWORK.NUM_CLASSES", CLASSES, "TRAIN.BATCH_SIZE", 2, "TRAIN.DATASET_SIZE", 4, "TRAIN.EPOCHS", 1,
        "DETECTION.ENABLE", True, "DETECTION.MAX_BOXES", K, "DATA.MULTI_LABEL", True, "AUG.ENABLE", True,
        "AVA.FPS", 2, "AVA.START_SEC", 900, "AVA.VALID_SECS", [900, 905]]

# video,sec,x1,y1,x2,y2,label,person: seconds 900..905 are frames 0, 2, .., 10 of the 12
TRAIN_GT = """\
vidA,899,0.100,0.100,0.500,0.500,1,0
vidA,900,0.100,0.200,0.600,0.900,3,1
vidA,900,0.100,0.200,0.600,0.900,5,1
vidA,900,0.500,0.100,0.950,0.800,,2
vidA,901,0.050,0.050,0.450,0.950,1,1
vidA,902,0.300,0.250,0.700,0.750,2,1
vidA,902,0.300,0.250,0.700,0.750,7,1
vidA,903,0.020,0.100,0.300,0.600,4,1
vidA,903,0.150,0.150,0.550,0.850,4,2
vidA,903,0.400,0.200,0.800,0.900,6,3
vidA,903,0.600,0.050,0.980,0.700,1,4
vidA,903,0.250,0.300,0.650,0.950,2,5
vidA,903,0.700,0.400,0.990,0.990,3,6
vidA,904,0.200,0.200,0.800,0.800,5,1
vidA,905,0.350,0.100,0.900,0.650,6,1
vidA,906,0.100,0.100,0.500,0.500,1,0
vidB,900,0.150,0.100,0.700,0.900,1,1
vidB,901,0.250,0.200,0.750,0.800,2,1
vidB,901,0.250,0.200,0.750,0.800,3,1
vidB,902,0.100,0.300,0.500,0.950,4,1
vidB,903,0.450,0.150,0.950,0.850,5,1
vidB,904,0.200,0.100,0.600,0.700,6,1
"""
# predicted training boxes: label, then score; 0.5 is under the threshold
TRAIN_PRED = """\
vidB,900,0.550,0.200,0.950,0.800,2,0.95
vidB,900,0.050,0.050,0.300,0.400,3,0.50
vidB,900,0.150,0.100,0.700,0.900,6,0.99
"""
# proposals of the evaluation: vidA 900..903 and vidB 900..902; vidA,901 has six, two of them tied at 0.97
TEST_PRED = """\
vidA,900,0.100,0.200,0.600,0.900,,0.99
vidA,900,0.520,0.120,0.930,0.790,,0.95
vidA,900,0.000,0.000,0.200,0.200,,0.30
vidA,901,0.050,0.050,0.450,0.950,,0.91
vidA,901,0.500,0.050,0.900,0.950,,0.97
vidA,901,0.100,0.100,0.300,0.300,,0.92
vidA,901,0.200,0.200,0.600,0.600,,0.97
vidA,901,0.600,0.600,0.900,0.900,,0.93
vidA,901,0.050,0.500,0.400,0.900,,0.99
vidA,902,0.320,0.240,0.710,0.760,,0.98
vidA,903,0.150,0.150,0.550,0.850,,0.96
vidA,903,0.420,0.210,0.790,0.880,,0.94
vidB,900,0.150,0.100,0.700,0.900,,0.99
vidB,901,0.600,0.100,0.950,0.500,,0.92
vidB,902,0.100,0.300,0.500,0.950,,0.97
"""
# annotated boxes of the evaluation: vidA,904 has ground truth but no proposal; vidB,902 is excluded
TEST_GT = """\
vidA,900,0.100,0.200,0.600,0.900,3,1
vidA,900,0.100,0.200,0.600,0.900,5,1
vidA,900,0.500,0.100,0.950,0.800,1,2
vidA,901,0.050,0.050,0.450,0.950,1,1
vidA,902,0.300,0.250,0.700,0.750,2,1
vidA,903,0.150,0.150,0.550,0.850,4,1
vidA,903,0.400,0.200,0.800,0.900,6,2
vidA,904,0.200,0.200,0.800,0.800,5,1
vidB,900,0.150,0.100,0.700,0.900,1,1
vidB,901,0.250,0.200,0.750,0.800,2,1
vidB,902,0.100,0.300,0.500,0.950,4,1
"""
EXCLUDED = "vidB,902\nvidB,1000\n"


def frame(video, index, h=H, w=W):
    """a smooth, textured frame that differs per video and index"""
    rng = np.random.default_rng(1000 * VIDEOS.index(video) + index)
    yy, xx = np.mgrid[0:h, 0:w]
    base = np.sin(yy / 5.0 + index)[..., None] * 60 + np.cos(xx[..., None] / 7.0 + np.arange(3)) * 60 + 128
    return np.clip(base + rng.normal(0, 6, base.shape), 0, 255).astype(np.uint8)


def write_dataset(root):
    """frames, frame lists and annotation files under `root`; returns the AVA.* overrides pointing at them"""
    from x3d_tf_amd.dataloader import encode_jpeg
    root = str(root)
    rows = [ava.FRAME_LIST_HEADER]
    for vi, v in enumerate(VIDEOS):
        os.makedirs(os.path.join(root, "frames", v), exist_ok=True)
        for i in range(F):
            rel = os.path.join(v, f"{v}_{i + 1:06d}.jpg")
            with open(os.path.join(root, "frames", rel), "wb") as f:
                f.write(encode_jpeg(frame(v, i)))
            rows.append(f'{v} {vi} {i} {rel} ""')
    os.makedirs(os.path.join(root, "lists"), exist_ok=True)
    os.makedirs(os.path.join(root, "ann"), exist_ok=True)
    for name in ("train.csv", "val.csv"):
        with open(os.path.join(root, "lists", name), "w") as f:
            f.write("\n".join(rows) + "\n")
    for name, text in (("train_gt.csv", TRAIN_GT), ("train_pred.csv", TRAIN_PRED), ("val_pred.csv", TEST_PRED),
                       ("val_gt.csv", TEST_GT), ("val_excluded.csv", EXCLUDED)):
        with open(os.path.join(root, "ann", name), "w") as f:
            f.write(text)
    return ["AVA.FRAME_DIR", os.path.join(root, "frames"), "AVA.FRAME_LIST_DIR", os.path.join(root, "lists"),
            "AVA.ANNOTATION_DIR", os.path.join(root, "ann"), "AVA.TRAIN_GT_BOX_LISTS", ["train_gt.csv"],
            "AVA.TRAIN_PREDICT_BOX_LISTS", ["train_pred.csv"], "AVA.TEST_PREDICT_BOX_LISTS", ["val_pred.csv"],
            "AVA.GROUNDTRUTH_FILE", "val_gt.csv", "AVA.EXCLUSION_FILE", "val_excluded.csv"]


def make_cfg(root, *over):
    return x.get_config("XS", BASE + write_dataset(root) + list(over))


def _close(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return bool(np.all(np.abs(a - b) <= 1e-12 * np.maximum(np.abs(b), 1e-300)))


# ---- 1. the maps against closed forms -----------------------------------------------------------------------------------------
BOXES = np.array([[3.0, 5.0, 20.0, 31.0], [0.0, 0.0, 64.0, 64.0], [10.25, 7.5, 11.75, 40.125]])


def test_maps_against_closed_forms():
    # identity: the short side already is the target, zero origin, S the frame
    p = dict(start=0, jitter=32.0, y0=0, x0=0, flip=False)
    b = BOXES / 2
    assert B.boxes_through_train(b, 32, 32, p, 32).dtype == np.float64
    assert _close(B.boxes_through_train(b, 32, 32, p, 32), b)
    assert _close(B.boxes_through_aug(b, 32, 32, neutral_params(jitter=32.0), 32), b)
    # a pure scale: 48 x 64 -> 24 x 32
    half = dict(start=0, jitter=24.0, y0=0, x0=0, flip=False)
    assert _close(B.boxes_through_train(BOXES, 48, 64, half, 24), BOXES / 2)
    # a pure shift: 48 x 64 stays, origin (5, 7)
    shift = dict(start=0, jitter=48.0, y0=5, x0=7, flip=False)
    assert _close(B.boxes_through_train(BOXES, 48, 64, shift, 32), BOXES - np.array([7.0, 5.0, 7.0, 5.0]))
    assert _close(B.boxes_through_aug(BOXES, 48, 64, neutral_params(jitter=48.0, y0=5, x0=7), 32),
                  BOXES - np.array([7.0, 5.0, 7.0, 5.0]))
    # both axes scaled differently (the long side is floored): 48 x 64 at 35 -> 35 x 46
    from x3d_tf_amd.views import train_resized_hw
    assert train_resized_hw(48, 64, 35.0) == (35, 46)
    got = B.boxes_through_train(BOXES, 48, 64, dict(start=0, jitter=35.0, y0=2, x0=9, flip=False), 32)
    want = BOXES * np.array([46 / 64, 35 / 48, 46 / 64, 35 / 48]) - np.array([9.0, 2.0, 9.0, 2.0])
    assert _close(got, want)
    # the mirror: x1' = S - x2, an involution, and it is what flip=True adds
    m = B.mirror(BOXES, 32)
    assert _close(m[:, 0], 32 - BOXES[:, 2]) and _close(m[:, 2], 32 - BOXES[:, 0]) and _close(m[:, [1, 3]], BOXES[:, [1, 3]])
    assert _close(B.mirror(m, 32), BOXES)
    assert _close(B.boxes_through_train(BOXES, 48, 64, dict(shift, flip=True), 32), B.mirror(BOXES - [7.0, 5.0, 7.0, 5.0], 32))
    assert _close(B.boxes_through_train(BOXES, 48, 64, dict(start=0, jitter=48.0, y0=5, x0=7), 32),       # flip defaults to True
                  B.mirror(BOXES - [7.0, 5.0, 7.0, 5.0], 32))
    assert _close(B.boxes_through_aug(BOXES, 48, 64, neutral_params(jitter=48.0, y0=5, x0=7, flip=True), 32),
                  B.mirror(BOXES - [7.0, 5.0, 7.0, 5.0], 32))
    # rrc of the whole frame is the scale case
    whole = neutral_params(crop="rrc", box=(0, 0, 64, 64))
    assert _close(B.boxes_through_aug(BOXES, 64, 64, whole, 32), B.boxes_through_aug(BOXES, 64, 64, neutral_params(jitter=32.0), 32))
    assert _close(B.boxes_through_aug(BOXES, 64, 64, whole, 32), BOXES / 2)
    # rrc of a part: (x - rx0) * S / rw
    part = neutral_params(crop="rrc", box=(4, 6, 40, 20), flip=True)
    want = (BOXES - np.array([6.0, 4.0, 6.0, 4.0])) * np.array([32 / 20, 32 / 40, 32 / 20, 32 / 40])
    assert _close(B.boxes_through_aug(BOXES, 64, 64, part, 32), B.mirror(want, 32))
    with pytest.raises(ValueError, match="crop mode"):
        B.boxes_through_aug(BOXES, 64, 64, neutral_params()._replace(crop="centre"), 32)


@pytest.mark.parametrize("hw", [(48, 64), (64, 48), (50, 75), (45, 64), (32, 32), (32, 57), (100, 33)])
def test_eval_geometry_is_the_centre_crop_of_views_hip(hw):
    """csrc/views.hip: the short side becomes `size` and the long side floor((long / short) * size) in float32 -- unchanged when
    the short side already is `size` -- and with one crop sidx is 1: yoff[1] = (nh - size + 1) / 2, xoff[1] = (nw - size + 1) / 2
    in integers, i.e. ceil((n - size) / 2)"""
    import math
    h, w = hw
    size = 32
    nh, nw = h, w
    if min(h, w) != size:
        ratio = np.float32(max(h, w)) / np.float32(min(h, w))
        long_side = int(np.floor(ratio * np.float32(size)))
        nh, nw = (long_side, size) if w < h else (size, long_side)
    y0, x0 = math.ceil((nh - size) / 2), math.ceil((nw - size) / 2)
    assert B.eval_geometry(h, w, size) == (nh, nw, y0, x0)
    want = BOXES * np.array([nw / w, nh / h, nw / w, nh / h]) - np.array([x0, y0, x0, y0], np.float64)
    assert _close(B.boxes_through_eval(BOXES, h, w, size), want)


# ---- 2. clip_and_pack ---------------------------------------------------------------------------------------------------------
def test_clip_and_pack():
    s, k = 32, 4
    boxes = np.array([[-40.0, 2.0, -3.0, 20.0],           # wholly outside
                      [4.0, 5.0, 20.0, 21.5],             # inside
                      [31.5, 3.0, 50.0, 20.0],            # a sliver of 0.5 px after the clamp
                      [np.nan, 1.0, 9.0, 9.0],            # not finite
                      [-5.0, -6.0, 10.0, 40.0],           # cut on three sides
                      [2.0, 2.0, 3.0, 30.0],              # exactly 1 px wide: kept
                      [1.0, 1.0, np.inf, 9.0]])
    labels = np.arange(7 * 3, dtype=np.float32).reshape(7, 3) + 1
    out, lab, n, kept = B.clip_and_pack(boxes, labels, s, k)
    assert out.dtype == np.float32 and out.shape == (k, 4) and lab.dtype == np.float32 and lab.shape == (k, 3)
    assert n == 3 and kept.tolist() == [1, 4, 5]                       # input order
    assert out[:3].tolist() == [[4.0, 5.0, 20.0, 21.5], [0.0, 0.0, 10.0, 32.0], [2.0, 2.0, 3.0, 30.0]]
    assert np.array_equal(lab[:3], labels[[1, 4, 5]])                  # the label rows follow their boxes
    assert not out[3:].any() and not lab[3:].any()                     # empty slots are zero
    # min_size
    assert B.clip_and_pack(boxes, labels, s, k, min_size=2.0)[2] == 2
    # num_boxes = 0 (also: no boxes at all, and no labels) and num_boxes = K
    out, lab, n, kept = B.clip_and_pack(boxes[[0, 2, 3]], labels[[0, 2, 3]], s, k)
    assert n == 0 and kept.size == 0 and not out.any() and not lab.any()
    out, lab, n, kept = B.clip_and_pack(np.zeros((0, 4)), None, s, k)
    assert n == 0 and lab is None and out.shape == (k, 4)
    full = np.array([[i, i, i + 8.0, i + 9.0] for i in range(4)])
    out, lab, n, kept = B.clip_and_pack(full, np.eye(4, dtype=np.uint8), s, k)
    assert n == k and kept.tolist() == [0, 1, 2, 3] and lab.dtype == np.uint8 and np.array_equal(lab, np.eye(4, dtype=np.uint8))
    # overflow beyond K: the first K survivors stay, the rest are counted
    six = np.array([[i, i, i + 8.0, i + 9.0] for i in range(6)])
    six[1] = np.nan
    stats = {"boxes_dropped": 5}
    out, lab, n, kept = B.clip_and_pack(six, np.arange(6, dtype=np.float32)[:, None], s, k, stats=stats)
    assert n == k and kept.tolist() == [0, 2, 3, 4] and lab[:, 0].tolist() == [0.0, 2.0, 3.0, 4.0]
    assert stats == {"boxes_dropped": 6}
    assert B.clip_and_pack(six, None, s, k)[2] == k                    # (no stats given: nothing to count into)
    with pytest.raises(ValueError, match="labels"):
        B.clip_and_pack(six, np.zeros((5, 2)), s, k)


# ---- 3. parsers and keyframe arithmetic -----------------------------------------------------------------------------------------
def test_parsers(tmp_path):
    cfg = make_cfg(tmp_path)
    ann = cfg.AVA.ANNOTATION_DIR
    videos = ava.read_frame_lists([os.path.join(cfg.AVA.FRAME_LIST_DIR, "train.csv")])
    assert list(videos) == list(VIDEOS) and all(len(v) == F for v in videos.values())
    assert videos["vidB"][3] == os.path.join("vidB", "vidB_000004.jpg")
    gt = ava.read_box_list(os.path.join(ann, "train_gt.csv"), CLASSES)
    # merged duplicates: one box with the union of the labels (0-based, in file order); an empty label: a box without one
    a900 = gt[("vidA", 900)]
    assert len(a900) == 2 and a900[0].labels == (2, 4) and a900[0].box == (0.1, 0.2, 0.6, 0.9) and a900[0].score == 1.0
    assert a900[0].key == ("0.100", "0.200", "0.600", "0.900")
    assert a900[1].labels == () and a900[1].box == (0.5, 0.1, 0.95, 0.8)
    assert gt[("vidA", 902)][0].labels == (1, 6) and len(gt[("vidA", 903)]) == 6
    # the threshold, and predicted rows joining a ground-truth box by their coordinate strings
    both = ava.read_box_list(os.path.join(ann, "train_pred.csv"), CLASSES, 0.9, into=gt)
    assert both is gt
    b900 = gt[("vidB", 900)]
    assert [b.key[0] for b in b900] == ["0.150", "0.550"] and b900[0].labels == (0, 5) and b900[1].labels == (1,)
    assert b900[1].score == 0.95
    low = ava.read_box_list(os.path.join(ann, "train_pred.csv"), CLASSES, 0.4)
    assert len(low[("vidB", 900)]) == 3
    # the same coordinates written differently are two boxes
    p = tmp_path / "strings.csv"
    p.write_text("v,900,0.1,0.2,0.6,0.9,1,1\nv,900,0.10,0.2,0.6,0.9,2,1\n")
    assert len(ava.read_box_list(str(p), CLASSES)[("v", 900)]) == 2
    # a label out of range names file and line
    bad = tmp_path / "bad.csv"
    bad.write_text("v,900,0.1,0.2,0.6,0.9,1,1\nv,900,0.1,0.2,0.6,0.9,%d,1\n" % (CLASSES + 1))
    with pytest.raises(ValueError, match="bad.csv:2"):
        ava.read_box_list(str(bad), CLASSES)
    bad.write_text("v,900,0.1,0.2,0.6,0.9,0,1\n")
    with pytest.raises(ValueError, match="bad.csv:1"):
        ava.read_box_list(str(bad), CLASSES)
    assert ava.read_exclusions(os.path.join(ann, "val_excluded.csv")) == {("vidB", 902), ("vidB", 1000)}
    # the best-scored K, ties to file order, in file order
    val = ava.read_box_list(os.path.join(ann, "val_pred.csv"), CLASSES, 0.9)
    assert len(val[("vidA", 900)]) == 2                                # 0.30 is under the threshold
    best = ava.best_scored(val[("vidA", 901)], 4)
    assert [b.score for b in best] == [0.97, 0.97, 0.93, 0.99]         # 0.91 and 0.92 leave
    assert [b.score for b in ava.best_scored(val[("vidA", 901)], 2)] == [0.97, 0.99]      # of the two 0.97 the first


def test_keyframe_arithmetic_and_the_clamped_window():
    assert ava.keyframe_index(902, 900, 30) == 60 and ava.keyframe_index(900, 900, 30) == 0
    assert ava.keyframe_index(903, 900, 2) == 6
    # T = 4, rate = 2: half = 4 -> c - 4, c - 2, c, c + 2
    assert ava.clip_frame_indices(6, 12, 4, 2) == [2, 4, 6, 8]
    assert ava.clip_frame_indices(0, 12, 4, 2) == [0, 0, 0, 2]         # the head clamps: the first index repeats
    assert ava.clip_frame_indices(2, 12, 4, 2) == [0, 0, 2, 4]
    assert ava.clip_frame_indices(10, 12, 4, 2) == [6, 8, 10, 11]      # (12 clamps to the last frame)
    assert ava.clip_frame_indices(11, 12, 4, 3) == [5, 8, 11, 11]      # the tail clamps: the last index repeats
    assert ava.clip_frame_indices(5, 12, 3, 1) == [4, 5, 6]            # odd T: half = T * rate // 2
    assert ava.clip_frame_indices(0, 1, 4, 2) == [0, 0, 0, 0]


def test_index_of_the_training_and_evaluation_sets(tmp_path):
    cfg = make_cfg(tmp_path)
    tr = ava.AvaReader(cfg, True, seed=0)
    assert [(r.video, r.sec) for r in tr.keyframes] == [("vidA", s) for s in range(900, 906)] + [("vidB", s) for s in range(900, 905)]
    assert tr.stats["boxes_dropped"] == 2 and len(tr.keyframes[3].boxes) == K          # vidA,903 has six boxes
    assert [b.key[0] for b in tr.keyframes[3].boxes] == ["0.020", "0.150", "0.400", "0.600"]       # the first K in file order
    assert len(tr.keyframes[6].boxes) == 2 and all(r.gt == () for r in tr.keyframes)
    ev = ava.AvaReader(cfg, False)
    # the union of the keyframes with a proposal and those with ground truth: vidA,904 has no proposal, vidB,902 no ground truth
    assert [(r.video, r.sec) for r in ev.keyframes] == [("vidA", s) for s in range(900, 905)] + [("vidB", s) for s in range(900, 903)]
    assert ev.keyframes[4].boxes == () and len(ev.keyframes[4].gt) == 1
    assert ev.keyframes[7].gt == () and len(ev.keyframes[7].boxes) == 1
    assert ev.stats["proposals_dropped"] == 2 and [b.score for b in ev.keyframes[1].boxes] == [0.97, 0.97, 0.93, 0.99]
    assert ev.keyframes[0].gt[0].labels == (2, 4)
    # a video the frame lists do not know
    with open(os.path.join(cfg.AVA.ANNOTATION_DIR, "train_gt.csv"), "a") as f:
        f.write("vidC,901,0.1,0.1,0.5,0.5,1,1\n")
    with pytest.raises(ValueError, match="vidC"):
        ava.AvaReader(cfg, True)


# ---- 4. determinism and sharding ------------------------------------------------------------------------------------------------
def _take(reader, batch, steps):
    out = []
    it = reader.host_batches(batch)
    for _ in range(steps):
        out.append(next(it))
    it.close()
    return out


@pytest.mark.parametrize("aug", [True, False], ids=["aug", "plain"])
def test_same_seed_same_order_and_draws(tmp_path, aug):
    cfg = make_cfg(tmp_path, "AUG.ENABLE", aug)
    runs = [_take(ava.AvaReader(cfg, True, seed=5, jpeg_decode=mode), 2, 7) for mode in ("host", "host", "device")]
    other = _take(ava.AvaReader(cfg, True, seed=6), 2, 7)
    order = [[(r.video, r.sec) for r in b[0]] for b in runs[0]]
    assert len({k for b in order[:5] for k in b}) == 10                # five batches of a pass of 11: ten different keyframes
    for run in runs[1:]:                                               # and the device mode draws what the host mode draws
        assert [[(r.video, r.sec) for r in b[0]] for b in run] == order
        assert [b[1] for b in run] == [b[1] for b in runs[0]]
        for a, b in zip(run, runs[0]):
            assert all(np.array_equal(u.numpy(), v.numpy()) for u, v in zip(a[2], b[2]))
    assert [[(r.video, r.sec) for r in b[0]] for b in other] != order and [b[1] for b in other] != [b[1] for b in runs[0]]
    recs, params, (targets, boxes, num) = runs[0][0]
    assert len(params) == 2 and tuple(targets.shape) == (2, K, CLASSES) and tuple(boxes.shape) == (2, K, 4) and tuple(num.shape) == (2,)
    assert all((p.start if aug else p["start"]) == 0 for p in params)
    for b in runs[0]:                                                  # the packed boxes are the maps of the keyframe's own
        for i, (rec, p) in enumerate(zip(b[0], b[1])):
            px = np.array([bx.box for bx in rec.boxes]) * [W, H, W, H]
            mapped = B.boxes_through_aug(px, H, W, p, S) if aug else B.boxes_through_train(px, H, W, p, S)
            want, _, n, kept = B.clip_and_pack(mapped, None, S, K)
            assert int(b[2][2][i]) == n and np.array_equal(b[2][1][i].numpy(), want)
            for slot, j in enumerate(kept):
                assert b[2][0][i, slot].nonzero().flatten().tolist() == sorted(rec.boxes[j].labels)
            assert not b[2][0][i, n:].any()


def test_shards(tmp_path):
    cfg = make_cfg(tmp_path)
    key = lambda recs: [(r.video, r.sec) for _, r in recs]             # noqa: E731
    whole = ava.AvaReader(cfg, True, seed=3, rank=0, world=1)
    ranks = [ava.AvaReader(cfg, True, seed=3, rank=r, world=2) for r in range(2)]
    for _ in range(2):                                                 # two passes: a fresh permutation each, the same on all ranks
        perm = key(whole._records(2))
        assert sorted(perm) == sorted((r.video, r.sec) for r in whole.keyframes) and len(perm) == 11
        mine = [key(r._records(1)) for r in ranks]
        assert mine[0] == perm[0:10:2] and mine[1] == perm[1:10:2]     # disjoint, and together the complete groups of two
    assert ranks[0].local_batch(4) == 2
    with pytest.raises(ValueError, match="divisible"):
        ranks[0].local_batch(3)
    # evaluation: contiguous shares of the complete global batches of 4 (8 keyframes) and of 6 (the last two are dropped)
    ev = [ava.AvaReader(cfg, False, rank=r, world=2) for r in range(2)]
    order = [(r.video, r.sec) for r in ev[0].keyframes]
    assert key(ev[0]._records(2)) == order[0:2] + order[4:6] and key(ev[1]._records(2)) == order[2:4] + order[6:8]
    assert key(ev[0]._records(3)) == order[0:3] and key(ev[1]._records(3)) == order[3:6]
    got = [[(r.video, r.sec) for b in e.host_batches(4) for r in b[0]] for e in ev]
    assert got == [order[0:2] + order[4:6], order[2:4] + order[6:8]]


def test_evaluation_host_batches(tmp_path):
    cfg = make_cfg(tmp_path)
    ev = ava.AvaReader(cfg, False)
    batches = list(ev.host_batches(2))
    assert len(batches) == 4 and all(b[1] == [] for b in batches)
    nh, nw, y0, x0 = B.eval_geometry(H, W, S)
    for recs, _, (none, boxes, num, gtb, gtl, ngt) in batches:
        assert none is None and tuple(boxes.shape) == tuple(gtb.shape) == (2, K, 4) and tuple(gtl.shape) == (2, K, CLASSES)
        assert gtl.dtype.is_floating_point is False and gtl.element_size() == 1
        for i, rec in enumerate(recs):
            for packed, n, src in ((boxes[i], num[i], rec.boxes), (gtb[i], ngt[i], rec.gt)):
                px = np.array([bx.box for bx in src]).reshape(-1, 4) * [W, H, W, H]
                want, _, m, _ = B.clip_and_pack(B.resize_crop(px, H, W, nh, nw, y0, x0), None, S, K)
                assert int(n) == m and np.array_equal(packed.numpy(), want)
    last = batches[2]                                                  # vidA,904: ground truth and no proposal
    assert (last[0][0].video, last[0][0].sec) == ("vidA", 904) and int(last[2][2][0]) == 0 and int(last[2][5][0]) == 1
    assert last[2][4][0, 0].nonzero().flatten().tolist() == [4]


# ---- 5. configuration and refusals ----------------------------------------------------------------------------------------------
def test_ava_section_and_settings():
    d = x.get_default_config()
    assert set(d.AVA) == {"FRAME_DIR", "FRAME_LIST_DIR", "ANNOTATION_DIR", "TRAIN_LISTS", "TEST_LISTS", "TRAIN_GT_BOX_LISTS",
                          "TRAIN_PREDICT_BOX_LISTS", "TEST_PREDICT_BOX_LISTS", "DETECTION_SCORE_THRESH", "GROUNDTRUTH_FILE",
                          "EXCLUSION_FILE", "FPS", "START_SEC", "VALID_SECS"}
    s = ava_settings(x.get_config("M"))
    assert (s.detection_score_thresh, s.fps, s.start_sec, s.valid_secs) == (0.9, 30, 900, (902, 1798))
    assert s.train_lists == ("train.csv",) and s.train_predict_box_lists == ()
    # a tree without the section: the defaults, and the other sections are what they were
    m = x.get_config("M", freeze=False)
    old = m.clone()
    del old["AVA"]
    assert ava_settings(old) == s and set(m) == set(old) | {"AVA"} and all(m[k] == old[k] for k in old)
    for over in (["AVA.FPS", 0], ["AVA.DETECTION_SCORE_THRESH", 1.5], ["AVA.VALID_SECS", [902]], ["AVA.VALID_SECS", [800, 1798]],
                 ["AVA.START_SEC", -1]):
        with pytest.raises(ValueError, match=over[0]):
            x.get_config("M", over)


@pytest.mark.parametrize("over, key", [
    (["DETECTION.ENABLE", False], "DETECTION.ENABLE"),
    (["DATA.MULTI_LABEL", False], "DATA.MULTI_LABEL"),
    (["AUG.AA_TYPE", "rand-m7-n2"], "AUG.AA_TYPE"),
    (["DETECTION.ENABLE", False, "TEST.NUM_SPATIAL_CROPS", 3], "TEST.NUM_SPATIAL_CROPS"),
    (["DETECTION.ENABLE", False, "TEST.NUM_TEMPORAL_VIEWS", 2], "TEST.NUM_SPATIAL_CROPS \\* TEST.NUM_TEMPORAL_VIEWS"),
])
def test_reader_refuses(tmp_path, over, key):
    cfg = make_cfg(tmp_path, *over)
    with pytest.raises(ValueError, match=key):
        ava_reader_check(cfg)
    for training in (True, False):
        with pytest.raises(ValueError, match=key):
            ava.AvaReader(cfg, training)
    with pytest.raises(ValueError, match="jpeg_decode"):
        ava.AvaReader(make_cfg(tmp_path), True, jpeg_decode="gpu")
