"""AVA-style action detection input: frame lists, box lists and the reader that turns keyframes into the batches the detection
head trains and validates on (`Trainer.step / fit`: (clips, targets, boxes, num_boxes); `Trainer.validate`: the seven items of its
frame-mAP).  The file layouts are the public AVA ones as PySlowFast's AVA dataset reads them [PSF-3p]; the config keys are its AVA
section's (config.ava_settings).

frame lists   space-separated, header `original_vido_id video_id frame_id path labels`: per video the ordered frame paths,
              relative to AVA.FRAME_DIR.
box lists     CSV rows `video,sec,x1,y1,x2,y2,label,score_or_person_id`: coordinates normalised to [0, 1], `label` 1-based and
              possibly empty (a box without a label).  A ground-truth file has a person id in the last column and counts as score
              1; a predicted file has a score, and rows below AVA.DETECTION_SCORE_THRESH are skipped.  Rows of one (video, sec)
              with the same four coordinate STRINGS are one box with the union of their labels.
exclusions    CSV rows `video,sec`: timestamps the evaluation leaves out of the ground truth.

Keyframes.  Second `sec` of a video is frame (sec - START_SEC) * FPS of its list; only seconds inside VALID_SECS count.  The clip
of a keyframe at frame c is frames c - half + j * rate, j < T = DATA.TEMP_DURATION, half = T * rate // 2, rate = DATA.FRAME_RATE,
each clamped to [0, F - 1]: the video ends clamp, they do not wrap as the classification sampler does.  Only those T files are
read; they are decoded into a compact [T, H, W, 3] video which the clip kernels read with start = 0, rate = 1, as
`InputReader._device_batch` hands over its frames.  The pixels go through the existing device calls (jpeg.decode_jpeg_batch,
views.make_train_batch_aug / make_train_clip / make_eval_views), the boxes through boxes.py on the host."""
import collections
import os
from typing import Dict, Iterator, List, Optional, Sequence, Tuple

import numpy as np
import torch

from .boxes import boxes_through_aug, boxes_through_eval, boxes_through_train, clip_and_pack
from .dataloader import InputReader, decode_jpeg

FRAME_LIST_HEADER = "original_vido_id video_id frame_id path labels"

# one box of a keyframe: `key` the four coordinate strings, `box` (x1, y1, x2, y2) normalised, `labels` 0-based class ids in the
# order they were first seen, `score` (1.0 for ground truth; the highest of its rows)
AvaBox = collections.namedtuple("AvaBox", "key box labels score")
# one keyframe: `boxes` what the ROI head pools (training: ground truth + thresholded predictions; evaluation: the proposals),
# `gt` the annotated boxes of the evaluation (empty in training)
Keyframe = collections.namedtuple("Keyframe", "video sec boxes gt")


# ---- parsers ----------------------------------------------------------------------------------------------------------------
def read_frame_lists(paths: Sequence[str]) -> Dict[str, List[str]]:
    """{video name: its frame paths in list order} from frame-list files (the header line is optional)"""
    videos: Dict[str, List[str]] = {}
    for path in paths:
        with open(path) as f:
            for no, line in enumerate(f, 1):
                row = line.split()
                if not row or " ".join(row) == FRAME_LIST_HEADER:
                    continue
                if len(row) < 4:
                    raise ValueError(f"{path}:{no}: a frame-list row is `{FRAME_LIST_HEADER}`, got {line.strip()!r}")
                videos.setdefault(row[0], []).append(row[3])
    return videos


def read_box_list(path: str, num_classes: int, score_thresh: Optional[float] = None,
                  into: Optional[Dict[Tuple[str, int], List[AvaBox]]] = None) -> Dict[Tuple[str, int], List[AvaBox]]:
    """{(video, sec): [AvaBox, ...] in file order} from one box list.  score_thresh None: a ground-truth file (last column a
    person id, score 1); else a predicted file whose rows below the threshold are skipped.  `into`: a dict of earlier files to
    extend (a box already there gains the labels).  A label outside [1, num_classes] raises ValueError naming file and line."""
    out = {} if into is None else into
    with open(path) as f:
        for no, line in enumerate(f, 1):
            row = [c.strip() for c in line.strip().split(",")]
            if row == [""]:
                continue
            if len(row) < 7:
                raise ValueError(f"{path}:{no}: a box row is `video,sec,x1,y1,x2,y2,label,score_or_person_id`, got {line.strip()!r}")
            score = 1.0
            if score_thresh is not None:
                score = float(row[7]) if len(row) > 7 and row[7] != "" else 1.0
                if score < score_thresh:
                    continue
            label = None
            if row[6] != "":
                label = int(row[6])
                if not 1 <= label <= num_classes:
                    raise ValueError(f"{path}:{no}: label {label} outside [1, {num_classes}] (NETWORK.NUM_CLASSES)")
            key = tuple(row[2:6])
            boxes = out.setdefault((row[0], int(row[1])), [])
            at = next((i for i, b in enumerate(boxes) if b.key == key), None)
            if at is None:
                boxes.append(AvaBox(key, tuple(float(c) for c in key), () if label is None else (label - 1,), score))
            else:
                b = boxes[at]
                labels = b.labels if label is None or label - 1 in b.labels else b.labels + (label - 1,)
                boxes[at] = b._replace(labels=labels, score=max(b.score, score))
    return out


def read_exclusions(path: str) -> set:
    """{(video, sec)} of an excluded-timestamps file"""
    out = set()
    with open(path) as f:
        for no, line in enumerate(f, 1):
            row = [c.strip() for c in line.strip().split(",")]
            if row == [""]:
                continue
            if len(row) < 2:
                raise ValueError(f"{path}:{no}: an exclusion row is `video,sec`, got {line.strip()!r}")
            out.add((row[0], int(row[1])))
    return out


def keyframe_index(sec: int, start_sec: int, fps: int) -> int:
    """the frame of second `sec` in a video's list"""
    return (int(sec) - int(start_sec)) * int(fps)


def clip_frame_indices(center: int, num_frames: int, t: int, rate: int) -> List[int]:
    """the T frames of the clip around frame `center` of a video of `num_frames`: clamped at both ends"""
    half = t * rate // 2
    return [min(max(center - half + j * rate, 0), num_frames - 1) for j in range(t)]


def best_scored(boxes: Sequence[AvaBox], k: int) -> List[AvaBox]:
    """the k best-scored boxes, ties to file order, returned in file order"""
    order = sorted(range(len(boxes)), key=lambda i: (-boxes[i].score, i))[:k]
    return [boxes[i] for i in sorted(order)]


# ---- the reader -------------------------------------------------------------------------------------------------------------
class AvaReader(InputReader):
    """`reader(batch_size)` iterates over detection batches of the AVA files cfg.AVA points at; a background thread keeps
    `prefetch` of them ready (InputReader's, with its own stream and event hand-over under jpeg_decode="device").

    Training: (clips [B, T, S, S, 3] on the device, targets [B, K, classes] fp32 multi-hot on the device, boxes [B, K, 4] fp32 and
    num_boxes [B] int64 on the host), K = DETECTION.MAX_BOXES, S = DATA.TRAIN_CROP_SIZE, endlessly.  The boxes of a keyframe are
    TRAIN_GT_BOX_LISTS plus the thresholded TRAIN_PREDICT_BOX_LISTS; more than K keeps the first K in file order and counts the
    rest in `stats["boxes_dropped"]`.  With AUG.ENABLE every clip's `aug.AugParams` are drawn with `aug.draw_aug_params`, the
    batch is one `views.make_train_batch_aug` call (and, with jpeg_decode="device", one `jpeg.decode_jpeg_batch` call) and the boxes
    go through `boxes_through_aug`; with AUG.ENABLE off `views.draw_train_params` / `make_train_clip` per clip, as InputReader
    does, and `boxes_through_train`.  Either way `clip_and_pack` drops what the crop removed (num_boxes may be 0).  The temporal
    position is the keyframe's: the draws' `start` is replaced by 0.  `last_params` holds the draws of the last batch.

    Evaluation: (clips [B, T, S, S, 3], None, boxes, num_boxes, gt_boxes [B, K, 4], gt_labels [B, K, classes] uint8, num_gt [B]),
    S = DATA.TEST_CROP_SIZE, one pass: what `Trainer.validate` takes for its frame-mAP.  The proposals are the K best-scored of the
    thresholded TEST_PREDICT_BOX_LISTS (`stats["proposals_dropped"]` counts the others), the ground truth GROUNDTRUTH_FILE minus
    EXCLUSION_FILE (beyond K: `stats["gt_boxes_dropped"]`), both through `boxes_through_eval` + `clip_and_pack`, the clips from
    `make_eval_views`.  The keyframes are the union of those with a proposal and those with a ground-truth box.

    Order and shards.  The keyframes are ordered by video (frame-list order) and second.  Training: every pass is a fresh
    permutation from the rank-independent generator, of which rank r takes records r, r + world, ...; evaluation: contiguous
    shares of the complete global batches (InputReader._shard).  `batch_size` is the GLOBAL batch (`local_batch`).

    Refused at construction (config.ava_reader_check): DETECTION.ENABLE or DATA.MULTI_LABEL off, AUG.AA_TYPE set, more than one
    test view."""

    def __init__(self, cfg, is_training: bool, device=None, dtype: torch.dtype = torch.float32, mixed_precision: bool = False,
                 seed: Optional[int] = None, num_workers: int = 4, prefetch: int = 2, rank: Optional[int] = None,
                 world: Optional[int] = None, jpeg_decode: str = "host"):
        from .config import ava_reader_check, detection_settings
        self._ava = ava_reader_check(cfg)
        super().__init__(cfg, is_training, True, mixed_precision=mixed_precision, device=device, dtype=dtype, seed=seed,
                         num_workers=num_workers, prefetch=prefetch, rank=rank, world=world, jpeg_decode=jpeg_decode)
        self._k = detection_settings(cfg).max_boxes
        self._t, self._rate = int(cfg.DATA.TEMP_DURATION), int(cfg.DATA.FRAME_RATE)
        self._size = int(cfg.DATA.TRAIN_CROP_SIZE if self._is_training else cfg.DATA.TEST_CROP_SIZE)
        self.stats = dict(boxes_dropped=0, proposals_dropped=0, gt_boxes_dropped=0)
        s = self._ava
        lists = s.train_lists if self._is_training else s.test_lists
        self._videos = read_frame_lists([os.path.join(s.frame_list_dir, p) for p in lists])
        self.keyframes: List[Keyframe] = self._index()

    def _index(self) -> List[Keyframe]:
        s, k, classes = self._ava, self._k, self._num_classes
        ann = lambda p: os.path.join(s.annotation_dir, p)      # noqa: E731
        boxes: Dict[Tuple[str, int], List[AvaBox]] = {}
        gt: Dict[Tuple[str, int], List[AvaBox]] = {}
        if self._is_training:
            for p in s.train_gt_box_lists:
                read_box_list(ann(p), classes, None, into=boxes)
            for p in s.train_predict_box_lists:
                read_box_list(ann(p), classes, s.detection_score_thresh, into=boxes)
        else:
            for p in s.test_predict_box_lists:
                read_box_list(ann(p), classes, s.detection_score_thresh, into=boxes)
            if s.groundtruth_file:
                read_box_list(ann(s.groundtruth_file), classes, None, into=gt)
            if s.exclusion_file:
                for key in read_exclusions(ann(s.exclusion_file)):
                    gt.pop(key, None)
        order = {v: i for i, v in enumerate(self._videos)}
        out = []
        for video, sec in sorted(set(boxes) | set(gt), key=lambda vs: (order.get(vs[0], len(order)), vs[0], vs[1])):
            if not s.valid_secs[0] <= sec <= s.valid_secs[1]:
                continue
            if video not in self._videos:
                raise ValueError(f"video {video!r} has boxes at second {sec} but no frames in the frame lists")
            c = keyframe_index(sec, s.start_sec, s.fps)
            if not 0 <= c < len(self._videos[video]):
                raise ValueError(f"video {video!r}: second {sec} is frame {c}, outside its {len(self._videos[video])} frames")
            mine, truth = boxes.get((video, sec), []), gt.get((video, sec), [])
            if self._is_training:
                self.stats["boxes_dropped"] += max(len(mine) - k, 0)
                mine = mine[:k]
            else:
                self.stats["proposals_dropped"] += max(len(mine) - k, 0)
                mine = best_scored(mine, k)
                self.stats["gt_boxes_dropped"] += max(len(truth) - k, 0)
                truth = truth[:k]
            out.append(Keyframe(video, sec, tuple(mine), tuple(truth)))
        return out

    # -- records and their frames (InputReader._decoded runs these on its thread pool) ----------------------------------------
    def _records(self, batch_size: Optional[int] = None) -> Iterator[Tuple[str, Keyframe]]:
        """one pass over this rank's keyframes as (name, keyframe) pairs, the form InputReader._decoded takes in multi-label
        mode"""
        recs = self.keyframes
        if self._is_training:
            recs = [recs[i] for i in self._rng_files.permutation(len(recs))]
        return self._shard(((f"{r.video}@{r.sec}", r) for r in recs), batch_size)

    def _clip_jpegs(self, rec: Keyframe) -> List[bytes]:
        frames = self._videos[rec.video]
        idx = clip_frame_indices(keyframe_index(rec.sec, self._ava.start_sec, self._ava.fps), len(frames), self._t, self._rate)
        data = {}
        for i in set(idx):
            with open(os.path.join(self._ava.frame_dir, frames[i]), "rb") as f:
                data[i] = f.read()
        return [data[i] for i in idx]

    def parse_and_decode(self, rec: Keyframe, all_labels: bool = False):
        """jpeg_decode="host": keyframe -> (its clip's frames uint8 [T, H, W, 3], keyframe)"""
        return np.stack([decode_jpeg(j) for j in self._clip_jpegs(rec)]), rec

    def parse_frames(self, rec: Keyframe, all_labels: bool = False):
        """jpeg_decode="device": keyframe -> ((the T JPEG strings, H, W), keyframe), no pixel decoded (a frame whose header does
        not parse goes to `decode_jpeg`, which raises)"""
        from .jpeg import parse_headers
        jpegs = self._clip_jpegs(rec)
        imgs, _ = parse_headers(jpegs)
        shapes = {decode_jpeg(j).shape[:2] if im.status == 2 else (int(im.height), int(im.width))     # 2: X3D_JPEG_MALFORMED
                  for j, im in zip(jpegs, imgs)}
        if len(shapes) > 1:
            raise ValueError(f"{rec.video}@{rec.sec}: all input arrays must have the same shape")
        h, w = shapes.pop()
        return (jpegs, int(h), int(w)), rec

    # -- the host half of a batch: draws and boxes ----------------------------------------------------------------------------
    def _pixel_boxes(self, boxes: Sequence[AvaBox], h: int, w: int) -> np.ndarray:
        b = np.array([bx.box for bx in boxes], np.float64).reshape(-1, 4)
        return b * np.array([w, h, w, h], np.float64)

    def _multi_hot(self, boxes: Sequence[AvaBox], dtype) -> np.ndarray:
        y = np.zeros((len(boxes), self._num_classes), dtype)
        for i, bx in enumerate(boxes):
            y[i, list(bx.labels)] = 1
        return y

    def _draw(self, h: int, w: int):
        """the draws of one training clip of a [T, H, W] compact video; its `start` is the keyframe's, 0"""
        if self._aug:
            from .aug import draw_aug_params
            return draw_aug_params(self._cfg, self._t, h, w, self._rng_aug)._replace(start=0)
        from .views import draw_train_params
        return dict(draw_train_params(self._t, h, w, self._cfg, self._gen), start=0)

    def _host_batch(self, recs: List[Keyframe], sizes: List[Tuple[int, int]]):
        """(params, the host items of the batch behind the clips): training (targets, boxes, num_boxes), evaluation (None, boxes,
        num_boxes, gt_boxes, gt_labels, num_gt)"""
        k, s = self._k, self._size
        params, packs, gts = [], [], []
        for rec, (h, w) in zip(recs, sizes):
            px = self._pixel_boxes(rec.boxes, h, w)
            if self._is_training:
                p = self._draw(h, w)
                params.append(p)
                mapped = boxes_through_aug(px, h, w, p, s) if self._aug else boxes_through_train(px, h, w, p, s)
                packs.append(clip_and_pack(mapped, self._multi_hot(rec.boxes, np.float32), s, k)[:3])
            else:
                packs.append(clip_and_pack(boxes_through_eval(px, h, w, s), None, s, k)[:3])
                gts.append(clip_and_pack(boxes_through_eval(self._pixel_boxes(rec.gt, h, w), h, w, s),
                                         self._multi_hot(rec.gt, np.uint8), s, k)[:3])
        boxes = torch.from_numpy(np.stack([p[0] for p in packs]))
        num = torch.tensor([p[2] for p in packs], dtype=torch.int64)
        if self._is_training:
            return params, (torch.from_numpy(np.stack([p[1] for p in packs])), boxes, num)
        return params, (None, boxes, num, torch.from_numpy(np.stack([g[0] for g in gts])),
                        torch.from_numpy(np.stack([g[1] for g in gts])), torch.tensor([g[2] for g in gts], dtype=torch.int64))

    def host_batches(self, batch_size: Optional[int] = None) -> Iterator[tuple]:
        """The batches without their clips, nothing touching the device: (keyframes, params, host items as `_host_batch` returns
        them), in the order and with the draws `reader(batch_size)` makes.  `batch_size` is the global batch."""
        for items, recs in self._loaded(self.local_batch(batch_size)):
            sizes = [(it[1], it[2]) if self._jpeg_decode == "device" else it.shape[1:3] for it in items]
            yield (recs,) + self._host_batch(recs, sizes)

    def _loaded(self, batch_size: Optional[int]) -> Iterator[Tuple[list, List[Keyframe]]]:
        """(the loaded frames, the keyframes) of every complete batch of this rank"""
        items, recs = [], []
        for item, (_, rec) in self._decoded(lambda: self._records(batch_size)):
            items.append(item)
            recs.append(rec)
            if len(items) == (batch_size or 1):
                yield items, recs
                items, recs = [], []
        # drop_remainder, as InputReader: a trailing partial batch is not emitted

    # -- the device half ------------------------------------------------------------------------------------------------------
    def _batches(self, batch_size: Optional[int]) -> Iterator[tuple]:
        from .jpeg import decode_jpeg_batch
        from .views import make_eval_views, make_train_clip
        for items, recs in self._loaded(batch_size):
            if self._jpeg_decode == "device":
                videos = [torch.empty((self._t, h, w, 3), dtype=torch.uint8, device=self._device) for _, h, w in items]
                decode_jpeg_batch([j for jpegs, _, _ in items for j in jpegs], self._device,
                                  out=[v[t] for v in videos for t in range(self._t)], on_corrupt="host")
            else:
                videos = [torch.from_numpy(v).to(self._device, non_blocking=True) for v in items]
            params, host = self._host_batch(recs, [tuple(v.shape[1:3]) for v in videos])
            if self._aug:
                clips = self._aug_batch(videos, params, rate=1)
            elif self._is_training:
                clips = torch.cat([make_train_clip(v, self._cfg, params=p, dtype=self._dtype, rate=1)[None]
                                   for v, p in zip(videos, params)], 0)
            else:
                clips = torch.cat([make_eval_views(v, self._cfg, dtype=self._dtype) for v in videos], 0)
            if self._is_training:
                host = (host[0].to(self._device, non_blocking=True),) + host[1:]
            yield (clips,) + host + (params, [])

    def __call__(self, batch_size: Optional[int] = None) -> Iterator[tuple]:
        """Iterate to get batches (class docstring).  `batch_size` is the GLOBAL batch; with world > 1 this rank yields its
        batch_size // world share."""
        batch_size = self.local_batch(batch_size)
        yield from self._prefetched(lambda: self._batches(batch_size), 4 if self._is_training else 7)
