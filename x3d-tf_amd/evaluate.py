"""Evaluation driver: the part of the reference's eval.py (:75-89) that runs after the model is built --
`model.load_weights(latest_checkpoint).expect_partial()`, then `model.evaluate(...)` with
SparseCategoricalCrossentropy, SparseCategoricalAccuracy ('acc') and SparseTopKCategoricalAccuracy(k=5)
('top_5_acc') (eval.py:48-66).  Videos come as decoded uint8 tensors; the views are built on the GPU (views.py).

With DATA.MULTI_LABEL the model's outputs are per-class sigmoids and the metrics are the binary cross-entropy and the mean
average precision over the classes (`DeviceMAP`, x3d_multilabel_ap).  With DETECTION.ENABLE the detection score is AVA's
frame-mAP (`DeviceFrameMAP`, x3d_frame_match / x3d_frame_ap), fed by `Trainer.validate`."""
from typing import Dict, Iterable, Tuple

import torch

from .views import make_eval_views, num_views


class Metrics:
    """Running means in the Keras sense: per-video loss / hits averaged over the videos seen so far."""

    def __init__(self, reg_loss: float = 0.0):
        self.reg_loss = float(reg_loss)   # the model's L2 term: Keras adds it to every reported `loss`
        self.n = 0
        self.loss = 0.0
        self.top1 = 0
        self.top5 = 0

    def update(self, probs: torch.Tensor, labels: torch.Tensor):
        """probs [videos, classes] fp32 (already view-averaged by the model); labels [videos]."""
        labels = labels.to(probs.device).long()
        # Keras CE from probabilities (the same expression as x3d_softmax_xent and the oracle):
        # q = clip(p, 1e-7, 1 - 1e-7); loss = -log q_y + log sum_j q_j
        q = probs.double().clamp(1e-7, 1.0 - 1e-7)
        self.loss += float((-q.gather(1, labels[:, None]).squeeze(1).log() + q.sum(1).log()).sum())
        top5 = probs.topk(min(5, probs.shape[1]), dim=1).indices
        self.top1 += int((top5[:, 0] == labels).sum())
        self.top5 += int((top5 == labels[:, None]).any(dim=1).sum())
        self.n += int(labels.numel())

    def all_reduce_(self, group=None, device=None):
        """Sum the numerators and the video count over the replicas (no-op without a multi-rank process group): under
        MirroredStrategy `model.evaluate` reports ONE metric over the whole dataset (reference eval.py:83-89,
        utils.py:160-167); here every rank evaluates its shard of the videos and only these four counters are exchanged
        ("eval -- replicas only ... only metric counters are reduced")."""
        import torch.distributed as dist
        if not (dist.is_available() and dist.is_initialized()) or dist.get_world_size(group) == 1:
            return self
        if device is None:
            device = "cuda" if dist.get_backend(group) == "nccl" else "cpu"
        t = torch.tensor([self.loss, float(self.top1), float(self.top5), float(self.n)], dtype=torch.float64, device=device)
        dist.all_reduce(t, group=group)
        self.loss, self.top1, self.top5, self.n = float(t[0]), int(round(float(t[1]))), int(round(float(t[2]))), int(round(float(t[3])))
        return self

    def result(self) -> Dict[str, float]:
        n = max(self.n, 1)
        return {"loss": self.loss / n + self.reg_loss, "acc": self.top1 / n, "top_5_acc": self.top5 / n, "videos": self.n}


class DeviceMetrics:
    """`Metrics` with the counters on the device: `update` launches one x3d_topk_metrics (no host read, no ATen op), the
    host reads the four fp64 counters once, in `result()`.  For the training loop, where a per-batch `int(...)` would
    synchronise every step.  Top-1 is the first-index argmax and top-5 is tf.math.in_top_k, ties at the 5th place
    counting as hits (include/x3d_hip.h); on tie-free rows both equal `Metrics`.

    per_class: also keeps int64 [classes] counters of the top-1 hits and the rows per class (one x3d_class_hits launch more
    per `update`), and `result()` gains "mean_class_acc": the mean of hits / rows over the classes that occurred (NaN when
    none did).  Off by default: launches and result are then what they were."""

    def __init__(self, reg_loss=0.0, k: int = 5, per_class: bool = False):
        self.reg_loss = reg_loss      # float, or a device tensor (model.regularization_loss()): read in result()
        self.k = int(k)
        self.acc = None               # [loss sum, top-1 hits, top-k hits, rows] fp64, on the device of the first batch
        self.per_class = bool(per_class)
        self.class_hits = self.class_counts = None   # per_class: int64 [classes], with the first batch

    def _counters(self, device):
        if self.acc is None:
            self.acc = torch.zeros(4, dtype=torch.float64, device=device)
        return self.acc

    def update(self, probs: torch.Tensor, labels: torch.Tensor):
        """probs [videos, classes] fp32 on the GPU; labels [videos] int32 / int64 (moved to probs' device if elsewhere)."""
        from . import ops
        if labels.device != probs.device:
            labels = labels.to(probs.device, non_blocking=True)
        ops.topk_metrics(probs, labels, self._counters(probs.device), self.k)
        if self.per_class:
            if self.class_hits is None:
                self.class_hits = torch.zeros(probs.shape[1], dtype=torch.int64, device=probs.device)
                self.class_counts = torch.zeros_like(self.class_hits)
            ops.class_hits(probs, labels, self.class_hits, self.class_counts)

    def all_reduce_(self, group=None, device=None):
        """Sums the four counters over the replicas, as `Metrics.all_reduce_` does (no-op without a multi-rank process
        group; the exchange runs on the CPU for gloo, on the GPU for RCCL)."""
        import torch.distributed as dist
        if not (dist.is_available() and dist.is_initialized()) or dist.get_world_size(group) == 1:
            return self
        if device is None:
            device = "cuda" if dist.get_backend(group) == "nccl" else "cpu"
        acc = self._counters(device)
        t = acc.to(device)
        dist.all_reduce(t, group=group)
        if t is not acc:
            acc.copy_(t)
        if self.per_class:
            if self.class_hits is None:
                raise ValueError("DeviceMetrics.all_reduce_: per_class counters need a batch on every rank")
            for c in (self.class_hits, self.class_counts):
                tc = c.to(device)
                dist.all_reduce(tc, group=group)
                if tc is not c:
                    c.copy_(tc)
        return self

    def result(self) -> Dict[str, float]:
        loss, top1, topk, n = self.acc.tolist() if self.acc is not None else (0.0, 0.0, 0.0, 0.0)
        reg = float(self.reg_loss.item()) if torch.is_tensor(self.reg_loss) else float(self.reg_loss)
        d = max(n, 1.0)
        r = {"loss": loss / d + reg, "acc": top1 / d, "top_5_acc": topk / d, "videos": int(round(n))}
        if self.per_class:
            r["mean_class_acc"] = float("nan")
            if self.class_hits is not None:
                hits, counts = self.class_hits.cpu().double(), self.class_counts.cpu().double()
                have = counts > 0
                if bool(have.any()):
                    r["mean_class_acc"] = float((hits[have] / counts[have]).mean())
        return r


class DeviceMAP:
    """Mean average precision of a multi-label evaluation: `update` appends the batch's probabilities and targets to device
    buffers (a device copy, no host read), `result()` runs x3d_multilabel_ap once over everything seen.

    result(): {"loss", "mAP", "videos", "classes"} -- loss = Keras BinaryCrossentropy of the probabilities, q = clip(p,
    1e-7, 1 - 1e-7), -(y log q + (1 - y) log(1 - q)) averaged over classes and videos in fp64, plus the L2 term; mAP = the
    mean of the per-class AP over the `classes` classes with a positive (classes without one are dropped, as SlowFast's
    get_map does; a NaN score makes its class's AP and so the mAP NaN)."""

    def __init__(self, reg_loss=0.0):
        self.reg_loss = reg_loss      # float, or a device tensor (model.regularization_loss()): read in result()
        self._scores = []
        self._targets = []

    def update(self, probs: torch.Tensor, targets: torch.Tensor):
        """probs [videos, classes] fp32 on the GPU; targets [videos, classes] (float / uint8 / bool, moved to probs' device)."""
        if probs.dim() != 2 or tuple(targets.shape) != tuple(probs.shape):
            raise ValueError(f"DeviceMAP: probs {tuple(probs.shape)} and targets {tuple(targets.shape)} must be one [N, M] shape")
        self._scores.append(probs.detach().to(torch.float32, copy=True))      # the model's output buffer is reused
        self._targets.append(targets.detach().to(probs.device, torch.float32, non_blocking=True, copy=True))

    def _cat(self):
        if len(self._scores) > 1:
            self._scores = [torch.cat(self._scores, 0)]
            self._targets = [torch.cat(self._targets, 0)]
        return (self._scores[0], self._targets[0]) if self._scores else (None, None)

    def all_reduce_(self, group=None, device=None):
        """All-gathers the scores and targets of every rank in rank order (no-op without a multi-rank process group).
        The shards are of equal size: the reader drops the trailing partial global batch (InputReader._shard)."""
        import torch.distributed as dist
        if not (dist.is_available() and dist.is_initialized()) or dist.get_world_size(group) == 1:
            return self
        s, t = self._cat()
        if s is None:
            raise ValueError("DeviceMAP.all_reduce_: no batch on this rank")
        if device is None:
            device = "cuda" if dist.get_backend(group) == "nccl" else "cpu"
        world = dist.get_world_size(group)
        out = []
        for x in (s, t):
            xs = x.to(device)
            parts = [torch.empty_like(xs) for _ in range(world)]
            dist.all_gather(parts, xs, group=group)
            out.append(torch.cat(parts, 0).to(s.device))
        self._scores, self._targets = [out[0]], [out[1]]
        return self

    def result(self) -> Dict[str, float]:
        from . import ops
        s, t = self._cat()
        reg = float(self.reg_loss.item()) if torch.is_tensor(self.reg_loss) else float(self.reg_loss)
        if s is None:
            return {"loss": float("nan"), "mAP": float("nan"), "videos": 0, "classes": 0}
        ap, npos = ops.multilabel_ap(s, t)
        q = s.double().clamp(1e-7, 1.0 - 1e-7)
        y = t.double()
        loss = float((-(y * q.log() + (1.0 - y) * (1.0 - q).log())).mean())
        ap, npos = ap.cpu(), npos.cpu()
        have = npos > 0
        m_ap = float(ap[have].mean()) if bool(have.any()) else float("nan")
        return {"loss": loss + reg, "mAP": m_ap, "videos": int(s.shape[0]), "classes": int(have.sum())}


class DeviceFrameMAP:
    """Frame-mAP of an action-detection evaluation (AVA): `update` matches a batch's proposals against its annotated boxes on
    the device (one x3d_frame_match launch, no host read) and keeps only the per-row scores (fp32), the true-positive flags
    (uint8) and the running ground-truth counts -- the boxes are not kept; `result()` sorts every class's column and runs
    x3d_frame_ap once over everything seen.  The rules (IoU matching, VOC AP, ties) are in include/x3d_hip.h.

    result(): {"frame_mAP", "classes", "detections", "gt_boxes", "ap"} -- frame_mAP = the mean of the per-class AP over the
    `classes` classes with ground truth (a class without is dropped; a NaN score makes its class's AP and so the mean NaN);
    detections = the valid proposal rows, gt_boxes = the valid annotated boxes, ap = the per-class list (NaN where dropped)."""

    def __init__(self, iou_threshold: float = 0.5):
        self.iou_threshold = float(iou_threshold)
        if not 0.0 < self.iou_threshold <= 1.0:
            raise ValueError(f"DeviceFrameMAP: iou_threshold = {iou_threshold} must be in (0, 1]")
        self._scores = []
        self._tp = []
        self.ngt = None               # int32 [classes], on the device of the first batch
        self.counts = None            # int64 [2]: valid proposals, valid annotated boxes
        self._slots = None            # ((K, G), the slot index of every column of the two box sets side by side)

    def _count_valid(self, boxes, num_boxes, gt_boxes, num_gt):
        """counts += (valid proposals, valid annotated boxes) by x3d_frame_match's rule; both box sets in one chain of device
        ops (the chain, not the launch, is what an `update` costs: DESIGN section 26), no host read"""
        k, g = boxes.shape[1], gt_boxes.shape[1]
        if self._slots is None or self._slots[0] != (k, g):
            self._slots = ((k, g), torch.cat([torch.arange(k, device=boxes.device), torch.arange(g, device=boxes.device)]))
        b = torch.cat([boxes, gt_boxes], 1)
        filled = torch.cat([num_boxes[:, None].expand(-1, k), num_gt[:, None].expand(-1, g)], 1)
        ok = (b[..., 2:] > b[..., :2]).all(-1) & torch.isfinite(b).all(-1) & (self._slots[1] < filled)
        self.counts += torch.stack([ok[:, :k].sum(), ok[:, k:].sum()])

    def update(self, probs: torch.Tensor, boxes, num_boxes, gt_boxes, gt_labels, num_gt):
        """probs [B*K, C] fp32 on the GPU (the model's output rows); boxes [B, K, 4], num_boxes [B] (the proposals); gt_boxes
        [B, G, 4], gt_labels [B, G, C] (non-zero = the box carries the class), num_gt [B].  The box arguments are tensors,
        arrays or sequences on any device: they are moved to probs' device and to the kernel's types."""
        from . import ops
        dev = probs.device
        conv = lambda t, dt: torch.as_tensor(t).to(dev, dt, non_blocking=True).contiguous()
        boxes, gt_boxes = conv(boxes, torch.float32), conv(gt_boxes, torch.float32)
        num_boxes, num_gt = conv(num_boxes, torch.int32), conv(num_gt, torch.int32)
        gt_labels = torch.as_tensor(gt_labels)
        gt_labels = conv(gt_labels if gt_labels.dtype == torch.uint8 else gt_labels != 0, torch.uint8)
        if self.ngt is None:
            self.ngt = torch.zeros(probs.shape[-1], dtype=torch.int32, device=dev)
            self.counts = torch.zeros(2, dtype=torch.int64, device=dev)
        rows = probs.detach().reshape(-1, probs.shape[-1]).to(torch.float32).contiguous()      # ([B, K, C] as the model returns it too)
        tp, det, _ = ops.frame_match(rows, boxes, num_boxes, gt_boxes, gt_labels, num_gt, self.iou_threshold, ngt=self.ngt)
        self._scores.append(det)      # the kernel's own output buffers: nothing of the model's is kept
        self._tp.append(tp)
        self._count_valid(boxes, num_boxes, gt_boxes, num_gt)

    def _cat(self):
        if len(self._scores) > 1:
            self._scores = [torch.cat(self._scores, 0)]
            self._tp = [torch.cat(self._tp, 0)]
        return (self._scores[0], self._tp[0]) if self._scores else (None, None)

    def all_reduce_(self, group=None, device=None):
        """All-gathers the scores and flags of every rank in rank order, as `DeviceMAP.all_reduce_` does, and sums the
        ground-truth counts (no-op without a multi-rank process group).  Every rank must hold the same number of rows: the
        gather receives into buffers of this rank's size.  A reader's shards are (InputReader._shard drops the trailing partial
        global batch); a caller that feeds its own batches, a detector's proposals for instance, gives every rank equally many
        images."""
        import torch.distributed as dist
        if not (dist.is_available() and dist.is_initialized()) or dist.get_world_size(group) == 1:
            return self
        s, t = self._cat()
        if s is None:
            raise ValueError("DeviceFrameMAP.all_reduce_: no batch on this rank")
        if device is None:
            device = "cuda" if dist.get_backend(group) == "nccl" else "cpu"
        world = dist.get_world_size(group)
        out = []
        for x in (s, t):
            xs = x.to(device)
            parts = [torch.empty_like(xs) for _ in range(world)]
            dist.all_gather(parts, xs, group=group)
            out.append(torch.cat(parts, 0).to(s.device))
        self._scores, self._tp = [out[0]], [out[1]]
        for c in (self.ngt, self.counts):
            tc = c.to(device)
            dist.all_reduce(tc, group=group)
            if tc is not c:
                c.copy_(tc)
        return self

    def result(self) -> Dict[str, float]:
        from . import ops
        s, t = self._cat()
        if s is None:
            return {"frame_mAP": float("nan"), "classes": 0, "detections": 0, "gt_boxes": 0, "ap": []}
        ap, _ = ops.frame_ap(t, s, self.ngt)
        ap, ngt, counts = ap.cpu(), self.ngt.cpu(), self.counts.cpu()
        have = ngt > 0
        m_ap = float(ap[have].mean()) if bool(have.any()) else float("nan")
        return {"frame_mAP": m_ap, "classes": int(have.sum()), "detections": int(counts[0]), "gt_boxes": int(counts[1]),
                "ap": ap.tolist()}


def _targets_of(label, num_classes: int) -> torch.Tensor:
    """a multi-label video's label: a [classes] target tensor / array, or class ids (an int or a sequence of them)"""
    import numpy as np
    if torch.is_tensor(label) or isinstance(label, np.ndarray):
        t = torch.as_tensor(label).float().cpu()
        if t.dim() == 1 and t.shape[0] == num_classes:
            return t
        if t.dim() != 1:
            raise ValueError(f"multi-label target of shape {tuple(t.shape)}, expected [{num_classes}]")
        label = t.long().tolist()
    from .dataloader import multi_hot
    ids = [int(label)] if isinstance(label, (int, np.integer)) else [int(c) for c in label]
    return multi_hot([ids], num_classes)[0]


def evaluate(model, cfg, videos: Iterable[Tuple[torch.Tensor, int]], batch_videos: int = None) -> Dict[str, float]:
    """videos: iterable of (uint8 [F, H, W, 3] GPU tensor, label).  Batches `batch_videos` videos
    (default cfg.TEST.BATCH_SIZE) of views x crops clips each through `model(clips, training=False)`.  Multi-label models
    (DATA.MULTI_LABEL): label = the video's class ids (an int or a sequence) or its [classes] targets; returns the
    DeviceMAP result."""
    bv = int(batch_videos or cfg.TEST.BATCH_SIZE)
    nv = num_views(cfg)
    # `model.evaluate` reports cross-entropy + the model's regularisation losses (weight_decay * sum w^2, model.py:47)
    reg = float(model.regularization_loss().item()) if hasattr(model, "regularization_loss") else 0.0
    multi = bool(getattr(model, "multi_label", False))
    m = DeviceMAP(reg) if multi else Metrics(reg)
    clips, labels = [], []

    def flush():
        if clips:
            probs = model(torch.cat(clips, 0), training=False)
            if multi:
                m.update(probs.float(), torch.stack(labels).to(probs.device))
            else:
                m.update(probs.float(), torch.tensor(labels))
            clips.clear()
            labels.clear()

    for video, label in videos:
        c = make_eval_views(video, cfg, dtype=model.dtype)
        assert c.shape[0] == nv
        clips.append(c)
        labels.append(_targets_of(label, model.num_classes) if multi else int(label))
        if len(clips) == bv:
            flush()
    flush()
    if hasattr(model, "release_plans"):
        model.release_plans(keep=1)     # the partial tail batch allocated a second multi-GB plan
    return m.result()


def evaluate_dataset(model, cfg, batches: Iterable[Tuple[torch.Tensor, torch.Tensor]], group=None) -> Dict[str, float]:
    """reference eval.py:83-89 `model.evaluate(InputReader(cfg, False, use_tfrecord)(pattern, cfg.TEST.BATCH_SIZE))`:
    `batches` yields (clips [B * views * crops, T, S, S, 3], labels [B]) as `dataloader.InputReader` does in evaluation
    mode (the views were built on the GPU while the batch was assembled).  Under torchrun the reader hands every rank its
    share of each global batch; the counters are summed over the ranks ONCE at the end, so every rank returns the metric of
    the whole dataset (the same videos the single-process run evaluates: the reader drops the same trailing partial batch).
    Multi-label models: `batches` yield (clips, targets [B, classes]) and the result is DeviceMAP's (the scores and targets
    of all ranks are gathered once)."""
    reg = float(model.regularization_loss().item()) if hasattr(model, "regularization_loss") else 0.0
    m = DeviceMAP(reg) if getattr(model, "multi_label", False) else Metrics(reg)
    dev = None
    for clips, labels in batches:
        m.update(model(clips, training=False).float(), labels)
        dev = clips.device
    if hasattr(model, "release_plans"):
        model.release_plans(keep=1)
    m.all_reduce_(group, dev)
    return m.result()
