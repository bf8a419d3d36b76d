"""NumPy fp64 restatement of the frame-mAP protocol (include/x3d_hip.h, "Frame-mAP for action detection"): IoU matching of an
image's proposals against its annotated boxes per class, and the PASCAL VOC average precision over an evaluation set.  Plain
loops, written from the rules and not from the kernels; tests/test_frame_map.py checks it against hand-worked cases, and
tests/test_frame_map_gpu.py holds x3d_frame_match / x3d_frame_ap to it."""
import numpy as np


def box_valid(b):
    """finite coordinates, x2 > x1 and y2 > y1 (b: four fp32 values)"""
    return bool(np.all(np.isfinite(b)) and b[2] > b[0] and b[3] > b[1])


def iou(a, b):
    """IEEE double from the fp32 coordinates, one rounding per operation (Python floats are doubles)"""
    ax1, ay1, ax2, ay2 = (float(v) for v in a)
    bx1, by1, bx2, by2 = (float(v) for v in b)
    iw = max(0.0, min(ax2, bx2) - max(ax1, bx1))
    ih = max(0.0, min(ay2, by2) - max(ay1, by1))
    inter = iw * ih
    ua = (ax2 - ax1) * (ay2 - ay1)
    ub = (bx2 - bx1) * (by2 - by1)
    return inter / (ua + ub - inter)


def frame_match(scores, boxes, num_boxes, gt_boxes, gt_labels, num_gt, iou_threshold=0.5, ngt=None):
    """scores [I*K, C] fp32, boxes [I, K, 4] fp32, num_boxes [I], gt_boxes [I, G, 4] fp32, gt_labels [I, G, C] uint8, num_gt [I]
    -> (tp [I*K, C] uint8, det_scores [I*K, C] fp32, ngt [C] int32; a given ngt is copied and incremented)"""
    scores = np.asarray(scores, np.float32)
    boxes, gt_boxes = np.asarray(boxes, np.float32), np.asarray(gt_boxes, np.float32)
    gt_labels = np.asarray(gt_labels)
    n_img, k_slots = boxes.shape[:2]
    g_slots, classes = gt_boxes.shape[1], scores.shape[1]
    thr = float(iou_threshold)
    tp = np.zeros((n_img * k_slots, classes), np.uint8)
    det = np.full((n_img * k_slots, classes), -np.inf, np.float32)
    ngt = np.zeros(classes, np.int32) if ngt is None else np.array(ngt, np.int32)
    for i in range(n_img):
        dets = [k for k in range(k_slots) if k < int(num_boxes[i]) and box_valid(boxes[i, k])]
        gts = [g for g in range(g_slots) if g < int(num_gt[i]) and box_valid(gt_boxes[i, g])]
        table = {(k, g): iou(boxes[i, k], gt_boxes[i, g]) for k in dets for g in gts}
        for c in range(classes):
            mine = [g for g in gts if gt_labels[i, g, c] != 0]
            ngt[c] += len(mine)
            s = {k: scores[i * k_slots + k, c] for k in dets}        # an empty or invalid slot is never read
            for k in dets:
                det[i * k_slots + k, c] = s[k]
            best = {}                                                # k -> g* for the candidates
            for k in dets:
                if not mine or np.isnan(s[k]):
                    continue
                gstar = mine[0]
                for g in mine[1:]:
                    if table[k, g] > table[k, gstar]:                # the lowest g among equals
                        gstar = g
                if table[k, gstar] >= thr:
                    best[k] = gstar
            # score descending, the lower slot first among equal scores
            ranked = sorted(best, key=lambda k: (-float(s[k]), k))
            claimed = set()
            for k in ranked:
                if best[k] not in claimed:                           # only the arg-max box is tried
                    claimed.add(best[k])
                    tp[i * k_slots + k, c] = 1
    return tp, det, ngt


def frame_ap(tp, det_scores, ngt):
    """tp [N, C] uint8, det_scores [N, C] fp32, ngt [C] -> (ap [C] float64, ntp [C] int32)"""
    tp, det_scores = np.asarray(tp), np.asarray(det_scores, np.float32)
    n, classes = det_scores.shape
    ap = np.full(classes, np.nan, np.float64)
    ntp = np.zeros(classes, np.int32)
    for c in range(classes):
        s = det_scores[:, c].astype(np.float64)
        order = np.argsort(-s, kind="stable")        # descending, equal scores by row index ascending
        flags = tp[order, c] != 0
        pos = np.nonzero(flags)[0] + 1               # 1-based positions of the true positives
        ntp[c] = len(pos)
        if int(ngt[c]) <= 0 or np.isnan(s).any():
            continue
        prec = np.arange(1, len(pos) + 1, dtype=np.float64) / pos.astype(np.float64)     # prec_t = t / pos_t
        env = np.maximum.accumulate(prec[::-1])[::-1]                                   # env_t = max over t' >= t
        total = 0.0
        for e in env.tolist():                       # sequential sum, t = 1..P
            total += e
        ap[c] = total / float(int(ngt[c]))
    return ap, ntp


def frame_map(ap, ngt):
    """the mean of ap over the classes with ground truth (NaN when there is none)"""
    have = np.asarray(ngt) > 0
    return float(np.mean(np.asarray(ap)[have])) if have.any() else float("nan")


def num_valid(boxes, num):
    boxes = np.asarray(boxes, np.float32)
    return sum(1 for i in range(boxes.shape[0]) for k in range(boxes.shape[1]) if k < int(num[i]) and box_valid(boxes[i, k]))
