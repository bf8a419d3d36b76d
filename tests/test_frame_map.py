"""Frame-mAP for action detection on the host: the fp64 reference (tests/frame_map_ref.py) against hand-worked cases, the two
declarations and their derived binding, the argument refusals of ops.frame_match / ops.frame_ap, and the empty DeviceFrameMAP."""
import ctypes
import math
import os
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from tests import frame_map_ref as R  # noqa: E402
from x3d_tf_amd import hip, ops  # noqa: E402
from x3d_tf_amd.evaluate import DeviceFrameMAP  # noqa: E402

UNIT = (0, 0, 1, 1)


def _image(dets, gts, classes=1):
    """one image: dets = [(box, [score per class])], gts = [(box, [classes carried])] -> the arguments of R.frame_match"""
    k, g = max(len(dets), 1), max(len(gts), 1)
    boxes, gt_boxes = np.zeros((1, k, 4), np.float32), np.zeros((1, g, 4), np.float32)
    scores, labels = np.zeros((k, classes), np.float32), np.zeros((1, g, classes), np.uint8)
    for j, (b, s) in enumerate(dets):
        boxes[0, j], scores[j] = b, s
    for j, (b, cs) in enumerate(gts):
        gt_boxes[0, j] = b
        labels[0, j, list(cs)] = 1
    return scores, boxes, [len(dets)], gt_boxes, labels, [len(gts)]


# ---- the AP formula -----------------------------------------------------------------------------------------------------
def _ap1(flags, scores, ngt):
    ap, ntp = R.frame_ap(np.array(flags, np.uint8)[:, None], np.array(scores, np.float32)[:, None], [ngt])
    return float(ap[0]), int(ntp[0])


def test_ap_tp_fp_tp():
    """prec 1, 1/2, 2/3 -> env 1, 2/3 over 2 ground-truth boxes: to the last bit of (1 + 2/3) / 2"""
    ap, ntp = _ap1([1, 0, 1], [0.9, 0.8, 0.7], 2)
    assert ap == (1.0 + 2.0 / 3.0) / 2.0 and ntp == 2
    assert abs(ap - 5.0 / 6.0) < 1e-15
    # the rows in any order in memory: the sort is by score
    assert _ap1([1, 1, 0], [0.7, 0.9, 0.8], 2)[0] == ap


def test_ap_all_none_and_no_ground_truth():
    assert _ap1([1, 1, 1], [0.3, 0.2, 0.1], 3) == (1.0, 3)
    assert _ap1([0, 0, 0], [0.3, 0.2, 0.1], 2) == (0.0, 0)
    ap, ntp = _ap1([0, 0], [0.3, 0.2], 0)
    assert math.isnan(ap) and ntp == 0
    # the class without ground truth is dropped from the mean
    aps, _ = R.frame_ap(np.array([[1, 0], [0, 0]], np.uint8), np.array([[0.5, 0.5], [0.4, 0.4]], np.float32), [1, 0])
    assert aps[0] == 1.0 and math.isnan(aps[1]) and R.frame_map(aps, [1, 0]) == 1.0
    assert math.isnan(R.frame_map(aps, [0, 0]))


def test_ap_envelope_ties_inf_rows_and_nan():
    # FP first: prec_1 = 1/2, prec_2 = 2/3 -> env 2/3, 2/3
    assert _ap1([0, 1, 1], [0.9, 0.8, 0.7], 2)[0] == (2.0 / 3.0 + 2.0 / 3.0) / 2.0
    # equal scores: the row index decides (a stable sort)
    assert _ap1([1, 0], [0.5, 0.5], 1)[0] == 1.0 and _ap1([0, 1], [0.5, 0.5], 1)[0] == 0.5
    # rows at -inf sort behind every detection and change nothing
    assert _ap1([0, 1, 0, 0, 1], [-np.inf, 0.9, -np.inf, 0.8, 0.7], 2)[0] == (1.0 + 2.0 / 3.0) / 2.0
    ap, ntp = _ap1([1, 0], [0.5, np.nan], 1)
    assert math.isnan(ap) and ntp == 1


# ---- the matching -------------------------------------------------------------------------------------------------------
def test_match_hit_miss_and_outputs():
    tp, det, ngt = R.frame_match(*_image([(UNIT, [0.9]), ((5, 5, 6, 6), [0.8])], [(UNIT, [0])]))
    assert tp[:, 0].tolist() == [1, 0] and det[:, 0].tolist() == [np.float32(0.9), np.float32(0.8)] and ngt.tolist() == [1]
    assert tp.dtype == np.uint8 and det.dtype == np.float32 and ngt.dtype == np.int32


def test_match_two_identical_boxes_argmax_only():
    """two identical ground-truth boxes of one class, two detections on them: both have g* = box 0 (the lowest among equals),
    so the second is a false positive although box 1 is free"""
    tp, _, ngt = R.frame_match(*_image([(UNIT, [0.9]), (UNIT, [0.8])], [(UNIT, [0]), (UNIT, [0])]))
    assert tp[:, 0].tolist() == [1, 0] and ngt.tolist() == [2]


def test_match_three_on_one_box_and_the_tie_rule():
    tp, _, _ = R.frame_match(*_image([(UNIT, [0.5]), (UNIT, [0.9]), (UNIT, [0.7])], [(UNIT, [0])]))
    assert tp[:, 0].tolist() == [0, 1, 0]
    tp, _, _ = R.frame_match(*_image([(UNIT, [0.5]), (UNIT, [0.5]), (UNIT, [0.5])], [(UNIT, [0])]))
    assert tp[:, 0].tolist() == [1, 0, 0]                     # equal scores: the lowest slot
    tp, _, _ = R.frame_match(*_image([(UNIT, [-0.0]), (UNIT, [0.0])], [(UNIT, [0])]))
    assert tp[:, 0].tolist() == [1, 0]                        # -0 equals +0


def test_match_one_box_two_classes():
    """one box carrying classes 0 and 2, matched for each class on its own; class 1 has no ground truth"""
    tp, _, ngt = R.frame_match(*_image([(UNIT, [0.9, 0.9, 0.1]), (UNIT, [0.1, 0.8, 0.9])], [(UNIT, [0, 2])], classes=3))
    assert tp.tolist() == [[1, 0, 0], [0, 0, 1]] and ngt.tolist() == [1, 0, 1]


def test_match_iou_exactly_half():
    wide = (0, 0, 2, 1)
    assert R.iou(np.float32(wide), np.float32(UNIT)) == 0.5
    tp, _, _ = R.frame_match(*_image([(wide, [0.9])], [(UNIT, [0])]))
    assert tp[0, 0] == 1
    above = (0, 0, np.nextafter(np.float32(2), np.float32(3)), 1)
    assert R.iou(np.float32(above), np.float32(UNIT)) < 0.5
    tp, _, _ = R.frame_match(*_image([(above, [0.9])], [(UNIT, [0])]))
    assert tp[0, 0] == 0
    tp, _, _ = R.frame_match(*_image([(wide, [0.9])], [(UNIT, [0])]), iou_threshold=0.75)
    assert tp[0, 0] == 0


def test_match_validity_nan_scores_and_increment():
    sc, bx, nb, gb, gl, ng = _image([(UNIT, [0.2]), (UNIT, [9.0]), ((0, 0, 0, 1), [8.0]), ((0, np.nan, 1, 1), [7.0])],
                                    [(UNIT, [0]), (UNIT, [0])])
    # slot 1 is empty (num_boxes = 1 would cut it; here it is cut by a count of 1), slots 2 and 3 are invalid boxes
    tp, det, ngt = R.frame_match(sc, bx, [1], gb, gl, [1], ngt=[5])
    assert tp[:, 0].tolist() == [1, 0, 0, 0] and det[1:, 0].tolist() == [-np.inf] * 3 and ngt.tolist() == [6]
    tp, det, _ = R.frame_match(sc, bx, [4], gb, gl, [2])
    assert tp[:, 0].tolist() == [0, 1, 0, 0] and det[:, 0].tolist() == [np.float32(0.2), 9.0, -np.inf, -np.inf]
    # a NaN score in a valid slot is never a candidate, claims nothing and is passed on
    sc[1, 0] = np.nan
    tp, det, _ = R.frame_match(sc, bx, [2], gb, gl, [2])
    assert tp[:, 0].tolist() == [1, 0, 0, 0] and math.isnan(det[1, 0])
    # no ground truth in the image: every detection is a false positive
    tp, _, ngt = R.frame_match(sc, bx, [2], gb, gl, [0])
    assert not tp.any() and ngt.tolist() == [0]


# ---- the header and the binding -----------------------------------------------------------------------------------------
def test_declarations_and_binding():
    text = " ".join(open(os.path.join(ROOT, "include", "x3d_hip.h")).read().split())
    match = ("int x3d_frame_match(const float* scores, const float* boxes, const int* num_boxes, const float* gt_boxes, "
             "const unsigned char* gt_labels, const int* num_gt, int I, int K, int G, int C, double iou_threshold, "
             "unsigned char* tp, float* det_scores, int* ngt, void* stream);")
    ap = ("int x3d_frame_ap(const unsigned char* tp, const float* det_scores, const long long* order, const int* ngt, int N, "
          "int C, double* ap, int* ntp, void* stream);")
    assert match in text and ap in text
    assert "#define X3D_ABI_VERSION 138" in text
    vp, i, d = ctypes.c_void_p, ctypes.c_int, ctypes.c_double
    want = {"x3d_frame_match": [vp] * 6 + [i] * 4 + [d] + [vp] * 4, "x3d_frame_ap": [vp] * 4 + [i] * 2 + [vp] * 3}
    lib = hip.load()
    for name, argtypes in want.items():
        assert name in hip.exported_symbols()
        assert hip._SIGS[name] == (argtypes, i)
        assert list(getattr(lib, name).argtypes) == argtypes and getattr(lib, name).restype is i


def test_c_abi_refusals_name_the_argument():
    """the entry points refuse before any launch (no GPU needed): the message names the argument"""
    lib = hip.load()
    buf = (ctypes.c_char * 64)()
    p = ctypes.addressof(buf)

    def match(i=1, k=1, g=1, c=1, thr=0.5, null=None):
        a = [p] * 6 + [i, k, g, c, thr] + [p] * 3
        if null is not None:
            a[null] = None
        return lib.x3d_frame_match(*a, None)

    def ap(n=1, c=1, null=None):
        a = [p] * 4 + [n, c] + [p] * 2
        if null is not None:
            a[null] = None
        return lib.x3d_frame_ap(*a, None)
    cases = [(lambda: match(i=0), b"I = 0"), (lambda: match(k=0), b"K = 0"), (lambda: match(k=65), b"K = 65"),
             (lambda: match(g=0), b"G = 0"), (lambda: match(g=65), b"G = 65"), (lambda: match(c=0), b"C = 0"),
             (lambda: match(i=1 << 20, k=64, c=32), b"I*K*C"), (lambda: match(thr=0.0), b"iou_threshold"),
             (lambda: match(thr=1.5), b"iou_threshold"), (lambda: match(thr=float("nan")), b"iou_threshold"),
             (lambda: match(null=0), b"scores"), (lambda: match(null=4), b"gt_labels"), (lambda: match(null=13), b"ngt"),
             (lambda: ap(n=0), b"N = 0"), (lambda: ap(c=0), b"C = 0"), (lambda: ap(n=1 << 16, c=1 << 15), b"N*C"),
             (lambda: ap(null=2), b"order"), (lambda: ap(null=6), b"ap is null")]
    for call, who in cases:
        assert call() != 0
        assert who in lib.x3d_last_error(), (who, lib.x3d_last_error())


# ---- ops ----------------------------------------------------------------------------------------------------------------
def _match_args(i=2, k=3, g=2, c=4, device="cpu"):
    return dict(scores=torch.zeros(i * k, c, device=device), boxes=torch.zeros(i, k, 4, device=device),
                num_boxes=torch.zeros(i, dtype=torch.int32, device=device), gt_boxes=torch.zeros(i, g, 4, device=device),
                gt_labels=torch.zeros(i, g, c, dtype=torch.uint8, device=device),
                num_gt=torch.zeros(i, dtype=torch.int32, device=device))


def test_ops_frame_match_refusals():
    for over, who in ((dict(k=65), "K = 65"), (dict(k=0), "K = 0"), (dict(g=0), "G = 0"), (dict(g=65), "G = 65"),
                      (dict(c=0), "C = 0"), (dict(i=0), "I = 0")):
        with pytest.raises(ValueError, match=who):
            ops.frame_match(**_match_args(**over))
    for thr in (0.0, -0.5, 1.01, float("nan")):
        with pytest.raises(ValueError, match="iou_threshold"):
            ops.frame_match(**_match_args(), iou_threshold=thr)
    a = _match_args()
    for name, bad in (("scores", a["scores"].double()), ("boxes", a["boxes"].double()), ("num_boxes", a["num_boxes"].long()),
                      ("gt_boxes", a["gt_boxes"].half()), ("gt_labels", a["gt_labels"].float()), ("num_gt", a["num_gt"].long()),
                      ("num_boxes", a["num_boxes"][:1]), ("gt_labels", a["gt_labels"][:, :, :3]),
                      ("gt_boxes", torch.zeros(3, 2, 4)), ("boxes", a["boxes"].to("meta")), ("num_gt", a["num_gt"].to("meta"))):
        with pytest.raises(ValueError, match=f"frame_match: {name} "):
            ops.frame_match(**dict(a, **{name: bad}))
    with pytest.raises(ValueError, match="scores has 5 rows"):
        ops.frame_match(**dict(a, scores=torch.zeros(5, 4)))
    for name, bad in (("tp", torch.zeros(6, 4)), ("det_scores", torch.zeros(6, 3)), ("ngt", torch.zeros(4, dtype=torch.int64))):
        with pytest.raises(ValueError, match=f"frame_match: {name} "):
            ops.frame_match(**a, **{name: bad})
    with pytest.raises(hip.X3DHipError, match="GPU tensors"):          # every check passed: no CPU fallback
        ops.frame_match(**a)


def test_ops_frame_ap_refusals():
    n, c = 5, 3
    a = dict(tp=torch.zeros(n, c, dtype=torch.uint8), det_scores=torch.zeros(n, c), ngt=torch.zeros(c, dtype=torch.int32))
    for name, bad in (("tp", a["tp"].float()), ("tp", a["tp"][:4]), ("det_scores", a["det_scores"].double()),
                      ("ngt", a["ngt"].long()), ("ngt", a["ngt"][:2]), ("tp", a["tp"].to("meta")),
                      ("order", torch.zeros(n, c, dtype=torch.int32)), ("order", torch.zeros(n, c + 1, dtype=torch.int64)),
                      ("ap", torch.zeros(c)), ("ntp", torch.zeros(c, dtype=torch.int64))):
        with pytest.raises(ValueError, match=f"frame_ap: {name} "):
            ops.frame_ap(**dict(a, **{name: bad}))
    with pytest.raises(ValueError, match="N = 0"):
        ops.frame_ap(torch.zeros(0, c, dtype=torch.uint8), torch.zeros(0, c), a["ngt"])
    with pytest.raises(ValueError, match="C = 0"):
        ops.frame_ap(torch.zeros(n, 0, dtype=torch.uint8), torch.zeros(n, 0), torch.zeros(0, dtype=torch.int32))
    with pytest.raises(hip.X3DHipError, match="GPU tensors"):
        ops.frame_ap(**a)


# ---- DeviceFrameMAP -----------------------------------------------------------------------------------------------------
def test_device_frame_map_empty_and_threshold():
    r = DeviceFrameMAP().result()
    assert math.isnan(r["frame_mAP"]) and r["classes"] == 0 and r["detections"] == 0 and r["gt_boxes"] == 0 and r["ap"] == []
    assert DeviceFrameMAP().iou_threshold == 0.5 and DeviceFrameMAP(0.75).iou_threshold == 0.75
    for thr in (0.0, 1.5, float("nan")):
        with pytest.raises(ValueError, match="iou_threshold"):
            DeviceFrameMAP(thr)
    assert DeviceFrameMAP().all_reduce_() is not None          # no process group: a no-op
