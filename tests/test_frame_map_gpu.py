"""Frame-mAP for action detection on the GPU: x3d_frame_match and x3d_frame_ap against tests/frame_map_ref.py (NumPy fp64, written
from the rules in include/x3d_hip.h), evaluate.DeviceFrameMAP over several batches, and Trainer.validate / fit on seven-item
detection batches.

frame_match is compared BIT FOR BIT (tp, det_scores) and exactly (ngt): the IoU is the same IEEE double sequence on both sides, so
no decision is "up to rounding".  frame_ap: ntp exactly; ap within (ntp[c] + 2) * 2^-52 absolute -- each env_t is a correctly
rounded quotient, the maximum is exact, and P terms of at most 1 are summed in some order and divided by ngt >= P."""
import math
import os
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from tests import frame_map_ref as R  # noqa: E402
from tests import roi_ref  # noqa: E402
from x3d_tf_amd import ops  # noqa: E402
from x3d_tf_amd.evaluate import DeviceFrameMAP  # noqa: E402

pytestmark = pytest.mark.gpu
GUARD = 256          # elements in front of and behind tp / det_scores
UNIT = (0, 0, 1, 1)


# ---- frame_match ----------------------------------------------------------------------------------------------------------
def _guarded(rows, c, dtype, fill, gpu):
    flat = torch.full((rows * c + 2 * GUARD,), fill, dtype=dtype, device=gpu)
    return flat, flat[GUARD:GUARD + rows * c].view(rows, c)


def _check_match(gpu, scores, boxes, nb, gtb, gtl, ng, thr=0.5):
    """one launch with guard bands around the outputs and ngt used as an increment on non-zero contents, against the reference:
    returns the reference's (tp, det_scores)"""
    scores, boxes, gtb = np.asarray(scores, np.float32), np.asarray(boxes, np.float32), np.asarray(gtb, np.float32)
    gtl = np.asarray(gtl, np.uint8)
    rows, c = scores.shape
    ngt0 = (np.arange(c) * 3 + 7).astype(np.int32)
    want_tp, want_det, want_ngt = R.frame_match(scores, boxes, nb, gtb, gtl, ng, thr, ngt=ngt0)
    tp_flat, tp = _guarded(rows, c, torch.uint8, 0xA5, gpu)
    det_flat, det = _guarded(rows, c, torch.float32, 12345.0, gpu)
    ngt = torch.from_numpy(ngt0.copy()).to(gpu)
    dev = lambda a, dt: torch.from_numpy(np.ascontiguousarray(a)).to(gpu, dt)
    out = ops.frame_match(dev(scores, torch.float32), dev(boxes, torch.float32), dev(np.asarray(nb), torch.int32),
                          dev(gtb, torch.float32), dev(gtl, torch.uint8), dev(np.asarray(ng), torch.int32), thr, tp=tp, det_scores=det,
                          ngt=ngt)
    assert out[0] is tp and out[1] is det and out[2] is ngt
    torch.cuda.synchronize()
    got_tp, got_det = tp.cpu().numpy(), det.cpu().numpy()
    assert np.array_equal(got_tp, want_tp), f"tp differs at {np.argwhere(got_tp != want_tp)[:5].tolist()}"
    assert np.array_equal(got_det.view(np.int32), want_det.view(np.int32)), "det_scores differ in their bits"
    assert ngt.cpu().numpy().tolist() == want_ngt.tolist()
    for flat, fill in ((tp_flat, 0xA5), (det_flat, 12345.0)):
        assert bool((flat[:GUARD] == fill).all()) and bool((flat[-GUARD:] == fill).all()), "a guard band was written"
    return want_tp, want_det


def _one(det_box, gt_box, score=0.75):
    return ([[score]], [[det_box]], [1], [[gt_box]], [[[1]]], [1])


@pytest.mark.parametrize("det_box, want", [(UNIT, 1), ((3, 3, 4, 4), 0), ((0, 0, 2, 1), 1),
                                           ((0, 0, float(np.nextafter(np.float32(2), np.float32(3))), 1), 0)],
                         ids=["hit", "miss", "iou-exactly-half", "iou-one-ulp-below-half"])
def test_match_single(gpu, det_box, want):
    tp, det = _check_match(gpu, *_one(det_box, UNIT))
    assert tp.tolist() == [[want]] and det.tolist() == [[0.75]]


def _random_case(seed, n_img, k, g, c, nb=None, grid=True, ng=None, intact=()):
    """seeded images.  grid: coordinates on a grid of 8 pixels (equal IoUs and exact 0.5s are frequent), else uniform fp32 ones
    (inexact products and quotients: the same on both sides); scores in sixteenths (ties are frequent); one to three classes per
    ground-truth box; about half the ground-truth boxes copy or shift a proposal.  Empty slots hold a huge score on a plausible
    box, some filled slots are invalid (a NaN coordinate, zero width), some valid slots have a NaN score.  nb / ng: every image's
    num_boxes / num_gt (else drawn in 0..K / 0..G); intact: the images none of whose slots is made invalid."""
    rng = np.random.default_rng(seed)

    def draw(shape):
        if grid:
            x1, y1 = 8.0 * rng.integers(0, 4, shape), 8.0 * rng.integers(0, 4, shape)
            return np.stack([x1, y1, x1 + 8.0 * rng.integers(1, 5, shape), y1 + 8.0 * rng.integers(1, 5, shape)], -1).astype(np.float32)
        x1, y1 = rng.uniform(0, 32, shape), rng.uniform(0, 32, shape)
        return np.stack([x1, y1, x1 + rng.uniform(4, 40, shape), y1 + rng.uniform(4, 40, shape)], -1).astype(np.float32)
    boxes, gtb = draw((n_img, k)), draw((n_img, g))
    for i in range(n_img):
        for j in range(g):
            if rng.random() < 0.5:
                gtb[i, j] = boxes[i, rng.integers(0, k)]
                if rng.random() < 0.5:
                    gtb[i, j, [0, 2]] += np.float32(8.0 if grid else rng.uniform(0, 6))
    num_b = rng.integers(0, k + 1, n_img) if nb is None else np.full(n_img, nb)
    num_g = rng.integers(0, g + 1, n_img) if ng is None else np.full(n_img, ng)
    scores = (rng.integers(0, 17, (n_img * k, c)) / 16.0).astype(np.float32)
    scores[rng.random(scores.shape) < 0.01] = np.nan
    for i in range(n_img):
        scores[i * k + int(num_b[i]):(i + 1) * k] = 1e30                  # empty slots: must claim nothing
        for j in range(int(num_b[i])):
            u = rng.random()
            if i in intact:
                continue
            if u < 0.04:
                boxes[i, j, rng.integers(0, 4)] = np.nan
            elif u < 0.08:
                boxes[i, j, 2] = boxes[i, j, 0]
        for j in range(int(num_g[i])):
            if rng.random() < 0.05 and i not in intact:
                gtb[i, j, 3] = gtb[i, j, 1]
    gtl = np.zeros((n_img, g, c), np.uint8)
    for i in range(n_img):
        for j in range(g):
            gtl[i, j, rng.choice(c, size=min(c, int(rng.integers(1, 4))), replace=False)] = rng.integers(1, 256)
    return scores, boxes, num_b, gtb, gtl, num_g


# full-waves: num_boxes = num_gt = 64 in both images, and in image 0 every one of the 64 + 64 slots is valid
MATCH_CASES = [("full-waves", dict(n_img=2, k=64, g=64, c=3, nb=64, ng=64, intact=(0,))),
               ("k64-nb63", dict(n_img=2, k=64, g=64, c=3, nb=63, ng=64)),
               ("k5-g7", dict(n_img=6, k=5, g=7, c=4)), ("c1", dict(n_img=8, k=8, g=6, c=1)), ("c80", dict(n_img=8, k=8, g=6, c=80)),
               ("c157", dict(n_img=4, k=8, g=6, c=157)), ("sweep", dict(n_img=300, k=8, g=6, c=80)),
               ("off-grid", dict(n_img=40, k=8, g=6, c=20, grid=False))]


@pytest.mark.parametrize("case", MATCH_CASES, ids=lambda c: c[0])
def test_match_random(gpu, case):
    args = _random_case(11, **case[1])
    tp, det = _check_match(gpu, *args)
    if case[0] == "sweep":            # the sweep exercises what it is there for
        assert tp.sum() > 300 and np.isnan(det).any() and np.isinf(det).any()
    if case[0] == "full-waves":
        assert R.num_valid(args[1][:1], args[2][:1]) == 64 and R.num_valid(args[3][:1], args[5][:1]) == 64
        assert (args[4][0, 48:] != 0).any(axis=0).all()          # every class is carried by boxes in the last ballot bits
        _check_match(gpu, *args, thr=0.3)
        _check_match(gpu, *args, thr=1.0)


def test_match_full_wave_every_box_claimed(gpu):
    """K = G = 64, every slot valid: 64 disjoint annotated boxes (an 8 x 8 board of unit cells), all carrying class 0 and the
    odd ones class 1, and the same 64 boxes as proposals in REVERSE order -- detection k can only match ground-truth box
    63 - k, so every ballot bit, every row of the [g][k] table and both lanes 63 decide a true positive"""
    cells = np.array([[x, y, x + 1, y + 1] for y in range(8) for x in range(8)], np.float32)
    gtb, boxes = cells[None], cells[::-1][None].copy()
    gtl = np.zeros((1, 64, 2), np.uint8)
    gtl[0, :, 0], gtl[0, 1::2, 1] = 1, 200
    scores = np.stack([np.arange(64) / 64.0, np.full(64, 0.5)], 1).astype(np.float32)
    tp, det = _check_match(gpu, scores, boxes, [64], gtb, gtl, [64])
    assert tp[:, 0].all() and tp[:, 1].tolist() == [1 - k % 2 for k in range(64)]      # box 63 - k is odd iff k is even
    # one proposal fewer / one annotated box fewer: slot 63 of either side drops out, and nothing else moves
    tp, _ = _check_match(gpu, scores, boxes, [63], gtb, gtl, [64])
    assert tp[:63, 0].all() and not tp[63].any()
    tp, _ = _check_match(gpu, scores, boxes, [64], gtb, gtl, [63])
    assert tp[1:, 0].all() and not tp[0].any()                                          # detection 0 sat on box 63


def test_match_empty_and_invalid_slots(gpu):
    """images without proposals and without ground truth; an empty slot with a huge score on the annotated box itself, which must
    claim nothing; invalid slots (a NaN coordinate, zero width) and a NaN score in a valid slot"""
    k, g, c = 4, 3, 2
    boxes, gtb = np.zeros((4, k, 4), np.float32), np.zeros((4, g, 4), np.float32)
    boxes[:], gtb[:] = UNIT, UNIT
    scores = np.full((4 * k, c), 0.5, np.float32)
    gtl = np.ones((4, g, c), np.uint8)
    nb, ng = [0, 2, 1, 4], [2, 0, 1, 1]
    boxes[2, 0] = (0, 0, 1.5, 1)                     # image 2: slot 0 passes at IoU 2/3; slot 1 is EMPTY, a perfect box, score 1e30
    scores[2 * k + 1] = 1e30
    boxes[3, 0, 1] = np.nan                          # image 3: slot 0 a NaN coordinate, slot 1 zero width, slot 2 a NaN score,
    boxes[3, 1, 2] = boxes[3, 1, 0]                  # slot 3 the true positive
    scores[3 * k:3 * k + 3] = 9.0
    scores[3 * k + 2, 0] = np.nan
    scores[3 * k + 3] = 0.25
    tp, det = _check_match(gpu, scores, boxes, nb, gtb, gtl, ng)
    assert not tp[:2 * k].any() and np.isinf(det[:k]).all()
    assert tp[2 * k:3 * k, 0].tolist() == [1, 0, 0, 0] and det[2 * k + 1, 0] == -np.inf
    assert tp[3 * k:, 0].tolist() == [0, 0, 0, 1] and tp[3 * k:, 1].tolist() == [0, 0, 1, 0]
    assert math.isnan(det[3 * k + 2, 0]) and det[3 * k, 0] == -np.inf and det[3 * k + 1, 0] == -np.inf


# ---- frame_ap -------------------------------------------------------------------------------------------------------------
KINDS = ("random", "all-tp", "none", "no-gt", "nan")


def _ap_case(seed, n, c, shift=0):
    """class j is of kind KINDS[(j + shift) % 5]: scores on 8 levels (heavy ties), about a third of the rows at -inf with tp = 0
    interleaved; "all-tp": every row a detection and a true positive, ngt = N; "none": no true positive; "no-gt": ngt = 0;
    "nan": one NaN score"""
    rng = np.random.default_rng(seed)
    det = (rng.integers(0, 8, (n, c)) / 8.0).astype(np.float32)
    tp = (rng.random((n, c)) < 0.15).astype(np.uint8)
    empty = rng.random((n, c)) < 0.3
    det[empty], tp[empty] = -np.inf, 0
    ngt = np.zeros(c, np.int32)
    for j in range(c):
        kind = KINDS[(j + shift) % len(KINDS)]
        if kind == "all-tp":
            det[:, j], tp[:, j] = (rng.integers(0, 8, n) / 8.0).astype(np.float32), 1
        elif kind == "none":
            tp[:, j] = 0
        elif kind == "nan":
            det[rng.integers(0, n), j] = np.nan
        extra = 0 if kind == "all-tp" else int(rng.integers(0, 4))
        ngt[j] = 0 if kind == "no-gt" else max(1, int(tp[:, j].sum()) + extra)
    return tp, det, ngt


def _check_ap(gpu, tp, det, ngt):
    want_ap, want_ntp = R.frame_ap(tp, det, ngt)
    d_tp, d_det, d_ngt = torch.from_numpy(tp).to(gpu), torch.from_numpy(det).to(gpu), torch.from_numpy(ngt).to(gpu)
    ap, ntp = ops.frame_ap(d_tp, d_det, d_ngt)
    ap2, ntp2 = ops.frame_ap(d_tp, d_det, d_ngt)
    torch.cuda.synchronize()
    ap, ntp = ap.cpu().numpy(), ntp.cpu().numpy()
    assert np.array_equal(ap.view(np.int64), ap2.cpu().numpy().view(np.int64)) and torch.equal(ntp2.cpu(), torch.from_numpy(ntp))
    assert ntp.tolist() == want_ntp.tolist()
    assert np.array_equal(np.isnan(ap), np.isnan(want_ap)), (ap, want_ap)
    ok = ~np.isnan(want_ap)
    err = np.abs(ap[ok] - want_ap[ok])
    bound = (want_ntp[ok] + 2) * 2.0 ** -52
    print(f"N = {tp.shape[0]} C = {tp.shape[1]}: worst |ap - ref| = {err.max() if err.size else 0.0:.3e}, bound there "
          f"{bound[err.argmax()] if err.size else 0.0:.3e}")
    assert (err <= bound).all()
    return ap, ntp


@pytest.mark.parametrize("c", [1, 3, 80])
@pytest.mark.parametrize("n", [1, 63, 64, 65, 1023, 1024, 1025, 5000, 70001])
def test_ap_matches_fp64(gpu, n, c):
    _check_ap(gpu, *_ap_case(n * 131 + c, n, c, shift=n))


def test_ap_every_kind_of_class(gpu):
    tp, det, ngt = _ap_case(5, 1025, 5)
    ap, ntp = _check_ap(gpu, tp, det, ngt)
    assert 0.0 < ap[0] < 1.0 and ntp[0] == tp[:, 0].sum()
    assert ap[1] == 1.0 and ntp[1] == 1025 and ngt[1] == 1025
    assert ap[2] == 0.0 and ntp[2] == 0 and ngt[2] > 0
    assert math.isnan(ap[3]) and ngt[3] == 0 and ntp[3] == tp[:, 3].sum()
    assert math.isnan(ap[4]) and ngt[4] > 0


def test_ap_hand_worked(gpu):
    """TP, FP, TP over 2 ground-truth boxes, rows at -inf in between: (1 + 2/3) / 2 to the last bit (two terms: one order)"""
    tp = np.array([[1], [0], [0], [1], [0]], np.uint8)
    det = np.array([[0.7], [-np.inf], [0.8], [0.9], [-np.inf]], np.float32)
    ap, ntp = _check_ap(gpu, tp, det, np.array([2], np.int32))
    assert ap[0] == (1.0 + 2.0 / 3.0) / 2.0 and ntp[0] == 2


def test_ap_both_signs_of_zero_are_one_score(gpu):
    """-0 and +0 in one column are equal scores, ordered by row index: the sort behind ops.frame_ap must not order the two bit
    patterns.  Six rows by hand (0.5 first, then the five zeros in row order: true positives at positions 3, 5, 6 -> env 1/2
    three times; +0 ahead of -0 would give positions 2, 3, 6), then 3000 rows drawn from {-0, +0, 0.25, -inf}"""
    det = np.array([[-0.0], [0.0], [-0.0], [0.0], [0.5], [-0.0]], np.float32)
    tp = np.array([[0], [1], [0], [1], [0], [1]], np.uint8)
    ap, ntp = _check_ap(gpu, tp, det, np.array([3], np.int32))
    assert ap[0] == 0.5 and ntp[0] == 3
    rng = np.random.default_rng(17)
    det = rng.choice(np.array([-0.0, 0.0, 0.25, -np.inf], np.float32), size=(3000, 3))
    tp = ((rng.random((3000, 3)) < 0.3) & ~np.isinf(det)).astype(np.uint8)
    assert (np.signbit(det) & (det == 0)).any() and (~np.signbit(det) & (det == 0)).any()
    _check_ap(gpu, tp, det, (tp.sum(0) + 2).astype(np.int32))


def test_ap_has_no_cap_on_true_positives(gpu):
    """more true positives in a class than x3d_multilabel_ap holds in LDS (X3D_AP_MAX_POSITIVES): every row a true positive"""
    from x3d_tf_amd import hip
    n, c = 40000, 2
    assert n > hip.AP_MAX_POSITIVES
    rng = np.random.default_rng(3)
    det = (rng.integers(0, 64, (n, c)) / 64.0).astype(np.float32)
    ap, ntp = _check_ap(gpu, np.ones((n, c), np.uint8), det, np.full(c, n, np.int32))
    assert ap.tolist() == [1.0, 1.0] and ntp.tolist() == [n, n]


def test_ap_takes_a_given_order(gpu):
    """`order` handed over (int64 [N, C], every class's own stable descending sort) gives what the default gives"""
    tp, det, ngt = _ap_case(9, 777, 3)
    d_tp, d_det, d_ngt = torch.from_numpy(tp).to(gpu), torch.from_numpy(det).to(gpu), torch.from_numpy(ngt).to(gpu)
    order = torch.sort(d_det, dim=0, descending=True, stable=True).indices
    a0, n0 = ops.frame_ap(d_tp, d_det, d_ngt)
    a1, n1 = ops.frame_ap(d_tp, d_det, d_ngt, order=order, ap=torch.empty(3, dtype=torch.float64, device=gpu),
                          ntp=torch.empty(3, dtype=torch.int32, device=gpu))
    assert torch.equal(a0.view(torch.int64), a1.view(torch.int64)) and torch.equal(n0, n1)


# ---- DeviceFrameMAP -------------------------------------------------------------------------------------------------------
def _ap_bound(ntp):
    return float((np.max(ntp) + 2) * 2.0 ** -52)


def test_device_frame_map_over_unequal_batches(gpu):
    k, g, c = 4, 3, 6
    parts = [_random_case(20 + b, n_img, k, g, c) for b, n_img in enumerate((3, 5, 2))]
    fm = DeviceFrameMAP()
    for scores, boxes, nb, gtb, gtl, ng in parts:
        # the arguments as a reader hands them over: host tensors, int64 counts, bool labels
        fm.update(torch.from_numpy(scores).to(gpu), torch.from_numpy(boxes), torch.from_numpy(nb), torch.from_numpy(gtb),
                  torch.from_numpy(gtl != 0), torch.from_numpy(ng))
    r = fm.result()
    cat = [np.concatenate([p[j] for p in parts]) for j in range(6)]
    tp, det, ngt = R.frame_match(*cat)
    ap, ntp = R.frame_ap(tp, det, ngt)
    assert r["detections"] == R.num_valid(cat[1], cat[2]) > 0 and r["gt_boxes"] == R.num_valid(cat[3], cat[5]) > 0
    assert r["classes"] == int((ngt > 0).sum())
    got = np.array(r["ap"])
    assert np.array_equal(np.isnan(got), np.isnan(ap))
    ok = ~np.isnan(ap)
    assert (np.abs(got[ok] - ap[ok]) <= (ntp[ok] + 2) * 2.0 ** -52).all()
    want = R.frame_map(ap, ngt)
    assert (math.isnan(want) and math.isnan(r["frame_mAP"])) or abs(r["frame_mAP"] - want) <= _ap_bound(ntp) + 2.0 ** -52
    # a NaN score is in the case by construction; without it the mean is finite
    clean = [np.nan_to_num(p[0], nan=0.25) for p in parts]
    fm = DeviceFrameMAP(0.75)
    for s, (_, boxes, nb, gtb, gtl, ng) in zip(clean, parts):
        fm.update(torch.from_numpy(s).to(gpu), torch.from_numpy(boxes).to(gpu), nb.tolist(), gtb, gtl, ng.astype(np.int32))
    r = fm.result()
    tp, det, ngt = R.frame_match(np.concatenate(clean), *cat[1:], iou_threshold=0.75)
    ap, ntp = R.frame_ap(tp, det, ngt)
    assert math.isfinite(r["frame_mAP"]) and abs(r["frame_mAP"] - R.frame_map(ap, ngt)) <= _ap_bound(ntp) + 2.0 ** -52


# ---- Trainer.validate / fit -----------------------------------------------------------------------------------------------
BASE = ["DATA.TEMP_DURATION", 4, "TEST.NUM_SPATIAL_CROPS", 1, "TEST.NUM_TEMPORAL_VIEWS", 1, "NETWORK.NUM_CLASSES", 11,
        "TRAIN.BATCH_SIZE", 2, "TRAIN.DATASET_SIZE", 4]
KB, GB = 3, 2
DET = ["DETECTION.ENABLE", True, "DETECTION.MAX_BOXES", KB, "DATA.MULTI_LABEL", True]
N, T, S = 2, 4, 64


def _trainer(gpu):
    import x3d_tf_amd as x
    from x3d_tf_amd.model import X3D
    from x3d_tf_amd.params import init_params, randomize_bn_
    from x3d_tf_amd.train import Trainer
    cfg = x.get_config("XS", BASE + DET)
    arch = x.build_arch(cfg)
    m = X3D(cfg, dtype=torch.float32, device=gpu, seed=0)
    m.load_state_dict(randomize_bn_(init_params(arch, seed=3), seed=4))
    return Trainer(m, cfg), m, arch.num_classes


def _batches(gpu, classes, seed, counts=((2, 3), (3, 1))):
    """seven-item batches: the proposals are roi_ref.box_mix's first three kinds (valid boxes), the annotated boxes two of them,
    one moved by a few pixels, carrying one to three classes"""
    g = torch.Generator().manual_seed(seed)
    rng = np.random.default_rng(seed)
    out = []
    for i, nb in enumerate(counts):
        boxes = roi_ref.box_mix(N, KB, S, S, seed=seed + i)
        gtb = boxes[:, :GB].copy()
        gtb[:, 1, [0, 2]] += np.float32(2.0)
        gtl = np.zeros((N, GB, classes), np.uint8)
        for a in range(N):
            for b in range(GB):
                gtl[a, b, rng.choice(classes, size=int(rng.integers(1, 4)), replace=False)] = 1
        out.append((torch.randn(N, T, S, S, 3, generator=g).to(gpu), (torch.rand(N, KB, classes, generator=g) < 0.3).float(),
                    torch.from_numpy(boxes), torch.tensor(nb), torch.from_numpy(gtb), torch.from_numpy(gtl),
                    torch.tensor([GB, 1 + i % 2])))
    return out


def _want_frame_map(m, batches, classes, thr=0.5):
    tps, dets, ngt = [], [], np.zeros(classes, np.int32)
    for clips, _, bx, nb, gtb, gtl, ng in batches:
        p = m(clips, boxes=bx, num_boxes=nb).float().cpu().numpy().reshape(N * KB, classes)
        tp, det, ngt = R.frame_match(p, bx.numpy(), nb.numpy(), gtb.numpy(), gtl.numpy(), ng.numpy(), thr, ngt=ngt)
        tps.append(tp)
        dets.append(det)
    ap, ntp = R.frame_ap(np.concatenate(tps), np.concatenate(dets), ngt)
    n_det = sum(R.num_valid(b[2].numpy(), b[3].numpy()) for b in batches)
    n_gt = sum(R.num_valid(b[4].numpy(), b[6].numpy()) for b in batches)
    return R.frame_map(ap, ngt), int((ngt > 0).sum()), n_det, n_gt, _ap_bound(ntp) + 2.0 ** -52


def test_validate_frame_map(gpu):
    tr, m, classes = _trainer(gpu)
    batches = _batches(gpu, classes, seed=50)
    four = [b[:4] for b in batches]
    today = tr.validate(four)
    assert set(today) == {"loss", "mAP", "videos", "classes"}                     # four-item sets: exactly today's keys
    for thr in (0.5, 0.97):
        r = tr.validate(batches, iou_threshold=thr)
        want, n_cls, n_det, n_gt, tol = _want_frame_map(m, batches, classes, thr)
        print(f"threshold {thr}: frame_mAP {r['frame_mAP']} vs {want}")
        assert set(r) == set(today) | {"frame_mAP", "frame_classes", "detections", "gt_boxes"}
        assert math.isfinite(want) and abs(r["frame_mAP"] - want) <= tol
        assert (r["frame_classes"], r["detections"], r["gt_boxes"]) == (n_cls, n_det, n_gt)
        assert {k: r[k] for k in today} == today                                  # the row-wise metric is what it was
    want = _want_frame_map(m, batches, classes)[0]
    # labels = None: the frame keys only
    r = tr.validate([(b[0], None) + b[2:] for b in batches])
    assert abs(r["frame_mAP"] - want) <= tol and math.isnan(r["loss"]) and math.isnan(r["mAP"]) and r["videos"] == 0
    assert set(r) == set(today) | {"frame_mAP", "frame_classes", "detections", "gt_boxes"}
    with pytest.raises(ValueError, match="four items"):
        tr.validate([batches[0], four[1]])
    with pytest.raises(ValueError, match="four items"):
        tr.validate([four[0], batches[1]])
    with pytest.raises(ValueError, match="in every batch of the set or in none"):      # labelled and unlabelled batches in one set
        tr.validate([batches[0], (batches[1][0], None) + batches[1][2:]])
    with pytest.raises(ValueError, match="labels may be None"):
        tr.validate([(four[0][0], None) + four[0][2:]])


def test_fit_records_val_frame_map(gpu):
    tr, m, classes = _trainer(gpu)
    train = [b[:4] for b in _batches(gpu, classes, seed=60)]
    val = _batches(gpu, classes, seed=70)
    tr.fit(iter(train), epochs=1, validation_data=lambda: val)
    assert tr.opt_step == 2 and len(tr.history["val_frame_mAP"]) == 1 and math.isfinite(tr.history["val_frame_mAP"][0])
    assert len(tr.history["val_mAP"]) == 1
    tr.fit(iter(train), epochs=2, validation_data=lambda: [b[:4] for b in val])      # one more epoch, four-item validation
    assert tr.epoch == 2 and "val_frame_mAP" not in tr.history and len(tr.history["val_mAP"]) == 1
