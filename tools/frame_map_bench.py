"""What the frame-mAP evaluation costs (profiles/frame_map_mi355x.txt).

    python tools/frame_map_bench.py [--out FILE] [--images 50000] [--no-forward]

Set level, at an AVA-val-like size (50 000 images, K = 8 proposal slots, G = 8 ground-truth slots, C = 80 classes, seeded
synthetic boxes: per image 1..K proposals and 1..G annotated boxes, about half of them near a proposal, one to three classes
each): x3d_frame_match over the whole set in one launch, the column sort (torch.sort, stable), x3d_frame_ap, and
DeviceFrameMAP.result() (concatenate + sort + x3d_frame_ap + the read-back).  Device events around 10 launches after 2 warm-up
launches; result(): host clock around the call, which ends in the read-back.
Batch level: what one validation batch adds -- DeviceFrameMAP.update (the launch, the host-to-device copies of the boxes and the
two counts), the same with the inputs already on the device, and the bare x3d_frame_match launch -- against that batch's
inference forward of X3D-M with DETECTION.ENABLE (bf16, one view), at the config's TEST.BATCH_SIZE and at 64 clips.  Three
alternating rounds in ONE process.  A record, not a gate."""
import argparse
import os
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
ap = argparse.ArgumentParser()
ap.add_argument("--out", help="also write the lines to this file")
ap.add_argument("--images", type=int, default=50000)
ap.add_argument("--no-forward", action="store_true", help="set level only")
args = ap.parse_args()
lines = []


def say(s):
    print(s, flush=True)
    lines.append(s)
    if args.out:
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


import x3d_tf_amd as x  # noqa: E402
from x3d_tf_amd import ops  # noqa: E402
from x3d_tf_amd.evaluate import DeviceFrameMAP  # noqa: E402
from x3d_tf_amd.model import X3D  # noqa: E402

dev = torch.device("cuda:0")
say(f"device: {torch.cuda.get_device_name(0)}")
K, G, C = 8, 8, 80


def synth(images, seed):
    """(scores [I*K, C], boxes, num_boxes, gt_boxes, gt_labels, num_gt) on the device"""
    g = torch.Generator().manual_seed(seed)
    ctr, half = 32 + 160 * torch.rand(images, K, 2, generator=g), 20 + 60 * torch.rand(images, K, 2, generator=g)
    boxes = torch.cat([ctr - half, ctr + half], 2).clamp(0, 224)
    gctr, ghalf = 32 + 160 * torch.rand(images, G, 2, generator=g), 20 + 60 * torch.rand(images, G, 2, generator=g)
    gt = torch.cat([gctr - ghalf, gctr + ghalf], 2).clamp(0, 224)
    near = torch.rand(images, G, generator=g) < 0.5             # about half the annotated boxes sit near a proposal
    pick = torch.randint(0, K, (images, G), generator=g)
    moved = torch.gather(boxes, 1, pick[:, :, None].expand(-1, -1, 4)) + 6 * torch.randn(images, G, 4, generator=g)
    gt = torch.where(near[:, :, None], moved, gt)
    gt = torch.cat([torch.minimum(gt[..., :2], gt[..., 2:] - 4), gt[..., 2:]], 2)
    labels = torch.zeros(images, G, C, dtype=torch.uint8)
    for _ in range(3):                                          # one to three classes per box
        labels.scatter_(2, torch.randint(0, C, (images, G, 1), generator=g), 1)
    nb = torch.randint(1, K + 1, (images,), generator=g, dtype=torch.int32)
    ng = torch.randint(1, G + 1, (images,), generator=g, dtype=torch.int32)
    scores = torch.rand(images * K, C, generator=g)
    return [t.contiguous().to(dev) for t in (scores, boxes, nb, gt, labels, ng)]


def timed(fn, reps=10, warm=2):
    for _ in range(warm):
        fn()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / reps


I = args.images
scores, boxes, nb, gt, labels, ng = synth(I, 2000)
tp, det, ngt = ops.frame_match(scores, boxes, nb, gt, labels, ng)
order = torch.sort(det, dim=0, descending=True, stable=True).indices
apv, ntp = ops.frame_ap(tp, det, ngt, order=order)
torch.cuda.synchronize()
have = ngt > 0
say(f"set level: {I} images, K = {K}, G = {G}, C = {C}: {I * K} rows, {int(nb.sum())} detections, {int(ng.sum())} annotated boxes, "
    f"{int(tp.sum())} true-positive flags, frame-mAP {float(apv[have].mean()):.4f}; scores {scores.numel() * 4 / 1e6:.0f} MB, order "
    f"{order.numel() * 8 / 1e6:.0f} MB; 10 launches between device events after 2 warm-up launches; three alternating rounds")
scratch = torch.zeros_like(ngt)
fm = DeviceFrameMAP()
fm._scores, fm._tp, fm.ngt, fm.counts = [det], [tp], ngt, torch.zeros(2, dtype=torch.int64, device=dev)
ARMS = [("x3d_frame_match (whole set)", lambda: ops.frame_match(scores, boxes, nb, gt, labels, ng, tp=tp, det_scores=det, ngt=scratch)),
        ("torch.sort (stable, dim 0)", lambda: torch.sort(det, dim=0, descending=True, stable=True)),
        ("x3d_frame_ap", lambda: ops.frame_ap(tp, det, ngt, order=order, ap=apv, ntp=ntp))]
for rnd in range(3):
    for name, fn in ARMS:
        say(f"round {rnd + 1}  {name:<32s} {timed(fn):9.3f} ms / launch")
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    r = fm.result()
    say(f"round {rnd + 1}  {'DeviceFrameMAP.result()':<32s} {(time.perf_counter() - t0) * 1e3:9.3f} ms (host clock, ends in the read-back)")
del order, scores, tp, det

if not args.no_forward:
    S, T = 224, 16
    cfg = x.get_config("M", ["TEST.NUM_SPATIAL_CROPS", 1, "TEST.NUM_TEMPORAL_VIEWS", 1, "DETECTION.ENABLE", True,
                             "DETECTION.MAX_BOXES", K, "NETWORK.NUM_CLASSES", C, "DATA.MULTI_LABEL", True])
    model = X3D(cfg, dtype=torch.bfloat16, device=dev, seed=0)
    g = torch.Generator(device=dev).manual_seed(3000)
    for B in (int(cfg.TEST.BATCH_SIZE), 64):
        clips = torch.randn((B, T, S, S, 3), generator=g, device=dev).to(torch.bfloat16)
        _, bx, nbx, gtb, gtl, ngx = synth(B, 2001 + B)
        h_boxes, h_nb = bx.cpu(), nbx.cpu()                     # the model takes num_boxes from the host
        probs = model(clips, boxes=h_boxes, num_boxes=h_nb).reshape(B * K, C).float()
        torch.cuda.synchronize()
        say(f"batch level: X3D-M, DETECTION.ENABLE, {B} x {T} x {S}^2, bf16, one view, K = {K}: the inference forward against "
            f"DeviceFrameMAP.update of its {B * K} rows (G = {G}, C = {C}; boxes and counts from the host) and against the bare "
            "x3d_frame_match launch on device tensors; 20 calls between device events after 3 warm-up calls; three alternating rounds")
        host = [t.cpu() for t in (bx, nbx, gtb, gtl, ngx)]
        o_tp, o_det, o_ngt = ops.frame_match(probs, bx, nbx, gtb, gtl, ngx)

        meter = DeviceFrameMAP()                               # one object, as in a validation loop: its counters and slot index exist

        def update(inputs):
            meter.update(probs, *inputs)
            meter._scores.clear()                               # (the timed calls must not grow what result() would concatenate)
            meter._tp.clear()
        arms = [("forward", lambda: model(clips, boxes=h_boxes, num_boxes=h_nb)),
                ("DeviceFrameMAP.update", lambda: update(host)),
                ("update, device inputs", lambda: update((bx, nbx, gtb, gtl, ngx))),      # no host-to-device copies
                ("x3d_frame_match", lambda: ops.frame_match(probs, bx, nbx, gtb, gtl, ngx, tp=o_tp, det_scores=o_det, ngt=o_ngt))]
        for rnd in range(3):
            ms = {name: timed(fn, reps=20, warm=3) for name, fn in arms}
            say(f"round {rnd + 1}  batch {B:3d}  forward {ms['forward']:8.3f} ms   update {ms['DeviceFrameMAP.update'] * 1e3:8.1f} us "
                f"({100.0 * ms['DeviceFrameMAP.update'] / ms['forward']:5.2f} % of the forward)   update, device inputs "
                f"{ms['update, device inputs'] * 1e3:7.1f} us   launch "
                f"{ms['x3d_frame_match'] * 1e3:7.1f} us ({100.0 * ms['x3d_frame_match'] / ms['forward']:5.2f} %)")
        del clips
