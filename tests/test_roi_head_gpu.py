"""x3d_roi_pool_fwd / x3d_roi_pool_bwd on the GPU against tests/roi_ref.py (fp64), the degenerate form against the classification
head's own launches, and the detection head at model and trainer level.

Inputs are drawn in fp32 and pre-rounded to the storage dtype, boxes lie on the 1/8-pixel grid and spatial_scale is 1/32, so
kernel and reference see the same geometry and only the fp32 accumulation separates them.

Bounds (derived, not fitted).  u = 2^-24, the fp32 unit roundoff.
  forward: a pooled value is a mean of gh*gw samples of four products each, of a map that is a mean over T of relu(s*x + t):
      |err| <= 4 * (T + 4*gh*gw + 8) * u * max|term|,  max|term| = max over the plane of |s*x| + |t|
      (a relu value is bounded by it, and so is the rounding of s*x + t where the two cancel).
  backward: dM/T sums K boxes of dpooled * weight (weight <= 1) the same way, so max|term| = sum_k |dpooled[k][c]| / T, and the stored
      g is that value rounded to the storage dtype: one unit in the last place of the dtype on top.
  sums: 256 threads add 4 * VEC products each and meet in a 6-step wave tree and a 4-term sum: 15 roundings, < 1e-6 of sum |terms|."""
import itertools

import numpy as np
import pytest
import torch

from tests import roi_ref
from x3d_tf_amd import hip, ops

pytestmark = pytest.mark.gpu

U = 2.0 ** -24
SCALE = 1.0 / 32
DTYPES = [torch.float32, torch.bfloat16, torch.float16]
SHAPES = [(1, 1, 1), (4, 7, 7), (3, 5, 3), (2, 8, 10), (1, 32, 32)]
COMBOS = list(itertools.product([1, 3, 24], [1, 3], [1, 2, 7], [0, 2]))    # C, K, R, sampling_ratio


def _ulp(v, dtype):
    """unit in the last place of |v| in dtype (fp64 tensor in, fp64 out)"""
    mant, emin = {torch.float32: (23, -126), torch.bfloat16: (7, -126), torch.float16: (10, -14)}[dtype]
    e = torch.floor(torch.log2(v.abs().clamp_min(2.0 ** -140))).clamp_min(emin)
    return torch.exp2(e - mant)


def _draw(c, t, h, w, dtype, seed, n=2):
    """x rounded to the storage dtype; scale_shift with t well above the noise of s*x so that few s*x + t sit at zero"""
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(n, c, t, h, w, generator=g).to(dtype)
    ss = torch.stack([(0.5 + torch.rand(c, generator=g)) * torch.where(torch.rand(c, generator=g) < 0.25, -1.0, 1.0),
                      0.25 + torch.rand(c, generator=g)], dim=1).contiguous()
    return x, ss


def _num_boxes(i, k):
    return [k, 0] if i % 2 == 0 else [k - 1, k]


def _counts(boxes, num_boxes, h, w, r, sr):
    """gh*gw per row (0 for an empty slot)"""
    n, k = boxes.shape[:2]
    out = np.zeros(n * k)
    for a in range(n):
        for b in range(k):
            geom = roi_ref.box_geometry(boxes[a, b], b < num_boxes[a], SCALE, h, w, r, sr)
            if geom is not None:
                out[a * k + b] = geom[4] * geom[5]
    return out


def _run_fwd(gpu, x, ss, boxes, nb, r, sr, with_argmax=True):
    n, c = x.shape[:2]
    k = boxes.shape[1]
    pooled = torch.full((n * k, c), 7.0, device=gpu)
    argmax = torch.full((n * k, c), 255, dtype=torch.uint8, device=gpu) if with_argmax else None
    ops.roi_pool_fwd(x.to(gpu), ss.to(gpu), torch.from_numpy(boxes).to(gpu), torch.tensor(nb, dtype=torch.int32, device=gpu),
                     pooled, argmax, resolution=r, sampling_ratio=sr, spatial_scale=SCALE)
    return pooled, argmax


def _run_bwd(gpu, dp, argmax, x, ss, boxes, nb, r, sr):
    c = x.shape[1]
    g = torch.full(x.shape, 3.0, dtype=x.dtype, device=gpu)
    sums = torch.zeros(c, 2, dtype=torch.float64, device=gpu)
    ops.roi_pool_bwd(dp.to(gpu), argmax, torch.from_numpy(boxes).to(gpu), torch.tensor(nb, dtype=torch.int32, device=gpu),
                     x.to(gpu), ss.to(gpu), g, sums, resolution=r, sampling_ratio=sr, spatial_scale=SCALE)
    return g, sums


@pytest.mark.parametrize("thw", SHAPES, ids=lambda s: "x".join(map(str, s)))
@pytest.mark.parametrize("dtype", DTYPES, ids=lambda d: str(d).split(".")[-1])
def test_parity(gpu, dtype, thw):
    """forward against roi_ref, the kernel's argmax within the bound of the reference maximum, and the backward teacher-forced on
    the kernel's argmax, for every (C, K, R, sampling_ratio)"""
    t, h, w = thw
    ambiguous = total = 0
    for i, (c, k, r, sr) in enumerate(COMBOS):
        x, ss = _draw(c, t, h, w, dtype, seed=1000 + i)
        boxes = roi_ref.box_mix(2, k, 32 * h, 32 * w, seed=i, first_kind=i)
        nb = _num_boxes(i, k)
        what = f"C={c} K={k} R={r} sr={sr} num_boxes={nb}"
        pooled, argmax = _run_fwd(gpu, x, ss, boxes, nb, r, sr)
        xn, ssn = x.double().numpy(), ss.double().numpy()
        ref_pooled, ref_bins, _, valid = roi_ref.forward(xn, ssn, boxes, nb, r, sr, SCALE)
        cnt = _counts(boxes, nb, h, w, r, sr)
        term = (np.abs(ssn[None, :, 0, None, None, None] * xn) + np.abs(ssn[None, :, 1, None, None, None])).max(axis=(2, 3, 4))  # [N][C]
        bound = 4 * (t + 4 * cnt[:, None] + 8) * U * np.repeat(term, k, axis=0)                                                 # [N*K][C]
        got, am = pooled.cpu().double().numpy(), argmax.cpu().numpy().astype(np.int64)
        err = np.abs(got - ref_pooled)
        print(f"{what}: fwd max err / bound = {(err / bound).max():.3f}")
        assert (err <= bound).all(), f"{what}: pooled off by {err.max():.3e} (bound {bound[err > bound].min():.3e})"
        assert (got[~valid] == 0).all() and (am[~valid] == 0).all(), f"{what}: an empty slot is not zero"
        assert (am < r * r).all()
        at_kernel = np.take_along_axis(ref_bins, am[:, :, None], axis=2)[:, :, 0]
        assert (at_kernel >= ref_pooled - bound)[valid].all(), f"{what}: the kernel's argmax is not a maximal bin"
        # backward, teacher-forced
        dp = torch.randn(2 * k, c, generator=torch.Generator().manual_seed(2000 + i))
        g, sums = _run_bwd(gpu, dp, argmax, x, ss, boxes, nb, r, sr)
        ref_g, z = roi_ref.backward(dp.double().numpy(), am, boxes, nb, xn, ssn, r, sr, SCALE)
        ref_g, z = torch.from_numpy(ref_g), torch.from_numpy(z)
        dpa = dp.double().abs().view(2, k, c) * torch.from_numpy(valid).view(2, k, 1)
        bterm = (dpa.sum(1) / t).view(2, c, 1, 1, 1)
        bbound = 4 * (k + 4 * float(cnt.max()) + 8) * U * bterm
        unmasked = torch.where(z > 0, ref_g, torch.zeros_like(ref_g))
        full = torch.from_numpy(roi_ref.backward(dp.double().numpy(), am, boxes, nb, xn, np.stack([0 * ssn[:, 0], 1 + 0 * ssn[:, 1]], 1),
                                                 r, sr, SCALE)[0])          # the gradient with every ReLU open
        gd = g.cpu().double()

        def close(ref):
            rr = ref.float().to(dtype).double()
            return (gd - rr).abs() <= _ulp(rr, dtype) + bbound

        amb = z.abs() <= 2.0 ** -20 * torch.from_numpy(ssn[:, 1]).abs().view(1, c, 1, 1, 1)
        ok = torch.where(amb, close(full) | (gd == 0), close(unmasked))
        ambiguous += int(amb.sum())
        total += amb.numel()
        assert ok.all(), f"{what}: {int((~ok).sum())} of {ok.numel()} elements of g out of bound, first {torch.nonzero(~ok)[0].tolist()}"
        yd = x.double()
        own = torch.stack([gd.sum(dim=(0, 2, 3, 4)), (gd * yd).sum(dim=(0, 2, 3, 4))], 1)
        scale = torch.stack([gd.abs().sum(dim=(0, 2, 3, 4)), (gd * yd).abs().sum(dim=(0, 2, 3, 4))], 1)
        assert ((sums.cpu() - own).abs() <= 1e-6 * scale).all(), f"{what}: sums {sums.cpu()} vs {own}"
    assert ambiguous < 0.01 * total, f"{ambiguous} of {total} elements within 2^-20 |t| of the ReLU's zero"


@pytest.mark.parametrize("thw", [(4, 7, 7), (2, 8, 10)], ids=lambda s: "x".join(map(str, s)))
@pytest.mark.parametrize("dtype", DTYPES, ids=lambda d: str(d).split(".")[-1])
def test_degenerate_form_is_the_old_head(gpu, dtype, thw):
    """R = 1, sampling_ratio = 0, K = 1, every box the full frame: the samples land on the pixel centres and the two launches are
    x3d_pool_fwd and x3d_relu_bn_bwd_reduce(dpool) up to the order of the fp32 sums"""
    t, h, w = thw
    c, n, p = 24, 2, t * h * w
    x, ss = _draw(c, t, h, w, dtype, seed=5)
    boxes = np.tile(np.array([0, 0, 32 * w, 32 * h], dtype=np.float32), (n, 1, 1))
    pooled, argmax = _run_fwd(gpu, x, ss, boxes, [1, 1], 1, 0)
    old = ops.pool_fwd(x.to(gpu), ss.to(gpu), torch.empty(n, c, device=gpu))
    assert ((pooled.double() - old.double()).abs() <= p * U * old.double().abs()).all()
    dp = torch.randn(n, c, generator=torch.Generator().manual_seed(6))
    g, sums = _run_bwd(gpu, dp, argmax, x, ss, boxes, [1, 1], 1, 0)
    g_old = torch.empty_like(g)
    sums_old = torch.zeros_like(sums)
    ops.relu_bn_bwd_reduce(None, dp.to(gpu), x.to(gpu), ss.to(gpu), g_old, sums_old)
    gd, god = g.double(), g_old.double()
    assert ((gd - god).abs() <= _ulp(god, dtype)).all()
    scale = torch.stack([god.abs().sum(dim=(0, 2, 3, 4)), (god * x.to(gpu).double()).abs().sum(dim=(0, 2, 3, 4))], 1)
    # (the stored g may differ by a unit in the last place: the sums of p such values by that share, plus the 1e-6 of their order)
    ulp_rel = {torch.float32: 2.0 ** -23, torch.bfloat16: 2.0 ** -7, torch.float16: 2.0 ** -10}[dtype]
    assert ((sums - sums_old).abs() <= (ulp_rel + 2e-6) * scale).all()


@pytest.mark.parametrize("dtype", DTYPES, ids=lambda d: str(d).split(".")[-1])
def test_reproducible(gpu, dtype):
    x, ss = _draw(24, 4, 7, 7, dtype, seed=9)
    boxes = roi_ref.box_mix(2, 3, 224, 224, seed=3)
    runs = []
    for _ in range(2):
        pooled, argmax = _run_fwd(gpu, x, ss, boxes, [3, 2], 7, 0)
        dp = torch.randn(6, 24, generator=torch.Generator().manual_seed(4))
        g, _ = _run_bwd(gpu, dp, argmax, x, ss, boxes, [3, 2], 7, 0)
        runs.append((pooled.cpu(), argmax.cpu(), g.cpu()))
    for a, b in zip(*runs):
        assert torch.equal(a.view(torch.uint8), b.view(torch.uint8))


def test_outputs_left_alone(gpu):
    """argmax == NULL is not written (guard bytes on both sides of pooled stay), and a refused call writes nothing"""
    x, ss = _draw(3, 4, 7, 7, torch.float32, seed=11)
    boxes = roi_ref.box_mix(2, 3, 224, 224, seed=5)
    d_boxes, d_nb = torch.from_numpy(boxes).to(gpu), torch.tensor([3, 1], dtype=torch.int32, device=gpu)
    guard = 64
    buf = torch.full((guard + 6 * 3 + guard,), -5.0, device=gpu)
    pooled = buf[guard:guard + 18].view(6, 3)
    ops.roi_pool_fwd(x.to(gpu), ss.to(gpu), d_boxes, d_nb, pooled, None, resolution=2, sampling_ratio=2, spatial_scale=SCALE)
    ref, _, _, _ = roi_ref.forward(x.double().numpy(), ss.double().numpy(), boxes, [3, 1], 2, 2, SCALE)
    assert (buf[:guard] == -5.0).all() and (buf[guard + 18:] == -5.0).all()
    assert np.abs(pooled.cpu().double().numpy() - ref).max() < 1e-4
    # refused by the library itself (the wrapper's own checks bypassed): R = 16, then H*W > 1024
    xg, sg = x.to(gpu), ss.to(gpu)
    am = torch.full((6, 3), 9, dtype=torch.uint8, device=gpu)
    before = buf.clone()
    g = torch.full(x.shape, 3.0, device=gpu)
    sums = torch.full((3, 2), 2.0, dtype=torch.float64, device=gpu)
    for (hh, ww, r) in ((7, 7, 16), (7, 7, 0), (33, 32, 7)):
        with pytest.raises(hip.X3DHipError):
            hip.call("x3d_roi_pool_fwd", xg.data_ptr(), sg.data_ptr(), d_boxes.data_ptr(), d_nb.data_ptr(), pooled.data_ptr(),
                     am.data_ptr(), 2, 3, 4, hh, ww, 3, r, 0, SCALE, hip.F32)
        with pytest.raises(hip.X3DHipError):
            hip.call("x3d_roi_pool_bwd", pooled.data_ptr(), am.data_ptr(), d_boxes.data_ptr(), d_nb.data_ptr(), xg.data_ptr(),
                     sg.data_ptr(), g.data_ptr(), sums.data_ptr(), 2, 3, 4, hh, ww, 3, r, 0, SCALE, hip.F32)
    torch.cuda.synchronize()
    assert torch.equal(buf, before) and (am == 9).all() and (g == 3.0).all() and (sums == 2.0).all()


# ---- model level ------------------------------------------------------------------------------------------------------------
BASE = ["DATA.TEMP_DURATION", 4, "TEST.NUM_SPATIAL_CROPS", 1, "TEST.NUM_TEMPORAL_VIEWS", 1, "NETWORK.NUM_CLASSES", 11]
KB = 3
DET = ["DETECTION.ENABLE", True, "DETECTION.MAX_BOXES", KB]


def _setup(over):
    import x3d_tf_amd as x
    from x3d_tf_amd.params import init_params, randomize_bn_
    cfg = x.get_config("XS", BASE + over)
    arch = x.build_arch(cfg)
    return cfg, arch, randomize_bn_(init_params(arch, seed=3), seed=4)


def _model(cfg, params, gpu):
    from x3d_tf_amd.model import X3D
    m = X3D(cfg, dtype=torch.float32, device=gpu, seed=0)
    m.load_state_dict(params)
    return m


def _clip_boxes(n, size, seed):
    """boxes [n][KB][4] in pixels of a size x size clip: an inside box, a box beyond the frame, the full frame"""
    return roi_ref.box_mix(n, KB, size, size, seed=seed)[:, :, :].copy()


def _rel_l2(a, b):
    return float((a.double() - b.double()).norm() / b.double().norm().clamp_min(1e-30))


@pytest.mark.parametrize("multi", [False, True], ids=["softmax", "sigmoid"])
def test_model_step_matches_the_head_restated_in_fp64(gpu, multi):
    """one forward_backward of the XS model with boxes: the trunk is the plan's own (c5_raw, bn5.ss), the head -- roi_ref pooling on
    the kernel's argmax, fc1, dropout, fc2, the loss as a mean over the valid boxes -- is restated in torch fp64; limits as the
    existing head tests' (loss 1e-5, probabilities 1e-4, dlogits 1e-6 of their maximum, gradients 1e-3 relative L2)"""
    cfg, arch, params = _setup(DET + (["DATA.MULTI_LABEL", True] if multi else []))
    n, t, s, classes = 2, 4, 64, arch.num_classes
    rows = n * KB
    g = torch.Generator().manual_seed(1)
    clips = torch.randn(n, t, s, s, 3, generator=g)
    boxes = _clip_boxes(n, s, seed=2)
    nb = [2, 0]
    valid = torch.tensor([1, 1, 0, 0, 0, 0], dtype=torch.bool)
    if multi:
        labels = (torch.rand(n, KB, classes, generator=g) < 0.3).float()
    else:
        labels = torch.randint(0, classes, (n, KB), generator=g)
        labels[1, 2] = -5                                   # an empty slot's label is not used
    mask = (torch.rand(rows, arch.fc1_out, generator=g) >= arch.dropout_rate).float()
    m = _model(cfg, params, gpu)
    m.set_dropout_mask(mask)
    pl = m.forward_backward(clips.to(gpu), labels, boxes=torch.from_numpy(boxes), num_boxes=nb)
    torch.cuda.synchronize()
    assert pl.rows == rows and tuple(pl.pooled.shape) == (rows, arch.conv5_out) and tuple(pl.dlogits.shape) == (rows, classes)
    c5, ss = pl.c5_raw.cpu().double().numpy(), pl.bn5.ss.cpu().double().numpy()
    am = pl.roi_argmax.cpu().numpy().astype(np.int64)
    h5 = s // 32
    _, bins, _, ref_valid = roi_ref.forward(c5, ss, boxes, nb, 7, 0, SCALE)
    assert ref_valid.tolist() == valid.tolist()
    pooled = torch.from_numpy(np.take_along_axis(bins, am[:, :, None], 2)[:, :, 0]).requires_grad_(True)
    assert (pl.pooled.cpu().double() - pooled.detach()).abs().max().item() <= 1e-4
    w1 = params["fc1/kernel"].double().reshape(arch.fc1_out, arch.conv5_out).requires_grad_(True)
    w2 = params["fc2/kernel"].double().reshape(classes, arch.fc1_out).requires_grad_(True)
    b2 = params["fc2/bias"].double().requires_grad_(True)
    scale = 1.0 / (1.0 - arch.dropout_rate) if arch.dropout_rate > 0 else 1.0
    z = (torch.relu(pooled @ w1.T) * (mask.double() * scale if arch.dropout_rate > 0 else 1.0)) @ w2.T + b2
    z.retain_grad()
    if multi:
        per_row = (z.clamp(min=0) - z * labels.double().view(rows, classes) + torch.log1p(torch.exp(-z.abs()))).mean(1)
        probs = torch.sigmoid(z)
    else:
        per_row = torch.nn.functional.cross_entropy(z, labels.view(rows).clamp(min=0), reduction="none")
        probs = torch.softmax(z, 1)
    loss = per_row[valid].sum() / int(valid.sum())
    loss.backward()
    got_loss = pl.loss_rows.double().sum().item() / rows
    print(f"loss {got_loss} vs {loss.item()}")
    assert abs(got_loss - loss.item()) <= 1e-5
    assert (pl.probs.cpu().double() - probs.detach()).abs().max().item() <= 1e-4
    dl = pl.dlogits.cpu().double()
    assert (dl - z.grad).abs().max().item() <= 1e-6 * z.grad.abs().max().item() + 1e-30
    assert (dl[~valid] == 0).all() and (dl[:2] != 0).any()
    for name, ref in (("fc1/kernel", w1.grad), ("fc2/kernel", w2.grad), ("fc2/bias", b2.grad)):
        e = _rel_l2(m.grads[name].cpu().reshape(ref.shape), ref)
        assert e < 1e-3, f"grad {name}: relative L2 error {e:.3e}"
    g5_ref, _ = roi_ref.backward(pooled.grad.numpy(), am, boxes, nb, c5, ss, 7, 0, SCALE)
    g5 = pl.backward.g5.cpu().double()
    assert _rel_l2(g5, torch.from_numpy(g5_ref)) < 1e-3
    assert (g5[1] == 0).all() and h5 == pl.h5               # the sample without boxes sends nothing down
    # call(): [N, K, classes], the empty slots zeroed
    out = m(clips.to(gpu), boxes=torch.from_numpy(boxes), num_boxes=nb)
    torch.cuda.synchronize()
    assert tuple(out.shape) == (n, KB, classes)
    flat = out.reshape(rows, classes).cpu()
    assert (flat[~valid] == 0).all() and (flat[valid] > 0).all() and torch.isfinite(flat).all()
    with pytest.raises(ValueError, match="boxes"):
        m(clips.to(gpu))


def test_switch_off_keeps_the_bits(gpu):
    """DETECTION.ENABLE False and a config without the section: the same logits, bit for bit, and refusal of boxes"""
    import x3d_tf_amd as x
    cfg_off, arch, params = _setup(["DETECTION.ENABLE", False, "DETECTION.MAX_BOXES", KB])
    absent = x.get_config("XS", BASE, freeze=False)
    del absent["DETECTION"]
    clips = torch.randn(2, 4, 64, 64, 3, generator=torch.Generator().manual_seed(3)).to(gpu)
    a = _model(cfg_off, params, gpu).logits(clips).clone()
    b = _model(absent, params, gpu).logits(clips).clone()
    assert torch.equal(a, b) and torch.isfinite(a).all()


def _ap_ref(scores, targets):
    """sklearn's average_precision_score for one class in fp64 (as tests/test_multilabel.py restates it)"""
    s = np.asarray(scores, dtype=np.float64).ravel()
    y = np.asarray(targets, dtype=np.float64).ravel() >= 0.5
    p = int(y.sum())
    if p == 0 or np.isnan(s).any():
        return float("nan")
    order = np.argsort(-s, kind="mergesort")
    s, y = s[order], y[order]
    last = np.r_[np.nonzero(np.diff(s))[0], len(s) - 1]
    tps = np.cumsum(y)[last].astype(np.float64)
    return float(np.sum(np.diff(np.r_[0.0, tps / p]) * (tps / (last + 1))))


def test_trainer_steps_and_validation_over_valid_rows(gpu):
    from x3d_tf_amd.train import Trainer
    cfg, arch, params = _setup(DET + ["DATA.MULTI_LABEL", True, "TRAIN.BATCH_SIZE", 2, "TRAIN.DATASET_SIZE", 4])
    cfg_cls, _, _ = _setup(["DATA.MULTI_LABEL", True, "TRAIN.BATCH_SIZE", 2, "TRAIN.DATASET_SIZE", 4])
    n, t, s, classes = 2, 4, 64, arch.num_classes
    m = _model(cfg, params, gpu)
    tr = Trainer(m, cfg)
    g = torch.Generator().manual_seed(5)
    batches = []
    for i, nb in enumerate(([2, 0], [3, 1])):
        batches.append((torch.randn(n, t, s, s, 3, generator=g).to(gpu), (torch.rand(n, KB, classes, generator=g) < 0.3).float(),
                        torch.from_numpy(_clip_boxes(n, s, seed=10 + i)), torch.tensor(nb)))
    losses = []
    for i in range(3):
        clips, y, bx, nb = batches[i % 2]
        pl = tr.step(clips, y, lr=0.01, boxes=bx, num_boxes=nb)
        losses.append(pl.loss_rows)
    torch.cuda.synchronize()
    assert all(bool(torch.isfinite(l).all()) for l in losses)
    # the step's launch lists are the classification step's but for the two ROI launches: nothing else was added to the replay
    m_cls = _model(cfg_cls, params, gpu)
    pc = m_cls._plan(n, t, s, s, True)
    # (and the head slot, which holds the _w entry point of the same head: the row weights carry the valid-box mean)
    swap = {"x3d_roi_pool_fwd": "x3d_pool_fwd", "x3d_roi_pool_bwd": "x3d_relu_bn_bwd_reduce", "x3d_sigmoid_bce_w": "x3d_sigmoid_bce"}
    for mine, theirs in ((pl.fwd, pc.fwd), (pl.bwd, pc.bwd)):
        assert [swap.get(e[0], e[0]) for e in mine] == [e[0] for e in theirs]
    with pytest.raises(ValueError, match="boxes"):
        tr.step(batches[0][0], batches[0][1], lr=0.01)
    # validate: loss and mAP over the valid rows only, against fp64 from the probabilities call() returns
    r = tr.validate(batches)
    scores, targets = [], []
    for clips, y, bx, nb in batches:
        p = m(clips, boxes=bx, num_boxes=nb).cpu().double().reshape(n * KB, classes)
        keep = (torch.arange(KB).view(1, KB) < nb.view(n, 1)).reshape(-1)
        scores.append(p[keep])
        targets.append(y.reshape(n * KB, classes).double()[keep])
    sc, tg = torch.cat(scores), torch.cat(targets)
    assert r["videos"] == 6 == sc.shape[0]
    q = sc.clamp(1e-7, 1 - 1e-7)
    want_loss = float((-(tg * q.log() + (1 - tg) * (1 - q).log())).mean()) + float(m.regularization_loss().item())
    aps = np.array([_ap_ref(sc[:, c].numpy(), tg[:, c].numpy()) for c in range(classes)])
    want_map = float(np.nanmean(aps))
    print(f"val loss {r['loss']} vs {want_loss}; mAP {r['mAP']} vs {want_map}")
    assert abs(r["loss"] - want_loss) <= 1e-9 * max(1.0, abs(want_loss)) and abs(r["mAP"] - want_map) <= 1e-12
