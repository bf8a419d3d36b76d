"""Soft-target training on the GPU: x3d_softmax_xent_soft / x3d_mix_clips / x3d_mix_targets against fp64 restatements and
torch indexing, the soft-target head of the model against the oracle's autograd, and Trainer.step / fit with mixup, CutMix
and label smoothing."""
import math
import os
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import x3d_tf_amd as x  # noqa: E402
from x3d_tf_amd import dataloader as DL  # noqa: E402
from x3d_tf_amd import hip, ops  # noqa: E402
from x3d_tf_amd.mix import draw_mix_params  # noqa: E402
from util import report  # noqa: E402

F32 = lambda v: float(np.float32(v))     # noqa: E731  (the kernels take lam / eps as float: references use the same value)


def _smooth_rows(labels, m, eps):
    return (1.0 - eps) * torch.nn.functional.one_hot(labels.long(), m).double() + eps / m


def _mixed_rows(labels, m, lam, eps):
    s = _smooth_rows(labels, m, eps)
    return lam * s + (1.0 - lam) * s.flip(0)


def _soft_xent_ref(logits, y, grad_scale):
    """the issue's formula in fp64 autograd, written with torch.clamp (whose gradient mask is the same closed interval)"""
    z = logits.double().requires_grad_(True)
    p = torch.softmax(z, -1)
    q = p.clamp(1e-7, 1 - 1e-7)
    yd = y.double()
    rows = (yd * -torch.log(q)).sum(1) + yd.sum(1) * torch.log(q.sum(1))
    (g,) = torch.autograd.grad(rows.sum() * grad_scale, [z])
    return p.detach(), rows.detach(), g


def _run_soft(gpu, z, y, gs):
    n, m = z.shape
    probs, rows, dl = torch.empty(n, m, device=gpu), torch.empty(n, device=gpu), torch.full((n, m), 7.0, device=gpu)
    ops.softmax_xent_soft(z.to(gpu), y.to(gpu), probs, rows, dl, gs)
    torch.cuda.synchronize()
    return probs, rows, dl


# ---- x3d_softmax_xent_soft --------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("n", [1, 7, 64])
@pytest.mark.parametrize("m", [1, 157, 400])
def test_softmax_xent_soft_matches_fp64(gpu, n, m):
    g = torch.Generator().manual_seed(n * 1000 + m)
    z = torch.randn(n, m, generator=g) * 2
    if m > 5:
        z[0] = 0.0
        z[0, 3] = 40.0                                     # the clipped regime: one logit 40 above the rest
    labels = torch.randint(0, m, (n,), generator=g)
    y = _mixed_rows(labels, m, F32(0.3), F32(0.1)).float()
    gs = 1.0 / n
    probs, rows, dl = _run_soft(gpu, z, y, gs)
    p_ref, r_ref, d_ref = _soft_xent_ref(z, y, gs)
    print(f"n={n} m={m}: probs {(probs.cpu().double() - p_ref).abs().max():.3e} loss "
          f"{(rows.cpu().double() - r_ref).abs().max():.3e} dlogits {(dl.cpu().double() - d_ref).abs().max():.3e}")
    report("probs", probs, p_ref, 1e-5, 1e-7)
    report("loss_rows", rows, r_ref, 1e-4, 1e-4)
    report("dlogits", dl, d_ref, 1e-3, 1e-6)


@pytest.mark.gpu
@pytest.mark.parametrize("n, m", [(7, 157), (64, 400), (3, 1)])
def test_softmax_xent_soft_one_hot_is_the_hard_loss(gpu, n, m):
    g = torch.Generator().manual_seed(n + m)
    z = torch.randn(n, m, generator=g) * 3
    labels = torch.randint(0, m, (n,), generator=g, dtype=torch.int32)
    y = torch.nn.functional.one_hot(labels.long(), m).float()
    gs = 0.37
    probs, rows, dl = _run_soft(gpu, z, y, gs)
    p0, r0, d0 = torch.empty(n, m, device=gpu), torch.empty(n, device=gpu), torch.empty(n, m, device=gpu)
    ops.softmax_xent(z.to(gpu), labels.to(gpu), p0, r0, d0, gs)
    torch.cuda.synchronize()
    assert torch.equal(probs, p0)                          # bit-identical
    report("loss_rows", rows, r0, 1e-4, 1e-4)
    report("dlogits", dl, d0, 1e-3, 1e-6)


@pytest.mark.gpu
def test_softmax_xent_soft_nan_rows_probs_only_and_refusal(gpu):
    n, m = 5, 157
    g = torch.Generator().manual_seed(7)
    z = torch.randn(n, m, generator=g)
    y = _mixed_rows(torch.randint(0, m, (n,), generator=g), m, 0.25, 0.0).float()
    y[2, 17] = float("nan")
    probs, rows, dl = _run_soft(gpu, z, y, 1.0)
    assert math.isnan(rows[2].item()) and bool(torch.isfinite(rows[[0, 1, 3, 4]]).all())
    assert dl[2].abs().sum().item() == 0 and bool(torch.isfinite(dl).all())
    assert all(dl[i].abs().sum().item() > 0 for i in (0, 1, 3, 4))
    p2 = torch.empty(n, m, device=gpu)
    ops.softmax_xent_soft(z.to(gpu), None, p2)
    torch.cuda.synchronize()
    assert torch.equal(p2, probs)
    with pytest.raises(ValueError):
        ops.softmax_xent_soft(z.to(gpu), None, p2, loss_rows=rows)
    with pytest.raises(hip.X3DHipError):
        hip.call("x3d_softmax_xent_soft", p2.data_ptr(), None, p2.data_ptr(), rows.data_ptr(), None, 1.0, n, m)


# ---- x3d_mix_clips ----------------------------------------------------------------------------------------------------
SHAPES = [(5, 3, 18, 22, 3), (2, 4, 64, 64, 3), (8, 13, 160, 160, 3)]
HEADLINE = (64, 16, 224, 224, 3)
DTYPES = {"fp32": torch.float32, "bf16": torch.bfloat16, "fp16": torch.float16}
CASES = [(s, d) for s in SHAPES for d in DTYPES] + [(HEADLINE, "bf16")]
STORAGE = {torch.float32: (23, -126), torch.bfloat16: (7, -126), torch.float16: (10, -14)}    # mantissa bits, min exponent


def _clips(shape, dtype, gpu, seed=0):
    g = torch.Generator(device=gpu).manual_seed(seed)
    n = shape[0]
    per = math.prod(shape[1:])
    out = torch.empty(shape, dtype=dtype, device=gpu)
    for i in range(n):                                     # clip by clip: the headline batch is 154 M elements
        out[i] = (torch.randn(per, generator=g, device=gpu) * 2).view(shape[1:]).to(dtype)
    return out


def _boxes(h, w):
    return [(0, 0, 0, 0), (3, 3, 0, w), (h // 2, h // 2 + 1, w // 3, w // 3 + 1), (0, h, 0, w), (0, h // 2, 0, w // 2),
            (h // 3, h, w // 2, w), (1, h - 1, 1, w - 1), (0, h, 1, w - 2), (2, h - 3, 0, w)]


@pytest.mark.gpu
@pytest.mark.parametrize("shape, dt", CASES, ids=[f"{'x'.join(map(str, s))}-{d}" for s, d in CASES])
@pytest.mark.parametrize("inplace", [False, True], ids=["out", "inplace"])
def test_cutmix_is_the_indexing_swap(gpu, shape, dt, inplace):
    a = _clips(shape, DTYPES[dt], gpu)
    h, w = shape[2], shape[3]
    boxes = _boxes(h, w) if shape != HEADLINE else [(h // 4, h // 4 + h // 2, w // 4 + 1, w // 4 + 1 + w // 2)]
    for (y0, y1, x0, x1) in boxes:
        src = a.clone()
        out = src if inplace else torch.full_like(a, 9.0)
        got = ops.mix_clips(src, "cutmix", 0.5, (y0, y1, x0, x1), out=out)
        torch.cuda.synchronize()
        assert got is out
        want = a.clone()
        want[:, :, y0:y1, x0:x1] = a.flip(0)[:, :, y0:y1, x0:x1]
        assert torch.equal(got.view(torch.uint8), want.view(torch.uint8)), (y0, y1, x0, x1)
        if inplace:                                        # outside the box nothing moved
            keep = torch.ones(h, w, dtype=torch.bool, device=gpu)
            keep[y0:y1, x0:x1] = False
            assert torch.equal(got[:, :, keep], a[:, :, keep])
        else:
            assert torch.equal(src, a)                     # the input is read only
        del src, out, got, want


def _mixup_check(a, got, lam):
    mant, emin = STORAGE[a.dtype]
    n = a.shape[0]
    worst = -math.inf
    for i in range(n):
        j = n - 1 - i
        if i == j:
            assert torch.equal(got[i].view(torch.uint8), a[i].view(torch.uint8))     # the middle clip: bit-identical
            continue
        ai, bj = a[i].double(), a[j].double()
        ref = lam * ai + (1.0 - lam) * bj
        ex = torch.frexp(ref)[1].double() - 1              # floor(log2 |ref|)
        half_ulp = torch.exp2(ex.clamp(min=emin) - mant - 1)
        bound = half_ulp + 2.0 ** -22 * ((lam * ai).abs() + ((1.0 - lam) * bj).abs())
        excess = ((got[i].double() - ref).abs() - bound).max().item()
        worst = max(worst, excess)
    return worst


@pytest.mark.gpu
@pytest.mark.parametrize("shape, dt", CASES, ids=[f"{'x'.join(map(str, s))}-{d}" for s, d in CASES])
@pytest.mark.parametrize("inplace", [False, True], ids=["out", "inplace"])
def test_mixup_within_half_an_ulp_of_fp64(gpu, shape, dt, inplace):
    a = _clips(shape, DTYPES[dt], gpu, seed=1)
    for lam in ([F32(0.3)] if shape == HEADLINE else [F32(0.3), F32(0.8157), 0.5]):
        src = a.clone()
        out = src if inplace else torch.full_like(a, 9.0)
        got = ops.mix_clips(src, "mixup", lam, out=out)
        torch.cuda.synchronize()
        worst = _mixup_check(a, got, lam)
        print(f"{shape} {dt} lam={lam}: worst error minus bound {worst:.3e}")
        assert worst <= 0.0
        if not inplace:
            assert torch.equal(src, a)
        del src, out, got
    if shape == HEADLINE:
        return
    for lam, want in ((1.0, a), (0.0, a.flip(0))):         # the input / the reversed batch, bit for bit
        src = a.clone()
        got = ops.mix_clips(src, "mixup", lam, out=src if inplace else torch.full_like(a, 9.0))
        torch.cuda.synchronize()
        assert torch.equal(got.view(torch.uint8), want.contiguous().view(torch.uint8)), lam


@pytest.mark.gpu
def test_mix_clips_unaligned_views(gpu):
    """batches that start on any element of an allocation (2-byte / 4-byte aligned only)"""
    for dt in DTYPES.values():
        shape = (4, 2, 9, 11, 3)
        per = math.prod(shape)
        base = torch.randn(per + 3, device=gpu).to(dt)
        a = base[3:].view(shape)
        assert a.data_ptr() % 16 != 0
        got = ops.mix_clips(a, "mixup", 0.25)
        torch.cuda.synchronize()
        assert _mixup_check(a, got, 0.25) <= 0.0
        got = ops.mix_clips(a, "cutmix", 0.25, (2, 7, 3, 10))
        want = a.clone()
        want[:, :, 2:7, 3:10] = a.flip(0)[:, :, 2:7, 3:10]
        torch.cuda.synchronize()
        assert torch.equal(got, want)


@pytest.mark.gpu
def test_mix_clips_refusals_leave_out_unwritten(gpu):
    shape = (4, 2, 8, 8, 3)
    n, t, h, w, c = shape
    a = torch.randn(shape, device=gpu)
    out = torch.full(shape, 9.0, device=gpu)
    flat = torch.zeros(2 * a.numel(), device=gpu)
    A, O_ = a.data_ptr(), out.data_ptr()
    mu, cm, f32 = hip.MIX_MIXUP, hip.MIX_CUTMIX, hip.F32
    bad = [
        (None, O_, mu, 0.5, 0, 0, 0, 0, n, t, h, w, c, f32), (A, None, mu, 0.5, 0, 0, 0, 0, n, t, h, w, c, f32),
        (A, O_, mu, 0.5, 0, 0, 0, 0, 0, t, h, w, c, f32), (A, O_, mu, 0.5, 0, 0, 0, 0, n, -1, h, w, c, f32),
        (A, O_, mu, 0.5, 0, 0, 0, 0, n, t, 0, w, c, f32), (A, O_, mu, 0.5, 0, 0, 0, 0, n, t, h, 0, c, f32),
        (A, O_, mu, 0.5, 0, 0, 0, 0, n, t, h, w, 0, f32),
        (A, O_, cm, 0.5, -1, 4, 0, 4, n, t, h, w, c, f32), (A, O_, cm, 0.5, 0, h + 1, 0, 4, n, t, h, w, c, f32),
        (A, O_, cm, 0.5, 0, 4, 2, w + 1, n, t, h, w, c, f32), (A, O_, cm, 0.5, 5, 4, 0, 4, n, t, h, w, c, f32),
        (A, O_, cm, 0.5, 0, 4, 6, 5, n, t, h, w, c, f32),
        (A, O_, mu, -0.01, 0, 0, 0, 0, n, t, h, w, c, f32), (A, O_, mu, 1.01, 0, 0, 0, 0, n, t, h, w, c, f32),
        (A, O_, mu, float("nan"), 0, 0, 0, 0, n, t, h, w, c, f32), (A, O_, cm, float("inf"), 0, 4, 0, 4, n, t, h, w, c, f32),
        (A, O_, mu, 0.5, 0, 0, 0, 0, n, t, h, w, c, 3), (A, O_, 0, 0.5, 0, 0, 0, 0, n, t, h, w, c, f32),
    ]
    for args in bad:
        with pytest.raises(hip.X3DHipError):
            hip.call("x3d_mix_clips", *args)
    # out overlapping x without being equal to it (one element, one clip apart)
    flat[:a.numel()] = a.flatten()
    before = flat.clone()
    for shift in (1, a.numel() // n, a.numel() - 1):
        with pytest.raises(hip.X3DHipError, match="overlaps"):
            hip.call("x3d_mix_clips", flat.data_ptr(), flat.data_ptr() + 4 * shift, mu, 0.5, 0, 0, 0, 0, n, t, h, w, c, f32)
        with pytest.raises(hip.X3DHipError, match="overlaps"):
            hip.call("x3d_mix_clips", flat.data_ptr() + 4 * shift, flat.data_ptr(), cm, 0.5, 0, 4, 0, 4, n, t, h, w, c, f32)
    torch.cuda.synchronize()
    assert bool((out == 9.0).all()) and torch.equal(flat, before)
    with pytest.raises(ValueError):
        ops.mix_clips(a, "mosaic", 0.5)
    with pytest.raises(ValueError):
        ops.mix_clips(a, "mixup", 0.5, out=out.to(torch.bfloat16))


# ---- x3d_mix_targets --------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("n, m", [(1, 1), (2, 5), (7, 157), (64, 400)])
def test_mix_targets_single_label(gpu, n, m):
    g = torch.Generator().manual_seed(n + m)
    labels = torch.randint(0, m, (n,), generator=g, dtype=torch.int32)
    for lam, eps in ((F32(0.3), F32(0.1)), (0.5, 0.0), (F32(0.7), 0.0), (1.0, F32(0.1)), (0.0, F32(0.2)), (F32(0.49999), 0.0)):
        hard = torch.full((n,), -7, dtype=torch.int32, device=gpu)
        y = ops.mix_targets(labels.to(gpu), m, lam, eps, hard=hard)
        torch.cuda.synchronize()
        want = _mixed_rows(labels, m, lam, eps)
        assert (y.cpu().double() - want).abs().max().item() <= 1e-7
        assert (y.cpu().double().sum(1) - 1.0).abs().max().item() <= 1e-7
        assert torch.equal(hard.cpu(), labels if lam >= 0.5 else labels.flip(0)), (lam, eps)
    # hard is optional
    y2 = ops.mix_targets(labels.to(gpu), m, 0.5, 0.0)
    torch.cuda.synchronize()
    assert (y2.cpu().double() - _mixed_rows(labels, m, 0.5, 0.0)).abs().max().item() <= 1e-7


@pytest.mark.gpu
def test_mix_targets_out_of_range_label_gives_two_nan_rows(gpu):
    n, m = 7, 17
    labels = torch.tensor([0, 99, 3, 5, 2, 16, 4], dtype=torch.int32)           # row 1 and its partner, row 5
    y = ops.mix_targets(labels.to(gpu), m, 0.25, 0.1)
    torch.cuda.synchronize()
    nan_rows = torch.isnan(y).all(1).cpu()
    assert nan_rows.tolist() == [False, True, False, False, False, True, False]
    assert bool(torch.isfinite(y[~nan_rows.to(gpu)]).all())
    labels[1] = -1
    y = ops.mix_targets(labels.to(gpu), m, 1.0, 0.0)
    torch.cuda.synchronize()
    assert torch.isnan(y).all(1).cpu().tolist() == [False, True, False, False, False, True, False]
    # the loss is then visibly non-finite, the rows contribute no gradient
    probs, rows, dl = _run_soft(gpu, torch.randn(n, m), y.cpu(), 1.0)
    assert torch.isnan(rows).cpu().tolist() == nan_rows.tolist() and bool(torch.isfinite(dl).all())


@pytest.mark.gpu
@pytest.mark.parametrize("n, m", [(1, 3), (4, 157), (7, 157)])
def test_mix_targets_multi_label_in_place(gpu, n, m):
    g = torch.Generator().manual_seed(n * m)
    t = (torch.rand(n, m, generator=g) < 0.1).float()
    t[0, :3] = torch.tensor([0.2, 0.9, 0.5])[:min(3, m)]
    lam = F32(0.3)
    want = lam * t.double() + (1.0 - lam) * t.double().flip(0)
    out = ops.mix_targets(t.to(gpu), m, lam)
    buf = t.to(gpu)
    same = ops.mix_targets(buf, m, lam, out=buf)
    torch.cuda.synchronize()
    assert same is buf and torch.equal(out, buf)
    assert (out.cpu().double() - want).abs().max().item() <= 1e-7
    if n % 2:
        assert torch.equal(out[n // 2].cpu(), t[n // 2])
    with pytest.raises(hip.X3DHipError):                   # smoothing is defined for class labels only
        ops.mix_targets(t.to(gpu), m, lam, 0.1)
    with pytest.raises(hip.X3DHipError):
        ops.mix_targets(t.to(gpu), m, lam, hard=torch.zeros(n, dtype=torch.int32, device=gpu))
    lab = torch.zeros(n, dtype=torch.int32, device=gpu)
    with pytest.raises(hip.X3DHipError):
        ops.mix_targets(lab, m, lam, hard=lab)
    with pytest.raises(hip.X3DHipError):
        ops.mix_targets(lab, m, 1.5)


# ---- the model --------------------------------------------------------------------------------------------------------
def _setup(name, overrides=None):
    from x3d_tf_amd.params import init_params, randomize_bn_
    cfg = x.get_config(name, overrides)
    arch = x.build_arch(cfg)
    return cfg, arch, randomize_bn_(init_params(arch, seed=3), seed=4)


def _model(cfg, params, dtype, gpu):
    from x3d_tf_amd.model import X3D
    m = X3D(cfg, dtype=dtype, device=gpu, seed=0)
    m.load_state_dict(params)
    return m


@pytest.mark.gpu
def test_soft_target_train_step_fp32_matches_oracle(gpu):
    from oracle import x3d_oracle as O
    from util import hip_relu_masks, rel_l2
    cfg, arch, params = _setup("XS")
    n, t, s = 4, 4, 64
    torch.manual_seed(1)
    clips = torch.randn(n, t, s, s, 3)
    labels = torch.randint(0, arch.num_classes, (n,))
    y = _mixed_rows(labels, arch.num_classes, F32(0.3), F32(0.1)).float()      # a real mix
    mask = (torch.rand(n, arch.fc1_out) >= arch.dropout_rate).float()
    m = _model(cfg, params, torch.float32, gpu)
    m.set_dropout_mask(mask)
    pl = m.forward_backward(clips.to(gpu), y)
    torch.cuda.synchronize()
    assert torch.equal(pl.targets.cpu(), y) and pl.fwd[pl.grad_scale_slot][0] == "x3d_softmax_xent_soft"

    names = O.trainable_names(params)
    leaf = {k: (v.detach().clone().requires_grad_(True) if k in names else v.clone()) for k, v in params.items()}
    probs, logits = O.forward(leaf, clips, arch, training=True, dropout_mask=mask, state=O.BNState(),
                              relu_masks=hip_relu_masks(pl), return_logits=True)
    p = torch.softmax(logits.double(), -1)
    q = p.clamp(1e-7, 1 - 1e-7)
    yd = y.double()
    ce = ((yd * -torch.log(q)).sum(1) + yd.sum(1) * torch.log(q.sum(1))).mean()
    reg = sum((leaf[k].double() ** 2).sum() for k in O.l2_names(leaf)) * arch.weight_decay
    loss = ce + reg
    grads = dict(zip(names, torch.autograd.grad(loss, [leaf[k] for k in names])))
    got_loss = pl.loss_rows.double().mean().item() + m.regularization_loss().item()
    print(f"loss {got_loss} vs {loss.item()}; probs {(pl.probs.cpu().double() - p).abs().max().item():.3e}")
    assert abs(got_loss - loss.item()) <= 1e-5, (got_loss, loss.item())
    assert (pl.probs.cpu().double() - p.detach()).abs().max().item() <= 1e-4
    for k, g_ref in grads.items():
        g = m.grads[k].cpu().double()
        if m.specs[k].l2:
            g = g + 2 * arch.weight_decay * params[k].double()
        e = rel_l2(g, g_ref.double())
        assert e < 1e-3, f"grad {k}: relative L2 error {e:.3e}"
    # host soft targets are checked; an [N] integer tensor takes the hard-label path again
    with pytest.raises(ValueError):
        m.forward_backward(clips.to(gpu), -y)
    with pytest.raises(ValueError):
        m.forward_backward(clips.to(gpu), y[:, :5])
    bad = y.clone()
    bad[0, 0] = float("inf")
    with pytest.raises(ValueError):
        m.forward_backward(clips.to(gpu), bad)
    pl = m.forward_backward(clips.to(gpu), labels)
    torch.cuda.synchronize()
    assert pl.fwd[pl.grad_scale_slot][0] == "x3d_softmax_xent" and torch.equal(pl.labels.cpu(), labels.int())
    hard_rows = pl.loss_rows.clone()
    pl = m.forward_backward(clips.to(gpu), torch.nn.functional.one_hot(labels, arch.num_classes).float().to(gpu))
    torch.cuda.synchronize()
    report("one-hot loss rows", pl.loss_rows, hard_rows, 1e-4, 1e-4)


@pytest.mark.gpu
def test_bf16_x3d_s_loss_goes_down_with_mixup(gpu):
    cfg, arch, params = _setup("S")
    torch.manual_seed(5)
    clips = torch.randn(4, 4, 64, 64, 3).to(gpu)
    labels = torch.randint(0, arch.num_classes, (4,), dtype=torch.int32).to(gpu)
    lam = F32(0.3)
    m = _model(cfg, params, torch.bfloat16, gpu)
    m.set_dropout_mask((torch.rand(4, arch.fc1_out) >= arch.dropout_rate).float())
    mixed = ops.mix_clips(clips.to(torch.bfloat16), "mixup", lam)
    y = ops.mix_targets(labels, arch.num_classes, lam, 0.1)
    losses = []
    for _ in range(5):
        pl = m.forward_backward(mixed, y)
        losses.append(float(pl.loss_rows.double().mean()))
        m.apply_sgd(1.0, 0.9)
    torch.cuda.synchronize()
    assert all(np.isfinite(losses)), losses
    assert losses[-1] < losses[0], losses


# ---- Trainer ----------------------------------------------------------------------------------------------------------
def _expected_mix(cfg, seed, steps, h, w):
    rng = np.random.default_rng(seed)
    return [draw_mix_params(cfg, h, w, rng) for _ in range(steps)]


@pytest.mark.gpu
@pytest.mark.parametrize("case", ["host-fp32", "device-storage", "device-fp32-to-bf16"])
def test_trainer_step_mixes_a_copy_and_never_the_callers_tensor(gpu, case):
    from x3d_tf_amd.train import Trainer
    cfg, arch, params = _setup("XS", ["MIXUP.ENABLE", True, "MIXUP.PROB", 1.0, "TRAIN.LABEL_SMOOTHING", 0.1])
    dtype = torch.bfloat16 if case == "device-fp32-to-bf16" else torch.float32
    m = _model(cfg, params, dtype, gpu)
    seed, n, t, s = 12, 4, 4, 64
    tr = Trainer(m, cfg, mix_seed=seed)
    want = _expected_mix(cfg, seed, 4, s, s)
    assert {p.mode for p in want} == {"mixup", "cutmix"}          # this seed shows both modes in four steps
    g = torch.Generator().manual_seed(3)
    for step, p in enumerate(want):
        clips = torch.randn(n, t, s, s, 3, generator=g)
        labels = torch.randint(0, arch.num_classes, (n,), generator=g)
        if case != "host-fp32":
            clips, labels = clips.to(gpu), labels.to(gpu)
        before = clips.clone()
        pl = tr.step(clips, labels, 0.01)
        torch.cuda.synchronize()
        assert tr.last_mix == p
        assert torch.equal(clips, before)                          # bit-identical to the clone taken before the step
        stored = before.to(gpu).to(dtype)
        mixed = ops.mix_clips(stored, p.mode, p.lam, (p.y0, p.y1, p.x0, p.x1))
        torch.cuda.synchronize()
        seen = pl._x_keepalive                                     # the batch the plan's launches were bound to
        assert seen.data_ptr() != clips.data_ptr()
        assert torch.equal(seen.to(mixed.dtype), mixed)
        lab = labels.cpu()
        assert torch.equal(pl.labels.cpu(), (lab if F32(p.lam) >= 0.5 else lab.flip(0)).int())
        assert (pl.targets.cpu().double() - _mixed_rows(lab, arch.num_classes, F32(p.lam), F32(0.1))).abs().max().item() <= 1e-7
        assert bool(torch.isfinite(pl.loss_rows).all())
    # a second trainer with the same seed repeats the draws, another seed does not
    tr2 = Trainer(m, cfg, mix_seed=seed)
    tr2.step(before, labels, 0.01)
    assert tr2.last_mix == want[0]
    tr3 = Trainer(m, cfg, mix_seed=seed + 1)
    tr3.step(before, labels, 0.01)
    assert tr3.last_mix != want[0]
    torch.cuda.synchronize()


@pytest.mark.gpu
def test_trainer_smoothing_only_leaves_the_clips_alone(gpu):
    from x3d_tf_amd.train import Trainer
    cfg, arch, params = _setup("XS", ["TRAIN.LABEL_SMOOTHING", 0.1])
    m = _model(cfg, params, torch.float32, gpu)
    tr = Trainer(m, cfg)
    torch.manual_seed(2)
    n = 4
    clips = torch.randn(n, 4, 64, 64, 3).to(gpu)
    labels = torch.randint(0, arch.num_classes, (n,))
    before = clips.clone()
    pl = tr.step(clips, labels, 0.0)
    torch.cuda.synchronize()
    assert tr.last_mix.mode == "none" and tr.last_mix.lam == 1.0
    assert torch.equal(clips, before) and pl._x_keepalive.data_ptr() == clips.data_ptr()     # bound where they lie
    assert torch.equal(pl.labels.cpu(), labels.int())
    y = _smooth_rows(labels, arch.num_classes, F32(0.1))
    assert (pl.targets.cpu().double() - y).abs().max().item() <= 1e-7
    _, rows, _ = _soft_xent_ref(pl.logits.cpu(), y, 1.0)
    report("loss_rows", pl.loss_rows, rows, 1e-4, 1e-4)
    # the default trainer draws nothing and takes the hard-label path
    cfg0, _, _ = _setup("XS")
    tr0 = Trainer(_model(cfg0, params, torch.float32, gpu), cfg0)
    pl0 = tr0.step(clips, labels, 0.0)
    torch.cuda.synchronize()
    assert not tr0._mix_active and pl0.targets is None and pl0.fwd[pl0.grad_scale_slot][0] == "x3d_softmax_xent"


@pytest.mark.gpu
def test_trainer_multi_label_mixup_and_smoothing_refusal(gpu):
    from x3d_tf_amd.model import X3D
    from x3d_tf_amd.train import Trainer
    over = ["DATA.MULTI_LABEL", True, "NETWORK.NUM_CLASSES", 157, "MIXUP.ENABLE", True, "MIXUP.CUTMIX_ALPHA", 0.0]
    cfg, arch, params = _setup("XS", over)
    m = _model(cfg, params, torch.float32, gpu)
    seed = 4
    tr = Trainer(m, cfg, mix_seed=seed)
    (p,) = _expected_mix(cfg, seed, 1, 64, 64)
    assert p.mode == "mixup"
    torch.manual_seed(3)
    n = 5                                                   # odd: the middle row stays what it was
    clips = torch.randn(n, 4, 64, 64, 3)
    y = (torch.rand(n, 157) < 0.05).float()
    y0 = y.clone()
    pl = tr.step(clips, y, 0.01)
    torch.cuda.synchronize()
    assert torch.equal(y, y0) and pl.labels is None
    lam = F32(p.lam)
    want = lam * y.double() + (1.0 - lam) * y.double().flip(0)
    assert (pl.targets.cpu().double() - want).abs().max().item() <= 1e-7
    assert torch.equal(pl.targets[n // 2].cpu(), y[n // 2])
    assert torch.equal(pl._x_keepalive, ops.mix_clips(clips.to(gpu), "mixup", p.lam))
    frozen = x.get_config("XS", over, freeze=False)
    frozen.TRAIN.LABEL_SMOOTHING = 0.1
    with pytest.raises(ValueError):
        Trainer(m, frozen)
    single = x.get_config("XS", ["NETWORK.NUM_CLASSES", 157, "TRAIN.LABEL_SMOOTHING", 0.1])
    with pytest.raises(ValueError):
        Trainer(m, single)                                  # a multi-label MODEL under a smoothing config


@pytest.mark.gpu
def test_fit_with_mixing_and_unmixed_validation(gpu, tmp_path):
    from test_multilabel_gpu import CLASSES, OPTS, _write
    from x3d_tf_amd.model import X3D
    from x3d_tf_amd.train import Trainer
    mix = ["MIXUP.ENABLE", True, "TRAIN.LABEL_SMOOTHING", 0.1]
    cfg_on, cfg_off = x.get_config("XS", OPTS + mix), x.get_config("XS", OPTS)
    train_pattern = _write(str(tmp_path / "train"), 4, seed=4)
    # a validation stream of constant clips: [B * views * crops, T, S, S, 3] with labels [B]
    g = torch.Generator().manual_seed(6)
    val = [(torch.full((6, 4, 32, 32, 3), float(v)), torch.randint(0, CLASSES, (2,), generator=g)) for v in (-0.5, 0.25, 1.0)]
    m = X3D(cfg_on, dtype=torch.float32, device=gpu, seed=1)
    tr_on, tr_off = Trainer(m, cfg_on, mix_seed=2), Trainer(m, cfg_off)
    r_on, r_off = tr_on.validate(val), tr_off.validate(val)
    assert r_on == r_off and np.isfinite(r_on["loss"])      # validation: hard labels, no smoothing, no mixing
    ds = DL.InputReader(cfg_on, True, True, device=gpu, seed=3)(train_pattern, cfg_on.TRAIN.BATCH_SIZE)
    seen = []
    hist = tr_on.fit(ds, validation_data=val, on_step=lambda t_, pl: seen.append(t_.last_mix.mode))
    ds.close()
    h = tr_on.history
    assert set(h) == {"loss", "lr", "acc", "top_5_acc", "val_loss", "val_acc", "val_top_5_acc"}
    assert all(len(v) == 2 for v in h.values()) and h["loss"] == hist
    for k, v in h.items():
        assert np.isfinite(v).all(), (k, v)
    assert all(0.0 <= v <= 1.0 for k in ("acc", "top_5_acc", "val_acc", "val_top_5_acc") for v in h[k])
    assert len(seen) == 4 and set(seen) <= {"mixup", "cutmix"}
    # the validation inside fit is the unmixed one: the same numbers Trainer.validate gives for the final weights
    r = tr_off.validate(val)
    assert abs(h["val_loss"][-1] - r["loss"]) <= 1e-9 and h["val_acc"][-1] == r["acc"]
