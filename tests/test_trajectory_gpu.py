"""Training steps that are NOT the first one of their model or plan, against the CPU oracle.

Every other model-level parity test builds a fresh model and runs one step: zeroed accumulators, zero velocity, freshly packed
weight panels, the initial moving statistics.  Here one model runs several steps -- replaying one plan, interleaving training,
inference and `logits()` plans, evicting and re-recording plans, switching loss heads on one plan, drawing new boxes and new
drop-path tables -- and every checked step starts the oracle from the state the DEVICE holds at that moment (parameters, moving
statistics, velocity: tests/test_model_gpu.py _check_step_fp32 / _check_step_half), so the limits are the single-step limits of
those runners and none grows with the step number.  A new batch, new labels, a new dropout mask and another learning rate at
every step.  All on X3D-XS, 5 classes, clips of 4 x 64 x 64, N = 4 (N = 2 as the second shape): state that survives a replay
does not depend on the plane size.

The negative controls patch Python attributes of the model under test only (the accumulator arena is not zeroed, the gradient
buffer is not zeroed, the weight panels are not repacked): wrong numbers, never a bad address.  Each must fail from the step on
that the stale state reaches, and pass before it.
"""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))       # (the *_ref modules import each other by bare name)

from tests import test_model_gpu as M  # noqa: E402
from tests.util import hip_relu_masks, rel_l2, relu_mask_mismatch, report

pytestmark = pytest.mark.gpu

OVER = ["NETWORK.NUM_CLASSES", 5]
T, S = 4, 64
LRS = (0.05, 0.02, 0.08, 0.03, 0.06)
MOMENTUM = 0.9


def _batch(arch, n, seed, dtype=None, rows=None):
    """clips [n, T, S, S, 3] (representable in `dtype`), labels [n], dropout keep mask [rows or n, fc1_out] of step `seed`"""
    g = torch.Generator().manual_seed(100 + seed)
    x = torch.randn(n, T, S, S, 3, generator=g)
    if dtype is not None:
        x = x.to(dtype).float()
    labels = torch.randint(0, arch.num_classes, (n,), generator=g)
    mask = (torch.rand(rows or n, arch.fc1_out, generator=g) >= arch.dropout_rate).float()
    return x, labels, mask


def _fp32_model(gpu, over=OVER):
    cfg, arch, params = M._setup("XS", over)
    return M._model(cfg, params, torch.float32, gpu), arch


def _fp32_step(m, arch, k, n=4, tag="replay"):
    x, labels, mask = _batch(arch, n, k)
    return M._check_step_fp32(m, x, labels, mask, LRS[k % len(LRS)], MOMENTUM, OVER, tag=f"{tag} step {k + 1}")


@pytest.fixture(autouse=True)
def plan_buffers_start_as_nans(monkeypatch):
    """The plan's buffers -- the ones created lazily after recording too: teacher, kd_rows, row_w -- come from torch.empty: zero
    pages in a fresh process, whatever an earlier test left behind late in a long one.  A launch that read one before anything
    wrote it would then be right or wrong depending on what ran before.  In this file every such buffer starts as NaNs (the
    two allocation methods of _Plan are wrapped: Python attributes only), so such a read fails every time, not now and then."""
    from x3d_tf_amd.plan import _Plan
    for name in ("act", "f32"):
        orig = getattr(_Plan, name)
        monkeypatch.setattr(_Plan, name, lambda self, *shape, _orig=orig: _orig(self, *shape).fill_(float("nan")))
    yield


def test_fresh_plan_buffers_hold_the_nans(gpu):
    """the fixture reaches the plan: a training plan recorded now, and not yet run, holds NaNs in its activation, gradient and
    head buffers (its zeroed accumulators and label buffer are not touched)"""
    m, arch = _fp32_model(gpu)
    pl = m._plan(4, T, S, S, True)
    torch.cuda.synchronize()
    for name, b in (("y0", pl.y0), ("a_raw", pl.blocks[0].a_raw), ("c5_raw", pl.c5_raw), ("h1", pl.h1), ("probs", pl.probs),
                    ("dlogits", pl.dlogits), ("loss_rows", pl.loss_rows)):
        assert torch.isnan(b).all(), name
    assert (pl.zero_buf == 0).all() and (pl.labels == 0).all()
    m16 = M._model(*M._setup("XS", OVER)[::2], torch.bfloat16, gpu)
    assert torch.isnan(m16._plan(4, T, S, S, True).blocks[0].a_raw).all()


# what the checkers say when a comparison fails (the controls must fail THERE, not on an assertion about the plan cache)
_CHECKER_SAYS = "out of tolerance|relative L2 error|ReLU signs differ"


# ---- one plan, replayed ---------------------------------------------------------------------------------------------------------
def test_replayed_plan_fp32(gpu):
    """three steps on one plan, each through the full fp32 checker: accumulators zeroed per step, a non-zero Nesterov velocity
    from step 2 on, moving statistics that moved"""
    m, arch = _fp32_model(gpu)
    first = None
    for k in range(3):
        pl = _fp32_step(m, arch, k)
        first = first or pl
        assert pl is first and len(m._plans) == 1, "not a replay of the first step's plan"
    assert m.flat_velocity.abs().max().item() > 0


def test_replayed_plan_fp32_dilated(gpu):
    """two steps on one plan of the NETWORK.RES5_DILATION = 2 model (N = 2) through the full checker, the oracle under
    DilatedStorage: the dilated kernels' a_sums and dw on a replay"""
    from tests import dilated_ref
    over = OVER + ["NETWORK.RES5_DILATION", 2]
    m, arch = _fp32_model(gpu, over)
    storage = dilated_ref.DilatedStorage(None, sites=dilated_ref.dilated_sites(arch))
    first = None
    for k in range(2):
        x, labels, mask = _batch(arch, 2, k)
        pl = M._check_step_fp32(m, x, labels, mask, LRS[k], MOMENTUM, over, storage=storage, tag=f"dilated replay step {k + 1}")
        first = first or pl
        assert pl is first and len(m._plans) == 1
    assert sum(e[0] == "x3d_dw3d_bwd_dil" for e in first.bwd if e is not None) == len(arch.stages[-1].blocks)


def test_control_arena_not_zeroed(gpu):
    """pl.zero_buf replaced by a dummy after step 1: the fp64 accumulators (stats, pool, a_sums, tail sums, BatchNorm backward
    sums) keep step 1's sums -- step 1 passes, step 2 must not"""
    m, arch = _fp32_model(gpu)
    pl = _fp32_step(m, arch, 0, tag="control (arena)")
    pl.zero_buf = torch.zeros(1, dtype=torch.float64, device=gpu)
    with pytest.raises(AssertionError, match=_CHECKER_SAYS) as e:
        _fp32_step(m, arch, 1, tag="control (arena)")
    print("CONTROL (arena) step 2:", str(e.value)[:160])


class _NeverZeroed(torch.Tensor):
    def zero_(self):
        return self


def test_control_gradients_not_zeroed(gpu):
    """flat_grads seen through a view whose zero_() does nothing: dw / dgamma / dbeta add onto step 1's -- step 1 passes, step 2
    must not"""
    m, arch = _fp32_model(gpu)
    _fp32_step(m, arch, 0, tag="control (grads)")
    m.flat_grads = m.flat_grads.as_subclass(_NeverZeroed)
    with pytest.raises(AssertionError, match="^grad ") as e:         # (the forward pass does not read the gradient buffer)
        _fp32_step(m, arch, 1, tag="control (grads)")
    print("CONTROL (grads) step 2:", str(e.value)[:160])


def _half_plain_steps(gpu, dtype, after_first_step=None):
    """two plain steps of a 16-bit model on one plan; (model, arch, plan)"""
    cfg, arch, params = M._setup("XS", OVER)
    m = M._model(cfg, params, dtype, gpu)
    ls = 1024.0 if dtype == torch.float16 else 1.0
    first = None
    for k in range(2):
        x, labels, mask = _batch(arch, 4, k, dtype)
        m.set_dropout_mask(mask)
        pl = m.forward_backward(x.to(gpu), labels.to(gpu), loss_scale=ls)
        m.apply_sgd(LRS[k], MOMENTUM, grad_scale=1.0 / ls)
        torch.cuda.synchronize()
        assert torch.isfinite(pl.loss_rows).all() and torch.isfinite(m.flat_params).all()
        first = first or pl
        assert pl is first
        if k == 0 and after_first_step is not None:
            after_first_step(m)
    return m, arch, first


def _half_checked_step(m, arch, first):
    """another parameter set, then the teacher-forced comparison on step 3 of the same plan.  Every weight changes at once: a
    panel left from the earlier weights is a gross error in each pointwise conv, not one hidden in the 2 % activation limit."""
    from x3d_tf_amd.params import init_params, randomize_bn_
    m.load_state_dict(randomize_bn_(init_params(arch, seed=5), seed=6))
    x, labels, mask = _batch(arch, 4, 2, m.dtype)
    pl = M._check_step_half(m, x, labels, mask, stem=True, tag="replay step 3")
    assert pl is first and len(m._plans) == 1, "not a replay of the first step's plan"


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16], ids=["bf16", "fp16"])
def test_replayed_plan_half(gpu, dtype):
    _half_checked_step(*_half_plain_steps(gpu, dtype))


def test_control_panels_not_repacked(gpu):
    """_pack_panels a no-op after step 1: the 16-bit weight panels keep the weights of step 1 -- the plain steps run, the bf16
    step-3 check must fail"""
    def stop_packing(m):
        m._pack_panels = lambda: None
    state = _half_plain_steps(gpu, torch.bfloat16, stop_packing)
    with pytest.raises(AssertionError, match=_CHECKER_SAYS) as e:
        _half_checked_step(*state)
    print("CONTROL (panels) step 3:", str(e.value)[:160])


# ---- several plans of one model ---------------------------------------------------------------------------------------------------
def test_interleaved_and_evicted_plans_fp32(gpu):
    """train N=4, inference (2 views), logits(), a forward-only training call, train N=4, the cached inference and logits()
    plans replayed, train N=2, inference and logits() at
    N=2 (which push the N=4 training plan out of the cache of MAX_PLANS = 3), train N=4 on the re-recorded plan.  The plans share
    flat_grads, the moving statistics and the batched eval-coefficient launch; every result is compared with the oracle on the
    parameters the device holds at that moment."""
    from oracle import x3d_oracle as O
    from x3d_tf_amd.model import X3D
    over = OVER + ["TEST.NUM_TEMPORAL_VIEWS", 2, "TEST.NUM_SPATIAL_CROPS", 1]
    cfg, arch, params = M._setup("XS", over)
    m = M._model(cfg, params, torch.float32, gpu)
    seen = {}

    def note():
        assert len(m._plans) <= X3D.MAX_PLANS
        for key, pl in m._plans.items():
            if not any(pl is q for q in seen.setdefault(key, [])):
                seen[key].append(pl)

    def train(k, n):
        x, labels, mask = _batch(arch, n, k)
        pl = M._check_step_fp32(m, x, labels, mask, LRS[k % len(LRS)], MOMENTUM, over, tag=f"interleaved step {k + 1}")
        note()
        return pl

    def infer(k, n, logits_only):
        x, _, _ = _batch(arch, n, k)
        now, _ = M._device_state(m)
        ref, ref_logits = O.forward(now, x, arch, training=False, return_logits=True)
        if logits_only:
            got = m.logits(x.to(gpu))
            torch.cuda.synchronize()
            M._scaled("logits()", got, ref_logits, 1e-4)
        else:
            out = m(x.to(gpu), training=False)
            torch.cuda.synchronize()
            assert tuple(out.shape) == (n // 2, arch.num_classes)
            M._scaled("logits", m._plans[(n, T, S, S, False)].logits, ref_logits, 1e-4)
            report("probs", out, ref, 0, 1e-4)
        after, _ = M._device_state(m)
        assert all(torch.equal(now[k_], after[k_]) for k_ in now), "an inference call wrote the model's state"
        note()

    first = train(0, 4)
    infer(1, 4, False)
    infer(2, 4, True)
    # forward only, training form: batch statistics, dropout, the moving statistics move
    x, _, mask = _batch(arch, 4, 3)
    now, _ = M._device_state(m)
    st = O.BNState()
    ref = O.forward({k: v.clone() for k, v in now.items()}, x, arch, training=True, dropout_mask=mask, state=st)
    m.set_dropout_mask(mask)
    out = m(x.to(gpu), training=True)
    torch.cuda.synchronize()
    report("probs (training=True)", out, ref, 0, 1e-4)
    for k, v in st.new_moving.items():
        report(k, m.params[k], v, 1e-4, 1e-5)
    assert m._plans[(4, T, S, S, True)] is first
    note()
    assert train(4, 4) is first
    # the cached inference and logits() plans again, now that a training step has moved weights and moving statistics: their
    # coefficient tables come from x3d_bn_eval_coef_batched at the head of every replay
    cached = (m._plans[(4, T, S, S, False)], m._plans[(4, T, S, S, False, "logits")])
    infer(9, 4, False)
    infer(10, 4, True)
    assert m._plans[(4, T, S, S, False)] is cached[0] and m._plans[(4, T, S, S, False, "logits")] is cached[1]
    assert len(seen) == 3, "a replay recorded a plan"
    small = train(5, 2)
    assert small is not first and len(m._plans) == X3D.MAX_PLANS
    infer(6, 2, False)
    infer(7, 2, True)
    assert (4, T, S, S, True) not in m._plans, "the N=4 training plan should have been evicted by now"
    last = train(8, 4)
    assert last is not first and len(seen[(4, T, S, S, True)]) == 2
    assert len(seen) > X3D.MAX_PLANS       # more plans were recorded than the cache holds: evictions happened


def _backward_from_dlogits(m, pl, x, mask):
    """Everything below the loss of the step `pl` has just run, teacher-forced: the oracle's forward pass on the parameters the
    device holds (forward_backward does not write the trainable ones) under the device's ReLU sign patterns, driven backwards
    by the device's own dlogits.  Limits: _check_step_fp32's -- logits 1e-4 of their maximum, every gradient below 1e-3 relative
    L2 and within 2e-3 of its maximum.  Returns the worst logits error and gradient relative L2, each over its limit."""
    from oracle import x3d_oracle as O
    now, _ = M._device_state(m)
    names = O.trainable_names(now)
    leaf = {k: (v.clone().requires_grad_(True) if k in names else v) for k, v in now.items()}
    _, logits = O.forward(leaf, x, m.arch, training=True, dropout_mask=mask, state=O.BNState(), relu_masks=hip_relu_masks(pl),
                          return_logits=True)
    w_logits = M._scaled("logits", pl.logits, logits, 1e-4) / (1e-4 * logits.detach().abs().max().item())
    grads = torch.autograd.grad(logits, [leaf[k] for k in names], grad_outputs=pl.dlogits.cpu().to(logits.dtype))
    w_grad = 0.0
    for k, g_ref in zip(names, grads):
        g = m.grads[k].cpu().double()            # (data gradients: the L2 term belongs to the optimizer)
        e = rel_l2(g, g_ref)
        w_grad = max(w_grad, e / 1e-3)
        assert e < 1e-3, f"grad {k}: relative L2 error {e:.3e}"
        M._scaled("grad " + k, g, g_ref, 2e-3)
    return w_logits, w_grad


# ---- loss heads recorded lazily on one plan ---------------------------------------------------------------------------------------
def test_head_switching_on_one_plan(gpu):
    """hard labels -> soft targets -> distillation -> sample weights -> hard labels on ONE plan: the head slot holds the right
    entry each time and nothing of the previous head (targets, teacher, row weights) leaks into the next.  The heads of the
    middle steps are held to the fp64 restatements of their kernels on the plan's own logits (tests/distill_ref.py,
    tests/loss_weights_ref.py, at loss_weights_ref.TOL: the limits of test_mix_gpu / test_distill_gpu / test_loss_weights_gpu) and
    everything below the loss to the oracle driven by the device's dlogits; the two hard-label steps go through the full
    checker.  The middle steps follow one another without a host synchronisation in between."""
    import distill_ref as D
    import loss_weights_ref as W
    m, arch = _fp32_model(gpu)
    n, classes = 4, arch.num_classes
    first = _fp32_step(m, arch, 0, tag="heads")
    assert first.fwd[first.grad_scale_slot][0] == "x3d_softmax_xent"

    def head_step(k, want, ref_of, **kw):
        x, labels, mask = _batch(arch, n, k)
        g = torch.Generator().manual_seed(200 + k)
        m.set_dropout_mask(mask)
        target, extra, ref_args = ref_of(labels, g)
        pl = m.forward_backward(x.to(gpu), target, **extra)
        torch.cuda.synchronize()
        assert pl is first and len(m._plans) == 1 and pl.fwd[pl.grad_scale_slot][0] == want
        z = pl.logits.cpu()
        p, rows, kd, dl = ref_args(z)
        got = dict(probs=pl.probs, loss_rows=pl.loss_rows, dlogits=pl.dlogits)
        refs = dict(probs=p, loss_rows=rows, dlogits=dl)
        if kd is not None:
            got["kd_rows"], refs["kd_rows"] = pl.kd_rows, kd
        scale = kw.get("scale", 1.0)
        for what, r in refs.items():
            rtol, atol = W.TOL[what]
            r = torch.as_tensor(np.asarray(r)) if not torch.is_tensor(r) else r
            err = report(f"{want} {what}", got[what], r, rtol, atol * scale)
            print(f"CHECKED heads step {k + 1} {want} {what}: max abs err {err:.3e}")
        assert torch.isfinite(m.flat_grads).all() and m.flat_grads.abs().max().item() > 0
        w_logits, w_grad = _backward_from_dlogits(m, pl, x, mask)
        print(f"CHECKED heads step {k + 1} {want}: worst error / limit logits {w_logits:.3f}, grad rel-L2 {w_grad:.3f}")
        m.apply_sgd(LRS[k], MOMENTUM)      # (no synchronisation before the next step's launches: as the trainer runs them)

    def soft(labels, g):
        hot = torch.nn.functional.one_hot(labels, classes).double()
        other = torch.nn.functional.one_hot(torch.randint(0, classes, (n,), generator=g), classes).double()
        lam = D.f32(0.3)
        y = (lam * (0.9 * hot + 0.1 / classes) + (1.0 - lam) * other).float()

        def ref(z):
            p, rows, grad = D.softmax_hard(z, targets=y)
            return p, rows, None, grad / n
        return y, {}, ref

    def distilled(labels, g):
        t = (torch.randn(n, classes, generator=g) * 3).float()

        def ref(z):
            return D.combine(D.softmax_hard(z, labels=labels), D.softmax_kd(z, t, 2.0), 0.5, 1.0 / n)
        return labels.to(gpu), dict(teacher_logits=t.to(gpu), distill=(0.5, 2.0)), ref

    rw = np.array([0.5, 0.0, 3.25, 1.5], dtype=np.float32)

    def weighted(labels, g):
        def ref(z):
            p, rows, _, dl = W.expected("labels", z, None, labels, None, None, None, None, rw, {}, 0.0, 1.0, 1.0 / n)
            return p, rows, None, dl
        return labels.to(gpu), dict(sample_weight=torch.from_numpy(rw)), ref

    head_step(1, "x3d_softmax_xent_soft", soft)
    head_step(2, "x3d_softmax_xent_kd", distilled)
    head_step(3, "x3d_softmax_xent_w", weighted, scale=W.weight_scale(None, None, rw))
    last = _fp32_step(m, arch, 4, tag="heads")
    assert last is first and len(m._plans) == 1 and last.fwd[last.grad_scale_slot][0] == "x3d_softmax_xent"


# ---- detection on the dilated model: new boxes, another image without a box -------------------------------------------------------
def _trunk_from_g5(m, pl, params, x, storage):
    """The trunk below the box head, teacher-forced: the oracle runs stem, blocks, conv5 and its BatchNorm on the parameters the
    device held before the step, with the device's ReLU sign patterns, and is driven backwards by the device's own gradient at
    the BatchNorm output (pl.backward.g5).  Limits: test_model_gpu._check_step_fp32's -- raw conv outputs 2e-4 of the tensor's
    maximum, every gradient below 1e-3 relative L2 and within 2e-3 of its maximum."""
    from oracle import x3d_oracle as O
    arch = m.arch
    names = [k for k in O.trainable_names(params) if not k.startswith(("fc1/", "fc2/"))]
    leaf = {k: (v.clone().requires_grad_(True) if k in names else v) for k, v in params.items()}
    masks = hip_relu_masks(pl)
    state = O.BNState()
    out = O.stem(storage.act(x.permute(0, 4, 1, 2, 3)), leaf, arch, True, state, masks, storage)
    for b in arch.blocks:
        out = O.res_block(out, leaf, b, arch, True, state, None, masks, storage)
    c5 = storage.act(O.pointwise(out, leaf["conv5/layer_with_weights-0/kernel"]))
    z5 = O.batch_norm(c5, leaf, "conv5/layer_with_weights-1", True, arch.bn_eps, arch.bn_momentum, state)
    worst = M._scaled("c5_raw", pl.c5_raw, c5, 2e-4) / (2e-4 * c5.detach().abs().max().item())
    grads = torch.autograd.grad(z5, [leaf[k] for k in names], grad_outputs=pl.backward.g5.cpu().to(z5.dtype))
    worst_g = 0.0
    for k, g_ref in zip(names, grads):
        g = m.grads[k].cpu().double()            # (data gradients: the L2 term belongs to the optimizer)
        e = rel_l2(g, g_ref)
        worst_g = max(worst_g, e / 1e-3)
        assert e < 1e-3, f"grad {k}: relative L2 error {e:.3e}"
        M._scaled("grad " + k, g, g_ref, 2e-3)
    return worst, worst_g


def test_detection_trajectory_on_the_dilated_model(gpu):
    """RES5_DILATION 2 + DETECTION.ENABLE, MAX_BOXES 2, three steps on one plan with num_boxes [2, 0], [0, 1], [1, 2] and new
    boxes each time: roi_argmax, box_mask and row_w are per-step device state, and the image without a box changes sides.  Per
    step the head restated in fp64 (test_dilated_res5_gpu._detection_step, its limits) and the trunk teacher-forced from g5 through
    the dilated oracle."""
    from tests import dilated_ref, roi_ref
    from tests import test_dilated_res5_gpu as DR
    from tests import test_roi_head_gpu as H
    cfg, arch, params = H._setup(DR.DET)
    m = H._model(cfg, params, gpu)
    storage = dilated_ref.DilatedStorage(None, sites=dilated_ref.dilated_sites(arch))
    n, kb = 2, 2
    first = None
    for k, nb in enumerate(([2, 0], [0, 1], [1, 2])):
        g = torch.Generator().manual_seed(300 + k)
        clips = torch.randn(n, T, S, S, 3, generator=g)
        boxes = roi_ref.box_mix(n, kb, S, S, seed=20 + k)
        labels = torch.randint(0, arch.num_classes, (n, kb), generator=g)
        mask = (torch.rand(n * kb, arch.fc1_out, generator=g) >= arch.dropout_rate).float()
        now, _ = M._device_state(m)
        pl = DR._detection_step(m, clips, boxes, nb, labels, mask)
        first = first or pl
        assert pl is first and len(m._plans) == 1
        assert pl.box_mask.cpu().tolist() == [float(j < nb[i]) for i in range(n) for j in range(kb)]
        w_act, w_grad = _trunk_from_g5(m, pl, now, clips, storage)
        print(f"CHECKED detection step {k + 1} num_boxes {nb}: worst error / limit c5_raw {w_act:.3f}, trunk grad rel-L2 {w_grad:.3f}; "
              f"max |logit| {pl.logits.abs().max().item():.2f}")
        # a tenth of the other tests' rates: the loss is the mean over one or two boxes, and at 0.05 the second step's logits reach
        # +-60 -- probabilities below Keras' 1e-7 clip, where the restated head (plain cross-entropy) is another function
        m.apply_sgd(0.1 * LRS[k], MOMENTUM)
    DR._check_plan_is_dilated(first, arch)


# ---- stochastic depth: a new table per replay ---------------------------------------------------------------------------------------
def test_drop_path_trajectory(gpu):
    """NETWORK.DROP_PATH_RATE 0.5 with the device draw: three steps from set_drop_path_state(seed, step).  Per step pl.dp_keep is
    tests/drop_path_ref.py's table for (seed, step + k), the counter advances by one, and the step is compared with
    drop_path_ref's forward / train_step under that table at the limits of test_drop_path_gpu (block outputs 2e-4, logits and
    probabilities 1e-4, moving statistics, loss 1e-5, every gradient below 1e-3 relative L2; a block that dropped every sample: a
    gradient of exactly zero), from the parameters the device holds."""
    from oracle import x3d_oracle as O
    from tests import drop_path_ref as R
    from x3d_tf_amd.arch import drop_path_rates
    over = OVER + ["NETWORK.DROP_PATH_RATE", 0.5]
    cfg, arch, params = M._setup("XS", over)
    rates = drop_path_rates(arch)
    m = M._model(cfg, params, torch.float32, gpu)
    # (seed, first step): the oracle's OWN fp32 error sets what this choice must avoid.  Run in fp32 and in fp64 on the CPU along
    # this trajectory, the reference's gradients differ by at most 1.7e-4 relative L2 with (1234, 7); with (20261021, 7) the
    # first table leaves the se_fc1 bias of block 0 a sum that cancels so far that the fp32 reference itself is 1.0e-3 off.
    seed, step0, n = 1234, 7, 4
    m.set_drop_path_state(seed, step0)
    first, tables = None, []
    for k in range(3):
        assert m.drop_path_step() == step0 + k
        x, labels, mask = _batch(arch, n, k)
        now, _ = M._device_state(m)
        m.set_dropout_mask(mask)
        pl = m.forward_backward(x.to(gpu), labels.to(gpu))
        torch.cuda.synchronize()
        first = first or pl
        assert pl is first and len(m._plans) == 1
        keep = torch.from_numpy(R.keep_table(seed, step0 + k, rates, n))
        assert torch.equal(pl.dp_keep.cpu(), keep), f"step {k + 1}: not the table of (seed, {step0 + k})"
        assert m.drop_path_step() == step0 + k + 1
        tables.append(keep)

        taps, st, free_masks = {}, O.BNState(), O.RecordMasks()
        probs_free = R.forward_dp({k_: v.clone() for k_, v in now.items()}, x, arch, keep, rates, dropout_mask=mask, state=st,
                                  taps=taps, relu_masks=free_masks)
        M._scaled("conv1/out", pl.y0, taps["conv1/out"], 2e-5)
        for B in pl.blocks:
            pre = O.block_prefix(B.spec)
            M._scaled(pre + "/out", B.y, taps[pre + "/out"], 2e-4)
        M._scaled("logits", pl.logits, taps["logits"], 1e-4)
        report("probs", pl.probs, probs_free, 0, 1e-4)
        for k_, v in st.new_moving.items():
            report(k_, m.params[k_], v, 1e-4, 1e-5)
        dev_masks = hip_relu_masks(pl)
        frac, bad, tot = relu_mask_mismatch(dev_masks, free_masks)
        assert frac <= 1e-5, f"{bad} of {tot} ReLU signs differ between the device and the free-running reference"
        r = R.train_step_dp({k_: v.clone() for k_, v in now.items()}, x, labels, arch, keep, rates, dropout_mask=mask,
                            relu_masks=dev_masks)
        loss = pl.loss_rows.mean() + m.regularization_loss().float()
        report("loss", loss.view(1), r["loss"].view(1), 1e-5, 1e-5)
        worst = 0.0
        for k_, g_ref in r["grads"].items():
            g = m.grads[k_].cpu().double()
            if m.specs[k_].l2:
                g = g + 2 * arch.weight_decay * now[k_].double()
            if g_ref.norm().item() == 0.0:
                assert g.abs().max().item() == 0.0, f"grad {k_}: the reference is exactly zero"
                continue
            e = rel_l2(g, g_ref)
            worst = max(worst, e)
            assert e < 1e-3, f"grad {k_}: relative L2 error {e:.3e}"
        print(f"CHECKED drop-path step {k + 1}: ReLU sign mismatches {bad} of {tot}; worst gradient relative L2 / limit {worst / 1e-3:.3f}; "
              f"kept {int((keep > 0).sum())} of {keep.numel()}")
        m.apply_sgd(LRS[k], MOMENTUM)
    assert not torch.equal(tables[0], tables[1]) and not torch.equal(tables[1], tables[2])
