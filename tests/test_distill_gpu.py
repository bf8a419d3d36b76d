"""Knowledge distillation on the GPU: x3d_softmax_xent_kd / x3d_sigmoid_bce_kd against the fp64 restatement in distill_ref.py
(limits: test_mix_gpu.py's for the sibling kernel -- the arithmetic is of the same kind), alpha = 0 against the three hard
kernels bit for bit, unusable teacher rows, X3D.logits, the head slot of forward_backward, and Trainer.step / fit."""
import json
import math
import os
import socket
import sys

import numpy as np
import pytest
import torch
import torch.multiprocessing as mp

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import x3d_tf_amd as x  # noqa: E402
from x3d_tf_amd import dataloader as DL  # noqa: E402
from x3d_tf_amd import hip, ops  # noqa: E402
import distill_ref as R  # noqa: E402
from util import rel_l2, report  # noqa: E402

PROBS, ROWS, DLOGITS = (1e-5, 1e-7), (1e-4, 1e-4), (1e-3, 1e-6)       # (rtol, atol), as test_mix_gpu.py
SENTINEL = 7.0
HEADS = ("labels", "targets", "multi")


def _run(gpu, head, z, t, labels, soft, multi, gs, alpha, T):
    """one launch of the head's KD entry point into sentinel-filled buffers: (probs, loss_rows, kd_rows, dlogits)"""
    n, m = z.shape
    probs, dl = torch.full((n, m), SENTINEL, device=gpu), torch.full((n, m), SENTINEL, device=gpu)
    rows, kd = torch.full((n,), SENTINEL, device=gpu), torch.full((n,), SENTINEL, device=gpu)
    tg = None if t is None else t.to(gpu)
    if head == "multi":
        ops.sigmoid_bce_kd(z.to(gpu), tg, multi.to(gpu), probs, rows, kd, dl, gs, alpha, T)
    else:
        ops.softmax_xent_kd(z.to(gpu), tg, probs, labels=labels.to(gpu) if head == "labels" else None,
                            targets=soft.to(gpu) if head == "targets" else None, loss_rows=rows, kd_rows=kd, dlogits=dl,
                            grad_scale=gs, alpha=alpha, temperature=T)
    torch.cuda.synchronize()
    return probs, rows, kd, dl


def _ref(head, z, t, labels, soft, multi, gs, alpha, T):
    if head == "multi":
        return R.combine(R.sigmoid_hard(z, multi), R.sigmoid_kd(z, t, T), alpha, gs)
    hard = R.softmax_hard(z, labels=labels) if head == "labels" else R.softmax_hard(z, targets=soft)
    return R.combine(hard, R.softmax_kd(z, t, T), alpha, gs)


# ---- the kernels against fp64 -----------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("head", HEADS)
@pytest.mark.parametrize("n", R.NS)
@pytest.mark.parametrize("m", R.MS)
def test_kd_kernels_match_fp64(gpu, head, n, m):
    z, t, labels, soft, multi = R.inputs(n, m)
    gs = 1.0 / n
    for T in R.TEMPS:
        for alpha in R.ALPHAS:
            a = R.f32(alpha)
            got = _run(gpu, head, z, t, labels, soft, multi, gs, a, T)
            ref = _ref(head, z, t, labels, soft, multi, gs, a, T)
            errs = [(g.cpu().double() - r).abs().max().item() for g, r in zip(got, ref)]
            print(f"{head} n={n} m={m} T={T} a={alpha}: probs {errs[0]:.3e} loss {errs[1]:.3e} kd {errs[2]:.3e} "
                  f"dlogits {errs[3]:.3e}")
            report("probs", got[0], ref[0], *PROBS)
            report("loss_rows", got[1], ref[1], *ROWS)
            report("kd_rows", got[2], ref[2], *ROWS)
            report("dlogits", got[3], ref[3], *DLOGITS)
            assert float(got[2].min()) >= -1e-4                       # a KL
            if alpha == 1.0 and R.has_same_row(n, m):                 # t = z: no KD loss, no gradient
                assert abs(got[2][R.SAME_ROW].item()) <= 1e-4
                assert got[3][R.SAME_ROW].abs().max().item() <= 1e-6


# ---- alpha = 0: the hard kernels, bit for bit -------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("head", HEADS)
@pytest.mark.parametrize("n, m", [(1, 1), (7, 157), (64, 257), (64, 400)])
def test_alpha_zero_is_the_hard_kernel_bit_for_bit(gpu, head, n, m):
    z, t, labels, soft, multi = R.inputs(n, m)
    gs = 0.37
    p0, r0, d0 = torch.empty(n, m, device=gpu), torch.empty(n, device=gpu), torch.empty(n, m, device=gpu)
    if head == "labels":
        ops.softmax_xent(z.to(gpu), labels.to(gpu), p0, r0, d0, gs)
    elif head == "targets":
        ops.softmax_xent_soft(z.to(gpu), soft.to(gpu), p0, r0, d0, gs)
    else:
        ops.sigmoid_bce(z.to(gpu), multi.to(gpu), p0, r0, d0, gs)
    for teacher in (None, t):                                         # a NULL teacher is accepted; a given one is not read
        for T in (1.0, 4.0):
            probs, rows, kd, dl = _run(gpu, head, z, teacher, labels, soft, multi, gs, 0.0, T)
            assert torch.equal(probs, p0) and torch.equal(rows, r0) and torch.equal(dl, d0)
            assert kd.abs().sum().item() == 0.0                       # (and with it: no sentinel left anywhere)
    # the probs of every alpha are those bits too
    probs, _, _, _ = _run(gpu, head, z, t, labels, soft, multi, gs, R.f32(0.3), 2.5)
    assert torch.equal(probs, p0)
    # a teacher full of NaN is not read either
    probs, rows, kd, dl = _run(gpu, head, z, torch.full_like(t, float("nan")), labels, soft, multi, gs, 0.0, 1.0)
    assert torch.equal(rows, r0) and torch.equal(dl, d0) and kd.abs().sum().item() == 0.0


# ---- unusable teacher rows --------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("head", HEADS)
def test_non_finite_teacher_logits_void_their_rows_only(gpu, head):
    n, m = 7, 257
    z, t, labels, soft, multi = R.inputs(n, m)
    clean = _run(gpu, head, z, t, labels, soft, multi, 1.0, 0.5, 2.0)
    bad = t.clone()
    bad[1, 256] = float("nan")                                        # the ragged last wave's only element
    bad[4, 17] = float("inf")
    probs, rows, kd, dl = _run(gpu, head, z, bad, labels, soft, multi, 1.0, 0.5, 2.0)
    good = [0, 2, 3, 5, 6]
    for r in (1, 4):
        assert math.isnan(rows[r].item()) and math.isnan(kd[r].item()) and dl[r].abs().sum().item() == 0.0
    assert bool(torch.isfinite(rows[good]).all()) and bool(torch.isfinite(kd[good]).all()) and bool(torch.isfinite(dl).all())
    assert all(dl[r].abs().sum().item() > 0 and rows[r].item() != 0 for r in good)
    assert torch.equal(probs, clean[0])
    assert torch.equal(rows[good], clean[1][good]) and torch.equal(dl[good], clean[3][good])
    # the hard term's own rule stays: a label outside [0, M) / a NaN target voids the row whatever the teacher says
    if head == "labels":
        lab = labels.clone()
        lab[3] = m
        _, rows, kd, dl = _run(gpu, head, z, t, lab, soft, multi, 1.0, 0.5, 2.0)
        assert math.isnan(rows[3].item()) and dl[3].abs().sum().item() == 0.0 and torch.equal(kd, clean[2])
    elif head == "targets":
        y = soft.clone()
        y[3, 9] = float("nan")
        _, rows, kd, dl = _run(gpu, head, z, t, labels, y, multi, 1.0, 0.5, 2.0)
        assert math.isnan(rows[3].item()) and dl[3].abs().sum().item() == 0.0 and torch.equal(kd, clean[2])


@pytest.mark.gpu
def test_ops_wrappers_check_their_tensors(gpu):
    n, m = 3, 11
    z, t = torch.zeros(n, m, device=gpu), torch.zeros(n, m, device=gpu)
    p, lab = torch.empty(n, m, device=gpu), torch.zeros(n, dtype=torch.int32, device=gpu)
    with pytest.raises(ValueError):
        ops.softmax_xent_kd(z, t, p)                                              # neither labels nor targets
    with pytest.raises(ValueError):
        ops.softmax_xent_kd(z, t, p, labels=lab, targets=z.clone())               # both
    with pytest.raises(ValueError):
        ops.softmax_xent_kd(z, t[:, :5].contiguous(), p, labels=lab)              # teacher shape
    with pytest.raises(ValueError):
        ops.softmax_xent_kd(z, t, p, labels=lab.long())                           # label type
    with pytest.raises(ValueError):
        ops.sigmoid_bce_kd(z, t, None, p)
    with pytest.raises(ValueError):
        ops.sigmoid_bce_kd(z, t, z.clone(), p, kd_rows=torch.empty(n + 1, device=gpu))
    with pytest.raises(hip.X3DHipError, match="alpha"):
        ops.softmax_xent_kd(z, t, p, labels=lab, alpha=1.5)
    with pytest.raises(hip.X3DHipError, match="temperature"):
        ops.sigmoid_bce_kd(z, t, z.clone(), p, temperature=0.0)
    with pytest.raises(hip.X3DHipError, match="teacher_logits"):
        ops.softmax_xent_kd(z, None, p, labels=lab, alpha=0.5)


# ---- the model --------------------------------------------------------------------------------------------------------
N, T_, S = 4, 4, 64               # the fp32 whole-model training step of test_mix_gpu.py
VIEWS = ["TEST.NUM_TEMPORAL_VIEWS", 1, "TEST.NUM_SPATIAL_CROPS", 3]


def _models(gpu, overrides=(), dtype=torch.float32):
    """(cfg, arch, student, teacher): two models of one config, initialised from different seeds, BatchNorm statistics
    randomised so that inference is no identity"""
    from x3d_tf_amd.model import X3D
    from x3d_tf_amd.params import init_params, randomize_bn_
    cfg = x.get_config("XS", VIEWS + list(overrides))
    arch = x.build_arch(cfg)
    out = []
    for seed in (3, 11):
        m = X3D(cfg, dtype=dtype, device=gpu, seed=0)
        m.load_state_dict(randomize_bn_(init_params(arch, seed=seed), seed=seed + 1))
        out.append(m)
    return cfg, arch, out[0], out[1]


def _batch(arch, n=N, seed=1):
    g = torch.Generator().manual_seed(seed)
    clips = torch.randn(n, T_, S, S, 3, generator=g)
    labels = torch.randint(0, arch.num_classes, (n,), generator=g)
    mask = (torch.rand(n, arch.fc1_out, generator=g) >= arch.dropout_rate).float()
    return clips, labels, mask


@pytest.mark.gpu
def test_logits_is_the_inference_plan_up_to_the_probabilities_and_writes_no_state(gpu):
    cfg, arch, _, teacher = _models(gpu)
    v = arch.num_preds
    assert v == 3 and N % v != 0
    before = teacher.flat_params.clone()
    g = torch.Generator().manual_seed(2)
    clips = torch.randn(2 * v, T_, S, S, 3, generator=g).to(gpu)
    got = teacher.logits(clips)
    assert got.dtype == torch.float32 and tuple(got.shape) == (2 * v, arch.num_classes) and got.is_cuda
    got = got.clone()
    out = teacher(clips, training=False)
    torch.cuda.synchronize()
    pl = teacher._plans[(2 * v, T_, S, S, False)]
    assert torch.equal(pl.logits, got)                                # the same launches on the same inputs
    assert tuple(out.shape) == (2, arch.num_classes)
    # a batch that `call` refuses: the clips are independent at inference, so its rows are those of the larger batch up to
    # the order of fp32 sums (other tilings): 1e-4 of the largest logit
    with pytest.raises(ValueError):
        teacher(clips[:N], training=False)
    part = teacher.logits(clips[:N])
    torch.cuda.synchronize()
    assert tuple(part.shape) == (N, arch.num_classes) and bool(torch.isfinite(part).all())
    err = (part.double() - got[:N].double()).abs().max().item()
    print(f"logits of {N} clips against the first {N} of {2 * v}: max abs err {err:.3e}, max |logit| {got.abs().max().item():.3e}")
    assert err <= 1e-4 * got.abs().max().item()
    assert got.std().item() > 0
    assert torch.equal(teacher.flat_params, before)                   # weights and moving statistics, bit for bit


@pytest.mark.gpu
def test_forward_backward_runs_the_kd_head_and_its_gradient_is_the_dense_target_gradient(gpu):
    cfg, arch, m, teacher = _models(gpu)
    clips, labels, mask = _batch(arch)
    clips = clips.to(gpu)
    m.set_dropout_mask(mask)
    tl = teacher.logits(clips).clone()
    classes = arch.num_classes

    # the head slot: what ops.softmax_xent_kd gives on the plan's logits
    pl = m.forward_backward(clips, labels, teacher_logits=tl, distill=(0.5, 2.0))
    torch.cuda.synchronize()
    assert pl.fwd[pl.grad_scale_slot][0] == "x3d_softmax_xent_kd" and torch.equal(pl.teacher, tl)
    p2, r2, k2, d2 = (torch.empty(N, classes, device=gpu), torch.empty(N, device=gpu), torch.empty(N, device=gpu),
                      torch.empty(N, classes, device=gpu))
    ops.softmax_xent_kd(pl.logits, tl, p2, labels=pl.labels, loss_rows=r2, kd_rows=k2, dlogits=d2, grad_scale=1.0 / N,
                        alpha=0.5, temperature=2.0)
    torch.cuda.synchronize()
    assert torch.equal(pl.dlogits, d2) and torch.equal(pl.loss_rows, r2) and torch.equal(pl.probs, p2)
    assert torch.equal(pl.kd_rows, k2) and bool((k2 > 0).all())

    # T = 1, a = 0.5 against the dense targets (1 - a) * onehot + a * softmax(teacher): the same gradient, algebraically
    a = 0.5
    pl = m.forward_backward(clips, labels, teacher_logits=tl, distill=(a, 1.0))
    torch.cuda.synchronize()
    g_kd = {k: g.clone() for k, g in m.grads.items()}
    pt = torch.softmax(tl.double(), -1)
    for p in (pl.probs.double(), pt):                                 # the precondition: nothing in the clipped regime
        assert p.min().item() >= 1e-7 and p.max().item() <= 1 - 1e-7
    y = ((1 - a) * torch.nn.functional.one_hot(labels.to(gpu), classes).double() + a * pt).float()
    pl = m.forward_backward(clips, y)
    torch.cuda.synchronize()
    assert pl.fwd[pl.grad_scale_slot][0] == "x3d_softmax_xent_soft"
    worst = 0.0
    for k, g in m.grads.items():
        e = rel_l2(g_kd[k], g)
        worst = max(worst, e)
        assert e <= 1e-3, f"grad {k}: relative L2 {e:.3e} between the KD head and the dense-target head"
    # ... and the teacher's share is no no-op: a = 0 gives another fc2 gradient
    pl = m.forward_backward(clips, labels, teacher_logits=tl, distill=(0.0, 1.0))
    torch.cuda.synchronize()
    diff = rel_l2(g_kd["fc2/kernel"], m.grads["fc2/kernel"])
    print(f"KD vs dense targets: worst relative L2 {worst:.3e}; a = 0.5 vs a = 0 in fc2/kernel: {diff:.3e}")
    assert diff > 1e-3
    # a = 0 through the slot is the hard-label loss on the same logits, bit for bit; and the plain call takes the recorded entry
    ops.softmax_xent(pl.logits, pl.labels, p2, r2, d2, 1.0 / N)
    torch.cuda.synchronize()
    assert torch.equal(pl.dlogits, d2) and torch.equal(pl.loss_rows, r2) and pl.kd_rows.abs().sum().item() == 0.0
    pl = m.forward_backward(clips, labels)
    torch.cuda.synchronize()
    assert pl.fwd[pl.grad_scale_slot][0] == "x3d_softmax_xent"

    # arguments
    with pytest.raises(ValueError):
        m.forward_backward(clips, labels, teacher_logits=tl[:, :7].contiguous(), distill=(0.5, 1.0))
    with pytest.raises(ValueError):
        m.forward_backward(clips, labels, teacher_logits=tl[:2].contiguous(), distill=(0.5, 1.0))
    with pytest.raises(ValueError):
        m.forward_backward(clips, labels, teacher_logits=tl)
    with pytest.raises(ValueError):
        m.forward_backward(clips, labels, teacher_logits=tl.cpu(), distill=(0.5, 1.0))


# ---- Trainer ----------------------------------------------------------------------------------------------------------
KD = ["DISTILL.ENABLE", True, "DISTILL.ALPHA", 0.5, "DISTILL.TEMPERATURE", 2.0]


@pytest.mark.gpu
def test_trainer_teacher_sees_the_mixed_clips(gpu):
    from x3d_tf_amd.mix import draw_mix_params
    from x3d_tf_amd.model import X3D
    from x3d_tf_amd.train import Trainer
    over = KD + ["MIXUP.ENABLE", True, "MIXUP.PROB", 1.0]
    cfg, arch, m, teacher = _models(gpu, over)
    seed = 12
    tr = Trainer(m, cfg, mix_seed=seed, teacher=teacher)
    assert tr.teacher is teacher and tr.distill.enable and tr._kd == (0.5, 2.0)
    before = teacher.flat_params.clone()
    clips, labels, mask = _batch(arch)
    clips = clips.to(gpu)
    pl = tr.step(clips, labels, 0.01)
    torch.cuda.synchronize()
    p = tr.last_mix
    assert p == draw_mix_params(cfg, S, S, np.random.default_rng(seed)) and p.mode in ("mixup", "cutmix")
    assert pl.fwd[pl.grad_scale_slot][0] == "x3d_softmax_xent_kd"
    held = pl.teacher.clone()
    mixed = ops.mix_clips(clips, p.mode, p.lam, (p.y0, p.y1, p.x0, p.x1))
    assert torch.equal(pl._x_keepalive, mixed)                        # what the student saw
    want = teacher.logits(mixed).clone()
    unmixed = teacher.logits(clips).clone()
    torch.cuda.synchronize()
    print(f"teacher buffer vs teacher.logits(mixed): max abs diff {(held - want).abs().max().item():.3e}; "
          f"vs teacher.logits(unmixed): {(held - unmixed).abs().max().item():.3e}")
    assert torch.equal(held, want)                                    # same inputs, same launch list
    assert not torch.equal(held, unmixed)
    assert bool(torch.isfinite(pl.loss_rows).all()) and bool((pl.kd_rows > 0).all())
    assert torch.equal(teacher.flat_params, before)
    # refusals
    other = x.get_config("XS", VIEWS + KD + ["NETWORK.NUM_CLASSES", 157])
    with pytest.raises(ValueError, match="classes"):
        Trainer(m, cfg, teacher=X3D(other, device=gpu))
    with pytest.raises(ValueError, match="DISTILL.TEACHER"):
        Trainer(m, cfg)                                               # enabled, no name and no object
    with pytest.raises(ValueError, match="DISTILL.TEACHER_CKPT"):
        Trainer(m, x.get_config("XS", VIEWS + KD + ["DISTILL.TEACHER", "XS"]))
    # off: the teacher is not kept and the step takes the path it always took
    cfg0 = x.get_config("XS", VIEWS)
    tr0 = Trainer(m, cfg0, teacher=teacher)
    assert tr0.teacher is None
    pl = tr0.step(clips, labels, 0.0)
    assert pl.fwd[pl.grad_scale_slot][0] == "x3d_softmax_xent"
    torch.cuda.synchronize()


@pytest.mark.gpu
def test_trainer_builds_the_teacher_from_the_config(gpu, tmp_path):
    from x3d_tf_amd.config import config_path
    from x3d_tf_amd.train import Trainer
    few = ["NETWORK.NUM_CLASSES", 11]
    cfg0, arch, m, teacher = _models(gpu, few)
    os.makedirs(tmp_path / "teacher")
    prefix = str(tmp_path / "teacher" / "ckpt-7")
    teacher.save_weights(prefix)
    clips, labels, mask = _batch(arch)
    for name, ckpt in (("XS", prefix), (config_path("XS"), str(tmp_path / "teacher"))):   # shipped name | yaml path; prefix | directory
        cfg = x.get_config("XS", VIEWS + few + KD + ["DISTILL.TEACHER", name, "DISTILL.TEACHER_CKPT", ckpt])
        tr = Trainer(m, cfg)
        built = tr.teacher
        assert built is not None and built is not teacher and built is not m
        assert built.num_classes == 11 and built.dtype == m.dtype and built.device == m.device and not built.multi_label
        assert torch.equal(built.flat_params, teacher.flat_params)            # the checkpoint's weights and moving statistics
        pl = tr.step(clips.to(gpu), labels, 0.01)
        torch.cuda.synchronize()
        assert pl.fwd[pl.grad_scale_slot][0] == "x3d_softmax_xent_kd" and bool((pl.kd_rows > 0).all())
        assert torch.equal(built.flat_params, teacher.flat_params)
    with pytest.raises(FileNotFoundError):
        Trainer(m, x.get_config("XS", VIEWS + few + KD + ["DISTILL.TEACHER", "XS", "DISTILL.TEACHER_CKPT",
                                                          str(tmp_path / "nothing" / "ckpt-1")]))


@pytest.mark.gpu
def test_trainer_kd_loss_goes_down_on_a_repeated_batch(gpu):
    from x3d_tf_amd.train import Trainer
    cfg, arch, m, teacher = _models(gpu, ["DISTILL.ENABLE", True, "DISTILL.ALPHA", 1.0, "DISTILL.TEMPERATURE", 2.0])
    tr = Trainer(m, cfg, teacher=teacher)
    clips, labels, mask = _batch(arch)
    clips = clips.to(gpu)
    m.set_dropout_mask(mask)
    kd = []
    for _ in range(10):
        pl = tr.step(clips, labels, 0.1)
        kd.append(pl.kd_rows.double().mean())
    kd = [float(v) for v in kd]
    print("mean kd_rows per step:", " ".join(f"{v:.5f}" for v in kd))
    assert all(np.isfinite(kd)) and kd[-1] < kd[0], kd
    # a = 1: the combined rows are the KD rows
    assert torch.equal(pl.loss_rows, pl.kd_rows)


@pytest.mark.gpu
def test_fit_records_kd_loss_and_the_checkpoint_knows_no_teacher(gpu, tmp_path):
    from test_multilabel_gpu import OPTS, _write
    from x3d_tf_amd.checkpoint import read_index
    from x3d_tf_amd.model import X3D
    from x3d_tf_amd.train import Trainer
    opts = OPTS + ["TRAIN.EPOCHS", 1]
    cfg_on, cfg_off = x.get_config("XS", opts + KD), x.get_config("XS", opts)
    pattern = _write(str(tmp_path / "train"), 4, seed=4)
    teacher = X3D(cfg_on, dtype=torch.float32, device=gpu, seed=2)
    t_before = teacher.flat_params.clone()
    keys = {}
    for name, cfg, kw in (("on", cfg_on, dict(teacher=teacher)), ("off", cfg_off, {})):
        m = X3D(cfg, dtype=torch.float32, device=gpu, seed=1)
        tr = Trainer(m, cfg, **kw)
        ds = DL.InputReader(cfg, True, True, device=gpu, seed=3)(pattern, cfg.TRAIN.BATCH_SIZE)
        hist = tr.fit(ds, model_dir=str(tmp_path / name))
        ds.close()
        h = tr.history
        assert len(hist) == 1 and np.isfinite(hist[0])
        if name == "on":
            assert set(h) == {"loss", "lr", "acc", "top_5_acc", "kd_loss"}
            assert len(h["kd_loss"]) == 1 and np.isfinite(h["kd_loss"][0]) and h["kd_loss"][0] > 0
        else:
            assert set(h) == {"loss", "lr", "acc", "top_5_acc"}
        keys[name] = set(read_index(str(tmp_path / name / "ckpt-1") + ".index")[1])
        assert sorted(os.listdir(tmp_path / name)) == sorted(os.listdir(tmp_path / "on"))
    assert keys["on"] == keys["off"] and len(keys["on"]) > 100
    assert torch.equal(teacher.flat_params, t_before)


@pytest.mark.gpu
def test_fp16_student_scales_the_kd_gradient_by_the_loss_scale(gpu):
    from x3d_tf_amd.train import Trainer
    cfg, arch, m, teacher = _models(gpu, KD, dtype=torch.float16)
    tr = Trainer(m, cfg, teacher=teacher)
    assert tr.dynamic_scale and tr.loss_scale == 2.0 ** 15
    clips, labels, mask = _batch(arch)
    m.set_dropout_mask(mask)
    scale = tr.loss_scale
    pl = tr.step(clips.to(gpu), labels, 0.01)
    torch.cuda.synchronize()
    classes = arch.num_classes
    p2, d2 = torch.empty(N, classes, device=gpu), torch.empty(N, classes, device=gpu)
    ops.softmax_xent_kd(pl.logits, pl.teacher, p2, labels=pl.labels, dlogits=d2, grad_scale=1.0, alpha=0.5, temperature=2.0)
    torch.cuda.synchronize()
    report("dlogits", pl.dlogits, d2.double() * (scale / N), *DLOGITS)
    assert torch.equal(pl.probs, p2) and pl.dlogits.abs().max().item() > 0


@pytest.mark.gpu
def test_multi_label_step_runs_the_sigmoid_kd_head(gpu):
    from x3d_tf_amd.train import Trainer
    cfg, arch, m, teacher = _models(gpu, KD + ["DATA.MULTI_LABEL", True, "NETWORK.NUM_CLASSES", 157])
    tr = Trainer(m, cfg, teacher=teacher)
    clips, _, mask = _batch(arch)
    m.set_dropout_mask(mask)
    y = (torch.rand(N, 157, generator=torch.Generator().manual_seed(5)) < 0.05).float()
    pl = tr.step(clips.to(gpu), y, 0.01)
    torch.cuda.synchronize()
    assert pl.fwd[pl.grad_scale_slot][0] == "x3d_sigmoid_bce_kd" and torch.equal(pl.targets.cpu(), y)
    p2, r2, k2, d2 = (torch.empty(N, 157, device=gpu), torch.empty(N, device=gpu), torch.empty(N, device=gpu),
                      torch.empty(N, 157, device=gpu))
    ops.sigmoid_bce_kd(pl.logits, pl.teacher, pl.targets, p2, r2, k2, d2, 1.0 / N, 0.5, 2.0)
    torch.cuda.synchronize()
    assert torch.equal(pl.dlogits, d2) and torch.equal(pl.loss_rows, r2) and torch.equal(pl.probs, p2)
    assert torch.equal(pl.kd_rows, k2) and bool((k2 > 0).all())


@pytest.mark.gpu
def test_accumulation_distils_every_micro_batch(gpu):
    from x3d_tf_amd.train import Trainer
    cfg, arch, m, teacher = _models(gpu, KD + ["SOLVER.ACCUM_STEPS", 2])
    tr = Trainer(m, cfg, teacher=teacher)
    clips, labels, mask = _batch(arch)
    m.set_dropout_mask(mask)
    for micro in range(2):
        pl = tr.step(clips.to(gpu), labels, 0.01)
        assert pl.fwd[pl.grad_scale_slot][0] == "x3d_softmax_xent_kd" and tr.opt_step == micro
    torch.cuda.synchronize()
    assert bool(torch.isfinite(pl.kd_rows).all()) and bool(torch.isfinite(m.flat_params).all())


def _rehearsal_worker(rank, port, tmp):
    """one rank with every collective live (X3D_DIST_REHEARSE=1): a distilled step and a plain one, every all-reduce counted"""
    sys.path.insert(0, ROOT)
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK="0", WORLD_SIZE="1", LOCAL_RANK="0",
                      X3D_DIST_BACKEND="gloo", X3D_DIST_REHEARSE="1")
    import torch.distributed as dist
    from x3d_tf_amd import dist as xd
    from x3d_tf_amd.train import Trainer
    xd.init_process_group()
    dev = torch.device("cuda:0")
    torch.cuda.set_device(dev)
    cfg, arch, m, teacher = _models(dev, KD)
    clips, labels, mask = _batch(arch)
    m.set_dropout_mask(mask)
    reduced = []
    real = dist.all_reduce

    def counting(t, *a, **k):
        reduced.append(int(t.numel()))
        return real(t, *a, **k)
    dist.all_reduce = counting
    out = {}
    for name, c, kw in (("on", cfg, dict(teacher=teacher)), ("off", x.get_config("XS", VIEWS), {})):
        tr = Trainer(m, c, **kw)
        assert tr.collectives
        del reduced[:]
        pl = tr.step(clips.to(dev), labels, 0.0)
        out[name] = dict(step=sorted(reduced), buckets=sum(b.numel() for b in tr.reducer.buckets))
        if name == "on":
            del reduced[:]
            out["kd_loss"] = float(tr.kd_loss(pl))
            out["kd_rows_mean"] = float(pl.kd_rows.double().mean())
            out["kd_reduced"] = list(reduced)
    with open(os.path.join(tmp, "rehearsal.json"), "w") as f:
        json.dump(out, f)
    dist.barrier()
    dist.destroy_process_group()


@pytest.mark.gpu
def test_distilled_step_under_collectives_exchanges_what_the_plain_step_does(gpu, tmp_path):
    """data parallelism: the teacher is in no bucket and no collective -- a distilled step all-reduces exactly the tensors of
    a plain one -- and `kd_loss` is the all-reduced mean of the KD rows"""
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    mp.spawn(_rehearsal_worker, args=(port, str(tmp_path)), nprocs=1, join=True)
    r = json.load(open(tmp_path / "rehearsal.json"))
    assert r["on"]["step"] == r["off"]["step"] and len(r["on"]["step"]) > 1
    assert r["on"]["buckets"] == r["off"]["buckets"]
    assert r["kd_reduced"] == [1] and r["kd_loss"] > 0
    assert abs(r["kd_loss"] - r["kd_rows_mean"]) <= 1e-6 * r["kd_rows_mean"]
