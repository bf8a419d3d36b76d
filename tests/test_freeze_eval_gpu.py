"""SOLVER.FREEZE_EVAL on the device: a training step whose frozen prefix runs in inference form and whose backward pass ends at
the seam.  The numerical reference is the CPU oracle with the prefix's BatchNorm layers in inference mode
(tests/freeze_eval_ref.py); the cut of the backward list is also pinned on its own, against the full list on one forward
state.  Then the trainer (clipping, EMA, checkpoints), two data-parallel ranks and precise BatchNorm over a cut plan.
"""
import json
import os
import sys

import numpy as np
import pytest
import torch
import torch.multiprocessing as mp

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from tests import freeze_eval_ref as R  # noqa: E402
from tests.util import rel_l2, report  # noqa: E402

pytestmark = pytest.mark.gpu

F2 = ["conv1/", "stages/0/", "stages/1/"]
F3 = F2 + ["stages/2/"]


def _setup(name, seed=4):
    import x3d_tf_amd as x
    from x3d_tf_amd.params import init_params
    cfg = x.get_config(name)
    arch = x.build_arch(cfg)
    return cfg, arch, R.randomize_all_bn_(init_params(arch, seed=3), seed)


def _model(cfg, params, dtype, gpu, options=None):
    from x3d_tf_amd.model import X3D
    m = X3D(cfg, dtype=dtype, device=gpu, seed=0, options=options)
    m.load_state_dict(params)
    return m


def _scaled(name, got, ref, rel):
    scale = ref.detach().abs().max().item() + 1e-30
    return report(name, got, ref, 0, rel * scale)


def _mid_stage1(arch):
    from x3d_tf_amd.arch import block_prefix
    n0 = len(arch.stages[0].blocks)
    return ["conv1/", "stages/0/"] + [block_prefix(b) + "/" for b in arch.blocks[n0:n0 + 2]]


FP32_CASES = {          # label -> (n, t, s, FREEZE list or a function of the architecture, seed of the clips)
    "stem": (4, 4, 64, ["conv1/"], 1),
    "stage0-strided-shortcut": (4, 4, 64, ["conv1/", "stages/0/"], 1),
    "mid-stage1-identity-shortcut": (4, 4, 64, _mid_stage1, 1),
    # (seed 3, not 1: with all blocks frozen the trained region has 35 840 ReLU sites, so the 1e-5 below allows none to differ,
    # and the clips of seed 1 put an fc1 pre-activation at 2e-6, 0.15 of the fp32 rounding bound on it -- measured: that one
    # site differed, 2.8e-5 of the sites.  freeze_eval_ref.head_sign_margin: 0.15 for seed 1, 2.3 for seed 3; the test asserts
    # it is above 1, so the signs it compares are determined by the input and not by the order of an fp32 sum)
    "all-blocks-conv5": (4, 4, 64, ["conv1/", "stages/"], 3),
    "stage2-even-pixel-copy": (2, 4, 78, F3, 1),
}


@pytest.mark.parametrize("case", list(FP32_CASES))
def test_cut_step_fp32_against_the_eval_prefix_oracle(gpu, case):
    """One fp32 training step of X3D-XS with the frozen prefix in inference form, at the limits of test_train_step_fp32: the
    seam tensor, logits, loss, every trained tensor's gradient (the oracle is handed the device's ReLU signs of the trained
    region) and the trained region's moving statistics against the oracle; every prefix tensor's gradient exactly zero and the
    prefix's moving statistics bit-identical to what they were."""
    from oracle import x3d_oracle as O
    n, t, s, freeze, seed = FP32_CASES[case]
    cfg, arch, params = _setup("XS")
    freeze = freeze(arch) if callable(freeze) else freeze
    torch.manual_seed(seed)
    x = torch.randn(n, t, s, s, 3)
    labels = torch.randint(0, arch.num_classes, (n,))
    mask = (torch.rand(n, arch.fc1_out) >= arch.dropout_rate).float()

    m = _model(cfg, params, torch.float32, gpu)
    m.set_dropout_mask(mask)
    m.set_finetune(freeze=freeze, freeze_eval=True)
    k, L = m.frozen_prefix, len(arch.blocks)
    layers = R.prefix_bn_layers(arch, params, k)
    frozen, trained = R.split_names(arch, params, k)
    assert k >= 1 and layers and frozen and trained
    before = m.moving_stats_flat().clone()
    pl = m.forward_backward(x.to(gpu), labels.to(gpu))
    torch.cuda.synchronize()
    assert pl.frozen_prefix == k and pl.fwd[0][0] == "x3d_bn_eval_coef_batched"
    if case == "stage2-even-pixel-copy":
        B = pl.blocks[k - 1]
        assert (B.hh, B.ho) == (5, 3) and B.xs is not None
    if case == "stage0-strided-shortcut":
        assert pl.blocks[k - 1].spec.has_shortcut_conv and pl.blocks[k - 1].spec.stride == 2
    if case == "mid-stage1-identity-shortcut":
        assert not pl.blocks[k - 1].spec.has_shortcut_conv and pl.blocks[k - 1].spec.index == 2
    if case == "all-blocks-conv5":
        assert k == L + 1

    # the two semantics must be far apart on this input, or the comparison below could not tell them apart
    tap = R.seam_tap(arch, k)
    taps_batch = {}
    O.forward({a: v.clone() for a, v in params.items()}, x, arch, training=True, dropout_mask=mask, taps=taps_batch)
    taps, st, free_masks = {}, O.BNState(), O.RecordMasks()
    with R.eval_prefix(layers):
        O.forward({a: v.clone() for a, v in params.items()}, x, arch, training=True, dropout_mask=mask, state=st, taps=taps,
                  relu_masks=free_masks)
    apart = (taps_batch[tap] - taps[tap]).abs().max().item() / taps[tap].abs().max().item()
    print(f"{case}: seam tensor, batch statistics against moving statistics in the prefix: {apart:.3e} of its magnitude")
    assert apart > 100 * 2e-4

    e_seam = _scaled("seam " + tap, pl.seam, taps[tap], 2e-4)
    e_log = _scaled("logits", pl.logits, taps["logits"], 1e-4)
    # moving statistics: the prefix's untouched, bit for bit; the trained region's as the oracle's
    stats_prefix = {f"{q}/{w}" for q in layers for w in ("moving_mean", "moving_variance")}
    assert not stats_prefix & set(st.new_moving)
    for name in stats_prefix:
        assert torch.equal(m.params[name].cpu(), params[name]), name
    lo = m.trained_moving_stats_flat().data_ptr() - m.moving_stats_flat().data_ptr()
    assert lo == 4 * sum((params[a].numel() + 3) // 4 * 4 for a in stats_prefix)
    assert torch.equal(m.moving_stats_flat()[:lo // 4], before[:lo // 4])
    assert len(st.new_moving) + len(stats_prefix) == sum(1 for a in params if "/moving_" in a)
    for name, v in st.new_moving.items():
        report(name, m.params[name], v, 1e-4, 1e-5)

    dev_masks = R.trained_relu_masks(pl, k)
    frac, bad, tot = R.mask_mismatch(dev_masks, free_masks)
    assert set(dev_masks) <= set(free_masks) and tot > 0
    if tot * 1e-5 < 1:          # not one site may differ: then the input must determine every sign (k = L + 1 only)
        margin = R.head_sign_margin(params, arch, taps[tap])
        assert k == L + 1 and margin > 1, f"a ReLU pre-activation of the trained region lies at {margin:.2f} of its fp32 rounding bound"
    assert frac <= 1e-5, f"{bad} of {tot} ReLU signs of the trained region differ between the device and the free-running oracle"
    with R.eval_prefix(layers):
        r = O.train_step({a: v.clone() for a, v in params.items()}, x, labels, arch, lr=None, dropout_mask=mask,
                         apply_update=False, relu_masks=dev_masks)
        r64 = O.train_step({a: v.clone().double() for a, v in params.items()}, x.double(), labels, arch, lr=None,
                           dropout_mask=mask.double(), apply_update=False, relu_masks=dev_masks)
    fit = R.reference_is_fit(r["grads"], r64["grads"], trained, 1e-3, 2e-3)
    loss = pl.loss_rows.mean() + m.regularization_loss().float()
    report("loss", loss.view(1), r["loss"].view(1), 1e-5, 1e-5)
    worst = 0.0
    for name in trained:
        g = m.grads[name].cpu().double()
        if m.specs[name].l2:
            g = g + 2 * arch.weight_decay * params[name].double()
        e = rel_l2(g, r["grads"][name])
        worst = max(worst, e)
        assert e < 1e-3, f"grad {name}: relative L2 error {e:.3e}"
        _scaled("grad " + name, g, r["grads"][name], 2e-3)
    for name in frozen:
        assert not bool(m.grads[name].any()), f"{name}: a gradient of the frozen prefix is not zero"
    print(f"{case}: k = {k}, seam {e_seam:.2e}, logits {e_log:.2e} (abs), worst trained-gradient rel-L2 {worst:.2e}, "
          f"{bad} of {tot} ReLU signs differ; the reference against its fp64 evaluation: {fit[0]:.1e} rel-L2, {fit[1]:.1e} of max")


# ---- the cut on its own: truncated against full backward list, one forward state --------------------------------------
def _record_truncated(m, pl, k, **options):
    """record_backward(first_unit=k) over the forward state of `pl`, as tests/util.record_alternate_backward records a full
    list: its new accumulators in a zeroed buffer of their own.  Returns (launches, that buffer, the record)."""
    from x3d_tf_amd.plan import record_backward
    first = len(pl._zero_chunks)
    rec = record_backward(m, pl, dict(m.opt, **{a: bool(v) for a, v in options.items()}), first_unit=k)
    extra = pl.carve(first)
    pl.resolve()
    assert not rec.input_slots
    return rec.launches, extra, rec


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16, torch.float16], ids=["fp32", "bf16", "fp16"])
@pytest.mark.parametrize("name,n,t,s", [("M", 2, 4, 128), ("S", 3, 5, 96)])
def test_truncated_backward_against_the_full_backward(gpu, name, n, t, s, dtype):
    """The cut of the backward list, independently of the BatchNorm change: on an ORDINARY training plan the list is recorded
    again with first_unit = k -- at the stem, at the start of stage 1, inside stage 2 and at conv5 -- and both lists run from
    the same snapshot of the accumulators.  Tensors above the seam's two convs come from the same launches (2e-5: summation
    order of atomics); the seam's own convs and their BatchNorms agree at 2e-5 when both lists are recorded unfused, and
    within the general limit of test_model_gpu.RC_DIFF_LIMITS under default options, where the full list may recompute the
    conv output; what lies below the seam stays exactly zero."""
    import x3d_tf_amd as x
    from x3d_tf_amd import hip
    from x3d_tf_amd.arch import block_prefix
    from x3d_tf_amd.params import init_params, randomize_bn_
    from tests.test_model_gpu import RC_DIFF_LIMITS
    from tests.util import record_alternate_backward
    cfg = x.get_config(name)
    arch = x.build_arch(cfg)
    params = randomize_bn_(init_params(arch, seed=3), seed=4)
    torch.manual_seed(3)
    xg = torch.randn(n, t, s, s, 3).to(dtype).to(gpu)
    labels = torch.randint(0, arch.num_classes, (n,)).to(gpu)
    m = _model(cfg, params, dtype, gpu)
    m.set_dropout_mask((torch.rand(n, arch.fc1_out) >= arch.dropout_rate).float())
    ls = 1024.0 if dtype == torch.float16 else 1.0
    pl = m.forward_backward(xg, labels, loss_scale=ls)
    torch.cuda.synchronize()
    assert pl.frozen_prefix == 0
    per, L = [len(st.blocks) for st in arch.stages], len(arch.blocks)
    ks = [1, 1 + per[0], 1 + per[0] + per[1] + 2, L + 1]
    unit = R.unit_of(arch)
    unfused = record_alternate_backward(m, pl, xg, fused_pw_bwd=False)
    cuts = {(k, fused): _record_truncated(m, pl, k, **({} if fused else {"fused_pw_bwd": False})) for k in ks for fused in (True, False)}

    m._pack_panels()
    pl.zero_buf.zero_()
    pl.run(pl.fwd, 0, pl.grad_scale_slot)
    hip.call("x3d_softmax_xent", pl.logits.data_ptr(), pl.labels.data_ptr(), pl.probs.data_ptr(), pl.loss_rows.data_ptr(),
             pl.dlogits.data_ptr(), ls / n, n, arch.num_classes)
    snap = pl.zero_buf.clone()

    def run(lst, extra=None):
        pl.zero_buf.copy_(snap)
        m.flat_grads.zero_()
        if extra is not None:
            extra.zero_()
        pl.run(lst)
        torch.cuda.synchronize()
        assert torch.isfinite(m.flat_grads).all()
        return {a: g.detach().double().cpu().clone() for a, g in m.grads.items()}

    general = 2e-5 if dtype == torch.float32 else RC_DIFF_LIMITS[dtype][1]
    for fused in (True, False):
        full = pl.bwd if fused else unfused.lst
        g0 = run(full) if fused else run(full, unfused.extra)
        scale = {a: max(v.norm().item(), 1e-30) for a, v in g0.items()}
        med = sorted(scale[a] / g0[a].numel() ** 0.5 for a in g0)[len(g0) // 2]
        for k in ks:
            lst, extra, rec = cuts[(k, fused)]
            names = [e[0] for e in lst]
            assert not {"x3d_stem_bwd", "x3d_dwt_bwd", "x3d_stem_s_wgrad"} & set(names) and names[-1] == "x3d_pw_wgrad"
            assert names.count("x3d_dw3d_bwd") == L - (k - 1) and len(lst) < len(full)
            g1 = run(lst, extra)
            if k <= L:
                q = block_prefix(arch.blocks[k - 1])
                seam = tuple(f"{q}/{w}" for w in ("bottleneck/a/", "bottleneck/bn_a/", "residual/", "bn_r/"))
            else:
                seam = ("conv5/",)
            errs = {a: (g1[a] - g0[a]).norm().item() / max(scale[a], 0.05 * med * g0[a].numel() ** 0.5) for a in g0 if unit(a) >= k}
            worst_above = max(e for a, e in errs.items() if not a.startswith(seam))
            worst_seam = max(e for a, e in errs.items() if a.startswith(seam))
            print(f"{name} {dtype} first_unit {k} ({'default' if fused else 'unfused'}): {len(lst)} of {len(full)} launches, "
                  f"worst above the seam {worst_above:.2e}, seam convs {worst_seam:.2e}")
            assert worst_above < 2e-5, sorted(errs.items(), key=lambda kv: -kv[1])[:3]
            assert worst_seam < (general if fused else 2e-5), {a: e for a, e in errs.items() if a.startswith(seam)}
            for a in g0:
                if unit(a) < k:
                    assert not bool(g1[a].any()), f"first_unit {k}: {a} lies below the seam and is not zero"


def test_cut_step_bf16_end_to_end(gpu):
    """bf16 storage against the eval-prefix fp32 oracle at the limits of test_train_step_bf16_end_to_end_sanity: probabilities
    within 3e-3 abs, cross-entropy within 2 %, finite gradients, the gradient norm over the trained tensors within 30 %."""
    from oracle import x3d_oracle as O
    cfg, arch, params = _setup("XS")
    n, t, s = 4, 4, 96
    torch.manual_seed(2)
    x = torch.randn(n, t, s, s, 3).bfloat16().float()
    labels = torch.randint(0, arch.num_classes, (n,))
    mask = (torch.rand(n, arch.fc1_out) >= arch.dropout_rate).float()
    m = _model(cfg, params, torch.bfloat16, gpu)
    m.set_dropout_mask(mask)
    m.set_finetune(freeze=F2, freeze_eval=True)
    k = m.frozen_prefix
    frozen, trained = R.split_names(arch, params, k)
    pl = m.forward_backward(x.to(gpu), labels.to(gpu))
    torch.cuda.synchronize()
    with R.eval_prefix(R.prefix_bn_layers(arch, params, k)):
        r = O.train_step({a: v.clone() for a, v in params.items()}, x, labels, arch, lr=None, dropout_mask=mask, apply_update=False)
    report("probs", pl.probs, r["probs"], 0, 3e-3)
    report("ce", pl.loss_rows.mean().view(1), r["ce"].view(1), 2e-2, 0)
    assert torch.isfinite(m.flat_grads).all()
    g_dev = torch.cat([m.grads[a].reshape(-1).cpu().double() for a in trained])
    g_ref = torch.cat([(r["grads"][a].double() - (2 * arch.weight_decay * params[a].double() if m.specs[a].l2 else 0)).reshape(-1)
                       for a in trained])
    ratio = g_dev.norm().item() / g_ref.norm().item()
    print(f"bf16 cut step: trained-gradient norm {ratio:.3f} of the oracle's")
    assert abs(ratio - 1.0) < 0.3
    assert all(not bool(m.grads[a].any()) for a in frozen)


# ---- trainer ------------------------------------------------------------------------------------------------------------------
CLASSES = 10
OPTS = ["DATA.TEMP_DURATION", 4, "DATA.TRAIN_CROP_SIZE", 32, "DATA.TEST_CROP_SIZE", 32, "TEST.NUM_TEMPORAL_VIEWS", 1,
        "TEST.NUM_SPATIAL_CROPS", 3, "TEST.BATCH_SIZE", 2, "NETWORK.NUM_CLASSES", CLASSES, "NETWORK.DROPOUT_RATE", 0.0,
        "TRAIN.BATCH_SIZE", 2, "TRAIN.DATASET_SIZE", 4, "TRAIN.EPOCHS", 2]
CUT = ["SOLVER.FREEZE", F2, "SOLVER.FREEZE_EVAL", True]


def _cfg(*extra):
    import x3d_tf_amd as x
    return x.get_config("XS", OPTS + ["TRAIN.OPTIMIZER", "sgd"] + list(extra))


def _batches(count, seed=5, n=2):
    gen = torch.Generator().manual_seed(seed)
    return [(torch.randn(n, 4, 32, 32, 3, generator=gen), torch.randint(0, CLASSES, (n,), generator=gen)) for _ in range(count)]


def _trainer(cfg, dev, seed=1):
    """A model whose moving statistics are not the initial 0 / 1 (a step that touched them would show), and its trainer."""
    from x3d_tf_amd.model import X3D
    from x3d_tf_amd.train import Trainer
    m = X3D(cfg, dtype=torch.float32, device=dev, seed=seed)
    m.moving_stats_flat().copy_(0.5 + torch.rand(m.moving_stats_flat().numel(), generator=torch.Generator().manual_seed(seed)))
    return m, Trainer(m, cfg)


def _prefix_slices(m):
    """(slices of the prefix's trainable tensors, slices of its moving statistics, where the trained region's moving statistics
    begin) in flat_params; tensor by tensor: the padding between tensors belongs to nobody (a checkpoint does not carry it)"""
    unit = R.unit_of(m.arch)
    tr = [slice(sg.offset, sg.offset + sg.length) for sg in m.segments if unit(sg.name) < m.frozen_prefix]
    st = [slice(m._offsets[a], m._offsets[a] + m.params[a].numel()) for a in m.param_order
          if not m.specs[a].trainable and unit(a) < m.frozen_prefix]
    lo = (m.trained_moving_stats_flat().data_ptr() - m.flat_params.data_ptr()) // 4
    assert st and all(m.n_trainable_flat <= sl.start and sl.stop <= lo for sl in st)
    return tr, st, lo


def test_trainer_leaves_the_prefix_alone_and_resumes(gpu, tmp_path):
    """Three SGD steps with clipping and weight EMA over a cut plan: the prefix's weights, velocity, EMA copy and moving statistics
    keep their bits, every trained tensor moves, the backward list has no stem backward and one depthwise backward per trained
    block; a checkpoint after the first step resumes into the uninterrupted run, bit for bit."""
    cfg = _cfg("SOLVER.CLIP_GRAD_L2NORM", 0.05, "SOLVER.EMA_DECAY", 0.9, *CUT)
    (x1, y1), (x2, y2), (x3, y3) = [(a.to(gpu), b.to(gpu)) for a, b in _batches(3)]
    m, tr = _trainer(cfg, gpu)
    assert tr.freeze_eval and m.frozen_prefix == 1 + len(m.arch.stages[0].blocks) + len(m.arch.stages[1].blocks)
    nt = m.n_trainable_flat
    # a velocity on every tensor, as tests/test_finetune_gpu.py seeds it: with it every trained tensor moves (a BatchNorm scale
    # whose gradient is below an ulp of 1 too), and a frozen tensor that the update touched would show
    cover = torch.zeros(nt)
    for sg in m.segments:
        cover[sg.offset:sg.offset + sg.length] = 1
    vel = 0.01 * torch.randn(nt, generator=torch.Generator().manual_seed(1))
    vel[cover == 0] = 0.0                     # (+0 in the padding: a product with 0 would leave -0 here and there)
    m.flat_velocity.copy_(vel)
    w0, v0, e0 = m.flat_params.clone(), m.flat_velocity.clone(), tr.ema.clone()
    pl = tr.step(x1, y1, 0.05)
    tr.save_checkpoint(str(tmp_path), 1)
    tr.step(x2, y2, 0.05)
    g2 = m.flat_grads.clone()
    after2 = [m.flat_params[:nt].clone(), m.flat_velocity.clone(), tr.ema[:nt].clone()]
    tr.step(x3, y3, 0.05)
    torch.cuda.synchronize()
    assert tr.opt_step == 3 and torch.isfinite(m.flat_params).all()
    names = [e[0] for e in pl.bwd]
    assert pl.frozen_prefix == m.frozen_prefix and not {"x3d_stem_bwd", "x3d_dwt_bwd", "x3d_stem_s_wgrad"} & set(names)
    assert names.count("x3d_dw3d_bwd") == len(m.arch.blocks) - (m.frozen_prefix - 1)
    prefix, stats, trained_stats = _prefix_slices(m)
    for sl in prefix + stats:
        assert torch.equal(m.flat_params[sl], w0[sl]) and torch.equal(tr.ema[sl], e0[sl])
    for sl in prefix:
        assert torch.equal(m.flat_velocity[sl], v0[sl]) and not bool(m.flat_grads[sl].any())
    unit = R.unit_of(m.arch)
    for sg in m.segments:
        sl = slice(sg.offset, sg.offset + sg.length)
        assert torch.equal(m.flat_params[sl], w0[sl]) == (unit(sg.name) < m.frozen_prefix), sg.name
    assert not torch.equal(m.flat_params[trained_stats:], w0[trained_stats:])    # the trained region's moving statistics follow the batches
    # resume from the checkpoint of step 1: the second update, on the gradient the uninterrupted run computed (a recomputed
    # one differs in the summation order of atomics), gives the uninterrupted run's state bit for bit
    m2, tr2 = _trainer(cfg, gpu, seed=9)
    assert tr2.resume(str(tmp_path)) == 1 and tr2.opt_step == 1 and m2.frozen_prefix == m.frozen_prefix
    for sl in prefix + stats:
        assert torch.equal(m2.flat_params[sl], w0[sl]) and torch.equal(tr2.ema[sl], e0[sl])
    m2.flat_grads.copy_(g2)
    tr2._update(None, 0.05)
    assert tr2.opt_step == 2
    for a, b in zip(after2, [m2.flat_params[:nt], m2.flat_velocity, tr2.ema[:nt]]):
        assert torch.equal(a.view(torch.int32), b.view(torch.int32))
    # ... and the resumed trainer goes on over a cut plan of its own
    pl2 = tr2.step(x3, y3, 0.05)
    assert [e[0] for e in pl2.bwd] == names and tr2.opt_step == 3
    for sl in prefix + stats:
        assert torch.equal(m2.flat_params[sl], w0[sl])


# ---- two ranks ----------------------------------------------------------------------------------------------------------------
def _free_port():
    import socket
    with socket.socket() as sk:
        sk.bind(("127.0.0.1", 0))
        return sk.getsockname()[1]


def _rank_worker(rank, world, port, tmp):
    sys.path.insert(0, ROOT)
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world),
                      LOCAL_RANK=str(rank), X3D_DIST_BACKEND="gloo")
    import torch.distributed as dist
    from x3d_tf_amd import dist as xd
    r, lr_, w = xd.init_process_group()
    dev = torch.device(f"cuda:{xd.local_device(lr_)}")
    torch.cuda.set_device(dev)
    x1, y1 = _batches(1, seed=3 + rank)[0]                                          # every rank its own shard
    m, tr = _trainer(_cfg("SOLVER.CLIP_GRAD_L2NORM", 0.05, *CUT), dev, seed=1 + rank)
    w0 = m.flat_params.cpu()                                                        # rank 0's variables, broadcast
    fired, hook = [], tr._on_stage_done
    tr._on_stage_done = lambda stage: (fired.append(stage), hook(stage))[1]
    tr.step(x1.to(dev), y1.to(dev), 0.05)
    torch.cuda.synchronize()
    torch.save(dict(w0=w0, w=m.flat_params.cpu(), v=m.flat_velocity.cpu(), g=m.flat_grads.cpu(), norm=tr.last_grad_norm.cpu()),
               os.path.join(tmp, f"rank{rank}.pt"))
    prefix, stats, trained_stats = _prefix_slices(m)
    with open(os.path.join(tmp, f"rank{rank}.json"), "w") as f:
        json.dump(dict(fired=fired, world=tr.world, collectives=bool(tr.collectives), k=m.frozen_prefix, stages=len(m.arch.stages),
                       prefix=[[sl.start, sl.stop] for sl in prefix], stats=[[sl.start, sl.stop] for sl in stats], trained_stats=trained_stats,
                       nt=m.n_trainable_flat), f)
    dist.barrier()
    dist.destroy_process_group()


def test_two_ranks_step_over_a_cut_plan(gpu, tmp_path):
    """Two data-parallel ranks (gloo, one GPU): the bucket hooks fire once each in the order they always fired -- the buckets of
    the prefix carry zeros --, both ranks end the step with the same parameters, and the prefix is untouched on both."""
    mp.spawn(_rank_worker, args=(2, _free_port(), str(tmp_path)), nprocs=2, join=True)
    r0, r1 = (torch.load(tmp_path / f"rank{r}.pt") for r in (0, 1))
    i0, i1 = (json.load(open(tmp_path / f"rank{r}.json")) for r in (0, 1))
    n_st = i0["stages"]
    assert i0["world"] == 2 and i0["collectives"] and i0["k"] == i1["k"] > 1
    assert i0["fired"] == i1["fired"] == ["fwd", n_st] + list(range(n_st - 1, -1, -1)) + [-1]
    nt = i0["nt"]
    assert torch.equal(r0["w0"], r1["w0"])
    for key in ("w", "v", "g", "norm"):
        assert torch.equal(r0[key], r1[key]), key
    assert bool(torch.isfinite(r0["w"]).all()) and float(r0["norm"]) > 0
    for r in (r0, r1):
        for lo, hi in i0["prefix"] + i0["stats"]:
            assert torch.equal(r["w"][lo:hi], r["w0"][lo:hi])
        for lo, hi in i0["prefix"]:
            assert not bool(r["g"][lo:hi].any()) and not bool(r["v"][lo:hi].any())
    assert not torch.equal(r0["w"][:nt], r0["w0"][:nt]) and not torch.equal(r0["w"][i0["trained_stats"]:], r0["w0"][i0["trained_stats"]:])


# ---- precise BatchNorm ------------------------------------------------------------------------------------------------------
def test_precise_bn_over_a_cut_plan(gpu):
    """Two batches through precise_bn.update_bn_stats on a model with a frozen prefix in inference form: the prefix's moving
    statistics keep their bits; every trained layer's are the pooled fp64 statistics of tests/precise_bn_ref.py, to the 1 ulp
    of tests/test_precise_bn_gpu.py (the reference pools the raw sums of a second run of the same forward passes)."""
    from tests import precise_bn_ref as PR
    from x3d_tf_amd import hip
    from x3d_tf_amd.model import X3D
    from x3d_tf_amd.precise_bn import update_bn_stats
    m = X3D(_cfg(), dtype=torch.float32, device=gpu, seed=1)
    gen = torch.Generator().manual_seed(11)
    m.moving_stats_flat().copy_(0.5 + torch.rand(m.moving_stats_flat().numel(), generator=gen))
    m.set_finetune(freeze=F2, freeze_eval=True)
    layers = R.prefix_bn_layers(m.arch, m.params, m.frozen_prefix)
    clips = [torch.randn(n, 4, 32, 32, 3, generator=gen).to(gpu) for n in (2, 3)]
    before = m.flat_params.clone()
    assert update_bn_stats(m, clips, 2) == 2
    torch.cuda.synchronize()
    assert torch.equal(m.flat_params[:m.n_trainable_flat], before[:m.n_trainable_flat])
    got = {a: v.detach().cpu().numpy().copy() for a, v in m.params.items() if a.endswith(("/moving_mean", "/moving_variance"))}
    for q in layers:
        for w in ("moving_mean", "moving_variance"):
            assert torch.equal(m.params[f"{q}/{w}"], before[m._offsets[f"{q}/{w}"]:][:m.params[f"{q}/{w}"].numel()]), q
    reps, lib = int(hip.load().x3d_stats_replicas()), hip.load()
    per_layer = {}
    for c in clips:
        m(c, training=True)
        pl = m._plan(*c.shape[:4], True)
        torch.cuda.synchronize()
        assert pl.frozen_prefix == m.frozen_prefix and pl.precise_bn_table().shape[0] == len(pl.bn_layers)
        for b in pl.bn_layers:
            raw = pl._zero_views[b.stats].cpu().numpy()
            per_layer.setdefault(b.prefix, []).append((PR.replica_sum(raw, b.c, reps, int(lib.x3d_stats_stride(b.c))), b.count))
    assert not set(per_layer) & set(layers) and (len(per_layer) + len(layers)) * 2 == len(got)
    worst = 0.0
    for q, parts in per_layer.items():
        sums, count = PR.pool(parts)
        mean, unb = PR.final(sums, count)
        worst = max(worst, PR.ulps(got[f"{q}/moving_mean"], mean).max(), PR.ulps(got[f"{q}/moving_variance"], unb).max())
        assert not np.array_equal(got[f"{q}/moving_mean"], before[m._offsets[f"{q}/moving_mean"]:][:len(mean)].cpu().numpy()), q
    print(f"precise BatchNorm over a cut plan: {len(per_layer)} layers, worst distance from the pooled fp64 reference {worst} ulp")
    assert worst <= 1.0
