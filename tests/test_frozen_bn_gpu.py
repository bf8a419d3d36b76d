"""SOLVER.FREEZE_BN on the device: the frozen form of the BatchNorm-backward rule in the kernels that carry it -- against fp64
closed forms written here, and bit for bit against the batch form where the expressions are shared -- and training steps whose
frozen layers normalise with their moving statistics, against the CPU oracle with those layers in inference mode
(tests/frozen_bn_ref.py).  Then the plan options, 16-bit storage, the composition with a frozen prefix, the trainer and two ranks.
"""
import json
import os
import sys

import pytest
import torch
import torch.multiprocessing as mp
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from tests import frozen_bn_ref as R  # noqa: E402
from tests.util import hip_relu_masks, rel_l2, report  # noqa: E402

pytestmark = pytest.mark.gpu

HALF = [torch.bfloat16, torch.float16]


def _ops():
    from x3d_tf_amd import ops
    return ops


def _gen(seed):
    return torch.Generator().manual_seed(seed)


def _plus_zero(t):
    """every element is +0.0: the bits, not the value (-0.0 == 0.0)"""
    return bool((t.contiguous().view(torch.int32) == 0).all())


def _bn_inputs(c, m_, gpu, seed):
    g_ = _gen(seed)
    sums = (torch.randn((c, 2), generator=g_, dtype=torch.float64) * m_ ** 0.5).to(gpu)
    mi = torch.stack([0.3 * torch.randn(c, generator=g_), 0.5 + torch.rand(c, generator=g_)], 1).contiguous().to(gpu)
    gamma = (1 + 0.3 * torch.randn(c, generator=g_)).to(gpu)
    return sums, mi, gamma


# ---- the rule in the finalize kernels -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("c", [1, 24, 223, 432])
def test_frozen_bn_bwd_finalize(gpu, c):
    """x3d_bn_bwd_finalize with a negative count: B and C exactly +0, A / dgamma / dbeta the bits of the batch form on the same
    sums and mean_invstd (the same expressions), all three at fp32 rounding of the fp64 closed form; x3d_bn_bwd_finalize_rc
    (C <= 223 with a panel job; any C without) writes the same bits."""
    ops = _ops()
    from x3d_tf_amd import hip
    m_ = 4 * 4 * 16 * 16
    sums, mi, gamma = _bn_inputs(c, m_, gpu, 70 + c)
    out = {}
    for tag, count in (("batch", float(m_)), ("frozen", -float(m_))):
        coef = torch.full((c, 4), 7.0, device=gpu)
        dga, dbe = torch.full((c,), 0.25, device=gpu), torch.full((c,), -0.5, device=gpu)
        ops.bn_bwd_finalize(sums, count, mi, gamma, coef, dga, dbe)
        torch.cuda.synchronize()
        out[tag] = (coef, dga, dbe)
    (cb, gb, bb), (cf, gf, bf) = out["batch"], out["frozen"]
    assert _plus_zero(cf[:, 1]) and _plus_zero(cf[:, 2]) and _plus_zero(cf[:, 3])
    assert bool((cb[:, 1] != 0).any()) and bool((cb[:, 2] != 0).any())                 # (the batch form is not trivially that)
    assert torch.equal(cf[:, 0], cb[:, 0]) and torch.equal(gf, gb) and torch.equal(bf, bb)
    a64, b64, c64, dga64, dbe64 = R.bn_bwd_closed_form(sums, mi, gamma)
    report("A", cf[:, 0], a64, 2e-7, 0)
    report("dgamma", gf - 0.25, dga64, 1e-6, 1e-6 * dga64.abs().max().item())
    report("dbeta", bf + 0.5, dbe64, 1e-6, 1e-6 * dbe64.abs().max().item())
    ab, bb64, cb64, _, _ = R.bn_bwd_closed_form(sums, mi, gamma, float(m_))
    report("B (batch)", cb[:, 1], bb64, 1e-6, 1e-6 * bb64.abs().max().item())
    report("C (batch)", cb[:, 2], cb64, 1e-6, 1e-6 * cb64.abs().max().item())
    # the merged launch: alone for any C, with the panel of a 24-channel conv in front of it where the form covers the layer
    lib, cin = hip.load(), (48 if c > 127 else 24)      # (a conv the recomputed-output form covers: x3d_pw_bwd_rc_panel_elems)
    for dtype in HALF:
        pe = int(lib.x3d_pw_bwd_rc_panel_elems(c, cin)) if c <= 223 else 0
        coef = torch.full((c, 4), 7.0, device=gpu)
        dga, dbe = torch.full((c,), 0.25, device=gpu), torch.full((c,), -0.5, device=gpu)
        prep = None
        if pe:
            w = (torch.randn((c, cin), generator=_gen(5)) * 0.2).to(gpu)
            prep = (w, torch.ones(pe, dtype=dtype, device=gpu), torch.ones(cin, device=gpu))
        ops.bn_bwd_finalize_rc(sums, -float(m_), mi, gamma, coef, dga, dbe, dtype, prep=prep)
        torch.cuda.synchronize()
        assert torch.equal(coef, cf) and torch.equal(dga, gf) and torch.equal(dbe, bf)
        if prep is not None:
            # the panel [W^T A | W^T B W] and c0 = W^T C of the recomputed-output form, taken as data: with B = C = 0 the second
            # block and c0 vanish -- the same bits as x3d_pw_bwd_rc_prepare on the frozen table
            pan, c0 = torch.ones(pe, dtype=dtype, device=gpu), torch.ones(cin, device=gpu)
            hip.call("x3d_pw_bwd_rc_prepare", w.data_ptr(), cf.data_ptr(), pan.data_ptr(), c0.data_ptr(), c, cin, hip.dtype_code(dtype))
            torch.cuda.synchronize()
            assert torch.equal(pan, prep[1]) and torch.equal(c0, prep[2]) and _plus_zero(c0)
    assert c == 432 or pe > 0


# ---- x3d_se_bnb_bwd -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("jobs", [0, 2])
@pytest.mark.parametrize("c,wd", [(8, 8), (54, 16)])
@pytest.mark.parametrize("n", [1, 3, 65])
@pytest.mark.parametrize("has_se", [True, False])
def test_frozen_se_bnb_bwd(gpu, has_se, n, c, wd, jobs):
    """tests/test_kernels_gpu.py::test_se_bnb_bwd with BN_b on CONSTANT statistics (P < 0): u = gamma * (braw - mean) * invstd + beta
    -> (SE gate) -> v ; L = sum(dv * v).  coef_nc[..., 1] is exactly +0; coef_nc[..., 0] = k1 * gate and coef_nc[..., 2] = k1 * dpool / P
    against fp64, the table reproduces dL/dbraw, and the six parameter gradients are autograd's -- at that test's tolerances.
    The reduce slots ride along as there."""
    ops = _ops()
    gj = _gen(90 + jobs)
    red = []
    for parts, elems in [(251, 96 * 216), (7, 20 * 12)][:jobs]:
        slab = torch.randn((parts * elems,), generator=gj).to(gpu)
        red.append((slab, torch.full((elems,), 0.5, device=gpu), parts))
    T, H, W = 2, 3, 4
    P = T * H * W
    g_ = _gen(9)
    braw = torch.randn((n, c, T, H, W), generator=g_, dtype=torch.float64)
    dv = torch.randn((n, c, T, H, W), generator=g_, dtype=torch.float64)
    gamma = (1 + 0.2 * torch.randn(c, generator=g_)).double().requires_grad_(True)
    beta = (0.2 * torch.randn(c, generator=g_)).double().requires_grad_(True)
    w1 = (torch.randn((wd, c), generator=g_) * 0.3).double().requires_grad_(True)
    b1 = (torch.randn(wd, generator=g_) * 0.1).double().requires_grad_(True)
    w2 = (torch.randn((c, wd), generator=g_) * 0.3).double().requires_grad_(True)
    b2 = (torch.randn(c, generator=g_) * 0.1).double().requires_grad_(True)
    # the moving statistics: constants that are NOT the batch's (rounded to fp32, as the device holds them)
    mu = (0.3 * torch.randn(c, generator=g_)).double()
    inv = (0.5 + torch.rand(c, generator=g_)).double()
    x_ = braw.clone().requires_grad_(True)
    sh = (1, -1, 1, 1, 1)
    u = (x_ - mu.view(sh)) * inv.view(sh) * gamma.view(sh) + beta.view(sh)
    if has_se:
        pooled = u.mean((2, 3, 4))
        h = F.relu(pooled @ w1.t() + b1)
        gate = torch.sigmoid(h @ w2.t() + b2)
        v = u * gate[:, :, None, None, None]
    else:
        v = u
    params = [x_, gamma, beta] + ([w1, b1, w2, b2] if has_se else [])
    grads = torch.autograd.grad((v * dv).sum(), params)
    f32 = lambda t_: t_.detach().float().to(gpu).contiguous()
    bss = torch.stack([(gamma * inv).detach(), (beta - mu * gamma * inv).detach()], 1)
    bmi = torch.stack([mu, inv], 1)
    nc_sums = torch.stack([dv.sum((2, 3, 4)), (dv * braw).sum((2, 3, 4))], -1).to(gpu)
    pool_sums = braw.sum((2, 3, 4)).to(gpu)
    coef_nc = torch.full((n, c, 4), 7.0, device=gpu)
    dgam, dbet = torch.zeros(c, device=gpu), torch.zeros(c, device=gpu)
    kw = {}
    if has_se:
        kw = dict(w1=f32(w1), b1=f32(b1), w2=f32(w2), b2=f32(b2), gate=f32(gate), hidden=f32(h),
                  dw1=torch.zeros((wd, c), device=gpu), db1=torch.zeros(wd, device=gpu),
                  dw2=torch.zeros((c, wd), device=gpu), db2=torch.zeros(c, device=gpu),
                  scratch=torch.empty(n * (2 * c + wd), device=gpu))
    ops.se_bnb_bwd(nc_sums, pool_sums if has_se else None, -float(P), f32(bss), f32(bmi), f32(gamma), dgam, dbet, coef_nc,
                   n, c, reduce=red, **kw)
    torch.cuda.synchronize()
    for slab, dwj, parts in red:
        ref = slab.double().view(parts, -1).sum(0) + 0.5
        report("slab sum", dwj, ref, 1e-6, 2e-6 * ref.abs().max().item())
    assert _plus_zero(coef_nc[:, :, 1]) and _plus_zero(coef_nc[:, :, 3])
    cf = coef_nc.cpu().double()
    k1 = (gamma * inv).detach()
    g64 = gate.detach() if has_se else torch.ones(n, c, dtype=torch.float64)
    report("coef_nc[0] = k1 * gate", cf[:, :, 0], k1.view(1, -1) * g64, 2e-4, 2e-5)
    # coef_nc[2] = k1 * dpool / P: what autograd's dL/dbraw holds beside k1 * gate * dv, the same at every point of (n, c)
    rest = grads[0] - (k1.view(1, -1) * g64)[:, :, None, None, None] * dv
    assert float((rest - rest.mean((2, 3, 4), keepdim=True)).abs().max()) < 1e-12
    report("coef_nc[2] = k1 * dpool / P", cf[:, :, 2], rest.mean((2, 3, 4)), 2e-4, 2e-5)
    if not has_se:
        assert _plus_zero(coef_nc[:, :, 2])
    dB = cf[:, :, 0, None, None, None] * dv + cf[:, :, 1, None, None, None] * braw + cf[:, :, 2, None, None, None]
    report("dbraw", dB, grads[0], 2e-4, 2e-5)
    report("dgamma_b", dgam, grads[1], 2e-4, 2e-4)
    report("dbeta_b", dbet, grads[2], 2e-4, 2e-4)
    if has_se:
        report("dw1", kw["dw1"], grads[3], 2e-4, 2e-5)
        report("db1", kw["db1"], grads[4], 2e-4, 2e-5)
        report("dw2", kw["dw2"], grads[5], 2e-4, 2e-5)
        report("db2", kw["db2"], grads[6], 2e-4, 2e-5)


# ---- model level, fp32, against the oracle under eval_prefix(frozen layers) ---------------------------------------------------
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


FP32_CASES = {          # label -> (n, t, s, SOLVER.FREEZE_BN, seed of the clips, moving statistics calibrated from a second batch)
    "all": (4, 4, 64, [""], 1, False),
    "stages23-conv5": (4, 4, 64, ["stages/2/", "stages/3/", "conv5/"], 1, False),
    "stage1": (4, 4, 64, ["stages/1/"], 1, False),
    "all-even-pixel-copy": (2, 4, 78, [""], 1, True),
}


def _frozen_step_fp32(gpu, label, n, t, s, finetune, seed, calibrate):
    """One fp32 step of X3D-XS under `finetune` (set_finetune's keywords) at the limits of
    test_cut_step_fp32_against_the_eval_prefix_oracle; the oracle runs every layer that is frozen -- or in the prefix -- in
    inference mode.  Returns (model, plan)."""
    from oracle import x3d_oracle as O
    cfg, arch, params = _setup("XS")
    torch.manual_seed(seed)
    x = torch.randn(n, t, s, s, 3)
    labels = torch.randint(0, arch.num_classes, (n,))
    mask = (torch.rand(n, arch.fc1_out) >= arch.dropout_rate).float()
    if calibrate:
        R.calibrated_moving_stats_(params, arch, torch.randn(n, t, s, s, 3, generator=_gen(77)))

    m = _model(cfg, params, torch.float32, gpu)
    m.set_dropout_mask(mask)
    m.set_finetune(**finetune)
    k = m.frozen_prefix
    layers = sorted(set(m.frozen_bn) | set(R.prefix_bn_layers(arch, params, k)))
    assert layers == sorted(set(R.frozen_layers(params, finetune["freeze_bn"])) | set(R.prefix_bn_layers(arch, params, k)))
    frozen, trained = R.split_names(arch, params, k)
    before = m.moving_stats_flat().clone()
    pl = m.forward_backward(x.to(gpu), labels.to(gpu))
    torch.cuda.synchronize()
    names = [e[0] for e in pl.fwd]
    assert names[0] == "x3d_bn_eval_coef_batched" and names.count(names[0]) == 1 and pl.fwd[0][2][1] == len(layers)
    assert names.count("x3d_bn_finalize") == len(R.bn_layers(params)) - len(layers)

    # the two semantics must be far apart on this input, or the comparison below could not tell them apart
    taps_batch = {}
    O.forward({a: v.clone() for a, v in params.items()}, x, arch, training=True, dropout_mask=mask, taps=taps_batch)
    taps, st, free_masks = {}, O.BNState(), O.RecordMasks()
    with R.eval_prefix(layers):
        O.forward({a: v.clone() for a, v in params.items()}, x, arch, training=True, dropout_mask=mask, state=st, taps=taps,
                  relu_masks=free_masks)
    apart = (taps_batch["logits"] - taps["logits"]).abs().max().item() / taps["logits"].abs().max().item()
    print(f"{label}: logits, batch statistics against moving statistics in {len(layers)} layers: {apart:.3e} of their magnitude")
    assert apart > 100 * 1e-4

    e_log = _scaled("logits", pl.logits, taps["logits"], 1e-4)
    # moving statistics: the frozen layers' untouched, bit for bit; the others' as the oracle's
    held = R.stat_names(layers)
    assert not held & set(st.new_moving) and len(st.new_moving) + len(held) == sum(1 for a in params if "/moving_" in a)
    for name in held:
        assert torch.equal(m.params[name].cpu(), params[name]), name
    if len(layers) == len(R.bn_layers(params)):
        assert torch.equal(m.moving_stats_flat(), before)
    for name, v in st.new_moving.items():
        report(name, m.params[name], v, 1e-4, 1e-5)

    dev_masks = R.trained_relu_masks(pl, k) if k else hip_relu_masks(pl)
    frac, bad, tot = R.mask_mismatch(dev_masks, free_masks)
    assert set(dev_masks) <= set(free_masks) and tot > 1e5
    assert frac <= 1e-5, f"{bad} of {tot} ReLU signs differ between the device and the free-running oracle"
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
    print(f"{label}: {len(layers)} layers on moving statistics, logits {e_log:.2e} (abs), worst gradient rel-L2 {worst:.2e}, {bad} of "
          f"{tot} ReLU signs differ; the reference against its fp64 evaluation: {fit[0]:.1e} rel-L2, {fit[1]:.1e} of max")
    return m, pl


@pytest.mark.parametrize("case", list(FP32_CASES))
def test_frozen_step_fp32_against_the_eval_prefix_oracle(gpu, case):
    """Logits 1e-4 of the maximum, loss 1e-5, every trainable tensor's gradient relative L2 < 1e-3 and 2e-3 of its largest
    value (the oracle is handed the device's ReLU signs, of which at most 1e-5 differ from the free-running oracle's), the frozen
    layers' moving statistics bit-identical, the others' as the oracle's -- which has no entry for a frozen layer.  The
    reference is first required to be within a tenth of the limits of its own fp64 evaluation, and the two semantics to be more
    than 100 logits tolerances apart on the input."""
    n, t, s, freeze_bn, seed, calibrate = FP32_CASES[case]
    m, pl = _frozen_step_fp32(gpu, case, n, t, s, dict(freeze_bn=freeze_bn), seed, calibrate)
    if case == "all-even-pixel-copy":
        B = next(B for B in pl.blocks if B.xs is not None and (B.hh, B.ho) == (5, 3))
        assert B.spec.stride == 2
    if case == "all":
        assert not pl.bn_layers and all(e[2][1] < 0 for e in pl.bwd if e[0].startswith("x3d_bn_bwd_finalize"))


def test_composition_with_freeze_and_a_frozen_prefix(gpu):
    """FREEZE = [conv1/, stages/0/] with FREEZE_EVAL and FREEZE_BN = [""]: one batched coefficient launch at slot 0 over the
    prefix layers and the frozen layers above them, the prefix's gradients exactly zero, everything above the seam against the
    oracle as above."""
    m, pl = _frozen_step_fp32(gpu, "prefix + every layer", 4, 4, 64,
                              dict(freeze=["conv1/", "stages/0/"], freeze_eval=True, freeze_bn=[""]), 1, False)
    assert pl.frozen_prefix == 1 + len(m.arch.stages[0].blocks) and pl.seam is not None
    assert not any(e[0] in ("x3d_stem_bwd", "x3d_dwt_bwd", "x3d_stem_s_wgrad") for e in pl.bwd)


# ---- off is off ---------------------------------------------------------------------------------------------------------------
def test_off_is_off(gpu):
    """freeze_bn = () against a model that was never given the argument: the same launch list, and one step from the same
    state leaves bit-identical gradients and moving statistics.

    Bit-identical as far as the step itself is: the backward pass flushes weight gradients and sums with floating-point atomics,
    so two runs of the SAME model on the same input differ in the last bits of some tensors (measured here: the first element of
    conv1/conv_s/kernel's gradient, 2 ulp, between two models of identical launch lists).  So the untold model runs twice: if
    those two runs reproduce every gradient bit for bit, so must the told model; if not, bit-identity of the gradients is not a
    property any implementation has, and the told model's must agree within the 2e-5 (relative L2) the suite allows the
    summation order of atomics (test_launch_saving_plan_options_do_not_change_the_gradients).  What the forward pass leaves --
    the loss rows and the moving statistics -- is bit-identical either way.  That the lists are equal argument by argument is
    tests/test_frozen_bn.py::test_with_the_key_off_a_plan_records_what_it_recorded."""
    cfg, arch, params = _setup("XS")
    torch.manual_seed(1)
    n, t, s = 2, 4, 32
    x = torch.randn(n, t, s, s, 3).to(gpu)
    labels = torch.randint(0, arch.num_classes, (n,)).to(gpu)
    mask = (torch.rand(n, arch.fc1_out) >= arch.dropout_rate).float()
    got = []
    for told in (False, False, True):
        m = _model(cfg, params, torch.float32, gpu)
        m.set_dropout_mask(mask)
        if told:
            m.set_finetune(freeze_bn=())
        pl = m.forward_backward(x, labels)
        torch.cuda.synchronize()
        tensors = {"grad " + a_: g.clone() for a_, g in m.grads.items()}
        tensors.update({a_: v.clone() for a_, v in m.params.items() if "/moving_" in a_})
        tensors["loss"] = pl.loss_rows.clone()
        got.append(([e[0] for e in pl.fwd], [e[0] for e in pl.bwd], tensors))
        assert (n, t, s, s, True) in m._plans
    a, a2, b = got
    assert a[0] == b[0] and a[1] == b[1] and a[0][0] != "x3d_bn_eval_coef_batched"
    same = lambda u, v: torch.equal(u.view(torch.int32), v.view(torch.int32))
    noisy = [k for k in a[2] if not same(a[2][k], a2[2][k])]
    print(f"off is off: {len(noisy)} of {len(a[2])} tensors differ between two runs of the untold model: {noisy[:6]}")
    assert not any("/moving_" in k for k in noisy) and "loss" not in noisy
    for k, v in a[2].items():
        if noisy and k.startswith("grad "):
            assert rel_l2(b[2][k], v) < 2e-5, k
        else:
            assert same(b[2][k], v), k


# ---- plan options -------------------------------------------------------------------------------------------------------------
ALT_OPTIONS = ["pw_bwd_rc", "coef_fold", "fused_pw_bwd", "dw_slab", "tail_bwd_fold"]


@pytest.mark.parametrize("name,n,t,s", [("M", 2, 4, 128), ("S", 3, 5, 96)])
def test_plan_options_over_frozen_layers(gpu, name, n, t, s):
    """FREEZE_BN = [""] in bf16, every launch-list option of the backward pass turned off in turn on ONE forward state
    (tests/util.record_alternate_backward): where the option changes no launch of this plan the lists are equal; where it does,
    the gradients agree within the bounds the batch-statistics tests hold the same switches to -- 2e-5 for the switches that move
    a computation without changing its operands (dw_slab: test_launch_saving_plan_options_do_not_change_the_gradients;
    tail_bwd_fold: the same kind; coef_fold changes no launch here -- a frozen layer's finalize is always a launch) and test_model_gpu.RC_DIFF_LIMITS for those that change an operand's rounding (pw_bwd_rc;
    fused_pw_bwd, which also turns the recomputed-output form off).  A form that assumed batch statistics would be an O(1)
    error on the tensors below it.  (stem_fused is a property of the forward list: test_frozen_step_half runs it.)"""
    from tests.test_model_gpu import RC_DIFF_LIMITS
    from tests.util import record_alternate_backward
    from x3d_tf_amd import hip
    cfg, arch, params = _setup(name)
    dtype = torch.bfloat16
    torch.manual_seed(3)
    x = torch.randn(n, t, s, s, 3).to(dtype).to(gpu)
    labels = torch.randint(0, arch.num_classes, (n,)).to(gpu)
    m = _model(cfg, params, dtype, gpu)
    m.set_dropout_mask((torch.rand(n, arch.fc1_out) >= arch.dropout_rate).float())
    m.set_finetune(freeze_bn=[""])
    pl = m.forward_backward(x, labels)
    torch.cuda.synchronize()
    assert pl.fwd[0][0] == "x3d_bn_eval_coef_batched" and not pl.bn_layers
    names = [e[0] for e in pl.bwd]
    assert not any(getattr(pl.structs.get((id(pl.bwd), i)), "coef_fold", None) for i in range(len(pl.bwd)))
    alts = {off: record_alternate_backward(m, pl, x, **{off: False}) for off in ALT_OPTIONS}
    m._pack_panels()
    pl.zero_buf.zero_()
    pl.run(pl.fwd, 0, pl.grad_scale_slot)
    hip.call("x3d_softmax_xent", pl.logits.data_ptr(), pl.labels.data_ptr(), pl.probs.data_ptr(), pl.loss_rows.data_ptr(),
             pl.dlogits.data_ptr(), 1.0 / n, n, arch.num_classes)
    snap = pl.zero_buf.clone()

    def run(runner):
        pl.zero_buf.copy_(snap)
        m.flat_grads.zero_()
        runner()
        torch.cuda.synchronize()
        assert torch.isfinite(m.flat_grads).all()
        return {a: g.detach().double().cpu().clone() for a, g in m.grads.items()}

    g1 = run(lambda: pl.run(pl.bwd))
    _, lim, lim_g, lim_se, _ = RC_DIFF_LIMITS[dtype]
    cls = lambda a: ("se" if a.endswith(("/se_fc1/bias", "/se_fc2/bias", "/se_fc1/kernel")) else ("gamma" if a.endswith("/gamma") else "general"))
    for off, alt in alts.items():
        alt_names = [e[0] for e in alt.lst]
        if alt_names == names and off != "dw_slab":
            print(f"{name} plan option {off}: changes no launch of this plan")
            continue
        g0 = run(alt.run)
        scale = {a: max(v.norm().item(), 1e-30) for a, v in g0.items()}
        med = sorted(scale[a] / g0[a].numel() ** 0.5 for a in g0)[len(g0) // 2]
        errs = {a: (g1[a] - g0[a]).norm().item() / max(scale[a], 0.05 * med * g0[a].numel() ** 0.5) for a in g0}
        worst = sorted(errs.items(), key=lambda kv: -kv[1])[:3]
        print(f"{name} plan option {off}: {len(alt_names)} launches against {len(names)}, worst {worst}")
        if off in ("coef_fold", "dw_slab", "tail_bwd_fold"):
            assert worst[0][1] < 2e-5, (off, worst)
        else:
            bad = {a: e for a, e in errs.items() if e > {"se": lim_se, "gamma": lim_g, "general": lim}[cls(a)]}
            assert not bad, (off, bad)


# ---- 16-bit storage -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("stem_fused", [True, False], ids=["stem-fused", "stem-two-kernels"])
@pytest.mark.parametrize("dtype", HALF, ids=["bf16", "fp16"])
def test_frozen_step_half(gpu, dtype, stem_fused, monkeypatch):
    """tests/test_model_gpu.py's teacher-forced 16-bit step (_train_step_half: every block, and the stem, replayed on the oracle
    with Storage(dtype) from the device's own stored input and upstream gradient) with every BatchNorm layer frozen on the device
    and in inference mode in the oracle -- that test's code and limits, unchanged; XS 4 x 4 x 64^2, with the fused stem and with
    the two-kernel stem (plan option stem_fused off)."""
    from tests import test_model_gpu as T
    real_model = T._model

    def frozen_model(cfg, params, dt, dev, options=None):
        m = real_model(cfg, params, dt, dev, options=dict(options or {}, **({} if stem_fused else {"stem_fused": False})))
        m.set_finetune(freeze_bn=[""])
        return m

    def setup(name, overrides=None):
        cfg, arch, params = _setup(name)
        assert overrides is None
        return cfg, arch, params

    monkeypatch.setattr(T, "_model", frozen_model)
    monkeypatch.setattr(T, "_setup", setup)
    layers = R.bn_layers(_setup("XS")[2])
    with R.eval_prefix(layers):
        pl = T._train_step_half(gpu, "XS", 4, 4, 64, dtype, stem=True)
    names = [e[0] for e in pl.fwd]
    assert names[0] == "x3d_bn_eval_coef_batched" and "x3d_bn_finalize" not in names and not pl.bn_layers
    assert pl.stem_fused == stem_fused and ("x3d_stem_fwd" in names) == stem_fused


# ---- trainer ------------------------------------------------------------------------------------------------------------------
FBN = ["SOLVER.FREEZE_BN", [""]]


def _stats_equal(m2, m, s0):
    """every moving statistic of m2 has the bits it has in s0, a copy of m.moving_stats_flat() -- tensor by tensor: the padding
    between tensors belongs to nobody (a checkpoint does not carry it)"""
    nt = m.n_trainable_flat
    for a in m.param_order:
        if not m.specs[a].trainable:
            lo = m._offsets[a] - nt
            if not torch.equal(m2.params[a].reshape(-1).view(torch.int32), s0[lo:lo + m.params[a].numel()].view(torch.int32)):
                return False
    return True


def test_trainer_leaves_the_statistics_alone_and_resumes(gpu, tmp_path):
    """Three SGD steps of X3D-XS with every BatchNorm layer frozen: `moving_stats_flat()` keeps its bits, every trainable tensor
    moves (gamma and beta too: whether they are updated is SOLVER.FREEZE's business); a checkpoint after the first step resumes
    into the uninterrupted run, bit for bit; precise BatchNorm finds nothing to recompute and leaves the statistics alone."""
    from tests.test_freeze_eval_gpu import _batches, _cfg, _trainer
    cfg = _cfg(*FBN, "NETWORK.BN.USE_PRECISE_STATS", True, "NETWORK.BN.NUM_BATCHES_PRECISE", 2)
    (x1, y1), (x2, y2), (x3, y3) = [(a.to(gpu), b.to(gpu)) for a, b in _batches(3)]
    m, tr = _trainer(cfg, gpu)
    assert tr.freeze_bn == ("",) and len(m.frozen_bn) == 84 and m.frozen_prefix == 0 and m._ft is None
    nt = m.n_trainable_flat
    # a velocity on every tensor, as tests/test_freeze_eval_gpu.py seeds it: with it every tensor moves (a BatchNorm scale whose
    # gradient is below an ulp of 1 too)
    cover = torch.zeros(nt)
    for sg in m.segments:
        cover[sg.offset:sg.offset + sg.length] = 1
    vel = 0.01 * torch.randn(nt, generator=torch.Generator().manual_seed(1))
    vel[cover == 0] = 0.0
    m.flat_velocity.copy_(vel)
    w0, s0 = m.flat_params[:nt].clone(), m.moving_stats_flat().clone()
    pl = tr.step(x1, y1, 0.05)
    tr.save_checkpoint(str(tmp_path), 1)
    tr.step(x2, y2, 0.05)
    g2 = m.flat_grads.clone()
    after2 = [m.flat_params[:nt].clone(), m.flat_velocity.clone()]
    tr.step(x3, y3, 0.05)
    torch.cuda.synchronize()
    assert tr.opt_step == 3 and torch.isfinite(m.flat_params).all()
    assert pl.fwd[0][0] == "x3d_bn_eval_coef_batched" and not any(e[0] == "x3d_bn_finalize" for e in pl.fwd)
    assert torch.equal(m.moving_stats_flat().view(torch.int32), s0.view(torch.int32))
    for sg in m.segments:
        sl = slice(sg.offset, sg.offset + sg.length)
        assert not torch.equal(m.flat_params[sl], w0[sl]), sg.name
    # precise BatchNorm: nothing to recompute, no batch drawn, the statistics as they were
    drawn = iter(_batches(2, seed=8))
    assert tr.precise_bn(drawn) == 0 and len(list(drawn)) == 2
    assert torch.equal(m.moving_stats_flat().view(torch.int32), s0.view(torch.int32))
    # resume from the checkpoint of step 1: the second update on the gradient the uninterrupted run computed
    m2, tr2 = _trainer(cfg, gpu, seed=9)
    assert tr2.resume(str(tmp_path)) == 1 and tr2.opt_step == 1 and m2.frozen_bn == m.frozen_bn
    assert _stats_equal(m2, m, s0)
    m2.flat_grads.copy_(g2)
    tr2._update(None, 0.05)
    assert tr2.opt_step == 2
    for a, b in zip(after2, [m2.flat_params[:nt], m2.flat_velocity]):
        assert torch.equal(a.view(torch.int32), b.view(torch.int32))
    pl2 = tr2.step(x3, y3, 0.05)
    torch.cuda.synchronize()
    assert [e[0] for e in pl2.fwd] == [e[0] for e in pl.fwd] and tr2.opt_step == 3
    assert _stats_equal(m2, m, s0)


# ---- two ranks ----------------------------------------------------------------------------------------------------------------
def _rank_worker(rank, world, port, tmp):
    sys.path.insert(0, ROOT)
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world),
                      LOCAL_RANK=str(rank), X3D_DIST_BACKEND="gloo")
    import torch.distributed as dist
    from tests.test_freeze_eval_gpu import _batches, _cfg, _trainer
    from x3d_tf_amd import dist as xd
    r, lr_, w = xd.init_process_group()
    dev = torch.device(f"cuda:{xd.local_device(lr_)}")
    torch.cuda.set_device(dev)
    x1, y1 = _batches(1, seed=3 + rank)[0]                                          # every rank its own shard
    m, tr = _trainer(_cfg(*FBN), dev, seed=1 + rank)
    w0 = m.flat_params.cpu()                                                        # rank 0's variables, broadcast
    tr.step(x1.to(dev), y1.to(dev), 0.05)
    torch.cuda.synchronize()
    torch.save(dict(w0=w0, w=m.flat_params.cpu(), v=m.flat_velocity.cpu(), g=m.flat_grads.cpu()), os.path.join(tmp, f"rank{rank}.pt"))
    with open(os.path.join(tmp, f"rank{rank}.json"), "w") as f:
        json.dump(dict(world=tr.world, collectives=bool(tr.collectives), nt=m.n_trainable_flat, layers=len(m.frozen_bn)), f)
    dist.barrier()
    dist.destroy_process_group()


def test_two_ranks_step_with_frozen_layers(gpu, tmp_path):
    """Two data-parallel ranks (gloo, one GPU; spawned children): both end a step with the same weights, and the moving
    statistics -- identical on both ranks before the step, written by neither, averaged over two ranks ((x + x) / 2 is x) --
    keep their bits."""
    from tests.test_freeze_eval_gpu import _free_port
    mp.spawn(_rank_worker, args=(2, _free_port(), str(tmp_path)), nprocs=2, join=True)
    r0, r1 = (torch.load(tmp_path / f"rank{r}.pt") for r in (0, 1))
    i0, i1 = (json.load(open(tmp_path / f"rank{r}.json")) for r in (0, 1))
    assert i0["world"] == 2 and i0["collectives"] and i0["layers"] == i1["layers"] == 84
    nt = i0["nt"]
    assert torch.equal(r0["w0"], r1["w0"])
    for key in ("w", "v", "g"):
        assert torch.equal(r0[key], r1[key]), key
    assert bool(torch.isfinite(r0["w"]).all()) and not torch.equal(r0["w"][:nt], r0["w0"][:nt])
    for r in (r0, r1):
        assert torch.equal(r["w"][nt:].view(torch.int32), r["w0"][nt:].view(torch.int32))
