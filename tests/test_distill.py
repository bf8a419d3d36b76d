"""Knowledge distillation on the host: the DISTILL.* config section, the two new entry points' declarations and refusals (they
come before any launch), the head slot of dry plans, and the fp64 restatement the GPU tests use against a second formulation
(the kernels, the model and the trainer are in test_distill_gpu.py)."""
import math
import os
import re
import sys

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import x3d_tf_amd as x  # noqa: E402
from x3d_tf_amd.config import distill_settings  # noqa: E402
import distill_ref as R  # noqa: E402

DEFAULTS = dict(ENABLE=False, TEACHER="", TEACHER_CKPT="", ALPHA=0.5, TEMPERATURE=1.0)


# ---- config -----------------------------------------------------------------------------------------------------------
def test_config_defaults_overrides_and_a_tree_without_the_section():
    d = x.get_default_config()
    assert dict(d.DISTILL) == DEFAULTS
    s = distill_settings(x.get_config("XS"))
    assert s == (False, "", "", 0.5, 1.0) and not s.enable
    c = x.get_config("XS", ["DISTILL.ENABLE", True, "DISTILL.TEACHER", "M", "DISTILL.TEACHER_CKPT", "/ckpt/m/ckpt-300",
                            "DISTILL.ALPHA", 0.9, "DISTILL.TEMPERATURE", 4])
    s = distill_settings(c)
    assert s == (True, "M", "/ckpt/m/ckpt-300", 0.9, 4.0)
    assert (s.enable, s.teacher, s.teacher_ckpt, s.alpha, s.temperature) == tuple(s)
    # the section deleted: off, and the rest of the tree is what it was
    old = c.clone()
    old.defrost()
    del old["DISTILL"]
    assert not distill_settings(old).enable and distill_settings(old) == (False, "", "", 0.5, 1.0)
    assert set(c) == set(old) | {"DISTILL"}
    assert set(c.TRAIN) == {"DATASET_SIZE", "BATCH_SIZE", "EPOCHS", "OPTIMIZER", "MOMENTUM", "BASE_LR", "WARMUP_EPOCHS",
                            "WARMUP_LR", "LABEL_SMOOTHING"}


@pytest.mark.parametrize("over, key", [
    (["DISTILL.ALPHA", -0.01], "DISTILL.ALPHA"), (["DISTILL.ALPHA", 1.01], "DISTILL.ALPHA"),
    (["DISTILL.ALPHA", float("nan")], "DISTILL.ALPHA"),
    (["DISTILL.TEMPERATURE", 0.0], "DISTILL.TEMPERATURE"), (["DISTILL.TEMPERATURE", -1.0], "DISTILL.TEMPERATURE"),
    (["DISTILL.TEMPERATURE", float("inf")], "DISTILL.TEMPERATURE"),
    (["DISTILL.TEMPERATURE", float("nan")], "DISTILL.TEMPERATURE"),
])
def test_config_value_refusals_name_the_key(over, key):
    with pytest.raises(ValueError, match=re.escape(key)):
        x.get_config("XS", over)                      # get_config checks the section like its siblings
    cfg = x.get_config("XS", freeze=False)
    cfg.merge_from_list(over)
    with pytest.raises(ValueError, match=re.escape(key)):
        distill_settings(cfg)


def test_enable_needs_a_teacher_name_or_a_teacher_object():
    cfg = x.get_config("XS", ["DISTILL.ENABLE", True])      # loads: a trainer may still be handed a teacher
    with pytest.raises(ValueError, match=re.escape("DISTILL.TEACHER")):
        distill_settings(cfg)
    assert distill_settings(cfg, have_teacher=True).enable
    assert distill_settings(x.get_config("XS", ["DISTILL.ENABLE", True, "DISTILL.TEACHER", "M"])).teacher == "M"
    assert not distill_settings(x.get_config("XS", ["DISTILL.TEACHER", ""])).enable          # off: nothing to name


# ---- ABI, export, refusals ----------------------------------------------------------------------------------------------
def test_abi_version_struct_count_and_the_two_symbols():
    from x3d_tf_amd import hip
    lib = hip.load()
    assert hip.ABI_VERSION == 138 == lib.x3d_version()
    with open(os.path.join(ROOT, "include", "x3d_hip.h")) as f:
        header = f.read()
    assert len(re.findall(r"typedef\s+struct", header)) == 16
    for name, nargs in (("x3d_softmax_xent_kd", 14), ("x3d_sigmoid_bce_kd", 13)):
        assert name in hip.exported_symbols()
        fn = getattr(lib, name)                       # exported by the library
        assert len(fn.argtypes) == nargs and re.search(rf"\bint {name}\(", header)


A, B, C_, D = 0x10000, 0x20000, 0x30000, 0x40000      # addresses that are never touched: every call below is refused first


def _softmax(lib, logits=A, teacher=B, labels=C_, targets=None, probs=D, loss=None, kd=None, dl=None, alpha=0.5, temp=1.0,
             n=2, m=3):
    return lib.x3d_softmax_xent_kd(logits, teacher, labels, targets, probs, loss, kd, dl, 1.0, alpha, temp, n, m, None)


def _sigmoid(lib, logits=A, teacher=B, targets=C_, probs=D, loss=None, kd=None, dl=None, alpha=0.5, temp=1.0, n=2, m=3):
    return lib.x3d_sigmoid_bce_kd(logits, teacher, targets, probs, loss, kd, dl, 1.0, alpha, temp, n, m, None)


REFUSALS = [
    (dict(logits=None), b"logits"), (dict(probs=None), b"probs"),
    (dict(alpha=-0.1), b"alpha"), (dict(alpha=1.5), b"alpha"), (dict(alpha=float("nan")), b"alpha"),
    (dict(temp=0.0), b"temperature"), (dict(temp=-2.0), b"temperature"), (dict(temp=float("inf")), b"temperature"),
    (dict(temp=float("nan")), b"temperature"),
    (dict(teacher=None), b"teacher_logits"), (dict(teacher=None, alpha=1.0), b"teacher_logits"),
    (dict(n=0), b"N="), (dict(m=0), b"M="), (dict(n=-1), b"N="), (dict(n=1 << 16, m=1 << 15), b"2^31"),
    (dict(teacher=D), b"teacher_logits"), (dict(teacher=D + 8), b"teacher_logits"), (dict(dl=B + 4), b"teacher_logits"),
    (dict(loss=B + 20), b"teacher_logits"), (dict(kd=B), b"teacher_logits"),
]


@pytest.mark.parametrize("kw, word", REFUSALS, ids=[f"{i}-{w.decode().strip('=')}" for i, (_, w) in enumerate(REFUSALS)])
def test_refusals_come_before_any_launch_and_name_the_argument(kw, word):
    from x3d_tf_amd import hip
    lib = hip.load()
    for call in (_softmax, _sigmoid):
        assert call(lib, **kw) != 0
        msg = lib.x3d_last_error()
        assert word in msg and (b"softmax_xent_kd" if call is _softmax else b"sigmoid_bce_kd") in msg, msg


def test_refusals_of_labels_and_targets():
    from x3d_tf_amd import hip
    lib = hip.load()
    assert _softmax(lib, labels=C_, targets=C_ + 0x1000) != 0 and b"labels / targets" in lib.x3d_last_error()
    assert _softmax(lib, labels=None, targets=None) != 0 and b"labels / targets" in lib.x3d_last_error()
    for call, kw in ((_softmax, dict(labels=None)), (_sigmoid, {})):
        assert call(lib, targets=D + 4, **kw) != 0 and b"targets overlaps" in lib.x3d_last_error()
        assert call(lib, targets=C_, kd=C_ + 16, **kw) != 0 and b"targets overlaps" in lib.x3d_last_error()
    assert _sigmoid(lib, targets=None) != 0 and b"targets" in lib.x3d_last_error()


# ---- dry plans --------------------------------------------------------------------------------------------------------
BASE = ["DATA.TEMP_DURATION", 4]


def _dry_plan(cfg):
    from x3d_tf_amd.model import X3D
    return X3D(cfg, dtype=torch.float32, device="dry")._plan(2, 4, 64, 64, True)


def _names(pl):
    return [e[0] for e in pl.fwd], [e[0] for e in pl.bwd]


def test_dry_plans_do_not_depend_on_the_config_section():
    cfg = x.get_config("XS", BASE)
    absent = cfg.clone()
    absent.defrost()
    del absent["DISTILL"]
    on = x.get_config("XS", BASE + ["DISTILL.ENABLE", True, "DISTILL.TEACHER", "M", "DISTILL.ALPHA", 0.7,
                                    "DISTILL.TEMPERATURE", 3.0])
    lists = [_names(_dry_plan(c)) for c in (absent, cfg, on)]
    assert lists[0] == lists[1] == lists[2]
    assert not any("_kd" in n for n in lists[0][0] + lists[0][1])


@pytest.mark.parametrize("head", ["labels", "targets", "multi"])
def test_a_distilled_call_swaps_only_the_head_slot_and_back(head):
    multi = head == "multi"
    pl = _dry_plan(x.get_config("XS", BASE + (["DATA.MULTI_LABEL", True, "NETWORK.NUM_CLASSES", 157] if multi else [])))
    slot = pl.grad_scale_slot
    assert pl.teacher is None and pl.kd_rows is None and list(pl._heads) == [(False, False)]   # nothing for distillation yet
    soft = head == "targets"
    pl.use_soft_targets(soft)
    f0, b0 = _names(pl)
    entry0 = pl.fwd[slot]
    hard_name = {"labels": "x3d_softmax_xent", "targets": "x3d_softmax_xent_soft", "multi": "x3d_sigmoid_bce"}[head]
    kd_name = "x3d_sigmoid_bce_kd" if multi else "x3d_softmax_xent_kd"
    assert entry0[0] == hard_name
    assert pl.teacher is None and pl.kd_rows is None
    # the distilled call
    pl.use_soft_targets(soft, distill=True)
    f1, b1 = _names(pl)
    assert b1 == b0 and [i for i, (p, q) in enumerate(zip(f0, f1)) if p != q] == [slot] and len(f1) == len(f0)
    name, _, args = pl.fwd[slot]
    classes = 157 if multi else 400
    assert name == kd_name and tuple(pl.teacher.shape) == (2, classes) and pl.kd_rows.numel() == 2
    assert args[0] == pl.logits.data_ptr() and args[1] == pl.teacher.data_ptr()
    if multi:
        assert args[2:7] == (pl.targets.data_ptr(), pl.probs.data_ptr(), pl.loss_rows.data_ptr(), pl.kd_rows.data_ptr(),
                             pl.dlogits.data_ptr())
    else:
        want = (None, pl.targets.data_ptr()) if soft else (pl.labels.data_ptr(), None)
        assert args[2:4] == want
        assert args[4:8] == (pl.probs.data_ptr(), pl.loss_rows.data_ptr(), pl.kd_rows.data_ptr(), pl.dlogits.data_ptr())
    assert args[-2:] == (2, classes)
    teacher = pl.teacher
    # and back: the recorded entry, the very tuple, with its pointers
    pl.use_soft_targets(soft)
    assert pl.fwd[slot] is entry0 and _names(pl) == (f0, b0)
    # a second distilled call reuses the buffers and the entry
    pl.use_soft_targets(soft, distill=True)
    assert pl.teacher is teacher and pl.fwd[slot][0] == kd_name
    if not multi:      # the other single-label head gets an entry of its own; the hard-label path is restored from either
        pl.use_soft_targets(not soft, distill=True)
        assert pl.fwd[slot][0] == kd_name and (pl.fwd[slot][2][2] is None) == (not soft)
        pl.use_soft_targets(False)
        assert pl.fwd[slot][0] == "x3d_softmax_xent" and pl.fwd[slot][2][1] == pl.labels.data_ptr()


def test_logits_plan_is_the_inference_list_without_its_last_two_launches():
    from x3d_tf_amd.model import X3D
    m = X3D(x.get_config("XS", BASE), dtype=torch.float32, device="dry")
    v = m.arch.num_preds                                       # views * crops
    assert v > 1
    infer = m._plan(v, 4, 64, 64, False)
    lg = m._plan(v, 4, 64, 64, False, logits_only=True)
    assert lg is not infer and m._plan(v, 4, 64, 64, False) is infer
    fi, fl = [e[0] for e in infer.fwd], [e[0] for e in lg.fwd]
    assert fl == fi[:-2] and fi[-2:] == ["x3d_softmax_xent", "x3d_view_mean"] and fl[-1] == "x3d_dense_fwd"
    assert not lg.training and lg.bwd == [] and tuple(lg.logits.shape) == (v, 400)
    # a batch that is no multiple of views * crops: refused by call's plan, fine for logits
    with pytest.raises(ValueError):
        m._plan(v + 1, 4, 64, 64, False)
    assert tuple(m._plan(v + 1, 4, 64, 64, False, logits_only=True).logits.shape) == (v + 1, 400)


# ---- the restatement against a second formulation ---------------------------------------------------------------------
def _kl_autograd(z, t, T):
    zz = z.double().requires_grad_(True)
    kl = torch.nn.functional.kl_div(torch.log_softmax(zz / T, -1), torch.softmax(t.double() / T, -1), reduction="none")
    rows = T * T * kl.sum(1)
    (g,) = torch.autograd.grad(rows.sum(), [zz])
    return rows.detach(), g


def _bernoulli_autograd(z, t, T):
    zz = z.double().requires_grad_(True)
    u, v = zz / T, t.double() / T
    ls = torch.nn.functional.logsigmoid
    kl = torch.sigmoid(v) * (ls(v) - ls(u)) + torch.sigmoid(-v) * (ls(-v) - ls(-u))
    rows = T * T * kl.mean(1)
    (g,) = torch.autograd.grad(rows.sum(), [zz])
    return rows.detach(), g


def _close(name, got, ref):
    assert bool(torch.isfinite(got).all()) and bool(torch.isfinite(ref).all()), name
    err = (got - ref).abs()
    assert bool((err <= 1e-10 + 1e-9 * ref.abs()).all()), (name, err.max().item())


@pytest.mark.parametrize("n", R.NS)
@pytest.mark.parametrize("m", R.MS)
def test_reference_agrees_with_autograd_of_the_textbook_forms(n, m):
    z, t, labels, soft, multi = R.inputs(n, m)
    for T in R.TEMPS:
        rows, grad = R.softmax_kd(z, t, T)
        r2, g2 = _kl_autograd(z, t, T)
        _close(f"softmax kd rows T={T}", rows, r2)
        _close(f"softmax kd grad T={T}", grad, g2)
        rows_s, grad_s = R.sigmoid_kd(z, t, T)
        r2, g2 = _bernoulli_autograd(z, t, T)
        _close(f"sigmoid kd rows T={T}", rows_s, r2)
        _close(f"sigmoid kd grad T={T}", grad_s, g2)
        assert float(rows.min()) >= -1e-12 and float(rows_s.min()) >= -1e-12          # a KL
        if R.has_same_row(n, m):
            assert rows[R.SAME_ROW].abs().item() <= 1e-12 and grad[R.SAME_ROW].abs().max().item() <= 1e-12
            assert rows_s[R.SAME_ROW].abs().item() <= 1e-12 and grad_s[R.SAME_ROW].abs().max().item() <= 1e-12
    # the hard terms against autograd of Keras' expressions (torch.clamp's gradient mask is the same closed interval)
    for kw in (dict(labels=labels), dict(targets=soft)):
        p, rows, grad = R.softmax_hard(z, **kw)
        zz = z.double().requires_grad_(True)
        q = torch.softmax(zz, -1).clamp(1e-7, 1 - 1e-7)
        y = torch.nn.functional.one_hot(labels.long(), m).double() if "labels" in kw else soft.double()
        r2 = (y * -torch.log(q)).sum(1) + y.sum(1) * torch.log(q.sum(1))
        (g2,) = torch.autograd.grad(r2.sum(), [zz])
        _close("softmax hard rows", rows, r2.detach())
        _close("softmax hard grad", grad, g2)
    p, rows, grad = R.sigmoid_hard(z, multi)
    zz = z.double().requires_grad_(True)
    r2 = torch.nn.functional.binary_cross_entropy_with_logits(zz, multi.double(), reduction="none").mean(1)
    (g2,) = torch.autograd.grad(r2.sum(), [zz])
    _close("sigmoid hard rows", rows, r2.detach())
    _close("sigmoid hard grad", grad, g2)
    # combine: the weights and the scale
    c = R.combine((p, rows, grad), R.sigmoid_kd(z, t, 2.5), 0.3, 0.5)
    assert torch.equal(c[2], R.sigmoid_kd(z, t, 2.5)[0]) and math.isclose(float(c[1][0]), 0.7 * float(rows[0]) + 0.3 * float(c[2][0]))
