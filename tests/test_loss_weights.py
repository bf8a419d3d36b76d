"""Class-imbalance losses on the host: the fp64 restatement the GPU tests use (loss_weights_ref.py) against torch.autograd, torch's
BCEWithLogitsLoss(pos_weight) and a transcription of Keras' focal losses; the LOSS.* config section; class_weights_from_counts;
the refusals of the new entry points (they come before any launch); the head slot of dry plans.  The kernels, the model and the
trainer are in test_loss_weights_gpu.py."""
import os
import re
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import x3d_tf_amd as x  # noqa: E402
from x3d_tf_amd.config import loss_settings  # noqa: E402
from x3d_tf_amd.losses import class_weights_from_counts  # noqa: E402
import distill_ref as R  # noqa: E402
import loss_weights_ref as W  # noqa: E402

SHAPES = [(n, m) for n in W.NS for m in W.MS]


def _t(w):
    return None if w is None else torch.from_numpy(np.asarray(w, dtype=np.float64))


def _rel(got, want):
    """largest |got - want| relative to the largest |want| of the case (both all zero: 0)"""
    scale = float(np.abs(want).max())
    return float(np.abs(got - want).max()) / scale if scale > 0 else float(np.abs(got).max())


# ---- the ref's gradients against autograd ------------------------------------------------------------------------------
def _stated_softmax(z, y, cw, rw, g):
    """the stated loss, written for autograd: clamp supplies the in-range mask"""
    p = torch.softmax(z, 1)
    q = p.clamp(1e-7, 1.0 - 1e-7)
    xh = q / q.sum(1, keepdim=True)
    f = -torch.log(xh) if g == 0.0 else (1.0 - xh) ** g * -torch.log(xh)
    return (rw[:, None] * cw[None, :] * y * f).sum(1)


def _stated_sigmoid(z, y, cw, pw, rw, gp, gn):
    s, oms = torch.sigmoid(z), torch.sigmoid(-z)      # 1 - s without the cancellation: at z = 40 `1 - s` is 0 and pow's slope inf
    sp, sn = torch.nn.functional.softplus(-z), torch.nn.functional.softplus(z)
    fp = sp if gp == 0.0 else oms ** gp * sp
    fn = sn if gn == 0.0 else s ** gn * sn
    return rw * (cw[None, :] * (y * pw[None, :] * fp + (1.0 - y) * fn)).mean(1)


@pytest.mark.parametrize("head", W.HEADS)
def test_ref_gradients_equal_autograd_in_float64(head):
    worst = 0.0
    for n, m in SHAPES:
        z, _, labels, soft, multi = R.inputs(n, m)
        p = torch.softmax(z.double(), 1)
        # no p within 1e-9 of a clip edge: the mask of clamp and the ref's [1e-7 <= p <= 1 - 1e-7] agree
        assert float(torch.minimum((p - 1e-7).abs(), (p - (1.0 - 1e-7)).abs()).min()) > 1e-9
        for name, mod in W.mods_of(head).items():
            cw, pw, rw = W.weights(n, m, mod)
            gp, gn = mod.get("gp", 0.0), mod.get("gn", 0.0)
            zz = z.double().requires_grad_(True)
            one = lambda w, k: torch.ones(k, dtype=torch.float64) if w is None else _t(w)
            if head == "multi":
                _, rows, grad = W.sigmoid_w(z.numpy(), multi.numpy(), cw, pw, rw, gp, gn)
                loss = _stated_sigmoid(zz, multi.double(), one(cw, m), one(pw, m), one(rw, n), gp, gn)
            else:
                y = torch.nn.functional.one_hot(labels.long(), m).double() if head == "labels" else soft.double()
                kw = dict(labels=labels.numpy()) if head == "labels" else dict(targets=soft.numpy())
                _, rows, grad = W.softmax_w(z.numpy(), class_w=cw, row_w=rw, gamma=gp, **kw)
                loss = _stated_softmax(zz, y, one(cw, m), one(rw, n), gp)
            assert np.isfinite(rows).all() and np.isfinite(grad).all(), (head, n, m, name)
            assert _rel(rows, loss.detach().numpy()) <= 1e-10, (head, n, m, name)
            if head != "multi" and m == 1:
                # one class: x = q / q = 1.  The rule is loss 0, gradient 0; autograd of (1 - x)^g at x = 1 is inf * 0 for g < 1
                assert not rows.any() and not grad.any()
                continue
            loss.sum().backward()
            err = _rel(grad, zz.grad.numpy())
            worst = max(worst, err)
            assert err <= 1e-10, (head, n, m, name, err)
    print(f"{head}: largest relative gradient difference {worst:.3g}")


# ---- correspondences ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n, m", SHAPES)
def test_gamma_zero_with_labels_is_class_weight_times_the_plain_loss(n, m):
    z, _, labels, soft, _ = R.inputs(n, m)
    cw, _, _ = W.weights(n, m, dict(cw=1))
    p, rows, grad = W.softmax_w(z.numpy(), labels=labels.numpy(), class_w=cw)
    p0, rows0, grad0 = (v.numpy() for v in R.softmax_hard(z, labels=labels))
    c = cw.astype(np.float64)[labels.numpy()]
    np.testing.assert_allclose(p, p0, rtol=1e-13, atol=0)
    np.testing.assert_allclose(rows, c * rows0, rtol=1e-12, atol=1e-15)
    np.testing.assert_allclose(grad, c[:, None] * grad0, rtol=1e-10, atol=1e-15)
    # and with nothing set both heads are the plain refs, dense rows included
    for kw in (dict(labels=labels), dict(targets=soft)):
        got = W.softmax_w(z.numpy(), **{k: v.numpy() for k, v in kw.items()})
        for g, w in zip(got, R.softmax_hard(z, **kw)):
            np.testing.assert_allclose(g, w.numpy(), rtol=1e-10, atol=1e-15)


@pytest.mark.parametrize("n, m", SHAPES)
def test_sigmoid_ref_at_gamma_zero_is_bce_with_logits_pos_weight(n, m):
    z, _, _, _, multi = R.inputs(n, m)
    cw, pw, rw = W.weights(n, m, dict(cw=1, pw=1, rw=1))
    _, rows, _ = W.sigmoid_w(z.numpy(), multi.numpy(), cw, pw, rw)
    el = torch.nn.functional.binary_cross_entropy_with_logits(z.double(), multi.double(), weight=_t(cw)[None, :].expand(n, m),
                                                              pos_weight=_t(pw), reduction="none")
    np.testing.assert_allclose(rows, (_t(rw) * el.mean(1)).numpy(), rtol=1e-12, atol=1e-15)
    _, rows, grad = W.sigmoid_w(z.numpy(), multi.numpy())
    for g, w in zip((rows, grad), R.sigmoid_hard(z, multi)[1:]):
        np.testing.assert_allclose(g, w.numpy(), rtol=1e-12, atol=1e-15)


@pytest.mark.parametrize("n, m", SHAPES)
def test_gamma_two_is_keras_focal(n, m):
    """keras.losses.CategoricalFocalCrossentropy / BinaryFocalCrossentropy (from_logits=False, their alpha as a per-class
    weight), transcribed: output /= sum(output); output = clip(output, eps, 1 - eps); alpha * (1 - output)^gamma * -(target *
    log(output)), summed over the classes -- and bce * (1 - p_t)^gamma, p_t = y p + (1 - y)(1 - p), averaged over them"""
    z, _, labels, _, multi = R.inputs(n, m)
    g = 2.0
    cw, _, _ = W.weights(n, m, dict(cw=1))
    y = np.eye(m)[labels.numpy().astype(np.int64)]
    out = torch.softmax(z.double(), 1).numpy()
    # this head clips first and renormalises the clipped values (as the plain kernel has since the start): feed Keras' formula q
    q = np.clip(out, 1e-7, 1 - 1e-7)
    out = q / q.sum(1, keepdims=True)
    keras = (cw.astype(np.float64)[None, :] * (1.0 - out) ** g * -(y * np.log(out))).sum(1)
    _, rows, _ = W.softmax_w(z.numpy(), labels=labels.numpy(), class_w=cw, gamma=g)
    np.testing.assert_allclose(rows, keras, rtol=1e-12, atol=1e-300)
    yb = multi.double().numpy()
    s = torch.sigmoid(z.double()).numpy()
    oms = torch.sigmoid(-z.double()).numpy()
    bce = -(yb * np.log(s) + (1 - yb) * np.log(oms))
    p_t = yb * s + (1 - yb) * oms
    keras = (bce * (1.0 - p_t) ** g).mean(1)
    _, rows, _ = W.sigmoid_w(z.numpy(), yb, gamma_pos=g, gamma_neg=g)
    np.testing.assert_allclose(rows, keras, rtol=1e-10, atol=1e-300)


# ---- config ------------------------------------------------------------------------------------------------------------
DEFAULTS = dict(CLASS_WEIGHTS=[], POS_WEIGHT=[], FOCAL_GAMMA=0.0, FOCAL_GAMMA_NEG=0.0)
SMALL = ["NETWORK.NUM_CLASSES", 3]


def test_config_defaults_overrides_and_a_tree_without_the_section():
    assert dict(x.get_default_config().LOSS) == DEFAULTS
    cfg = x.get_config("XS")
    s = loss_settings(cfg)
    assert s == ((), (), 0.0, 0.0) and (s.class_weights, s.pos_weight, s.focal_gamma, s.focal_gamma_neg) == tuple(s)
    c = x.get_config("XS", SMALL + ["LOSS.CLASS_WEIGHTS", [1, 0, 2.5], "LOSS.FOCAL_GAMMA", 2])
    assert loss_settings(c) == ((1.0, 0.0, 2.5), (), 2.0, 0.0)
    c = x.get_config("XS", SMALL + ["DATA.MULTI_LABEL", True, "LOSS.POS_WEIGHT", [3, 1, 0], "LOSS.FOCAL_GAMMA_NEG", 4.0])
    assert loss_settings(c) == ((), (3.0, 1.0, 0.0), 0.0, 4.0)
    old = c.clone()
    old.defrost()
    del old["LOSS"]
    assert loss_settings(old) == ((), (), 0.0, 0.0)
    assert set(c) == set(old) | {"LOSS"}
    assert set(c.TRAIN) == {"DATASET_SIZE", "BATCH_SIZE", "EPOCHS", "OPTIMIZER", "MOMENTUM", "BASE_LR", "WARMUP_EPOCHS",
                            "WARMUP_LR", "LABEL_SMOOTHING"}
    assert set(c.SOLVER) == {"CLIP_GRAD_L2NORM", "ACCUM_STEPS", "EMA_DECAY", "EMA_EVAL"}


MULTI = SMALL + ["DATA.MULTI_LABEL", True]
CONFIG_REFUSALS = [
    (SMALL + ["LOSS.CLASS_WEIGHTS", [1.0, -0.5, 1.0]], "LOSS.CLASS_WEIGHTS"),
    (SMALL + ["LOSS.CLASS_WEIGHTS", [1.0, float("nan"), 1.0]], "LOSS.CLASS_WEIGHTS"),
    (SMALL + ["LOSS.CLASS_WEIGHTS", [1.0, float("inf"), 1.0]], "LOSS.CLASS_WEIGHTS"),
    (SMALL + ["LOSS.CLASS_WEIGHTS", [0.0, 0.0, 0.0]], "LOSS.CLASS_WEIGHTS"),
    (SMALL + ["LOSS.CLASS_WEIGHTS", [1.0, 1.0]], "LOSS.CLASS_WEIGHTS"),
    (SMALL + ["LOSS.CLASS_WEIGHTS", [1.0, 1.0, 1.0, 1.0]], "LOSS.CLASS_WEIGHTS"),
    (MULTI + ["LOSS.POS_WEIGHT", [1.0, -1.0, 1.0]], "LOSS.POS_WEIGHT"),
    (MULTI + ["LOSS.POS_WEIGHT", [0.0, 0.0, 0.0]], "LOSS.POS_WEIGHT"),
    (MULTI + ["LOSS.POS_WEIGHT", [1.0]], "LOSS.POS_WEIGHT"),
    (SMALL + ["LOSS.POS_WEIGHT", [1.0, 1.0, 1.0]], "LOSS.POS_WEIGHT"),
    (SMALL + ["LOSS.FOCAL_GAMMA_NEG", 1.0], "LOSS.FOCAL_GAMMA_NEG"),
    (SMALL + ["LOSS.FOCAL_GAMMA", -0.5], "LOSS.FOCAL_GAMMA"), (SMALL + ["LOSS.FOCAL_GAMMA", 8.5], "LOSS.FOCAL_GAMMA"),
    (SMALL + ["LOSS.FOCAL_GAMMA", float("nan")], "LOSS.FOCAL_GAMMA"), (SMALL + ["LOSS.FOCAL_GAMMA", float("inf")], "LOSS.FOCAL_GAMMA"),
    (MULTI + ["LOSS.FOCAL_GAMMA_NEG", -1.0], "LOSS.FOCAL_GAMMA_NEG"), (MULTI + ["LOSS.FOCAL_GAMMA_NEG", 9.0], "LOSS.FOCAL_GAMMA_NEG"),
    (MULTI + ["LOSS.FOCAL_GAMMA_NEG", float("nan")], "LOSS.FOCAL_GAMMA_NEG"),
]


@pytest.mark.parametrize("over, key", CONFIG_REFUSALS, ids=[f"{i}-{k}" for i, (_, k) in enumerate(CONFIG_REFUSALS)])
def test_config_refusals_name_the_key(over, key):
    with pytest.raises(ValueError, match=re.escape(key)):
        x.get_config("XS", over)                      # get_config checks the section like its siblings
    cfg = x.get_config("XS", freeze=False)
    cfg.merge_from_list(over)
    with pytest.raises(ValueError, match=re.escape(key)):
        loss_settings(cfg)


def test_config_accepts_the_edges():
    c = x.get_config("XS", MULTI + ["LOSS.FOCAL_GAMMA", 8.0, "LOSS.FOCAL_GAMMA_NEG", 8.0, "LOSS.CLASS_WEIGHTS", [0.0, 0.0, 1e-3]])
    assert loss_settings(c) == ((0.0, 0.0, 1e-3), (), 8.0, 8.0)


# ---- class_weights_from_counts -----------------------------------------------------------------------------------------
def test_class_weights_from_counts():
    counts = [100, 10, 0, 1, 1000]
    have = np.array(counts) > 0
    inv = class_weights_from_counts(counts)
    assert inv.dtype == np.float64 and inv.shape == (5,) and inv[2] == 0.0
    assert abs(inv[have].mean() - 1.0) < 1e-12
    np.testing.assert_allclose(inv[have] * np.array(counts)[have], (inv[0] * 100) * np.ones(4), rtol=1e-12)   # w proportional to 1 / n
    beta = 0.99
    eff = class_weights_from_counts(counts, "effective", beta=beta)
    raw = np.array([(1 - beta) / (1 - beta ** c) if c else 0.0 for c in counts])
    np.testing.assert_allclose(eff, raw * 4 / raw.sum(), rtol=1e-12)
    assert eff[2] == 0.0 and abs(eff[have].mean() - 1.0) < 1e-12
    assert eff[3] > eff[1] > eff[0] > eff[4] > 0                      # rarer classes weigh more
    np.testing.assert_allclose(class_weights_from_counts(counts, "effective", beta=0.0)[have], np.ones(4), rtol=1e-12)
    big = class_weights_from_counts([10, 20, 40], "effective", beta=1 - 1e-12)     # beta -> 1 approaches "inverse"
    np.testing.assert_allclose(big, class_weights_from_counts([10, 20, 40]), rtol=1e-6)
    assert class_weights_from_counts(counts, "effective").shape == (5,)              # default beta 0.999
    np.testing.assert_allclose(class_weights_from_counts([7, 7, 7]), np.ones(3), rtol=1e-15)
    for bad, kw in (([0, 0], {}), ([1, -1], {}), ([1, float("nan")], {}), ([], {}), ([[1, 2]], {}), ([1, 2], dict(scheme="sqrt")),
                    ([1, 2], dict(scheme="effective", beta=1.0)), ([1, 2], dict(scheme="effective", beta=-0.1))):
        with pytest.raises(ValueError):
            class_weights_from_counts(bad, **kw)


# ---- the entry points: declared, exported, and their refusals come before any launch -----------------------------------
def test_abi_is_additive_and_the_entry_points_are_declared_and_exported():
    from ctypes import c_float as f, c_int as i, c_void_p as vp
    from x3d_tf_amd import hip
    lib = hip.load()
    assert hip.ABI_VERSION == 138 and lib.x3d_version() == 138
    sigs = {"x3d_softmax_xent_w": [vp] * 10 + [f] * 4 + [i, i, vp],
            "x3d_sigmoid_bce_w": [vp] * 10 + [f] * 5 + [i, i, vp],
            "x3d_class_hits": [vp, vp, i, vp, vp, i, i, vp]}
    for name, argtypes in sigs.items():
        assert name in hip.exported_symbols()
        fn = getattr(lib, name)
        assert list(fn.argtypes) == argtypes and fn.restype is i, name


A, B, C_, D, E, F, G = (0x10000 * k for k in range(1, 8))      # addresses that are never touched: every call below is refused first


def _softmax(lib, logits=A, teacher=B, labels=C_, targets=None, cw=None, rw=None, probs=D, loss=None, kd=None, dl=None, g=0.0,
             alpha=0.5, temp=1.0, n=2, m=3):
    return lib.x3d_softmax_xent_w(logits, teacher, labels, targets, cw, rw, probs, loss, kd, dl, 1.0, g, alpha, temp, n, m, None)


def _sigmoid(lib, logits=A, teacher=B, targets=C_, cw=None, pw=None, rw=None, probs=D, loss=None, kd=None, dl=None, g=0.0, gn=0.0,
             alpha=0.5, temp=1.0, n=2, m=3):
    return lib.x3d_sigmoid_bce_w(logits, teacher, targets, cw, pw, rw, probs, loss, kd, dl, 1.0, g, gn, alpha, temp, n, m, None)


inf, nan = float("inf"), float("nan")
REFUSALS = [
    (dict(g=-0.5), b"gamma"), (dict(g=nan), b"gamma"), (dict(g=inf), b"gamma"), (dict(g=8.5), b"gamma"),
    (dict(cw=D), b"class_w"), (dict(cw=D + 20), b"class_w"), (dict(cw=E, dl=E + 8), b"class_w"), (dict(cw=E, loss=E + 4), b"class_w"),
    (dict(cw=E, kd=E), b"class_w"),
    (dict(rw=D + 4), b"row_w"), (dict(rw=F, dl=F), b"row_w"), (dict(rw=F, loss=F + 4), b"row_w"), (dict(rw=F, kd=F), b"row_w"),
    # the distillation block's own conditions
    (dict(logits=None), b"logits"), (dict(probs=None), b"probs"), (dict(alpha=-0.1), b"alpha"), (dict(alpha=nan), b"alpha"),
    (dict(temp=0.0), b"temperature"), (dict(temp=inf), b"temperature"), (dict(teacher=None), b"teacher_logits"),
    (dict(n=0), b"N="), (dict(m=0), b"M="), (dict(n=1 << 16, m=1 << 15), b"2^31"), (dict(teacher=D), b"teacher_logits"),
    (dict(kd=B), b"teacher_logits"),
]


@pytest.mark.parametrize("kw, word", REFUSALS, ids=[f"{i}-{w.decode().strip('=')}" for i, (_, w) in enumerate(REFUSALS)])
def test_refusals_come_before_any_launch_and_name_the_argument(kw, word):
    from x3d_tf_amd import hip
    lib = hip.load()
    for call in (_softmax, _sigmoid):
        assert call(lib, **kw) == 1                    # X3D_ERR_INVALID
        msg = lib.x3d_last_error()
        assert word in msg and (b"softmax_xent_w" if call is _softmax else b"sigmoid_bce_w") in msg, msg


def test_refusals_of_the_sigmoid_head_and_of_labels_and_targets():
    from x3d_tf_amd import hip
    lib = hip.load()
    for kw, word in ((dict(gn=-1.0), b"gamma_neg"), (dict(gn=nan), b"gamma_neg"), (dict(gn=8.01), b"gamma_neg"),
                     (dict(g=9.0), b"gamma_pos"), (dict(pw=D + 8), b"pos_w"), (dict(pw=G, dl=G), b"pos_w"),
                     (dict(pw=G, kd=G + 4), b"pos_w"), (dict(targets=None), b"targets"), (dict(targets=D + 4), b"targets overlaps")):
        assert _sigmoid(lib, **kw) == 1 and word in lib.x3d_last_error(), kw
    assert _softmax(lib, labels=C_, targets=C_ + 0x1000) == 1 and b"labels / targets" in lib.x3d_last_error()
    assert _softmax(lib, labels=None, targets=None) == 1 and b"labels / targets" in lib.x3d_last_error()
    assert _softmax(lib, labels=None, targets=D + 4) == 1 and b"targets overlaps" in lib.x3d_last_error()
    from ctypes import c_void_p
    assert lib.x3d_class_hits(A, B, 2, C_, D, 4, 3, None) == 1 and b"label_bytes" in lib.x3d_last_error()
    assert lib.x3d_class_hits(A, B, 4, C_, D, 4, 0, None) == 1 and b"M=" in lib.x3d_last_error()
    assert lib.x3d_class_hits(A, B, 4, None, D, 4, 3, None) == 1 and b"null" in lib.x3d_last_error()
    assert lib.x3d_class_hits(A, B, 4, C_ + 4, D, 4, 3, None) == 1 and b"aligned" in lib.x3d_last_error()
    assert lib.x3d_class_hits(A, B, 8, C_, D, 1 << 16, 1 << 15, None) == 1 and b"2^31" in lib.x3d_last_error()
    assert lib.x3d_class_hits(None, None, 4, None, None, 0, 3, c_void_p()) == 0      # N = 0: a no-op


# ---- dry plans ---------------------------------------------------------------------------------------------------------
BASE = ["DATA.TEMP_DURATION", 4]


def _dry_model(cfg):
    from x3d_tf_amd.model import X3D
    m = X3D(cfg, dtype=torch.float32, device="dry")
    s = loss_settings(cfg)
    if s != ((), (), 0.0, 0.0):                       # what the trainer does with the section
        m.set_loss(class_weights=s.class_weights or None, pos_weight=s.pos_weight or None, focal_gamma=s.focal_gamma,
                   focal_gamma_neg=s.focal_gamma_neg)
    return m


def _names(pl):
    return [e[0] for e in pl.fwd], [e[0] for e in pl.bwd]


@pytest.mark.parametrize("multi", [False, True])
def test_dry_plans_with_loss_off_are_those_of_a_config_without_the_section(multi):
    extra = ["DATA.MULTI_LABEL", True, "NETWORK.NUM_CLASSES", 157] if multi else []
    cfg = x.get_config("XS", BASE + extra)
    absent = cfg.clone()
    absent.defrost()
    del absent["LOSS"]
    plans = [_dry_model(c)._plan(2, 4, 64, 64, True) for c in (absent, cfg)]
    assert _names(plans[0]) == _names(plans[1])
    for pl in plans:
        assert pl.fwd[pl.grad_scale_slot][0] == ("x3d_sigmoid_bce" if multi else "x3d_softmax_xent")
        assert list(pl._heads) == [(False, False)] and pl.row_w is None and pl.model.loss_mods is None
        assert not any(n.endswith("_w") for n in _names(pl)[0])


MOD_SETS = [(False, ["LOSS.FOCAL_GAMMA", 2.0]), (False, ["LOSS.CLASS_WEIGHTS", [1.0] * 400]),
            (True, ["LOSS.POS_WEIGHT", [2.0] * 157]), (True, ["LOSS.FOCAL_GAMMA_NEG", 4.0]),
            (True, ["LOSS.CLASS_WEIGHTS", [0.5] * 157, "LOSS.FOCAL_GAMMA", 1.0])]


@pytest.mark.parametrize("multi, over", MOD_SETS, ids=[o[0] for _, o in MOD_SETS])
def test_dry_plans_with_a_modifier_differ_in_the_head_slot_only(multi, over):
    extra = ["DATA.MULTI_LABEL", True, "NETWORK.NUM_CLASSES", 157] if multi else []
    off = _dry_model(x.get_config("XS", BASE + extra))._plan(2, 4, 64, 64, True)
    m = _dry_model(x.get_config("XS", BASE + extra + over))
    on = m._plan(2, 4, 64, 64, True)
    slot = on.grad_scale_slot
    (f0, b0), (f1, b1) = _names(off), _names(on)
    assert b0 == b1 and len(f0) == len(f1) and [i for i, (p, q) in enumerate(zip(f0, f1)) if p != q] == [slot]
    name, _, args = on.fwd[slot]
    assert name == ("x3d_sigmoid_bce_w" if multi else "x3d_softmax_xent_w")
    mods = m.loss_mods
    tables = (mods.class_w, mods.pos_w) if multi else (mods.class_w,)
    k = 3 if multi else 4
    assert args[0] == on.logits.data_ptr() and args[1] is None                       # no teacher
    assert args[k:k + len(tables)] == tuple(None if t is None else t.data_ptr() for t in tables)
    assert args[k + len(tables)] is None and on.row_w is None                        # no sample weights yet, no buffer for them
    assert args[-2:] == (2, 157 if multi else 400)
    # a step with sample weights: the buffer comes into being, the entry point stays; and back to the plain entry with everything off
    on.use_soft_targets(False, row_w=True)
    assert on.fwd[slot][0] == name and on.row_w is not None and on.row_w.numel() == 2
    assert on.head_launch(False, False, 0.5, weighted=True, row_w=True)[1][k + len(tables)] == on.row_w.data_ptr()
    m.set_loss()
    assert m.loss_mods is None
    on.use_soft_targets(False)
    assert on.fwd[slot][0] == f0[slot] and _names(on) == (f0, b0)


def test_set_loss_checks_its_arguments():
    m = _dry_model(x.get_config("XS", BASE + ["NETWORK.NUM_CLASSES", 3]))
    for kw in (dict(class_weights=[1, 2]), dict(class_weights=[1, -1, 1]), dict(class_weights=[0, 0, 0]),
               dict(class_weights=[1, float("nan"), 1]), dict(focal_gamma=-1), dict(focal_gamma=9), dict(focal_gamma=float("nan")),
               dict(pos_weight=[1, 1, 1]), dict(focal_gamma_neg=1.0)):
        with pytest.raises(ValueError):
            m.set_loss(**kw)
    assert m.loss_mods is None
    m.set_loss(class_weights=np.array([1.0, 0.0, 2.0]), focal_gamma=2)
    assert m.loss_mods.class_w.dtype == torch.float32 and m.loss_mods.class_w.tolist() == [1.0, 0.0, 2.0]
    assert (m.loss_mods.pos_w, m.loss_mods.gamma, m.loss_mods.gamma_neg) == (None, 2.0, 0.0)
