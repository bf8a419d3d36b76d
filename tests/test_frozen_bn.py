"""SOLVER.FREEZE_BN on the host: the config key, the layer matcher, and the launch lists of training plans with frozen BatchNorm
layers, recorded dry at the full sizes of the five shipped configs -- no x3d_bn_finalize for a frozen layer, one
x3d_bn_eval_coef_batched at slot 0 over all of them, a backward finalize LAUNCH in the frozen form for every frozen layer (the
consumers that derive the table themselves have no frozen form), and with the key off the lists a model records that never heard
of it.
"""
import pytest
import torch

import x3d_tf_amd as x
from x3d_tf_amd import hip
from x3d_tf_amd import plan as P
from x3d_tf_amd.config import freeze_bn_settings

from tests import frozen_bn_ref as R
from tests.test_freeze_eval import _canonical



def _full_size(variant, dtype):
    """(variant, clips, frames, crop, storage): the training batch of a shipped yaml on one GPU"""
    cfg = x.get_config(variant)
    return (variant, cfg.TRAIN.BATCH_SIZE, cfg.DATA.TEMP_DURATION, cfg.DATA.TRAIN_CROP_SIZE, dtype)


# the five shipped configs at their full training sizes (storage types as tests/test_model_gpu.py FULL_SIZE_TRAIN runs them)
FULL = [_full_size("XS", torch.float32), _full_size("S", torch.float32), _full_size("M", torch.bfloat16),
        _full_size("L", torch.bfloat16), _full_size("XL", torch.float16)]
IDS = [c[0] for c in FULL]


def _dry(variant, dtype, overrides=None):
    from x3d_tf_amd.model import X3D
    return X3D(x.get_config(variant, overrides), dtype=dtype, device="dry")


def _record(m, shape, **finetune):
    m.release_plans()
    m.set_finetune(**finetune)
    P._FakeBuf._next = 0x7000_0000_0000
    return m._plan(*shape, True)


# ---- config -----------------------------------------------------------------------------------------------------------------
def test_the_key_parses_is_optional_and_typed():
    on = x.get_config("XS", ["SOLVER.FREEZE_BN", [""]])           # (KeyError, "non-existent key", before the feature)
    assert freeze_bn_settings(on) == ("",) and dict(on.SOLVER)["FREEZE_BN"] == [""]
    cfg = x.get_config("XS")
    assert dict(cfg.SOLVER) == dict(CLIP_GRAD_L2NORM=0.0, ACCUM_STEPS=1, EMA_DECAY=0.0, EMA_EVAL=True)
    assert freeze_bn_settings(cfg) == () and cfg.SOLVER.FREEZE_BN == []
    assert freeze_bn_settings(x.get_config("M", ["SOLVER.FREEZE_BN", ["stages/2/", "conv1/bn"]])) == ("stages/2/", "conv1/bn")
    for bad in ("stages/2/", 1, True, [1], [["conv1/bn"]], [None]):
        with pytest.raises(ValueError):
            x.get_config("XS", ["SOLVER.FREEZE_BN", bad])
    c = cfg.clone()
    c.defrost()
    c.SOLVER.FREEZE_BN = ["conv1/bn", 3]                          # (set past the merge's type check)
    with pytest.raises(ValueError):
        freeze_bn_settings(c)
    bare = cfg.clone()
    bare.defrost()
    del bare["SOLVER"]
    assert freeze_bn_settings(bare) == ()


def test_the_matcher_and_an_unmatched_prefix():
    from x3d_tf_amd.arch import build_arch, param_specs
    from x3d_tf_amd.finetune import frozen_bn_layers
    specs = param_specs(build_arch(x.get_config("XS")), 3)
    every = [s.name[:-len("/gamma")] for s in specs if s.name.endswith("/gamma")]
    assert len(every) == 84 and frozen_bn_layers(specs, [""]) == tuple(every) and frozen_bn_layers(specs, []) == ()
    assert frozen_bn_layers(specs, ["conv1/bn"]) == ("conv1/bn",)
    got = frozen_bn_layers(specs, ["stages/2/", "conv5/"])
    assert got == tuple(q for q in every if q.startswith(("stages/2/", "conv5/"))) and "conv5/layer_with_weights-1" in got
    for bad in (["stages/9/"], ["conv1/bn", "bn_a"], ["conv1/conv_s"]):
        with pytest.raises(ValueError, match="matches no BatchNorm layer"):
            frozen_bn_layers(specs, bad)
    m = _dry("XS", torch.float32)
    with pytest.raises(ValueError, match="matches no BatchNorm layer"):
        m.set_finetune(freeze_bn=["stages/2/", "nowhere/"])
    with pytest.raises(ValueError):
        m.set_finetune(freeze_bn="stages/2/")
    assert m.frozen_bn == ()
    m.set_finetune(freeze_bn=["stages/2/"])
    assert m.frozen_bn and all(q.startswith("stages/2/") for q in m.frozen_bn) and m.frozen_names == [] and m._ft is None
    m.set_finetune(freeze=["conv1/"], freeze_bn=["conv1/bn"])
    assert m.frozen_bn == ("conv1/bn",) and m.frozen_names
    m.set_finetune()
    assert m.frozen_bn == ()


# ---- dry plans ----------------------------------------------------------------------------------------------------------------
def _bwd_finalizes(pl):
    """[(kind, count, address of gamma)] of every BatchNorm-backward finalize of the plan's backward list: the launches, and the
    derivations of coef_fold consumers (one per BatchNorm: the publishing consumer's)."""
    out = []
    for i, e in enumerate(pl.bwd):
        if e[0] in ("x3d_bn_bwd_finalize", "x3d_bn_bwd_finalize_rc"):
            out.append((e[0], e[2][1], e[2][3]))
        st = pl.structs.get((id(pl.bwd), i))
        if st is not None and getattr(st, "coef_fold", None):
            f = hip.FOLDS[st.coef_fold]
            assert f.count > 0
            if f.dgamma:
                out.append(("coef_fold", f.count, f.gamma))
    return out


def _check_backward(m, pl, bwd0, fin0, layers):
    """The backward list of a plan whose `layers` are frozen, against the default plan's (names bwd0, finalizes fin0): nothing
    but finalize launches differs; every BatchNorm keeps exactly one finalize, with the same element count; a frozen layer's
    is a LAUNCH with a negative count (or x3d_se_bnb_bwd with P < 0 for bn_b), any other layer's is what it was."""
    plain = ("x3d_bn_bwd_finalize",)
    assert [e for e in (x[0] for x in pl.bwd) if e not in plain] == [e for e in bwd0 if e not in plain]
    frozen_gamma = {m.params[q + "/gamma"].data_ptr() for q in layers}
    fin = _bwd_finalizes(pl)
    assert sorted((g, abs(c)) for _, c, g in fin) == sorted((g, c) for _, c, g in fin0) and all(c > 0 for _, c, _ in fin0)
    was = {g: kind for kind, _, g in fin0}
    for kind, c, g in fin:
        if g in frozen_gamma:
            assert c < 0 and kind != "coef_fold" and (kind == was[g] or was[g] == "coef_fold"), (kind, c, was[g])
        else:
            assert c > 0 and kind == was[g]
    se = [(pl.structs[(id(pl.bwd), i)].P, pl.structs[(id(pl.bwd), i)].gamma_b) for i, e in enumerate(pl.bwd) if e[0] == "x3d_se_bnb_bwd"]
    assert len(se) == len(m.arch.blocks) and all((p < 0) == (g in frozen_gamma) for p, g in se)
    assert len(fin) + len(se) == len(R.bn_layers(m.params))
    return fin, se


@pytest.fixture(scope="module")
def full_plans():
    got = {}
    for variant, n, t, s, dtype in FULL:
        m = _dry(variant, dtype)
        plain = _record(m, (n, t, s, s))
        names = ([e[0] for e in plain.fwd], [e[0] for e in plain.bwd], _bwd_finalizes(plain))
        got[variant] = (m, names)
    return got


@pytest.mark.parametrize("variant,n,t,s,dtype", FULL, ids=IDS)
def test_every_layer_frozen(full_plans, variant, n, t, s, dtype):
    m, (fwd0, bwd0, fin0) = full_plans[variant]
    pl = _record(m, (n, t, s, s), freeze_bn=[""])
    layers = R.bn_layers(m.params)
    F = [e[0] for e in pl.fwd]
    assert "x3d_bn_finalize" not in F and fwd0.count("x3d_bn_finalize") == len(layers)
    assert F[0] == "x3d_bn_eval_coef_batched" and pl.fwd[0][2][1] == len(layers) == len(pl.bn_eval_items) and F.count(F[0]) == 1
    assert F[1:] == [e for e in fwd0 if e != "x3d_bn_finalize"]                  # nothing else moved
    assert not pl.bn_layers and sorted(pl.prefix_bn) == sorted(layers)
    # no producer accumulates statistics any more
    for i, e in enumerate(pl.fwd):
        st = pl.structs.get((id(pl.fwd), i))
        if e[0] in ("x3d_pw_fwd", "x3d_dw3d_fwd"):
            assert not st.stats, (i, e[0])
        if e[0] in ("x3d_stem_fwd", "x3d_dwt_fwd"):
            assert e[2][4 if e[0] == "x3d_stem_fwd" else 3] is None
    # backward: one finalize per BatchNorm as before, every one a launch in the frozen form; no consumer derives a table
    fin, se = _check_backward(m, pl, bwd0, fin0, layers)
    assert all(kind != "coef_fold" and c < 0 for kind, c, _ in fin) and all(p < 0 for p, _ in se)
    assert not any(getattr(pl.structs.get((id(pl.bwd), i)), "coef_fold", None) for i in range(len(pl.bwd)))
    # the same kernels behind every pointwise / depthwise launch: dropping the accumulator selects no other instantiation
    from x3d_tf_amd import dispatch as D
    m.release_plans()
    m.set_finetune()
    plain = m._plan(n, t, s, s, True)
    assert sorted((e, k) for e, k, _ in D.plan_kernels(pl)) == sorted((e, k) for e, k, _ in D.plan_kernels(plain))


@pytest.mark.parametrize("variant,n,t,s,dtype", FULL, ids=IDS)
def test_one_stage_frozen(full_plans, variant, n, t, s, dtype):
    m, (fwd0, bwd0, fin0) = full_plans[variant]
    pl = _record(m, (n, t, s, s), freeze_bn=["stages/2/"])
    layers = R.frozen_layers(m.params, ["stages/2/"])
    assert layers and tuple(layers) == m.frozen_bn
    gamma = {m.params[q + "/gamma"].data_ptr(): q for q in R.bn_layers(m.params)}
    finalized = sorted(gamma[e[2][2]] for e in pl.fwd if e[0] == "x3d_bn_finalize")
    assert finalized == sorted(set(gamma.values()) - set(layers)) == sorted(b.prefix for b in pl.bn_layers)
    assert pl.fwd[0][0] == "x3d_bn_eval_coef_batched" and pl.fwd[0][2][1] == len(layers)
    _without(fwd0, len(layers), pl)
    fin, se = _check_backward(m, pl, bwd0, fin0, layers)
    n2 = len(m.arch.stages[2].blocks)
    assert sum(1 for _, c, _ in fin if c < 0) + sum(1 for p, _ in se if p < 0) == len(layers) and sum(1 for p, _ in se if p < 0) == n2
    table = pl.precise_bn_table()
    assert table.shape[0] == len(gamma) - len(layers)


def _without(fwd0, dropped, pl):
    """fwd0 without the finalize launches the plan `pl` no longer has: the names of pl.fwd[1:] must be fwd0 less `dropped`
    x3d_bn_finalize entries, in order."""
    names = [e[0] for e in pl.fwd[1:]]
    assert len(names) == len(fwd0) - dropped
    assert [e for e in names if e != "x3d_bn_finalize"] == [e for e in fwd0 if e != "x3d_bn_finalize"]
    return names


@pytest.mark.parametrize("variant,n,t,s,dtype", [FULL[0], FULL[2]], ids=["XS", "M"])
def test_with_the_key_off_a_plan_records_what_it_recorded(variant, n, t, s, dtype):
    """freeze_bn = () -- and SOLVER.FREEZE_BN = [] through the config -- against a model that was never given the argument: the
    same forward and backward lists, names and arguments; and the comparison has teeth."""
    shape = (2, 4, 64, 64)
    off = _dry(variant, dtype, ["SOLVER.FREEZE_BN", []])
    P._FakeBuf._next = 0x7000_0000_0000
    ref_pl = off._plan(*shape, True)                               # (set_finetune was never called on this model)
    lists = (_canonical(off, ref_pl, ref_pl.fwd), _canonical(off, ref_pl, ref_pl.bwd))
    pl = _record(off, shape, freeze_bn=())
    assert pl is not ref_pl and (shape + (True,)) in off._plans and off.frozen_bn == ()
    assert (_canonical(off, pl, pl.fwd), _canonical(off, pl, pl.bwd)) == lists and pl.bwd_stage_marks == ref_pl.bwd_stage_marks
    assert pl.fwd[0][0] != "x3d_bn_eval_coef_batched" and not pl.prefix_bn and not pl.bn_eval_items
    on = _record(off, shape, freeze_bn=["conv5/"])
    assert _canonical(off, on, on.fwd) != lists[0] and _canonical(off, on, on.bwd) != lists[1]
    # the plan cache tells the sets apart, and inference plans do not depend on them
    assert on is not pl and off._plan(*shape, True) is on
    v = off.arch.num_preds
    inf = off._plan(v, 4, 64, 64, False)
    assert not inf.frozen_bn and (v, 4, 64, 64, False) in off._plans


def test_composition_with_a_frozen_prefix_is_one_table():
    m = _dry("XS", torch.float32)
    pl = _record(m, (2, 4, 64, 64), freeze=["conv1/", "stages/0/"], freeze_eval=True, freeze_bn=[""])
    layers = R.bn_layers(m.params)
    names = [e[0] for e in pl.fwd]
    assert names[0] == "x3d_bn_eval_coef_batched" and names.count(names[0]) == 1 and pl.fwd[0][2][1] == len(layers)
    assert "x3d_bn_finalize" not in names and pl.frozen_prefix == 1 + len(m.arch.stages[0].blocks)
    prefix = R.prefix_bn_layers(m.arch, m.params, pl.frozen_prefix)
    assert sorted(pl.prefix_bn) == sorted(layers) and 0 < len(prefix) < len(layers)
    # precise BatchNorm has nothing to recompute
    from x3d_tf_amd.precise_bn import recomputed_layers, update_bn_stats
    assert recomputed_layers(m) == [] and update_bn_stats(m, iter(()), 2) == 0
    m.set_finetune(freeze_bn=["stages/"])
    assert recomputed_layers(m) == ["conv1/bn", "conv5/layer_with_weights-1"]
