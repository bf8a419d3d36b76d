"""SOLVER.FREEZE_EVAL on the host: the config key, finetune.frozen_prefix, and the launch lists of cut training plans, recorded
dry -- the frozen prefix in inference form behind one x3d_bn_eval_coef_batched, the seam tensor in a buffer of its own, a
backward list that ends with the seam unit's weight gradients and touches nothing of the prefix, stage marks the trainer's
bucket hooks can hang on as before, and no launch that dispatches to an instantiation the class-parity suites do not run.
With the key off a plan records what it always recorded.
"""
import ctypes as C

import pytest
import torch

import x3d_tf_amd as x
from x3d_tf_amd import dispatch as D
from x3d_tf_amd import plan as P
from x3d_tf_amd.config import FinetuneSettings, finetune_settings, freeze_eval_settings
from x3d_tf_amd.finetune import frozen_prefix

from tests import freeze_eval_ref as R

S3 = ["conv1/", "stages/0/", "stages/1/", "stages/2/"]


# ---- config ---------------------------------------------------------------------------------------------------------------
def test_the_key_is_optional_and_typed():
    cfg = x.get_config("M")
    assert dict(cfg.SOLVER) == dict(CLIP_GRAD_L2NORM=0.0, ACCUM_STEPS=1, EMA_DECAY=0.0, EMA_EVAL=True)
    assert cfg.SOLVER.FREEZE_EVAL is False and freeze_eval_settings(cfg) is False
    on = x.get_config("M", ["SOLVER.FREEZE", ["conv1/"], "SOLVER.FREEZE_EVAL", True])
    assert freeze_eval_settings(on) is True and dict(on.SOLVER)["FREEZE_EVAL"] is True and len(dict(on.SOLVER)) == 6
    # FinetuneSettings stays the 3-tuple of the solver step, whatever the new key holds
    assert finetune_settings(on) == FinetuneSettings(1.0, (), ("conv1/",)) == (1.0, (), ("conv1/",))
    assert finetune_settings(cfg) == (1.0, (), ())
    for bad in (1, "yes", 0.5, [True]):
        with pytest.raises(ValueError):
            x.get_config("M", ["SOLVER.FREEZE_EVAL", bad])
    c = cfg.clone()
    c.defrost()
    c.SOLVER.FREEZE_EVAL = 1                       # (set past the merge's type check)
    with pytest.raises(ValueError):
        freeze_eval_settings(c)
    bare = cfg.clone()
    bare.defrost()
    del bare["SOLVER"]
    assert freeze_eval_settings(bare) is False


# ---- frozen_prefix ----------------------------------------------------------------------------------------------------------
def _frozen(specs, freeze):
    return [s.name for s in specs if s.trainable and s.name.startswith(tuple(freeze))] if freeze else []


@pytest.mark.parametrize("variant", ["XS", "XL"])
def test_frozen_prefix(variant):
    from x3d_tf_amd.arch import block_prefix, build_arch, param_specs
    arch = build_arch(x.get_config(variant))
    specs = param_specs(arch, 3)
    L, per = len(arch.blocks), [len(st.blocks) for st in arch.stages]
    k = lambda freeze: frozen_prefix(arch, specs, _frozen(specs, freeze))
    assert k([]) == 0
    assert k(["conv1/"]) == 1
    assert k(["conv1/", "stages/0/"]) == 1 + per[0]
    mid = [block_prefix(b) + "/" for b in arch.blocks[per[0]:per[0] + 2]]
    assert k(["conv1/", "stages/0/"] + mid) == 1 + per[0] + 2
    assert k(["conv1/", "stages/0/", mid[1]]) == 1 + per[0]            # the run ends at the first block that is not frozen
    assert k(["conv1/", "stages/"]) == L + 1
    assert k(["conv1/", "stages/", "conv5/", "fc1/"]) == L + 1         # conv5 and the head are never part of it
    assert k(["stages/0/"]) == 0                                       # a hole: the stem is not frozen
    assert k(["conv1/conv_s/", "stages/0/"]) == 0                      # ... or not all of it
    # a block with one tensor left to train is not in the prefix
    names = _frozen(specs, ["conv1/", "stages/0/"])
    assert frozen_prefix(arch, specs, names[:-1]) == per[0]


def test_freeze_eval_without_a_prefix_is_refused():
    from x3d_tf_amd.model import X3D
    m = X3D(x.get_config("XS"), dtype=torch.float32, device="dry")
    with pytest.raises(ValueError, match="conv1/conv_s/kernel"):
        m.set_finetune(freeze=["stages/0/"], freeze_eval=True)
    with pytest.raises(ValueError, match="conv1/bn/gamma"):
        m.set_finetune(freeze=["conv1/conv_s/", "conv1/conv_t/", "stages/0/"], freeze_eval=True)
    with pytest.raises(ValueError):
        m.set_finetune(freeze_eval=True)
    assert m.frozen_prefix == 0
    m.set_finetune(freeze=["conv1/", "stages/0/"], freeze_eval=True)
    assert m.frozen_prefix == 1 + len(m.arch.stages[0].blocks)
    m.set_finetune(freeze=["conv1/", "stages/0/"])
    assert m.frozen_prefix == 0 and m.frozen_names
    m.set_finetune(freeze=["conv1/"], freeze_eval=True)
    m.set_finetune()
    assert m.frozen_prefix == 0


# ---- dry plans ----------------------------------------------------------------------------------------------------------------
def _dry(variant, dtype=torch.float32, overrides=None):
    from x3d_tf_amd.model import X3D
    return X3D(x.get_config(variant, overrides), dtype=dtype, device="dry")


def _canonical(m, pl, lst):
    """A launch list as comparable values: entry point names and every argument, argument structs field by field.  Addresses of a
    dry plan's stand-in buffers and of the model's own tensors are kept; accumulator addresses become offsets into the plan's
    zeroed block, and any other host allocation of the plan (labels, tables, host structs) becomes a token."""
    from x3d_tf_amd import hip
    z0 = pl.zero_buf.data_ptr()
    z1 = z0 + pl.zero_buf.numel() * 8
    own = [(t.data_ptr(), t.data_ptr() + t.numel() * t.element_size()) for t in (m.flat_params, m.flat_grads)]
    if getattr(m, "_panel_buf", None) is not None:
        own.append((m._panel_buf.data_ptr(), m._panel_buf.data_ptr() + m._panel_buf.numel() * m._panel_buf.element_size()))

    def val(v):
        if isinstance(v, C.Structure):
            return tuple((f[0], val(getattr(v, f[0]))) for f in v._fields_)
        if isinstance(v, C.Array):
            return tuple(val(e) for e in v)
        if hasattr(v, "_obj"):                      # byref(struct)
            return val(v._obj)
        if isinstance(v, C._Pointer):               # a typed pointer field: what it points to (NULL: None)
            return val(v.contents) if v else None
        if isinstance(v, int) and not isinstance(v, bool) and v >= 1 << 32:
            if v in hip.FOLDS:                      # a host struct referred to by address (x3d_bn_bwd_fold)
                return val(hip.FOLDS[v])
            if 0x7000_0000_0000 <= v < P._FakeBuf._next or any(lo <= v < hi for lo, hi in own):
                return v
            return ("acc", v - z0) if z0 <= v < z1 else "host"
        return v

    return [(e[0], tuple(val(a) for a in e[2])) for e in lst]


def _record(m, shape, freeze=(), freeze_eval=False):
    """A fresh dry training plan of `m` with the stand-in addresses starting where they always start."""
    m.release_plans()
    m.set_finetune(freeze=freeze, freeze_eval=freeze_eval)
    P._FakeBuf._next = 0x7000_0000_0000
    return m._plan(*shape, True)


@pytest.mark.parametrize("variant,dtype", [("XS", torch.float32), ("M", torch.bfloat16)])
def test_with_the_key_off_a_plan_records_what_it_recorded(variant, dtype):
    """FREEZE set, FREEZE_EVAL off or absent, against no FREEZE at all: the same forward and backward lists, names and arguments."""
    m = _dry(variant, dtype)
    shape = (2, 4, 64, 64)
    plain = _record(m, shape)
    lists = (_canonical(m, plain, plain.fwd), _canonical(m, plain, plain.bwd))
    marks = dict(plain.bwd_stage_marks)
    assert plain.frozen_prefix == 0 and plain.seam is None and not plain.prefix_bn and plain.fwd[0][0] != "x3d_bn_eval_coef_batched"
    for freeze in (["conv1/", "stages/0/", "stages/1/"], ["conv1/", "stages/"]):
        pl = _record(m, shape, freeze)
        assert pl is not plain and m.frozen_names and m.frozen_prefix == 0
        assert (_canonical(m, pl, pl.fwd), _canonical(m, pl, pl.bwd)) == lists and pl.bwd_stage_marks == marks
    # and the comparison has teeth: a cut plan differs
    cut = _record(m, shape, ["conv1/"], True)
    assert _canonical(m, cut, cut.fwd) != lists[0] and _canonical(m, cut, cut.bwd) != lists[1]
    # record_backward's default is the full list
    again = P.record_backward(m, plain, m.opt)
    assert [e[0] for e in again.launches] == [e[0] for e in plain.bwd] and again.stage_marks == marks


def _cuts(arch):
    """{label: FREEZE list}: the stem, every stage boundary, one mid-stage block, all blocks."""
    from x3d_tf_amd.arch import block_prefix
    per = [len(st.blocks) for st in arch.stages]
    cuts = {"stem": ["conv1/"], "all": ["conv1/", "stages/"]}
    for s in range(len(per) - 1):
        cuts[f"stage{s}"] = ["conv1/"] + [f"stages/{i}/" for i in range(s + 1)]
    first2 = sum(per[:2])
    cuts["mid"] = ["conv1/", "stages/0/", "stages/1/"] + [block_prefix(b) + "/" for b in arch.blocks[first2:first2 + 2]]
    return cuts


CUT_LABELS = ("stem", "stage0", "stage1", "stage2", "mid", "all")


def _span(buf):
    return (buf.data_ptr(), buf.data_ptr() + buf.numel() * torch.empty(0, dtype=buf.dtype).element_size())


def _pointers(pl, lst, i):
    return D._pointer_values(lst[i][2], pl.structs.get((id(lst), i)))


@pytest.fixture(scope="module")
def cut_plans():
    """{(variant, label): (model, plan)} at (2, 4, 64): XS and XL in fp32, M in bf16 (the fused and recomputed-output forms)."""
    got = {}
    for variant, dtype in (("XS", torch.float32), ("M", torch.bfloat16), ("XL", torch.float32)):
        for label in CUT_LABELS:
            m = _dry(variant, dtype, ["NETWORK.DROP_PATH_RATE", 0.2] if variant == "XS" else None)
            m.set_finetune(freeze=_cuts(m.arch)[label], freeze_eval=True)
            got[(variant, label)] = (m, m._plan(2, 4, 64, 64, True))
    return got


@pytest.mark.parametrize("label", CUT_LABELS)
@pytest.mark.parametrize("variant", ["XS", "M", "XL"])
def test_cut_plan_forward_list(cut_plans, variant, label):
    m, pl = cut_plans[(variant, label)]
    k, L, F = m.frozen_prefix, len(m.arch.blocks), pl.fwd
    assert pl.frozen_prefix == k >= 1 and (label != "all" or k == L + 1) and len(pl.blocks) == L
    layers = R.prefix_bn_layers(m.arch, m.params, k)
    # slot 0: the coefficients of exactly the prefix's layers, from the moving statistics
    assert F[0][0] == "x3d_bn_eval_coef_batched" and F[0][2][1] == len(layers) == len(pl.bn_eval_items) > 0
    assert sorted(pl.prefix_bn) == sorted(layers) and not any(e[0] == "x3d_bn_eval_coef_batched" for e in F[1:])
    # batch statistics (and the moving update) for every other layer, for no layer of the prefix
    every = [n[:-len("/gamma")] for n in m.params if n.endswith("/gamma")]
    gamma = {m.params[q + "/gamma"].data_ptr(): q for q in every}
    finalized = sorted(gamma[e[2][2]] for e in F if e[0] == "x3d_bn_finalize")
    assert finalized == sorted(set(every) - set(layers)) == sorted(b.prefix for b in pl.bn_layers)
    mm = {m.params[q + "/moving_mean"].data_ptr() for q in layers} | {m.params[q + "/moving_variance"].data_ptr() for q in layers}
    assert not any(mm & set(_pointers(pl, F, i)) for i in range(1, len(F)))       # nobody else is handed the prefix's moving statistics
    # prefix blocks: inference form, never dropped; trained blocks: training form
    for B in pl.blocks[:k - 1]:
        assert B.c_raw is None and B.dp_keep is None and B.bn_a.stats is None and B.bn_c.stats is None
    for l, B in enumerate(pl.blocks[k - 1:], k - 1):
        assert B.c_raw is not None and B.bn_a.stats is not None and (B.dp_keep is not None) == (m.drop_path_rates[l] > 0.0)
    assert pl.t_raw is None and not any(e[0] in ("x3d_tail_fwd", "x3d_tail_fwd_dp") and i < 2 for i, e in enumerate(F))
    # the seam tensor: one writer, then readers only -- nothing later overwrites what the backward pass reads again
    seam = pl.seam.data_ptr()
    assert seam == (pl.blocks[k - 1].x.data_ptr() if k <= L else pl.y_last.data_ptr())
    assert not any(lo <= seam < hi for lo, hi in map(_span, pl.prefix_bufs))
    uses = [i for i in range(1, len(F)) if seam in _pointers(pl, F, i)]
    st0 = pl.structs.get((id(F), uses[0]))
    assert (F[uses[0]][0] == "x3d_pw_fwd" and st0.y == seam) if k > 1 else F[uses[0]][0] in ("x3d_stem_fwd", "x3d_dwt_fwd")
    assert len(uses) >= 2
    for i in uses[1:]:
        st = pl.structs.get((id(F), i))
        if F[i][0] == "x3d_subsample2":
            assert F[i][2][0] == seam and F[i][2][1] != seam
        elif F[i][0] in ("x3d_tail_fwd", "x3d_tail_fwd_dp"):      # the seam block's identity shortcut
            assert F[i][2][2] == seam and seam not in F[i][2][:2] + F[i][2][3:]
        else:                                                     # a conv on it, or one that adds it as the identity shortcut
            assert F[i][0] == "x3d_pw_fwd" and seam in (st.x, st.in_add) and seam not in (st.y, st.in_store), (i, F[i][0])
    # the first trained unit reads it as a materialised, activated input: no tail built on load
    first = pl.blocks[k - 1].sa if k <= L else pl.s5
    assert first.x == seam and not first.in_add and not first.in_store and not first.in_scale_shift


@pytest.mark.parametrize("label", CUT_LABELS)
@pytest.mark.parametrize("variant", ["XS", "M", "XL"])
def test_cut_plan_backward_list(cut_plans, variant, label):
    m, pl = cut_plans[(variant, label)]
    k, L, Bk, g = m.frozen_prefix, len(m.arch.blocks), pl.bwd, m.grads
    names = [e[0] for e in Bk]
    frozen, trained = R.split_names(m.arch, {n: None for n in m.param_order}, k)
    assert frozen and trained and set(frozen) <= set(m.frozen_names)
    # nothing of the prefix: not its buffers (but the seam tensor), not its tensors' gradients
    spans = [_span(b) for b in pl.prefix_bufs] + [_span(g[n]) for n in frozen]
    for B in pl.blocks[:k - 1]:
        spans += [_span(t) for t in (B.xs, B.gate, B.hidden) if t is not None]
    for i in range(len(Bk)):
        for v in _pointers(pl, Bk, i):
            assert not any(lo <= v < hi for lo, hi in spans), f"{names[i]} (bwd launch {i}) is handed an address of the frozen prefix"
    # no stem backward, and only trained blocks have a depthwise / SE / tail backward
    assert not {"x3d_stem_bwd", "x3d_dwt_bwd", "x3d_stem_s_wgrad"} & set(names) and not pl.backward.input_slots
    live = pl.blocks[k - 1:]
    a_raw = {B.a_raw.data_ptr() for B in live}
    for entry, field in (("x3d_dw3d_bwd", "araw"), ("x3d_se_bnb_bwd", None)):
        idx = [i for i, n in enumerate(names) if n == entry]
        assert len(idx) == len(live)
        if field:
            assert {getattr(pl.structs[(id(Bk), i)], field) for i in idx} == a_raw
    ys = {B.y.data_ptr() for B in live}
    for i, n in enumerate(names):
        if n in ("x3d_tail_bwd", "x3d_tail_bwd_dp"):
            assert ys & set(Bk[i][2]), f"{n} (bwd launch {i}) belongs to no trained block"
    # the seam unit: weight gradients only for the convs that read the seam tensor
    seam_in = {pl.seam.data_ptr()} | ({pl.blocks[k - 1].xs.data_ptr()} if k <= L and pl.blocks[k - 1].xs is not None else set())
    readers = [i for i in range(len(Bk)) if seam_in & set(_pointers(pl, Bk, i))]
    spec = pl.blocks[k - 1].spec if k <= L else None
    assert [names[i] for i in readers] == ["x3d_pw_wgrad"] * (1 if spec is None else 1 + int(spec.has_shortcut_conv))
    assert readers[-1] == len(Bk) - 1 and names[readers[-1] - 1] == "x3d_bn_bwd_finalize"
    for i in readers:
        st = pl.structs[(id(Bk), i)]
        assert not st.dw_slab and not st.coef_fold and st.x in seam_in
    if spec is not None:
        q = P.block_prefix(spec)
        seam_w = {f"{q}/bottleneck/a/kernel"} | ({f"{q}/residual/kernel"} if spec.has_shortcut_conv else set())
    else:
        seam_w = {"conv5/layer_with_weights-0/kernel"}
    writes = D.gradient_writes(m, pl)
    assert {e for _, e, n in writes if n in seam_w} == {"x3d_pw_wgrad"}
    assert pl.blocks[k - 1].dx_view is None if k <= L else True
    # marks: every key, in today's order, non-decreasing; every trained tensor's gradient is final at its stage's mark
    n_st = len(m.arch.stages)
    marks = pl.bwd_stage_marks
    order = [n_st] + list(range(n_st - 1, -1, -1)) + [-1]
    assert list(marks) == order and [st for st, _ in sorted(marks.items(), key=lambda kv: kv[1])] == order
    assert all(marks[a] <= marks[b] for a, b in zip(order, order[1:])) and marks[-1] == len(Bk)
    seam_stage = spec.stage if spec is not None else n_st
    assert all(marks[st] == len(Bk) for st in order if st <= min(seam_stage, n_st - 1))
    seen = set()
    for i, entry, name in writes:
        assert i < marks[D.stage_of(m, name)], f"{entry} (bwd launch {i}) writes {name} at or after its stage's mark"
        seen.add(name)
    assert seen == set(trained)
    assert not D.scratch_hazards(pl)


def _uncovered(rows):
    from tests import pw_classes as PC
    pw, pwb, dw = _classes()
    return {(e, kname): shape for e, kname, shape in rows
            if (e, kname) not in pw and (e, kname) not in PC.FULL_SIZE_ONLY and not (e == "x3d_pw_bwd" and kname in pwb)
            and (e, kname) not in dw}


_CLASSES = []


def _classes():
    if not _CLASSES:
        from tests import dw_classes as DC
        from tests import pw_bwd_classes as PB
        from tests import pw_classes as PC
        _CLASSES.append((PC.enumerate_classes(), PB.enumerate_classes(), DC.enumerate_classes()))
    return _CLASSES[0]


def test_a_cut_plan_dispatches_to_enumerated_instantiations_only(cut_plans):
    """Every pointwise and depthwise launch of the cut plans above -- the seam's unslabbed weight gradients, the first trained
    conv on a materialised input, the inference-form prefix inside a training plan -- and of L and XL at their BASELINE shapes
    cut at the stage boundaries runs an instantiation that tests/pw_classes.py, tests/pw_bwd_classes.py or tests/dw_classes.py
    enumerate (and the class-parity suites therefore run): a seam reaches no untested kernel."""
    missing = {}
    for (variant, label), (m, pl) in cut_plans.items():
        for key, shape in _uncovered(D.plan_kernels(pl)).items():
            missing.setdefault(key, f"X3D-{variant} cut {label}: {shape}")
    for variant, n, t, s, dtype in (("L", 16, 16, 312, torch.bfloat16), ("XL", 8, 16, 312, torch.float16)):
        m = _dry(variant, dtype)
        for label in ("stem", "stage0", "stage1", "stage2", "all"):
            m.release_plans()
            m.set_finetune(freeze=_cuts(m.arch)[label], freeze_eval=True)
            for key, shape in _uncovered(D.plan_kernels(m._plan(n, t, s, s, True))).items():
                missing.setdefault(key, f"X3D-{variant} {n}x{t}x{s} cut {label}: {shape}")
    assert not missing, "dispatched by a cut plan but in no class enumeration:\n" + "\n".join(
        f"  {k[0]} {k[1]}   <- {v}" for k, v in sorted(missing.items()))


def test_the_plan_cache_tells_prefixes_apart():
    m = _dry("XS")
    full = m._plan(2, 4, 64, 64, True)
    m.set_finetune(freeze=["conv1/"], freeze_eval=True)
    cut1 = m._plan(2, 4, 64, 64, True)
    m.set_finetune(freeze=["conv1/", "stages/0/"], freeze_eval=True)
    cut2 = m._plan(2, 4, 64, 64, True)
    assert len({id(full), id(cut1), id(cut2)}) == 3 and (cut1.frozen_prefix, cut2.frozen_prefix) == (1, 1 + len(m.arch.stages[0].blocks))
    assert m._plan(2, 4, 64, 64, True) is cut2
    m.set_finetune()
    assert m._plan(2, 4, 64, 64, True) is full and m._plans[(2, 4, 64, 64, True)] is full
    # inference plans do not depend on it
    m.set_finetune(freeze=["conv1/"], freeze_eval=True)
    v = m.arch.num_preds
    assert m._plan(v, 4, 64, 64, False).frozen_prefix == 0 and (v, 4, 64, 64, False) in m._plans


def test_precise_bn_table_of_a_cut_plan_has_the_trained_layers_only():
    from x3d_tf_amd import hip
    m = _dry("XS")
    lay = m.precise_bn_layout()
    full = m._plan(2, 4, 64, 64, True).precise_bn_table()
    m.set_finetune(freeze=S3, freeze_eval=True)
    pl = m._plan(2, 4, 64, 64, True)
    table = pl.precise_bn_table()
    layers = R.prefix_bn_layers(m.arch, m.params, m.frozen_prefix)
    keep = [l for l, q in enumerate(lay.prefixes) if q not in layers]
    assert 0 < len(keep) == table.shape[0] == len(lay.prefixes) - len(layers) < full.shape[0]
    for col in (hip.PBN_C, hip.PBN_MEAN, hip.PBN_VAR, hip.PBN_POOLED):
        assert table[:, col].tolist() == full[keep][:, col].tolist()
    # row r's count slot is pooled[r]; every layer's sums lie behind ALL count slots of the layout: no overlap for any subset
    assert table.shape[0] <= len(lay.prefixes) <= int(table[:, hip.PBN_POOLED].min())
    ends = [int(r[hip.PBN_POOLED]) + 2 * int(r[hip.PBN_C]) for r in table]
    assert max(ends) <= lay.pooled_size and all(a <= int(b[hip.PBN_POOLED]) for a, b in zip(ends, table[1:]))
    frozen_stats = {lay.mean_offsets[l] for l, q in enumerate(lay.prefixes) if q in layers}
    assert not frozen_stats & set(table[:, hip.PBN_MEAN].tolist())
    pl.bn_layers.append(pl.bn_layers[0])
    pl._pbn_table = None
    with pytest.raises(ValueError):
        pl.precise_bn_table()
