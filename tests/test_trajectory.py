"""What a replayed training plan must find zeroed -- checked on dry plans, without a GPU.

The library's accumulating outputs are `+=` and the caller zeroes them (include/x3d_hip.h).  The model zeroes two things per
step: the plan's fp64 arena (`pl.zero_buf`) and `flat_grads`.  An accumulator that a feature allocated anywhere else is right on
step 1 and wrong from step 2 on, which no single-step parity test sees (tests/test_trajectory_gpu.py runs the steps; this file
reaches the launch forms small clips do not take: slabs, the recomputed-output backward, the 16-bit fused stem).

ACC_FIELDS / ACC_ARGS are the table of every pointer the header documents as `+=`, by argument struct and field or by entry point and
argument position, kept like dispatch._STRUCT_ACCESS / _ARG_ACCESS; a test parses the header and fails with the name of any such
pointer the table lacks.  For every launch of the recorded plans each of these pointers must lie in the arena or in `flat_grads`.
(The weight-gradient slabs are plain stores, not `+=`: what adds them up accumulates into `flat_grads`.  No accumulating pointer
of any recorded plan lies in scratch that a launch overwrites first, so the check has no such case.)
"""
import ctypes as C
import os
import re

import pytest
import torch

from tests import shapes as S
from x3d_tf_amd import dispatch, hip
from x3d_tf_amd.config import get_config
from x3d_tf_amd.model import X3D

HEADER = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "x3d_hip.h")

# ---- the table --------------------------------------------------------------------------------------------------------------------
# argument struct -> fields that are `+=`
ACC_FIELDS = {
    "PwFwdArgs": ("stats",),
    "BnBwdFold": ("dgamma", "dbeta"),
    "PwDgradArgs": ("nc_sums",),
    "PwBwdArgs": ("dw", "tail_sums_c", "tail_sums_r", "rc_sums"),
    "DwReduceJob": ("dw",),
    "PwWgradArgs": ("dw",),
    "Dw3dFwdArgs": ("stats", "pool"),
    "Dw3dBwdArgs": ("a_sums", "dw"),
    "SeBnbBwdArgs": ("dw1", "db1", "dw2", "db2", "dgamma_b", "dbeta_b"),
}
# entry point -> {argument position: name} of the arguments that are `+=`
ACC_ARGS = {
    "x3d_stem_s_wgrad": {2: "dw"},
    "x3d_dwt_fwd": {3: "stats"},
    "x3d_dwt_bwd": {7: "dw"},
    "x3d_stem_fwd": {4: "stats"},
    "x3d_stem_bwd": {7: "dw_s", 8: "dw_t"},
    "x3d_bn_bwd_finalize": {5: "dgamma", 6: "dbeta"},
    "x3d_bn_bwd_finalize_rc": {5: "dgamma", 6: "dbeta"},
    "x3d_pw_bwd_rc_finish": {3: "dw"},
    "x3d_tail_bwd": {4: "sums_c", 5: "sums_r"},
    "x3d_tail_bwd_dp": {6: "sums_c", 7: "sums_r"},
    "x3d_relu_bn_bwd_reduce": {5: "sums"},
    "x3d_roi_pool_bwd": {7: "sums"},
    "x3d_dense_bwd": {8: "dw", 9: "db"},
    # not launches of a plan (metrics, solver, regulariser): listed so that the table is the header's whole `+=` surface
    "x3d_topk_metrics": {3: "acc"},
    "x3d_class_hits": {3: "hits", 4: "counts"},
    "x3d_grad_accum": {0: "acc"},
    "x3d_l2_sumsq": {2: "out"},
}
# `name +=` in the header that is a statement of pseudo-code, not an operand
PSEUDO_CODE = {"v": "x3d_pw_fwd's epilogue: v += add", "n": "the equalize look-up table: n += h[i]"}
# a name that is `+=` under one prototype and a plain store wherever else it appears
ONLY_UNDER = {"out": ("x3d_l2_sumsq",)}


# ---- the header's own statement ---------------------------------------------------------------------------------------------------
_PLUS_EQ = re.compile(r"((?:\w+\s*,\s*)*\w+)\s*((?:\[[^\][]*\])*)\s*(?:double|float)?\s*\+=")


def _class_name(cname):
    return "".join(w.capitalize() for w in cname[4:].split("_"))          # x3d_pw_fwd_args -> PwFwdArgs, as hip.py names them


def header_accumulators(text):
    """(fields, args) in the form of ACC_FIELDS / ACC_ARGS, read from the header: a writable (non-const) pointer whose field
    comment says `+=`, or whose name some comment documents as `name [dims] +=`"""
    names = set()
    for m in _PLUS_EQ.finditer(text):
        names |= set(re.split(r"\s*,\s*", m.group(1)))
    names -= set(PSEUDO_CODE)
    fields, args = {}, {}
    for m in re.finditer(r"typedef\s+struct\s*\{(.*?)\}\s*(x3d_\w+)\s*;", text, flags=re.S):
        body = re.sub(r"^\s*/\*.*?\*/", "", m.group(1), flags=re.S | re.M)          # (block comments on lines of their own)
        for d in re.finditer(r"([^;{}]*?)\b(\w+)((?:\[\d+\])*)\s*;[ \t]*(/\*.*?\*/)?", body, flags=re.S):
            ty = re.sub(r"/\*.*?\*/", "", d.group(1), flags=re.S)
            if "*" in ty and "const" not in ty and ("+=" in (d.group(4) or "") or (d.group(2) in names and d.group(2) not in ONLY_UNDER)):
                fields.setdefault(_class_name(m.group(2)), []).append(d.group(2))
    plain = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    for m in re.finditer(r"\bint\s+(x3d_\w+)\s*\(([^(){};]*)\)\s*;", plain):
        for i, p in enumerate(m.group(2).split(",")):
            ty, name = re.match(r"(.*?)(\w+)$", " ".join(p.split())).groups()
            if "*" in ty and "const" not in ty and name in names and m.group(1) in ONLY_UNDER.get(name, (m.group(1),)):
                args.setdefault(m.group(1), {})[i] = name
    return {k: tuple(v) for k, v in fields.items()}, args


def _missing(fields, args, table_fields, table_args):
    lacks = [f"{s}.{f}" for s, fs in fields.items() for f in fs if f not in table_fields.get(s, ())]
    lacks += [f"{e}({n} at {i})" for e, ps in args.items() for i, n in ps.items() if table_args.get(e, {}).get(i) != n]
    extra = [f"{s}.{f}" for s, fs in table_fields.items() for f in fs if f not in fields.get(s, ())]
    extra += [f"{e}({n} at {i})" for e, ps in table_args.items() for i, n in ps.items() if args.get(e, {}).get(i) != n]
    return lacks, extra


def test_the_table_lists_every_accumulating_pointer_of_the_header():
    with open(HEADER) as fh:
        fields, args = header_accumulators(fh.read())
    assert len(fields) >= 9 and len(args) >= 17           # (the parse found the header's structs and prototypes at all)
    lacks, extra = _missing(fields, args, ACC_FIELDS, ACC_ARGS)
    assert not lacks, f"documented `+=` in include/x3d_hip.h but not in the table: {lacks}"
    assert not extra, f"in the table but not a writable `+=` pointer of include/x3d_hip.h: {extra}"
    # the table's structs are the binding's, field for field
    for s, fs in ACC_FIELDS.items():
        have = {n for n, _ in getattr(hip, s)._fields_}
        assert set(fs) <= have, (s, set(fs) - have)


def test_an_entry_taken_out_of_the_table_is_named():
    """the completeness test is looking: without one struct field / one argument it fails with that name"""
    with open(HEADER) as fh:
        fields, args = header_accumulators(fh.read())
    for s, fs in ACC_FIELDS.items():
        for f in fs:
            lacks, _ = _missing(fields, args, dict(ACC_FIELDS, **{s: tuple(x for x in fs if x != f)}), ACC_ARGS)
            assert lacks == [f"{s}.{f}"]
    for e, ps in ACC_ARGS.items():
        for i, n in ps.items():
            lacks, _ = _missing(fields, args, ACC_FIELDS, dict(ACC_ARGS, **{e: {j: x for j, x in ps.items() if j != i}}))
            assert lacks == [f"{e}({n} at {i})"]


# ---- the plans --------------------------------------------------------------------------------------------------------------------
def _dry(variant, dtype, over=(), finetune=None):
    m = X3D(get_config(variant, list(over) or None), dtype=dtype, device="dry")
    if finetune:
        m.set_finetune(**finetune)
    return m


def _baseline(index):
    variant, batch, t, s, dtype, training, over = dispatch.BASELINE_CONFIGS[index]
    assert training
    return _dry(variant, dtype, [v for kv in over.items() for v in kv]), (batch, t, s, s)


XS = (4, 4, 64, 64)
DET = S.DILATED_DETECTION + ["TEST.NUM_TEMPORAL_VIEWS", 1, "TEST.NUM_SPATIAL_CROPS", 1]      # (the box head takes one view per clip)
PLANS = {
    "baseline-2": lambda: _baseline(2),
    "baseline-3": lambda: _baseline(3),
    "baseline-4": lambda: _baseline(4),
    "xs-dilated-detection-fp32": lambda: (_dry("XS", torch.float32, DET), XS),
    "xs-dilated-detection-bf16": lambda: (_dry("XS", torch.bfloat16, DET), XS),
    "xs-drop-path-fp32": lambda: (_dry("XS", torch.float32, ["NETWORK.DROP_PATH_RATE", 0.5]), XS),
    "xs-drop-path-bf16": lambda: (_dry("XS", torch.bfloat16, ["NETWORK.DROP_PATH_RATE", 0.5]), XS),
    "xs-frozen-prefix-bf16": lambda: (_dry("XS", torch.bfloat16, finetune=dict(freeze=["conv1/", "stages/0/"], freeze_eval=True)), XS),
    "xs-frozen-bn-fp32": lambda: (_dry("XS", torch.float32, finetune=dict(freeze_bn=[""])), XS),
    "xs-frozen-bn-fp16": lambda: (_dry("XS", torch.float16, finetune=dict(freeze_bn=["stages/2/"])), XS),
}


def _walk(st, out):
    """(struct class name, field, value) of every pointer field of an argument struct, through nested structs, arrays of
    structs, the fold a `coef_fold` address names and the fold an `in_bn` pointer names"""
    name = type(st).__name__
    for fname, ftype in st._fields_:
        v = getattr(st, fname)
        if isinstance(v, C.Structure):
            _walk(v, out)
        elif isinstance(v, C.Array):
            for item in v:
                if isinstance(item, C.Structure):
                    _walk(item, out)
        elif isinstance(v, int) and not isinstance(v, bool) and ftype is C.c_void_p:
            out.append((name, fname, v))
            if fname == "coef_fold" and v in hip.FOLDS:
                _walk(hip.FOLDS[v], out)
        elif isinstance(v, C._Pointer) and bool(v):          # POINTER(struct), not NULL: in_bn
            _walk(v.contents, out)


def accumulator_uses(pl):
    """(list name, index, entry point, what, address) for every accumulating pointer a recorded launch is handed"""
    out = []
    for lname, lst in (("fwd", pl.fwd), ("bwd", pl.bwd)):
        for i, item in enumerate(lst):
            if item is None:
                continue
            entry, _, args = item
            for pos, what in ACC_ARGS.get(entry, {}).items():
                if pos < len(args) and isinstance(args[pos], int) and args[pos]:
                    out.append((lname, i, entry, what, args[pos]))
            structs = [pl.structs[(id(lst), i)]] if (id(lst), i) in pl.structs else []
            for a in args:
                if isinstance(a, C.Array):
                    structs += [job for job in a if isinstance(job, C.Structure)]
            seen = []
            for st in structs:
                _walk(st, seen)
            for sname, fname, v in seen:
                if v and fname in ACC_FIELDS.get(sname, ()):
                    out.append((lname, i, entry, f"{sname}.{fname}", v))
    return out


def unzeroed_accumulators(m, pl, arena=None, grads=None):
    """the accumulating pointers of `pl` that nothing brings to a defined state at the start of a step"""
    arena = pl.zero_buf if arena is None else arena
    grads = m.flat_grads if grads is None else grads
    spans = [(t.data_ptr(), t.data_ptr() + t.numel() * t.element_size()) for t in (arena, grads)]
    return [f"{lname}[{i}] {entry} {what} at {addr:#x}" for lname, i, entry, what, addr in accumulator_uses(pl)
            if not any(lo <= addr < hi for lo, hi in spans)]


@pytest.fixture(scope="module", params=sorted(PLANS))
def recorded(request):
    m, shape = PLANS[request.param]()
    return request.param, m, m._plan(*shape, True)


def test_every_accumulator_is_zeroed_each_step(recorded):
    name, m, pl = recorded
    uses = accumulator_uses(pl)
    whats = {w for _, _, _, w, _ in uses}
    # the walk reaches what it should: batch statistics, backward sums, weight and BatchNorm gradients -- or nothing is checked
    assert {"Dw3dBwdArgs.a_sums", "Dw3dBwdArgs.dw", "dw", "db"} <= whats and whats & {"dgamma", "BnBwdFold.dgamma"}, whats
    assert "Dw3dFwdArgs.stats" in whats or name == "xs-frozen-bn-fp32", whats       # (every layer frozen: no batch statistics)
    assert len(uses) > 10 * len(pl.blocks)
    bad = unzeroed_accumulators(m, pl)
    assert not bad, f"{name}: accumulating outputs outside pl.zero_buf / flat_grads: {bad[:6]}"
    if name == "baseline-4":              # the forms small clips do not take
        assert "PwBwdArgs.rc_sums" in whats and "DwReduceJob.dw" in whats and "x3d_stem_bwd" in {e for _, _, e, _, _ in uses}
    if "detection" in name:
        assert "x3d_roi_pool_bwd" in {e for _, _, e, _, _ in uses}
    if "drop-path" in name:
        assert "x3d_tail_bwd_dp" in {e for _, _, e, _, _ in uses}


def test_rc_sums_is_in_the_arena_or_zeroed_by_a_launch(recorded):
    """x3d_hip.h: rc_sums is `+=` over all points, "zero it before the launch" -- it must lie in the arena (or in flat_grads), or
    the list must hold an explicit zeroing launch of that address in front of it"""
    name, m, pl = recorded
    lo, hi = pl.zero_buf.data_ptr(), pl.zero_buf.data_ptr() + pl.zero_buf.numel() * 8
    for lname, i, entry, what, addr in accumulator_uses(pl):
        if what != "PwBwdArgs.rc_sums":
            continue
        zeroed = any(it is not None and "zero" in it[0] and addr in [a for a in it[2] if isinstance(a, int)] for it in pl.bwd[:i])
        assert lo <= addr < hi or zeroed, f"{name}: bwd[{i}] {entry} adds into rc_sums at {addr:#x}, which nothing zeroes"


def test_scratch_is_written_before_it_is_read(recorded):
    name, m, pl = recorded
    assert dispatch.scratch_hazards(pl) == []


def test_an_accumulator_outside_the_arena_is_found():
    """the check is looking: with an arena that does not hold them, every fp64 accumulator is named; with a gradient buffer that
    does not hold them, every weight gradient"""
    m, shape = PLANS["xs-drop-path-fp32"]()
    pl = m._plan(*shape, True)
    assert unzeroed_accumulators(m, pl) == []
    elsewhere = torch.zeros(4, dtype=torch.float64)
    bad = unzeroed_accumulators(m, pl, arena=elsewhere)
    assert any("Dw3dFwdArgs.stats" in b for b in bad) and any("a_sums" in b for b in bad) and not any(".dw " in b for b in bad)
    bad = unzeroed_accumulators(m, pl, grads=elsewhere)
    assert any("Dw3dBwdArgs.dw" in b for b in bad) and any("dgamma" in b for b in bad) and not any("stats" in b for b in bad)
