"""The class enumeration of the six stem entry points (tests/stem_classes.py) and its committed cases, checked on the CPU through
the library's dry-run dispatch (x3d_stem_kernel_name): the enumeration is not empty and has not shrunk; every class has its cases
inside the caps and every case lands in its own class; the class names are the committed list; the two kernels the product build
cannot reach are absent; the dimensions the module says the dispatch does not read (N, T, the conv_t entries' channel count and
launch form) still do not change a name; and every stem launch of the dry plans -- BASELINE, the shipped yamls, the same with
NETWORK.C1_TEMP_FILTER 1, 3 and 7, the same with the plan options stem_fused / stem_nthwc off -- is a class of the enumeration.
tests/test_stem_classes_gpu.py runs the classes."""
import functools
import json

import numpy as np
import pytest

from tests import shapes as S
from tests import stem_classes as SC


@pytest.fixture(scope="module")
def classes():
    return SC.enumerate_classes()


def test_the_enumeration_is_not_empty_and_has_not_shrunk(classes):
    assert classes and len(classes) >= SC.CLASSES_AT_LEAST, f"{len(classes)} classes: the admitted domain of the stem entry points shrank"
    assert {c[0] for c in classes} == set(SC.ENTRIES)
    assert {dt for dt, _ in classes.values()} == set(S.DTYPES)


def test_the_domain_is_the_stated_one():
    """KT 1 / 3 / 5 / 7 against clip lengths T <= KT / 2, T < KT and T > KT; planes that make Ho * Wo odd, = 2 mod 4, = 4 mod 8 and
    a multiple of 8; one, a ragged, two and three segments per row; rows that are not whole vectors; the four offsets."""
    assert set(SC.KTS) == {1, 3, 5, 7} and set(SC.TS) >= {1, 2, 3, 4, 6, 9} and set(SC.COUTS) == {8, 16, 24, 32}
    for kt in (3, 5, 7):
        assert any(t <= kt // 2 for t in SC.TS) and any(kt // 2 < t < kt for t in SC.TS) and any(t > kt for t in SC.TS)
    assert set(SC.WS) >= {8, 16, 24, 72, 136, 312, 9, 10, 11, 20} and {1, 2, 3} <= set(SC.HS)
    hw = {ho * wo for ho, wo in (SC.out_hw(h, w) for h, w in SC.PLANES)}
    assert any(p % 2 == 1 for p in hw) and any(p % 4 == 2 for p in hw) and any(p % 8 == 4 for p in hw) and any(p % 8 == 0 for p in hw)
    assert max(hw) > 1024          # more than one workgroup of the 4-element conv_t kernels
    assert SC.OFFS == (0, 1, 2, 4) and set(SC.CINS) == {1, 2, 3} and SC.LAYOUTS == (0, 1)


def test_every_class_has_its_cases(classes):
    """every class has 1 .. MAX_CASES cases, no tensor above MAX_ELEMS elements, and every case dispatches to its own class (the
    round trip through the name query); per class the rules of class_cases hold: every T of the domain (entries with a conv_t),
    N = 3, every Cout, Cin, layout and operand offset the class admits, every launch form it admits."""
    total = launches = 0
    for cls, (dtype, m) in classes.items():
        cases = SC.class_cases(cls)
        assert 1 <= len(cases) <= SC.MAX_CASES and len(set(cases)) == len(cases), cls
        total += len(cases)
        for c in cases:
            ho, wo = SC.out_hw(c.h, c.w)
            assert max(c.n * c.cout * c.t * ho * wo, c.n * c.cin * c.t * c.h * c.w) <= SC.MAX_ELEMS, (cls, c)
            assert c.entry == cls[0] and c.dtype == dtype and SC.dispatch(c) == cls, (cls, c, SC.dispatch(c))
        col = lambda name: set(m[:, SC.MEMBER_COLS.index(name)].tolist())
        if SC.has_conv_t(cls[0]):
            assert {c.t for c in cases} >= col("T") == set(SC.TS), cls
        assert {c.n for c in cases} == {1, 3}, cls
        assert {c.cout for c in cases} == col("cout") and {c.cin for c in cases} == col("cin"), cls
        assert {c.layout for c in cases} == col("layout") and {c.off for c in cases} == col("off"), cls
        assert len({(c.w - 1) // 2 // 64 for c in cases}) == len({(w - 1) // 2 // 64 for w in col("W")}), cls       # segments per row
        forms = {f for c in cases for f in SC.case_forms(c, cls)}
        assert forms == {SC.FORMS[i] for i in col("form")}, (cls, forms)
        launches += sum(len(SC.case_forms(c, cls)) for c in cases)
    print(f"{len(classes)} classes, {total} cases, {launches} launch forms")


def test_class_names_are_the_committed_list(classes):
    """tests/golden/stem_classes.json: a change that adds or removes an instantiation updates the list in the same change
    (python -m tests.stem_classes) and cannot silently lose its cases."""
    with open(SC.GOLDEN) as f:
        want = json.load(f)
    got = SC.golden()
    names = lambda g: [tuple(c[:2]) for c in g["classes"]]
    assert names(got) == names(want), (f"not listed: {sorted(set(names(got)) - set(names(want)))}; "
                                       f"listed but not reached: {sorted(set(names(want)) - set(names(got)))}")
    assert got == want, "the case counts differ from the committed list"
    assert want["count"] == SC.CLASSES_AT_LEAST


def test_the_two_unreachable_kernels_are_absent(classes):
    """stem_s_wgrad_kernel (past 2^31 row segments, or the X3D_STEM_WGRAD_ROWS hook) and dwt_bwd_kernel<., 8, .> (the
    X3D_DWT_BWD_VEC hook) exist in csrc/stem.hip; the product build reaches neither over the domain."""
    import os
    src = open(os.path.join(os.path.dirname(SC.GOLDEN), "..", "..", "x3d-tf_amd", "csrc", "stem.hip")).read()
    assert "void stem_s_wgrad_kernel(" in src and "dwt_bwd_kt<bf16, 8>" in src
    for _, name in classes:
        assert not name.startswith(SC.UNREACHABLE), name
    assert any(n.startswith("stem_s_wgrad_rows_kernel<") for _, n in classes) and any(n.startswith("dwt_bwd_kernel<bf16,4,") for _, n in classes)


def _without(m, name):
    j = SC.MEMBER_COLS.index(name)
    return {tuple(r[:j]) + tuple(r[j + 1:]) for r in m.tolist()}


def test_what_the_dispatch_does_not_read(classes):
    """T never changes a name; the channel count and the launch form never change one for x3d_dwt_fwd / x3d_dwt_bwd, nor the form
    for x3d_stem_bwd: every value of the dimension has the same members.  x3d_stem_fwd reads the inference epilogue (a template
    argument) but not out_act, nor whether statistics are given."""
    j = SC.MEMBER_COLS.index
    for cls, (_, m) in classes.items():
        def same_over(name, values=None):
            vals = sorted(set(m[:, j(name)].tolist())) if values is None else values
            sets = [_without(m[m[:, j(name)] == v], name) for v in vals]
            return all(s == sets[0] and s for s in sets)
        assert same_over("T", list(SC.TS)), cls
        if cls[0].startswith("x3d_dwt"):
            assert same_over("cout", list(SC.COUTS)), cls
        if cls[0] in ("x3d_dwt_fwd", "x3d_dwt_bwd", "x3d_stem_bwd"):
            assert same_over("form", [SC.FORMS.index(f) for f in SC.ENTRY_FORMS[cls[0]]]), cls
        if cls[0] == "x3d_stem_fwd":
            want = ("infer0", "infer1") if cls[1].endswith(",infer>") else ("stats", "plain")
            assert cls[1].endswith((",infer>", ",train>")) and same_over("form", [SC.FORMS.index(f) for f in want]), cls
            assert set(m[:, j("form")].tolist()) == {SC.FORMS.index(f) for f in want}, cls


def test_n_does_not_change_a_name(classes):
    """the walk runs at N = 1: the same walk at N = 3 (two clip lengths) puts every point into the same class"""
    ts = (1, 6)
    other = SC.walk(3, ts)
    assert set(other) == set(classes)
    t = SC.MEMBER_COLS.index("T")
    for cls, (dtype, m) in classes.items():
        sub = m[np.isin(m[:, t], ts)]
        assert other[cls][0] == dtype and {tuple(r) for r in sub.tolist()} == {tuple(r) for r in other[cls][1].tolist()}, cls


# ---- the stem launches of the dry plans --------------------------------------------------------------------------------------
STEM_OPTIONS = ({}, {"stem_fused": False}, {"stem_nthwc": False})
PLAN_KTS = (None, 1, 3, 7)          # NETWORK.C1_TEMP_FILTER: the yaml's (5), and the other three conv_t instantiations


@functools.lru_cache(maxsize=None)
def _plan_stem(variant, n, t, s, dtype, training, kt, options, overrides=()):
    """((entry point, instantiation), ...) of the stem launches of one dry plan, with pl.stem_fused and pl.x_cl"""
    from x3d_tf_amd.config import get_config
    from x3d_tf_amd.model import X3D
    flat = list(overrides) + ([] if kt is None else ["NETWORK.C1_TEMP_FILTER", kt])
    m = X3D(get_config(variant, flat or None), dtype=dtype, device="dry", options=dict(options) or None)
    pl = m._plan(n, t, s, s, training)
    out = tuple((e, k) for e, k, _ in SC.plan_stem_classes(pl)), pl.stem_fused, pl.x_cl
    m.release_plans()
    return out


def _all_plans():
    """(description, plan key) of every dry plan of the sweep: the five BASELINE plans and the shipped yamls' plans (three storage
    types, training and inference), each with the yaml's conv_t and with KT 1 / 3 / 7, and each with the stem's plan options off"""
    from x3d_tf_amd.dispatch import BASELINE_CONFIGS
    from tests.test_dispatch_coverage import SHIPPED_VARIANTS, shipped_config_plans
    base = [(f"BASELINE {i}", (v, n, t, s, dt, tr), tuple(x for kv in over.items() for x in kv))
            for i, (v, n, t, s, dt, tr, over) in BASELINE_CONFIGS.items()]
    base += [(f"X3D-{v}", (v, n, t, s, dt, tr), ()) for v in SHIPPED_VARIANTS for dt in S.DTYPES for n, t, s, tr in shipped_config_plans(v)]
    out = []
    for what, key, over in base:
        out += [(f"{what} {key[1:]} KT {kt or 'yaml'}", key + (kt, (), over)) for kt in PLAN_KTS]
        out += [(f"{what} {key[1:]} {opt}", key + (None, tuple(opt.items()), over)) for opt in STEM_OPTIONS[1:]]
    return out


def test_every_stem_launch_of_the_dry_plans_is_a_class(classes):
    """The argument tuples come from the plans' recorded launches (as tests/test_dispatch_coverage.py takes the aux entries'),
    the names from the dry-run dispatch over them."""
    import torch
    missing, seen, fused_kt = {}, set(), set()
    plans = _all_plans()
    for what, key in plans:
        launches, fused, x_cl = _plan_stem(*key)
        training, kt, options = key[5], key[6], dict(key[7])
        names = [e for e, _ in launches]
        if fused:
            assert names == ["x3d_stem_fwd"] + (["x3d_stem_bwd"] if training else []), (what, names)
            assert kt is None and key[4] != torch.float32 and not options, what
        else:
            assert names == ["x3d_stem_s_fwd", "x3d_dwt_fwd"] + (["x3d_dwt_bwd", "x3d_stem_s_wgrad"] if training else []), (what, names)
        if kt is not None or options:           # the fused kernels take KT = 5 on an in-place channels-last batch only
            assert not fused, what
        if options.get("stem_nthwc") is False:
            assert not x_cl, what
        for cls in launches:
            seen.add(cls)
            if cls not in classes:
                missing.setdefault(cls, what)
    assert not missing, "stem launches of the dry plans that are no class of tests/stem_classes.py:\n" + "\n".join(
        f"  {k}   <- {v}" for k, v in sorted(missing.items()))
    assert {e for e, _ in seen} == set(SC.ENTRIES)
    for kt in (1, 3, 7):       # a 16-bit model with another C1_TEMP_FILTER runs the two-kernel path in training form
        assert ("x3d_dwt_bwd", f"dwt_bwd_kernel<bf16,4,{kt}>") in seen and ("x3d_dwt_fwd", f"dwt_fwd_kernel<f16,4,{kt}>") in seen, kt
    print(f"{len(plans)} dry plans, {len(seen)} of the {len(classes)} classes launched by one")
