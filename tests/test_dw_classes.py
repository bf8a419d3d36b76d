"""The class enumeration of the depthwise entry points (tests/dw_classes.py) and its committed cases, checked on the CPU through
the library's dry-run dispatch: the enumeration holds everything the registered lists, the fuzz slice, the BASELINE plans and the
shipped-config plans dispatch; it has not shrunk; every class has its cases inside the caps and every case lands in its class; the
class names are the committed list; and the dimensions the module leaves out of the walk (N and C, the forward without a prologue,
statistics / pool given or absent) still do not change a name.  tests/test_dw_classes_gpu.py runs the classes."""
import ctypes as C
import json

import numpy as np
import pytest

from tests import dw_classes as DC
from tests import shapes as S


@pytest.fixture(scope="module")
def classes():
    return DC.enumerate_classes()


def test_enumeration_holds_every_listed_and_planned_instantiation(classes):
    """(a) what shapes.DW, shapes.DW_FULL and the fuzz slice dispatch over all three storage types, and what every BASELINE dry
    plan and every shipped-config dry plan launches, is a subset of the enumeration."""
    from x3d_tf_amd import dispatch as D
    from tests.test_dispatch_coverage import shipped_config_kernels
    need = dict(DC.registered_names())
    for k, v in DC.fuzz_slice_names().items():
        need.setdefault(k, v)
    for index in D.BASELINE_CONFIGS:
        for entry, kern, shape in D.baseline_kernels(index):
            if entry.startswith("x3d_dw3d"):
                need.setdefault((entry, kern), f"config {index}: {shape}")
    for (entry, kern), what in shipped_config_kernels().items():
        if entry.startswith("x3d_dw3d"):
            need.setdefault((entry, kern), what)
    assert need
    missing = {k: v for k, v in need.items() if k not in classes}
    print(f"x3d_dw3d_fwd / _bwd: {len(classes)} reachable instantiations, {len(need)} of them listed or planned")
    assert not missing, "dispatched but not enumerated:\n" + "\n".join(f"  {k}   <- {v}" for k, v in sorted(missing.items()))


def test_the_domain_has_not_shrunk(classes):
    """(b) the floor is the count the enumeration found when it was written; 202 is what the domain without the operand offsets,
    the folded prologue and the listed planes gives."""
    assert DC.CLASSES_AT_LEAST >= 202
    assert len(classes) >= DC.CLASSES_AT_LEAST, f"{len(classes)} classes: the admitted domain of x3d_dw3d_fwd / _bwd shrank"
    assert set(DC.SWEEP_TS) <= set(DC.TS) and {(h, h) for h in DC.HS} <= set(DC.PLANES) and DC.OFFS == (0, 1, 2, 4)


def test_every_class_has_its_cases(classes):
    """(c) every class has 1 .. MAX_CASES cases, no tensor above MAX_ELEMS elements, every case dispatches to its class; and per
    class the rules of class_cases hold: every T of the sweep the class admits, (N, C) = (3, 5) and N = 16, every non-zero
    offset the class admits, every launch form (table / folded BatchNorm) the class admits."""
    total, launches = 0, [0, 0]
    for cls, (dtype, m) in classes.items():
        cases = DC.class_cases(cls)
        assert 1 <= len(cases) <= DC.MAX_CASES and len(set(cases)) == len(cases), cls
        total += len(cases)
        for case in cases:
            assert case.n * case.c * case.t * case.h * case.w <= DC.MAX_ELEMS, (cls, case)
            assert case.dtype == dtype and DC.dispatch(case) == cls, (cls, case, DC.dispatch(case))
        ts = set(m[:, 1].tolist())
        assert {c.t for c in cases} >= ({t for t in ts if t in DC.SWEEP_TS} or ts), cls
        assert {(c.n, c.c) for c in cases} >= set(DC.NCS[1:]), cls
        assert {c.off for c in cases} >= set(m[:, 4].tolist()) - {0}, cls
        # every launch form the class admits is run: the runner takes a case through DC.case_forms
        forms = {f for c in cases for f in DC.case_forms(c, cls)}
        assert forms == {DC.FORMS[i] if DC.FORMS[i] != "bwd" else None for i in set(m[:, 5].tolist())}, (cls, forms)
        for c in cases:
            assert all(DC.dispatch(c._replace(pro=f)) == cls for f in DC.case_forms(c, cls)), (cls, c)
        launches[0] += sum(f == "ss" for c in cases for f in DC.case_forms(c, cls))
        launches[1] += sum(f == "bn" for c in cases for f in DC.case_forms(c, cls))
    print(f"{len(classes)} classes, {total} cases; forward launches: {launches[0]} with the table, {launches[1]} with the folded BatchNorm")
    assert launches[1] > 0


def test_class_names_are_the_committed_list(classes):
    """(d) tests/golden/dw_classes.json: a rewrite that adds or removes an instantiation updates the list in the same change
    (python -m tests.dw_classes) and cannot silently lose its case."""
    with open(DC.GOLDEN) as f:
        want = json.load(f)
    got = DC.golden()
    names = lambda g: [tuple(c[:2]) for c in g["classes"]]
    assert names(got) == names(want), (f"not listed: {sorted(set(names(got)) - set(names(want)))}; "
                                       f"listed but not reached: {sorted(set(names(want)) - set(names(got)))}")
    assert got == want, "the case counts differ from the committed list"


@pytest.mark.parametrize("nc", DC.NCS[1:])
def test_n_and_c_do_not_change_a_name(nc):
    """the walk runs at (N, C) = (1, 2): the same walk at (3, 5) and at (16, 2) gives the same instantiation at every point"""
    ids0, names0 = DC.walk()
    ids1, names1 = DC.walk(*nc)
    assert names0 == names1 and np.array_equal(ids0, ids1)


def test_prologue_and_sums_do_not_change_a_name():
    """the forward without a prologue, and with statistics / pool absent, dispatches as the "ss" form with both: asked over every
    storage type, stride, plane and offset of the domain at three clip lengths"""
    from x3d_tf_amd import hip
    name_of = hip.load().x3d_dw3d_kernel_name
    buf = C.create_string_buffer(128)

    def name(st):
        return buf.value if name_of(C.byref(st), None, buf, 128) == 0 else None
    for dtype in S.DTYPES:
        for off in DC.OFFS:
            ref = DC.case_struct(DC.Case("fwd", dtype, 1, 2, 1, 3, 3, 1, off, "ss"))
            bare = DC.case_struct(DC.Case("fwd", dtype, 1, 2, 1, 3, 3, 1, off, "ss"))
            bare.stats = bare.pool = None
            plain = DC.case_struct(DC.Case("fwd", dtype, 1, 2, 1, 3, 3, 1, off, "ss"))
            plain.in_scale_shift, plain.in_act = None, 0
            for stride in DC.STRIDES:
                for h, w in DC.PLANES:
                    for t in (1, 4, 13):
                        for st in (ref, bare, plain):
                            st.stride, st.H, st.W, st.T = stride, h, w, t
                        want = name(ref)
                        assert name(bare) == want and name(plain) == want, (dtype, off, stride, t, h, w)
