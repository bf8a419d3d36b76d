"""Every kernel instantiation the six stem entry points can dispatch, as data, and the committed parity cases of each.

tests/test_kernels_gpu.py (test_stem, test_stem_fused) and tests/test_full_size_gpu.py run the stem -- csrc/stem.hip and
csrc/stem_fused.hip: x3d_stem_s_fwd, x3d_stem_s_wgrad, x3d_dwt_fwd, x3d_dwt_bwd, x3d_stem_fwd, x3d_stem_bwd -- on hand-picked shapes;
which instantiations those reach is an accident of the lists (KT = 5 only, Cout 24 / 32, every operand aligned).  This module looks
from the other side, as tests/dw_classes.py does for the depthwise entry points: it walks a domain of launches through the
library's dry-run dispatch (x3d_stem_kernel_name: no GPU, nothing launched) and returns every (entry point, instantiation) it
meets -- a CLASS -- with the points of the domain that dispatch to it.  class_cases() then picks the committed cases of a class
from its own members by fixed rules, so nothing is drawn and nothing is declined.  tests/test_stem_classes.py (CPU) checks the
enumeration, tests/test_stem_classes_gpu.py runs every class against fp64 (tests/stem_checks.py).

The domain: the three storage types; the clip planes H in HS x W in WS (one segment of 64 output columns, a ragged one, two and
three segments per row; W = 9, 10, 11, 20: rows that are not whole vectors; Ho * Wo odd, = 2 mod 4, = 4 mod 8 and a multiple of 8,
which is what pick_vec reads); T in TS (T <= KT / 2, T < KT, T > KT for every KT); conv_t with KT in KTS; conv_s with Cout in
COUTS, Cin = 3 (x3d_stem_s_wgrad also 1 and 2), the batch planar and channels-last; every tensor operand OFFS elements off its
16-byte-aligned allocation; every launch form of FORMS.  The conv_t entries run on the conv_s output, so their plane is Ho x Wo
and their channel count Cout.

What the dispatch does NOT read, found by asking it over the whole domain (tests/test_stem_classes.py keeps asking):
  * N (every entry): the walk runs at N = 1, the cases also take N = 3;
  * T (every entry) and, for the conv_t entries, the channel count: no name changes along them, so a class holds every T and
    every Cout and the case rules sweep them;
  * the launch form of x3d_dwt_fwd (statistics, inference epilogue with out_act 0 / 1, neither) and of x3d_dwt_bwd / x3d_stem_bwd
    (relu_scale_shift given or not): the same name everywhere.  x3d_stem_fwd DOES read it: the inference epilogue is a template
    argument (stem_fwd_fused_kernel<., ., infer> / <., ., train>), out_act is not.
The runner launches every case in every form of its entry that keeps it in its class (case_forms).

In the source but not reachable by the product build at any testable size (UNREACHABLE; tests/test_stem_classes.py asserts that
the enumeration holds neither):
  * stem_s_wgrad_kernel, the flattened-point form: past 2^31 row segments, or with the X3D_STEM_WGRAD_ROWS hook of an
    X3D_EXPERIMENTS build;
  * dwt_bwd_kernel<., 8, .>: only with the X3D_DWT_BWD_VEC hook.

Found when this was written: 91 classes, 1 657 cases, 3 933 launches with the forms (tests/golden/stem_classes.json lists every class
with its case count; python -m tests.stem_classes rewrites it and prints every case of every class).  By family (T = float, f16,
bf16 unless said; cases per class):
  x3d_stem_s_fwd    stem_s_fwd_kernel<T,3,Cout>, Cout 8 / 16 / 24 / 32 (the direct kernel: fp32, W % 8 != 0, or x / y off 16 bytes)   12 x 14
                    stem_s_fwd_bf16_kernel<f16 | bf16,4,ncthw | nhwc> (matrix cores)                                                 4 x 14
  x3d_stem_s_wgrad  stem_s_wgrad_rows_kernel<T> (fp32, W % 8 != 0, or x / dy off 16 bytes; Cin 1, 2, 3)                              3 x 19
                    stem_s_wgrad_bf16_kernel<f16 | bf16,4,ncthw> (Cin 1, 2, 3) 2 x 16, <.,4,nhwc> (Cin 3)                            2 x 14
  x3d_dwt_fwd       dwt_fwd_kernel<T,VEC,KT>, KT 1 / 3 / 5 / 7: VEC 4 12 x 19, VEC 1 (Ho * Wo % 4 != 0 or an operand off its vector)    12 x 21
  x3d_dwt_bwd       dwt_bwd_kernel<T,VEC,KT>: float VEC 2 / 1, f16 and bf16 VEC 4 / 2 / 1: VEC 4 8 x 19, VEC 2 12 x 20, VEC 1         12 x 21
  x3d_stem_fwd      stem_fwd_fused_kernel<f16 | bf16,NR,train | infer>, NR 3 (Cout <= 24) 4 x 17, NR 4 (Cout 32)                     4 x 15
  x3d_stem_bwd      stem_bwd_fused_kernel<f16 | bf16,NR>: NR 3 2 x 17, NR 4                                                          2 x 15
The cases of one class, dwt_bwd_kernel<bf16,1,7> (the 2-byte buffer loads and stores; T <= 3 = KT / 2 in the first three):
  T 1, 2, 3, 4, 6, 9 at 1x8 (-> 1x4) off 1; 1x136, 1x312, 1x72, 16x8, 16x312 (8 x 156: five workgroups), 3x8 at T 1; Cout 16, 24, 32;
  1x9 (Ho * Wo = 5, odd) at off 0, 2 and 4; N = 3 at T 1, at T 2 and at T 2 on 3x136 -- each with and without relu_scale_shift.
"""
import ctypes as C
import functools
import os
from collections import namedtuple

import numpy as np

from tests import shapes as S

ENTRIES = ("x3d_stem_s_fwd", "x3d_stem_s_wgrad", "x3d_dwt_fwd", "x3d_dwt_bwd", "x3d_stem_fwd", "x3d_stem_bwd")
KTS = (1, 3, 5, 7)
TS = (1, 2, 3, 4, 6, 9)
COUTS = (8, 16, 24, 32)
CINS = (3, 1, 2)                           # 1 and 2: x3d_stem_s_wgrad only (the others require 3)
LAYOUTS = (0, 1)                           # X3D_LAYOUT_NCTHW, X3D_LAYOUT_NTHWC
WS = (8, 16, 24, 72, 136, 312, 9, 10, 11, 20)
HS = (1, 2, 3, 4, 5, 6, 7, 10, 16)           # 16 x 312 -> 8 x 156 = 1248 points: more than one workgroup at every vector width
PLANES = tuple((h, w) for h in HS for w in WS)
OFFS = (0, 1, 2, 4)                        # elements; tests/aux_checks.py _Bands(gpu, off)
# launch forms: the forward entries with a conv_t (statistics / the inference epilogue with out_act 0, 1 / neither), the
# backward entries with a conv_t (relu_scale_shift given: "masked"); x3d_stem_s_fwd / x3d_stem_s_wgrad have one form
FWD_FORMS = ("stats", "infer0", "infer1", "plain")
BWD_FORMS = ("plain", "masked")
ENTRY_FORMS = {"x3d_stem_s_fwd": (None,), "x3d_stem_s_wgrad": (None,), "x3d_dwt_fwd": FWD_FORMS, "x3d_dwt_bwd": BWD_FORMS,
               "x3d_stem_fwd": FWD_FORMS, "x3d_stem_bwd": BWD_FORMS}
FORMS = (None,) + FWD_FORMS + ("masked",)  # index = the member column

MAX_ELEMS = 1 << 19                        # no tensor of a case is larger
MAX_CASES = 24                             # per class
CLASSES_AT_LEAST = 91                      # reachable instantiations when this was written: a narrower dispatch must say so here
UNREACHABLE = ("stem_s_wgrad_kernel<", "dwt_bwd_kernel<float,8,", "dwt_bwd_kernel<f16,8,", "dwt_bwd_kernel<bf16,8,")

# one committed case: the launch (h, w: the CLIP's extents; the conv_t entries run on the conv_s output plane Ho x Wo with
# C = cout channels) and `off`, the element offset of every tensor operand
Case = namedtuple("Case", "entry dtype n cin t h w cout kt layout off form")

_BASE = 0x5000_0000_0000


def out_hw(h, w):
    return (h - 1) // 2 + 1, (w - 1) // 2 + 1


def has_conv_t(entry):
    return entry != "x3d_stem_s_fwd" and entry != "x3d_stem_s_wgrad"


def _flags(form):
    from x3d_tf_amd import hip
    return {None: 0, "plain": 0, "stats": hip.STEM_NAME_STATS, "infer0": hip.STEM_NAME_OUT_SS,
            "infer1": hip.STEM_NAME_OUT_SS | hip.STEM_NAME_OUT_RELU, "masked": hip.STEM_NAME_RELU_SS}[form]


def _operands(entry):
    """number of tensor operands x3d_stem_kernel_name reads for an entry (include/x3d_hip.h)"""
    return {"x3d_dwt_bwd": 4, "x3d_stem_bwd": 3}.get(entry, 2)


def query(case):
    """The arguments of x3d_stem_kernel_name (without out, cap) for a case over address-only operands: every tensor `off` elements
    of its own type past a 16-byte boundary."""
    from x3d_tf_amd import hip
    es = 4 if case.dtype == S.F32 else 2
    ops = [_BASE + (k << 32) + case.off * es for k in range(1, _operands(case.entry) + 1)] + [None] * (4 - _operands(case.entry))
    h, w = out_hw(case.h, case.w) if case.entry.startswith("x3d_dwt") else (case.h, case.w)
    return (case.entry.encode(), *ops, _flags(case.form), case.n, case.cin, case.t, h, w, case.cout, case.kt,
            hip.dtype_code(case.dtype), case.layout)


def dispatch(case):
    """The class (entry point, instantiation name) the dry run gives for a case; None where the library refuses the launch."""
    from x3d_tf_amd import hip
    buf = C.create_string_buffer(128)
    if hip.load().x3d_stem_kernel_name(*query(case), buf, 128) != 0:
        return None
    return (case.entry, buf.value.decode())


MEMBER_COLS = ("layout", "cin", "cout", "kt", "T", "H", "W", "off", "form")
_LAY, _CIN, _COUT, _KT, _T, _H, _W, _OFF, _FORM = range(9)


def entry_axes(entry):
    """(layouts, cins, kts, forms) of an entry's part of the domain"""
    conv_s = not entry.startswith("x3d_dwt")
    return (LAYOUTS if conv_s else (0,), (CINS if entry == "x3d_stem_s_wgrad" else (3,)) if conv_s else (0,),
            KTS if has_conv_t(entry) else (0,), ENTRY_FORMS[entry])


def walk(n=1, ts=TS):
    """{(entry point, instantiation): (storage type, members)} over the domain at N = n; the members of a class are the rows of
    an int32 array with the columns of MEMBER_COLS (the points of the domain the dry run sends to it; refused points are in no
    class)."""
    from x3d_tf_amd import hip
    name_of = hip.load().x3d_stem_kernel_name
    buf = C.create_string_buffer(128)
    found = {}
    for entry in ENTRIES:
        layouts, cins, kts, forms = entry_axes(entry)
        ent = entry.encode()
        nops = _operands(entry)
        plane = out_hw if entry.startswith("x3d_dwt") else (lambda h, w: (h, w))
        for dtype in S.DTYPES:
            es, code = (4 if dtype == S.F32 else 2), hip.dtype_code(dtype)
            for off in OFFS:
                ops = [_BASE + (k << 32) + off * es for k in range(1, nops + 1)] + [None] * (4 - nops)
                for form in forms:
                    fl, fi = _flags(form), FORMS.index(form)
                    for lay in layouts:
                        for cin in cins:
                            for cout in COUTS:
                                for kt in kts:
                                    for h, w in PLANES:
                                        ph, pw = plane(h, w)
                                        for t in ts:
                                            if name_of(ent, *ops, fl, n, cin, t, ph, pw, cout, kt, code, lay, buf, 128) == 0:
                                                found.setdefault((entry, buf.value, dtype), []).append((lay, cin, cout, kt, t, h, w, off, fi))
    out = {}
    for (entry, name, dtype), rows in found.items():
        cls = (entry, name.decode())
        assert cls not in out, f"{cls} in two storage types"
        out[cls] = (dtype, np.asarray(rows, dtype=np.int32))
    return dict(sorted(out.items()))


@functools.lru_cache(maxsize=None)
def enumerate_classes():
    """{(entry point, instantiation name): (storage type, member points)} over the domain (dry run, no GPU)."""
    return walk()


def _first(m, *keys):
    """The row of m that is smallest under the given sort keys (ties broken by the row itself: no dependence on the walk's order)."""
    order = np.lexsort(tuple(m[:, j] for j in reversed(range(m.shape[1]))) + tuple(reversed(keys)))
    return m[order[0]]


def _elems(entry, m, n=1):
    """elements of the largest tensor of each member at batch n: the clip (conv_s entries) and the conv output"""
    ho, wo = (m[:, _H] - 1) // 2 + 1, (m[:, _W] - 1) // 2 + 1
    out = n * m[:, _COUT].astype(np.int64) * m[:, _T] * ho * wo
    if entry.startswith("x3d_dwt"):
        return out
    return np.maximum(out, n * m[:, _CIN].astype(np.int64) * m[:, _T] * m[:, _H] * m[:, _W])


def class_cases(cls):
    """The committed cases of a class, chosen from its members by fixed rules (no random draws); "smallest" = fewest elements in
    its largest tensor, ties by the member's columns:
      1. the smallest member;
      2. clip lengths: entries with a conv_t -- at the smallest plane, one case for every T of TS (T <= KT / 2, T < KT, T > KT all
         occur for every KT); x3d_stem_s_fwd / x3d_stem_s_wgrad, whose T only enters the segment walk -- T = 1 and T = 3;
      3. rows: the smallest member with one, with two and with three 64-column segments per output row (W <= 128, 136, 312),
         the smallest with a ragged last segment (W = 72), the member with the most rows at the smallest W and the one with
         the most output points (several workgroups of the plane-wise kernels; the last one partly past the plane), and the
         smallest with an odd H of three rows or more (several output rows, the last one reading the bottom pad);
      4. the smallest member at every Cout, every Cin and every layout the class admits (a template argument fixes some);
      5. the smallest member at each operand offset the class admits (0 too: a class whose smallest member sits at an offset);
      6. N = 3 (odd; N never changes the class) on the smallest member, on the smallest member with T > 1 and on the smallest with
         T > 1, three rows or more and two segments per row (the (n, t, row, segment) walk of the segment kernels with every
         extent above 1).
    Every case runs in every launch form of its entry that keeps it in the class (case_forms), so the forms add launches, not
    cases; the cases themselves are taken at the class's first form.  No tensor of a case exceeds MAX_ELEMS elements."""
    dtype, m = enumerate_classes()[cls]
    entry = cls[0]
    m = m[m[:, _FORM] == m[:, _FORM].min()]
    el = _elems(entry, m)
    ok = el <= MAX_ELEMS
    assert ok.any(), f"{cls}: no member under {MAX_ELEMS} elements"
    m, el = m[ok], el[ok]

    def case(row, n=1):
        return Case(entry, dtype, n, int(row[_CIN]), int(row[_T]), int(row[_H]), int(row[_W]), int(row[_COUT]), int(row[_KT]),
                    int(row[_LAY]), int(row[_OFF]), FORMS[int(row[_FORM])])

    def smallest(sel):
        return _first(m[sel], el[sel])

    rows = [smallest(np.ones(len(m), bool))]                                                   # 1
    base = rows[0]
    same = np.ones(len(m), bool)
    for j in (_LAY, _CIN, _COUT, _KT, _H, _W, _OFF):
        same &= m[:, j] == base[j]
    for t in (TS if has_conv_t(entry) else (1, 3)):                                            # 2
        sel = same & (m[:, _T] == t)
        if not sel.any():
            sel = m[:, _T] == t
        if sel.any():
            rows.append(smallest(sel))
    nws = ((m[:, _W] - 1) // 2 + 1 + 63) // 64
    for k in (1, 2, 3):                                                                        # 3
        if (nws == k).any():
            rows.append(smallest(nws == k))
    if (m[:, _W] == 72).any():
        rows.append(smallest(m[:, _W] == 72))
    wmin = m[:, _W] == m[:, _W].min()
    rows.append(_first(m[wmin], -m[wmin][:, _H], el[wmin]))
    pts = ((m[:, _H] - 1) // 2 + 1) * ((m[:, _W] - 1) // 2 + 1)
    rows.append(_first(m, -pts, el))
    odd = (m[:, _H] >= 3) & (m[:, _H] % 2 == 1)
    if odd.any():
        rows.append(smallest(odd))
    for j in (_COUT, _CIN, _LAY):                                                              # 4
        for v in sorted(set(m[:, j].tolist())):
            rows.append(smallest(m[:, j] == v))
    for off in sorted(set(m[:, _OFF].tolist())):                                               # 5
        rows.append(smallest(m[:, _OFF] == off))
    cases = []
    for r in rows:
        if case(r) not in cases:
            cases.append(case(r))
    ok3 = _elems(entry, m, 3) <= MAX_ELEMS                                                     # 6
    cases.append(case(_first(m[ok3], el[ok3]), 3))
    long = ok3 & (m[:, _T] > 1)
    if long.any():
        cases.append(case(_first(m[long], el[long]), 3))
    wide = long & (m[:, _H] >= 3) & (nws >= 2)
    if wide.any():
        cases.append(case(_first(m[wide], el[wide]), 3))
    assert 1 <= len(cases) <= MAX_CASES, (cls, len(cases))
    return cases


def case_forms(case, cls):
    """The launch forms the runner takes a case through: every form of its entry in which the same launch dispatches to the
    same class (its own first)."""
    return tuple(f for f in ENTRY_FORMS[case.entry] if f == case.form or dispatch(case._replace(form=f)) == cls)


def case_id(c):
    lay = "" if c.entry.startswith("x3d_dwt") else ("-nthwc" if c.layout else "-ncthw")
    return (f"{str(c.dtype)[6:]}-N{c.n}-T{c.t}-{c.h}x{c.w}" + (f"-ci{c.cin}" if c.cin not in (0, 3) else "") + f"-co{c.cout}"
            + (f"-kt{c.kt}" if c.kt else "") + lay + (f"-{c.form}" if c.form else "") + (f"-off{c.off}" if c.off else ""))


def class_id(cls):
    return f"{cls[0][4:]}:{cls[1]}"


# ---- the stem launches of a recorded plan ------------------------------------------------------------------------------------
_INPUT_ARG = {"x3d_stem_s_fwd": 0, "x3d_stem_s_wgrad": 0, "x3d_stem_fwd": 0, "x3d_stem_bwd": 4}


def plan_stem_classes(pl):
    """[(entry point, instantiation, its recorded arguments)] of every stem launch of a recorded plan (dry or real), named by
    the dry-run dispatch over the recorded argument tuples.  A plan that reads the caller's batch in place records no address
    for it until a batch is bound (model._bind_input, which hands over a 16-byte-aligned one): an aligned placeholder here."""
    from x3d_tf_amd import hip
    out = []
    for lst in (pl.fwd, pl.bwd):
        for item in lst:
            if item is None or item[0] not in ENTRIES:
                continue
            name, args = item[0], list(item[2])
            k = _INPUT_ARG.get(name)
            if k is not None and not args[k]:
                assert pl.x_cl, f"{name}: no input address in a plan with a planar batch"
                args[k] = _BASE
            out.append((name, hip.stem_kernel_name(name, *args), tuple(args)))
    return out


# ---- the committed list (tests/golden/stem_classes.json): names and counts only ----------------------------------------------
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "stem_classes.json")


def golden():
    """What tests/golden/stem_classes.json must hold: the sorted classes, each with its number of committed cases."""
    classes = enumerate_classes()
    return {"count": len(classes), "cases": sum(len(class_cases(c)) for c in classes),
            "classes": [[c[0], c[1], len(class_cases(c))] for c in sorted(classes)]}


if __name__ == "__main__":          # python -m tests.stem_classes: rewrite the list after a deliberate change of the dispatch
    import json
    g = golden()
    with open(GOLDEN, "w") as f:        # one class per line
        f.write('{"count": %d, "cases": %d, "classes": [\n' % (g["count"], g["cases"]))
        f.write(",\n".join(json.dumps(c) for c in g["classes"]) + "\n]}\n")
    for cls in enumerate_classes():
        print(class_id(cls) + ": " + " ".join(case_id(c) for c in class_cases(cls)))
    print(f"{GOLDEN}: {g['count']} classes, {g['cases']} cases")
