"""Every kernel instantiation x3d_dw3d_fwd / x3d_dw3d_bwd can dispatch, as data, and the committed parity cases of each.

tests/shapes.py lists the depthwise parity cases plane by plane (DW, DW_FULL) and tests/fuzz.py draws random ones; which
instantiations they reach is an accident of the lists.  This module looks from the other side, as tests/pw_bwd_classes.py does
for the fused pointwise backward: it walks a domain of launches through the library's dry-run dispatch
(x3d_dw3d_kernel_name: no GPU, nothing launched) and returns every (entry point, instantiation) it meets -- a CLASS -- with the
points of the domain that dispatch to it.  class_cases() then picks the committed cases of a class from its own members by
fixed rules, so nothing is drawn and nothing is declined.  tests/test_dw_classes.py (CPU) checks the enumeration,
tests/test_dw_classes_gpu.py runs every class against fp64 (tests/dw_checks.py).

The domain: the three storage types, stride 1 / 2, T in TS, planes of H in 3 .. 180 rows with W in {H, H - 3, H // 2 + 2} (and
the planes and clip lengths of the registered lists and of the fuzz slice, so that what those dispatch is inside),
every tensor operand OFFS elements off its 16-byte-aligned allocation (the dispatch reads the alignment of x / y, of araw / ga
and of dv / braw), the backward and the forward with its prologue given as a scale / shift table ("ss") or as a folded BatchNorm
finalize ("bn": x3d_bn_fold; the matrix-core and packed forward kernels decline it).

What the dispatch does NOT read, found by asking it over the whole domain (tests/test_dw_classes.py keeps asking):
  * N and C (both entry points): the walk runs at (N, C) = (1, 2), the cases also take (3, 5) and (16, 2) -- the packed and
    grouped kernels put several planes in a wave;
  * the forward without a prologue (in_scale_shift = NULL, in_act = 0): the same name as the "ss" form everywhere;
  * statistics / pool given or absent: the same name everywhere.
So the forward's launch form is one dimension of two values here, and every forward case is launched in each of the two that
keeps it in its class (case_forms); the runner also launches the no-prologue, no-sums form next to the "ss" form (as
test_dw3d_fwd does), on the same instantiation.
"""
import ctypes as C
import functools
import os
from collections import namedtuple

import numpy as np

from tests import shapes as S

SWEEP_TS = (1, 2, 3, 4, 5, 6, 7, 8, 13, 16)   # the time loops are unrolled by 6, ring depths are 3 / 4, T below the prefetch depth
NCS = ((1, 2), (3, 5), (16, 2))
HS = tuple(range(3, 181))
OFFS = (0, 1, 2, 4)                        # elements; tests/aux_checks.py _Bands(gpu, off)
FORMS = ("bwd", "ss", "bn")                # x3d_dw3d_bwd; x3d_dw3d_fwd with a scale / shift table; ... with the folded BatchNorm
STRIDES = (1, 2)


def listed_shapes():
    """(T, H, W) of every depthwise case of the registered lists (shapes.DW, shapes.DW_FULL) and of the seeded fuzz slice
    (tests/fuzz.py slice_calls): the walk takes their planes and clip lengths in, so the enumeration holds what they dispatch."""
    from tests import fuzz
    got = {(t, h, w) for _, _, t, h, w, _ in S.DW} | {(c[4], c[5], c[6]) for c in S.DW_FULL}
    return got | {(a[1][2], a[1][3], a[1][4]) for _, fn, a in fuzz.slice_calls() if fn == "test_dw3d_fwd"}


_LISTED = listed_shapes()
TS = tuple(sorted(set(SWEEP_TS) | {t for t, _, _ in _LISTED}))
PLANES = tuple(sorted({(h, w) for h in HS for w in (h, h - 3, h // 2 + 2) if w >= 1} | {(h, w) for _, h, w in _LISTED}))

MAX_ELEMS = 1 << 21                        # no tensor of a case is larger
MAX_CASES = 16                             # per class
CLASSES_AT_LEAST = 250                     # reachable instantiations when this was written: a narrower dispatch must say so here

# one committed case: the launch (entry "fwd" / "bwd"; pro "ss" / "bn" for the forward, None for the backward) and `off`, the
# element offset of every tensor operand
Case = namedtuple("Case", "entry dtype n c t h w stride off pro")

_BASE = 0x5000_0000_0000


def _addr(k, off, elem_bytes):
    return _BASE + (k << 32) + off * elem_bytes


def case_struct(case):
    """The argument struct of a case over address-only operands: every tensor `off` elements of its own type past a 16-byte
    boundary (the forward in the launch form of S.dw_full_struct, the backward in that of S.dw_bwd_struct)."""
    from x3d_tf_amd import hip
    es = 4 if case.dtype == S.F32 else 2
    a = lambda k, e: _addr(k, case.off, e)
    code = hip.dtype_code(case.dtype)
    if case.entry == "bwd":
        return hip.Dw3dBwdArgs(a(1, es), a(2, es), a(3, 4), a(4, es), a(5, 4), a(6, 4), a(7, es), a(8, 8), a(9, 4),
                               case.n, case.c, case.t, case.h, case.w, case.stride, code)
    fold = hip.BnFold(a(10, 8), 1.0, a(11, 4), a(12, 4), a(13, 4), a(14, 4), 1e-5, 0.9, 1, a(15, 4), a(16, 4)) if case.pro == "bn" else None
    st = hip.Dw3dFwdArgs(a(1, es), a(2, 4), a(3, es), None if fold else a(4, 4), 1, a(5, 8), a(6, 8), case.n, case.c, case.t,
                         case.h, case.w, case.stride, code, None if fold is None else C.pointer(fold))
    st._fold = fold            # (the struct holds a raw pointer to it)
    return st


def dispatch(case):
    """The class (entry point, instantiation name) the dry run gives for a case; None where the library refuses the launch."""
    from x3d_tf_amd import hip
    st = case_struct(case)
    buf = C.create_string_buffer(128)
    fwd, bwd = (C.byref(st), None) if case.entry == "fwd" else (None, C.byref(st))
    if hip.load().x3d_dw3d_kernel_name(fwd, bwd, buf, 128) != 0:
        return None
    return ("x3d_dw3d_" + case.entry, buf.value.decode())


def walk(n=1, c=2, ts=TS):
    """(ids, names): ids[dtype, stride, plane, off, T, form] = index into `names` of the instantiation the dry run selects at that
    point of the domain for N = n, C = c (-1: the library refuses the launch), names = [(entry point, instantiation), ...] in
    the order met."""
    from x3d_tf_amd import hip
    lib = hip.load()
    name_of = lib.x3d_dw3d_kernel_name
    buf = C.create_string_buffer(128)
    ids = np.full((len(S.DTYPES), len(STRIDES), len(PLANES), len(OFFS), len(ts), len(FORMS)), -1, dtype=np.int16)
    index = {}
    for di, dtype in enumerate(S.DTYPES):
        for oi, off in enumerate(OFFS):
            for fi, form in enumerate(FORMS):
                entry = "bwd" if form == "bwd" else "fwd"
                # one struct per storage type, offset and form; only the extents change along the walk
                st = case_struct(Case(entry, dtype, n, c, 1, 3, 3, 1, off, None if form == "bwd" else form))
                ref = C.byref(st)
                args = (ref, None, buf, 128) if entry == "fwd" else (None, ref, buf, 128)
                full = "x3d_dw3d_" + entry
                for si, stride in enumerate(STRIDES):
                    st.stride = stride
                    for pi, (h, w) in enumerate(PLANES):
                        st.H, st.W = h, w
                        row = ids[di, si, pi, oi]
                        for ti, t in enumerate(ts):
                            st.T = t
                            if name_of(*args) == 0:
                                key = (full, buf.value)
                                k = index.get(key)
                                if k is None:
                                    k = index[key] = len(index)
                                row[ti, fi] = k
    return ids, [(e, b.decode()) for e, b in index]


@functools.lru_cache(maxsize=None)
def enumerate_classes():
    """{(entry point, instantiation name): member points} over the domain (dry run, no GPU).  The member points of a class
    are the rows of an int32 array with the columns of MEMBER_COLS; its storage type is in its name."""
    ids, names = walk()
    out = {}
    for k, cls in enumerate(names):
        di, si, pi, oi, ti, fi = np.nonzero(ids == k)
        assert len(set(di.tolist())) == 1, cls
        planes = np.asarray(PLANES, dtype=np.int32)[pi]
        m = np.stack([np.asarray(STRIDES, dtype=np.int32)[si], np.asarray(TS, dtype=np.int32)[ti], planes[:, 0], planes[:, 1],
                      np.asarray(OFFS, dtype=np.int32)[oi], fi.astype(np.int32)], 1)
        out[cls] = (S.DTYPES[int(di[0])], m)
    return dict(sorted(out.items()))


MEMBER_COLS = ("stride", "T", "H", "W", "off", "form")
_STRIDE, _T, _H, _W, _OFF, _FORM = range(6)


def _first(m, *keys):
    """The row of m that is smallest under the given sort keys (arrays over the rows; ties broken by the row itself, so the
    choice does not depend on the walk's order)."""
    order = np.lexsort(tuple(m[:, j] for j in reversed(range(m.shape[1]))) + tuple(reversed(keys)))
    return m[order[0]]


def _volume(m):
    return m[:, _T].astype(np.int64) * m[:, _H] * m[:, _W]


def class_cases(cls):
    """The committed cases of a class, chosen from its members by fixed rules (no random draws):
      1. the member of smallest volume;
      2. the members of smallest and of largest W and the one with the most rows, at the smallest T the class admits;
      3. at the smallest plane, one case for every T of the domain the class admits (a T the class only takes on larger planes:
         on the smallest plane that has it);
      4. the smallest member with (N, C) = (3, 5) and with (16, 2): N and C never change the class, so every class has them;
      5. the smallest member at each non-zero operand offset the class admits;
      6. the forward's folded-BatchNorm form: every case runs in both prologue forms where both stay in the class
         (case_forms); a class whose cases never meet the fold gets its smallest "bn" member too.
    Rules 1 - 3 and 5 run at (N, C) = (1, 2).  No tensor of a case exceeds MAX_ELEMS elements (a rule whose member would: the
    largest member under the cap, by the rule's own order); at most MAX_CASES cases -- where the rules give more, rule 4's
    (N, C) move onto the first cases of rule 5 or, in a class with no offset member, of rule 3 instead of adding cases."""
    dtype, m = enumerate_classes()[cls]
    entry = cls[0][len("x3d_dw3d_"):]
    vol = _volume(m)

    def case(row, nc=(1, 2)):
        form = FORMS[int(row[_FORM])]
        return Case(entry, dtype, nc[0], nc[1], int(row[_T]), int(row[_H]), int(row[_W]), int(row[_STRIDE]), int(row[_OFF]),
                    None if form == "bwd" else form)

    def fits(nc):
        return vol * (nc[0] * nc[1]) <= MAX_ELEMS

    base = fits(NCS[0])
    assert base.any(), f"{cls}: no member under {MAX_ELEMS} elements"
    mb, vb = m[base], vol[base]
    rows = [_first(mb, vb)]                                                     # 1
    tmin = mb[:, _T].min()
    at = mb[mb[:, _T] == tmin]
    rows += [_first(at, at[:, _W], at[:, _H]), _first(at, -at[:, _W], at[:, _H]), _first(at, -at[:, _H], at[:, _W])]   # 2
    plane = mb[:, _H].astype(np.int64) * mb[:, _W]
    sweep = []
    admitted = sorted(set(mb[:, _T].tolist()))
    for t in [t for t in admitted if t in SWEEP_TS] or admitted:                 # 3 (SWEEP_TS; a clip length only the lists have: if no other)
        sel = mb[:, _T] == t
        sweep.append(_first(mb[sel], plane[sel], mb[sel][:, _OFF]))
    offs = []
    for off in sorted(set(mb[:, _OFF].tolist()) - {0}):                          # 5
        sel = mb[:, _OFF] == off
        offs.append(_first(mb[sel], vb[sel]))
    cases = []
    for r in rows + sweep + offs:
        if case(r) not in cases:
            cases.append(case(r))
    extra = []
    for nc in NCS[1:]:                                                           # 4
        ok = fits(nc)
        assert ok.any(), f"{cls}: no member under {MAX_ELEMS} elements at (N, C) = {nc}"
        extra.append(case(_first(m[ok], vol[ok]), nc))
    if len(cases) + len(extra) > MAX_CASES:
        # (N, C) onto existing cases: the offset cases first, then the T sweep from its far end; each stays under the cap
        pool = [case(r) for r in offs] + [case(r) for r in reversed(sweep)]
        for nc in NCS[1:]:
            for cand in pool:
                if cand in cases and cand.n == 1 and cand.t * cand.h * cand.w * nc[0] * nc[1] <= MAX_ELEMS:
                    cases[cases.index(cand)] = cand._replace(n=nc[0], c=nc[1])
                    break
            else:
                raise AssertionError(f"{cls}: no case can carry (N, C) = {nc}")
    else:
        cases += [e for e in extra if e not in cases]
    # 6: the folded-BatchNorm form.  The runner launches every forward case in every form that keeps it in the class
    # (case_forms); a class that meets the fold only at other points than its cases gets its smallest "bn" member as well
    bn = m[:, _FORM] == FORMS.index("bn")
    if bn.any() and not any("bn" in case_forms(c, cls) for c in cases):
        ok = bn & base
        assert ok.any(), f"{cls}: no folded-BatchNorm member under {MAX_ELEMS} elements"
        cases.append(case(_first(m[ok], vol[ok])))
    assert 1 <= len(cases) <= MAX_CASES, (cls, len(cases))
    return cases


def case_forms(case, cls):
    """The launch forms the runner takes a case through: its own, and for a forward case the other prologue form ("ss" / "bn")
    where the same launch in that form dispatches to the same class."""
    if case.entry == "bwd":
        return (None,)
    other = "bn" if case.pro == "ss" else "ss"
    return (case.pro, other) if dispatch(case._replace(pro=other)) == cls else (case.pro,)


def case_id(case):
    form = "" if case.pro is None else f"-{case.pro}"
    return (f"{case.entry}-{str(case.dtype)[6:]}-N{case.n}-C{case.c}-T{case.t}-{case.h}x{case.w}-s{case.stride}{form}"
            + (f"-off{case.off}" if case.off else ""))


def class_id(cls):
    return f"{cls[0][4:]}:{cls[1]}"


# ---- what else dispatches depthwise kernels: the registered lists, the fuzz slice, the dry plans ------------------------------
def registered_names():
    """{class: first registered kernel-level case that runs it} over shapes.DW and shapes.DW_FULL, all three storage types."""
    from x3d_tf_amd import hip
    got = {}
    for dt in S.DTYPES:
        for shp in S.DW:
            got.setdefault(("x3d_dw3d_fwd", hip.kernel_name(S.dw_fwd_struct(shp, dt))), f"DW {shp} {dt}")
            got.setdefault(("x3d_dw3d_bwd", hip.kernel_name(S.dw_bwd_struct(shp, dt))), f"DW {shp} {dt}")
    for full in S.DW_FULL:
        for dt in S.DTYPES:
            c = (full[0], dt) + tuple(full[2:])
            got.setdefault(("x3d_dw3d_" + c[0], hip.kernel_name(S.dw_full_struct(c))), f"DW_FULL {S.dw_full_id(c)}")
    return got


def fuzz_slice_names():
    """{class: first case} over the depthwise calls of the seeded fuzz slice (tests/fuzz.py slice_calls), all three storage types."""
    from tests import fuzz
    from x3d_tf_amd import hip
    got = {}
    for seed, fn, args in fuzz.slice_calls():
        if fn in ("test_dw3d_fwd", "test_dw3d_bwd"):
            for dt in S.DTYPES:
                st = (S.dw_fwd_struct if fn == "test_dw3d_fwd" else S.dw_bwd_struct)(args[1], dt)
                got.setdefault(("x3d_" + fn[5:], hip.kernel_name(st)), f"fuzz seed {seed}: {args[1]} {dt}")
    return got


# ---- the committed list (tests/golden/dw_classes.json): names and counts only ------------------------------------------------
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "dw_classes.json")


def golden():
    """What tests/golden/dw_classes.json must hold: the sorted classes, each with its number of committed cases."""
    classes = enumerate_classes()
    return {"count": len(classes), "cases": sum(len(class_cases(c)) for c in classes),
            "classes": [[c[0], c[1], len(class_cases(c))] for c in sorted(classes)]}


if __name__ == "__main__":          # python -m tests.dw_classes: rewrite the list after a deliberate change of the dispatch
    import json
    g = golden()
    with open(GOLDEN, "w") as f:        # one class per line
        f.write('{"count": %d, "cases": %d, "classes": [\n' % (g["count"], g["cases"]))
        f.write(",\n".join(json.dumps(c) for c in g["classes"]) + "\n]}\n")
    print(f"{GOLDEN}: {golden()['count']} classes, {golden()['cases']} cases")
