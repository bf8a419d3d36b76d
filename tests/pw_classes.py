"""Every kernel instantiation x3d_pw_fwd / x3d_pw_dgrad / x3d_pw_wgrad can dispatch, as data, and the committed parity cases
of each.

tests/shapes.py lists the pointwise parity cases layer by layer from the shipped configurations and tests/fuzz.py draws random
ones; which instantiations they reach is an accident of the lists.  This module looks from the other side, as
tests/pw_bwd_classes.py does for the fused backward and tests/dw_classes.py for the depthwise entry points: it walks a domain of
launches through the library's dry-run dispatch (x3d_pw_kernel_name: no GPU, nothing launched) and returns every
(entry point, instantiation name) it meets -- a CLASS -- with the parameter boxes that dispatch to it.  class_cases() then picks
the committed cases of a class from its boxes by FIXED RULES (deterministic, as tests/dw_classes.py; nothing is drawn), every one
re-checked against the dry run.  tests/test_pw_classes.py (CPU) checks the enumeration and the cases,
tests/test_pw_classes_gpu.py runs the kernel tests of tests/test_kernels_gpu.py on them.

The launch forms (FORMS), built with the struct builders of tests/shapes.py:
  fwd        S.pw_fwd_struct, stride 1       prologue None / "relu" / "swish"
  fwd_s2     S.pw_fwd_struct, stride 2       None
  fwd_tail   S.pw_fwd_struct                 "tail" / "tail_conv" / "tail1"
  fwd_infer  S.pw_fwd_infer_struct           (prologue, residual None / "identity" / "conv", out_act None / "relu")
  dgrad      S.pw_dgrad_struct               S.PW_DGRAD_EPI
  wgrad      S.pw_wgrad_struct               (stride, prologue): (1, None), (1, "swish"), (2, None)
each in the three storage types, fwd* and dgrad in the 16-bit types with and without the weight panel.

The walk knows nothing of the dispatch rules.  Per form, storage type and plane it asks the dry run on a (Cin, Cout) grid in two
levels: first at every multiple of 16 up to 640 (X3D-XL's 630) and at every width of the registered lists and the fuzz slice;
then, between every two neighbours across which any answer of that matrix changes, at both neighbours of every multiple of 16
(and 32) and at the multiples of 8 in between.  (That refinement is an assumption about the dispatch: a class confined to
channel counts strictly between two level-1 neighbours whose answers agree would be missed -- as one strictly between two
values of any grid would.  A flat walk of both full axes -- 165 values each, ten times the calls, 216 s -- found the same 676 classes when this was written.)
The channel axes are cut wherever an answer changes; a box is one cell.  The
planes (PLANES / PLANES_S2) hold P % 8 == 0, P % 8 != 0 (odd and even, P >= 8), P < 8, P < 16, both sides of a 32-, 64- and
128-point tile boundary, whole 256-point tiles, 13-frame planes, and for stride 2 input rows of every gather group with
P % 8 == 0 and not.  The channel counts of the registered lists (PW_FWD, PW_FWD_XL, PW_FWD_TAIL, PW_FWD_INFER, PW_DGRAD,
PW_WGRAD) and of the pointwise calls of the fuzz slice are on the grid, and a listed shape whose class the grid walk did not meet
on its own planes comes in as a single-point box, so the enumeration holds what they dispatch (today the walk meets them all;
what the full-size lists PW_FULL / PW_F32_FULL and the shipped configurations dispatch is checked by tests/test_pw_classes.py).
The A/B environment switches of the library are not read or set: the enumeration describes the product's dispatch.

What the dispatch does NOT read inside this domain, found by asking it (tests/test_pw_classes.py keeps asking, on every box):
  * N (the walk runs at N = 2; the cases take 2, 3 and 5);
  * T and H beyond the point count: (T, H, W) and (T * Ho, 1, W) give the same name (W stays: the strided gather and the
    strided-add epilogue read the row length).
Outside it two rules do read N: the weights-streamed kernel is taken up to 1024 128-point tiles (N ceil(P / 128): past the size
budget here), and pw_f32p / pw_wgrad_f32p hand tensors of about 2 GB over to pw_f32r_kernel<4, 2, 4, 0, 100> and
pw_wgrad_f32r_kernel<2, 1, 0>.  Those two instantiations exist only at that size; they stay with
test_pw_f32_past_buffer_offsets_fp64 (shapes.PW_F32_FULL) and are excluded here BY NAME (FULL_SIZE_ONLY), not by a size rule that
could hide others.  The weights-stationary kernels' runs of several tiles per workgroup need more tiles than CUs x occupancy:
that regime stays with tests/test_full_size_gpu.py and is out of scope here.

The scalar kernels (VEC = 1 in their names) take aligned launches only below 8 points (16-bit) per sample; planes of several
tiles reach them through operands that are off their 16-byte alignment, and that is how class_cases() runs them (rule 4).  32
classes are left that no launch above 3 points per sample reaches, aligned or not: the generic fp32 kernels of stride 1,
pw_gemm_kernel<float, 1, ., ., ., ., 0> (24) and pw_wgrad_kernel<float, 1, ., ., 0> (8), which the dispatch takes below 4 points
only (pw_f32r / pw_wgrad_f32r take everything from 4 points on).  Their cases are on the plane of 3 points.

Measured when this was written (CPU, dry run): 676 classes; 244 of them had no case in the registered lists, the fuzz slice or
shapes.PW_FULL (the number a coarser walk put at 228 of 646), see test_pw_classes.py::test_gap_report.
"""
import ctypes as C
import functools
import os
import re
from collections import namedtuple

import numpy as np

from tests import shapes as S

_PROS = (None, "relu", "swish")
FORMS = ([("fwd", p) for p in _PROS] + [("fwd_s2", None)] + [("fwd_tail", t) for t in ("tail", "tail_conv", "tail1")]
         + [("fwd_infer", (p, r, o)) for p in _PROS for r in (None, "identity", "conv") for o in (None, "relu")]
         + [("dgrad", e) for e in S.PW_DGRAD_EPI] + [("wgrad", v) for v in ((1, None), (1, "swish"), (2, None))])
ENTRY = {"fwd": "x3d_pw_fwd", "fwd_s2": "x3d_pw_fwd", "fwd_tail": "x3d_pw_fwd", "fwd_infer": "x3d_pw_fwd", "dgrad": "x3d_pw_dgrad",
         "wgrad": "x3d_pw_wgrad"}

# (T, H, W), stride 1: P = 3, 8, 12, 25, 34, 66, 98, 128, 129, 130, 256, 392, 325, 1300
PLANES = ((1, 1, 3), (1, 2, 4), (1, 3, 4), (1, 5, 5), (1, 2, 17), (1, 33, 2), (2, 7, 7), (2, 8, 8), (1, 3, 43), (2, 5, 13), (4, 8, 8),
          (8, 7, 7), (13, 5, 5), (13, 10, 10))
# input planes of the strided forms: rows of 8 k (gather groups of 4), 4 k (2), 4 k + 2 and odd (1), 7 and 3 (one group wide), each
# with P = T Ho Wo a multiple of 8 and not; the shortcut planes 28 -> 14, 39 -> 20, 20 -> 10, an odd row of 23, 256 whole points
PLANES_S2 = ((1, 4, 8), (1, 6, 8), (2, 4, 16), (1, 5, 16), (4, 2, 12), (1, 6, 12), (8, 2, 14), (1, 6, 14), (8, 3, 13), (1, 5, 13), (2, 7, 7),
             (1, 5, 7), (4, 3, 3), (3, 3, 3), (1, 5, 3), (2, 28, 28), (1, 39, 39), (1, 20, 20), (2, 11, 23), (4, 16, 16), (1, 32, 31),   # (... and an odd row: 31 -> 16)
             # ragged planes of more than 128 points in every gather group: P = 132, 130, 133, 154, 132, 134
             (1, 65, 8), (1, 26, 20), (1, 38, 14), (1, 21, 27), (1, 66, 7), (1, 134, 3))
CMAX = 640
WALK_N = 2

MAX_ELEMS = 1 << 21          # no tensor of a case is larger
MAX_POINTS = 3500            # per sample, as pw_bwd_classes.MAX_POINTS
CLASSES_AT_LEAST = 676       # reachable instantiations when this was written (a coarser walk: 646): a narrower dispatch must say so here
# instantiations that exist only where a tensor reaches 2 GB (shapes.PW_F32_FULL, test_pw_f32_past_buffer_offsets_fp64)
FULL_SIZE_ONLY = (("x3d_pw_fwd", "pw_f32r_kernel<4, 2, 4, 0, 100>"), ("x3d_pw_wgrad", "pw_wgrad_f32r_kernel<2, 1, 0>"))

# one box of a class: launch form and its value, storage type, weight panel, inclusive channel ranges, the planes seen to keep it
Box = namedtuple("Box", "form val dtype panel cin cout planes")
# one committed case; off: every activation operand `off` elements past its 16-byte-aligned allocation
Case = namedtuple("Case", "form val dtype panel n cin cout t h w off")

# the activation operands of each argument struct (the offset of a case moves these addresses)
_ACT_FIELDS = {"x3d_pw_fwd": ("x", "y", "in_add", "in_store", "out_add"), "x3d_pw_dgrad": ("g", "yraw", "dx", "braw", "add"),
               "x3d_pw_wgrad": ("g", "yraw", "x")}


def stride_of(form, val):
    return 2 if form == "fwd_s2" else (val[0] if form == "wgrad" else 1)


def case_shape(case):
    """The shape tuple the kernel tests and the struct builders take."""
    head = (case.n, case.cin, case.cout, case.t, case.h, case.w)
    if case.form in ("fwd", "fwd_s2", "fwd_tail"):
        return head + (stride_of(case.form, case.val), case.val)
    if case.form == "fwd_infer":
        return head + tuple(case.val)
    if case.form == "dgrad":
        return head
    return head + tuple(case.val)


def case_struct(case):
    """The argument struct of a case over address-only operands, from the builders of tests/shapes.py; with case.off every
    activation operand's address is moved by that many elements (as dw_classes._addr does)."""
    shape = case_shape(case)
    if case.form in ("fwd", "fwd_s2", "fwd_tail"):
        st = S.pw_fwd_struct(shape, case.dtype, case.panel)
    elif case.form == "fwd_infer":
        st = S.pw_fwd_infer_struct(shape, case.dtype, case.panel)
    elif case.form == "dgrad":
        st = S.pw_dgrad_struct(shape, case.val, case.dtype, case.panel)
    else:
        st = S.pw_wgrad_struct(shape, case.dtype)
    if case.off:
        es = 4 if case.dtype == S.F32 else 2
        for f in _ACT_FIELDS[ENTRY[case.form]]:
            if getattr(st, f):
                setattr(st, f, getattr(st, f) + case.off * es)
    return st


def _slots(form, ref):
    return {"x3d_pw_fwd": (ref, None, None, None), "x3d_pw_dgrad": (None, ref, None, None), "x3d_pw_wgrad": (None, None, ref, None)}[ENTRY[form]]


def dispatch(case):
    """The class (entry point, instantiation name) the dry run gives for a case; None where the library refuses the launch."""
    from x3d_tf_amd import hip
    st = case_struct(case)
    buf = C.create_string_buffer(160)
    if hip.load().x3d_pw_kernel_name(*_slots(case.form, C.byref(st)), buf, 160) != 0:
        return None
    return (ENTRY[case.form], buf.value.decode())


def points(case):
    s = stride_of(case.form, case.val)
    return case.t * (-(-case.h // s)) * (-(-case.w // s))


def _plane_points(form, val, plane):
    s = stride_of(form, val)
    return plane[0] * (-(-plane[1] // s)) * (-(-plane[2] // s))


# ---- the registered lists, the fuzz slice, the full-size plans -----------------------------------------------------------------
def listed_cases():
    """[(Case, where)] of every registered kernel-level case of the three entry points (as tests/test_dispatch_coverage.py
    _kernel_case_names reads the lists) and of the pointwise calls of the seeded fuzz slice, in every storage type."""
    from tests import fuzz
    out = []

    def add(form, val, dt, panel, shp, what):
        n, ci, co, t, h, w = shp[:6]
        out.append((Case(form, val, dt, panel, n, ci, co, t, h, w, 0), what))

    for dt in S.DTYPES:
        panels = (False, True) if dt != S.F32 else (False,)
        for panel in panels:
            for shp in S.PW_FWD + S.PW_FWD_XL:
                add("fwd" if shp[6] == 1 else "fwd_s2", shp[7], dt, panel, shp, f"test_pw_fwd[{shp}]")
            for shp in S.PW_FWD_TAIL:
                add("fwd_tail", shp[7], dt, panel, shp, f"test_pw_fwd_tail[{shp}]")
            for shp in S.PW_FWD_INFER:
                add("fwd_infer", tuple(shp[6:]), dt, panel, shp, f"test_pw_fwd_infer[{shp}]")
            for shp in S.PW_DGRAD:
                for epi in S.PW_DGRAD_EPI:
                    add("dgrad", epi, dt, panel, shp, f"test_pw_dgrad[{shp}, {epi}]")
        for shp in S.PW_WGRAD:
            add("wgrad", (shp[6], shp[7]), dt, False, shp, f"test_pw_wgrad[{shp}]")
    for seed, fn, args in fuzz.slice_calls():
        # (the slice runs a call in the one storage type its seed drew: only that one counts as covered)
        if fn == "test_pw_fwd":
            dt, shp, panel = args
            add("fwd" if shp[6] == 1 else "fwd_s2", shp[7], dt, bool(panel), shp, f"fuzz seed {seed}: test_pw_fwd{shp}")
        elif fn == "test_pw_dgrad":
            dt, shp, epi, panel = args
            add("dgrad", epi, dt, bool(panel), shp, f"fuzz seed {seed}: test_pw_dgrad{shp} {epi}")
        elif fn == "test_pw_wgrad":
            dt, shp = args
            add("wgrad", (shp[6], shp[7]), dt, False, shp, f"fuzz seed {seed}: test_pw_wgrad{shp}")
    return out


def listed_names():
    """{class: first registered or fuzz-slice case that runs it}; a case the library refuses (a tail form in fp32 it does not
    cover) has no class."""
    got = {}
    for case, what in listed_cases():
        cls = dispatch(case)
        if cls is not None:
            got.setdefault(cls, f"{what} {case.dtype}{' panel' if case.panel else ''}")
    return got


def full_size_names():
    """{class: first case} over the non-`bwd` rows of shapes.PW_FULL and over shapes.PW_F32_FULL."""
    from x3d_tf_amd import hip
    ent = {"fwd": "x3d_pw_fwd", "dgrad": "x3d_pw_dgrad", "wgrad": "x3d_pw_wgrad"}
    got = {}
    for c in S.PW_FULL:
        if c[0] != "bwd":
            got.setdefault((ent[c[0]], hip.kernel_name(S.pw_full_struct(c))), f"PW_FULL {S.pw_full_id(c)}")
    for c in S.PW_F32_FULL:
        got.setdefault((ent[c[0]], hip.kernel_name(S.pw_f32_full_struct(c))), f"PW_F32_FULL {c}")
    return got


@functools.lru_cache(maxsize=None)
def _level1():
    ch = {c for case, _ in listed_cases() for c in (case.cin, case.cout) if c <= CMAX}
    return tuple(sorted(set(range(16, CMAX + 1, 16)) | {8} | ch))


# level 2: both neighbours of every multiple of 16 (and 32), the multiples of 8 between them
_LEVEL2 = tuple(sorted({16 * k + d for k in range(0, CMAX // 16) for d in (1, 8, 15)} - {1}))


def _refine(axis, changed):
    """axis (sorted level-1 values) + the level-2 values inside every interval (axis[i], axis[i + 1]) flagged in `changed`"""
    add = [v for i in np.nonzero(changed)[0] for v in _LEVEL2 if axis[i] < v < axis[i + 1]]
    return sorted(set(axis) | set(add))


def _cells(values, breaks):
    """[(lo, hi)] index ranges of walked values between the break positions (a break after index i)."""
    out, lo = [], 0
    for i in range(len(values)):
        if i == len(values) - 1 or breaks[i]:
            out.append((lo, i))
            lo = i + 1
    return out


@functools.lru_cache(maxsize=None)
def enumerate_classes():
    """{(entry point, instantiation name): [Box, ...]} over the domain (dry run, no GPU).  Also asserts, on every walked point of
    the tail forms, that x3d_pw_fwd_tail_supported() and the dispatch agree: an admitted launch has a kernel, a declined one is
    refused."""
    from x3d_tf_amd import hip
    lib = hip.load()
    name_of, tail_ok = lib.x3d_pw_kernel_name, lib.x3d_pw_fwd_tail_supported
    buf = C.create_string_buffer(160)
    ids = {}
    boxes = {}
    l1 = list(_level1())
    l1set = set(l1)
    for form, val in FORMS:
        planes = PLANES_S2 if stride_of(form, val) == 2 else PLANES
        for dtype in S.DTYPES:
            for panel in ((False, True) if dtype != S.F32 and form != "wgrad" else (False,)):
                for plane in planes:
                    # one struct per form, storage type and plane from the builder; only the two channel counts change along the walk
                    st = case_struct(Case(form, val, dtype, panel, WALK_N, 8, 8, *plane, 0))
                    ref = C.byref(st)
                    args = _slots(form, ref) + (buf, 160)
                    tail = form == "fwd_tail"

                    def ask(cins, couts):
                        """the answers on cins x couts as a list of rows (-1: refused)"""
                        rows = []
                        for cin in cins:
                            st.Cin = cin
                            row = []
                            for cout in couts:
                                st.Cout = cout
                                if name_of(*args) == 0:
                                    k = ids.get(buf.value)
                                    if k is None:
                                        k = ids[buf.value] = len(ids)
                                    row.append(k)
                                else:
                                    row.append(-1)
                                if tail:
                                    assert (row[-1] >= 0) == bool(tail_ok(ref)), \
                                        (f"x3d_pw_fwd_tail_supported() and the dispatch disagree at {val} {cin}->{cout} {plane} {dtype}: "
                                         f"{lib.x3d_last_error().decode()}")
                            rows.append(row)
                        return rows

                    m1 = np.array(ask(l1, l1), dtype=np.int32)
                    if not (m1 >= 0).any():
                        continue
                    ci_ax = _refine(l1, (m1[1:] != m1[:-1]).any(axis=1))
                    co_ax = _refine(l1, (m1[:, 1:] != m1[:, :-1]).any(axis=0))
                    # level 2: the new rows on every column, the new columns on the level-1 rows
                    m = np.full((len(ci_ax), len(co_ax)), -2, dtype=np.int32)
                    rows1 = [ci_ax.index(v) for v in l1]
                    cols1 = [co_ax.index(v) for v in l1]
                    m[np.ix_(rows1, cols1)] = m1
                    new_ci = [v for v in ci_ax if v not in l1set]
                    new_co = [v for v in co_ax if v not in l1set]
                    if new_ci:
                        m[[ci_ax.index(v) for v in new_ci]] = np.array(ask(new_ci, co_ax), dtype=np.int32)
                    if new_co:
                        m[np.ix_(rows1, [co_ax.index(v) for v in new_co])] = np.array(ask(l1, new_co), dtype=np.int32)
                    assert (m >= -1).all()
                    bi = np.append((m[1:] != m[:-1]).any(axis=1), True)
                    bj = np.append((m[:, 1:] != m[:, :-1]).any(axis=0), True)
                    for i0, i1 in _cells(ci_ax, bi):
                        for j0, j1 in _cells(co_ax, bj):
                            k = int(m[i0, j0])
                            assert (m[i0:i1 + 1, j0:j1 + 1] == k).all()
                            if k >= 0:
                                boxes.setdefault((k, form, val, dtype, panel, (ci_ax[i0], ci_ax[i1]), (co_ax[j0], co_ax[j1])), []).append(plane)
    names = {v: k.decode() for k, v in ids.items()}
    out = {}
    for (k, form, val, dtype, panel, cin, cout), planes in boxes.items():
        out.setdefault((ENTRY[form], names[k]), []).append(Box(form, val, dtype, panel, cin, cout, tuple(planes)))
    # the registered lists and the fuzz slice: a shape whose class the grid walk did not meet comes in as a single-point box
    for case, _ in listed_cases():
        cls = dispatch(case)
        if cls is not None and cls not in out and cls not in FULL_SIZE_ONLY:
            out.setdefault(cls, []).append(Box(case.form, case.val, case.dtype, case.panel, (case.cin, case.cin), (case.cout, case.cout),
                                               ((case.t, case.h, case.w),)))
    for cls in FULL_SIZE_ONLY:
        assert cls not in out, f"{cls} is reachable inside the size budget: take it out of FULL_SIZE_ONLY"
    key = lambda b: (b.cin[0] * b.cout[0], FORMS.index((b.form, b.val)), S.DTYPES.index(b.dtype), b.panel, b.cin, b.cout)
    return {cls: sorted(bs, key=key) for cls, bs in sorted(out.items())}


# ---- tile regimes ---------------------------------------------------------------------------------------------------------------
def _csrc(fname):
    return open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "x3d-tf_amd", "csrc", fname)).read()


@functools.lru_cache(maxsize=None)
def tile_constants():
    """From the kernel headers: WS_BN (point tile of the weights-stationary / -streamed kernels), PWB_BN (of the resident-panel
    kernel) and that kernel's minimum run of tiles per workgroup as [(K at least, run), ...] (pw_bf16_launch_cfg: tpb_min)."""
    ws = int(re.search(r"^#define\s+WS_BN\s+(\d+)\b", _csrc("pw_gemm_ws.h"), re.M).group(1))
    text = _csrc("pw_gemm_bf16.h")
    pwb = int(re.search(r"^#define\s+PWB_BN\s+(\d+)\b", text, re.M).group(1))
    m = re.search(r"int tpb_min = a\.K >= (\d+) \? (\d+) : \(a\.K >= (\d+) \? (\d+) : 1\);", text)
    assert m, "pw_gemm_bf16.h: the tpb_min rule of pw_bf16_launch_cfg is not where tests/pw_classes.py reads it"
    k1, r1, k2, r2 = map(int, m.groups())
    return dict(WS_BN=ws, PWB_BN=pwb, runs=((k1, r1), (k2, r2)))


WHOLE = 256      # every point tile of these kernels (32: WS_BN, the fp32 / generic weight-gradient steps; 64: the 16-bit weight-gradient
RAGGED = 32      # steps; 128: PWB_BN; 32 NT with NT <= 8: the fp32 GEMMs) divides 256 and is a multiple of 32


def is_resident_panel(cls):
    return cls[1].startswith("pw_gemm_bf16_kernel<")


def gemm_k(case):
    """the contraction length of the GEMM behind a case: Cin forward, Cout in the data gradient"""
    return case.cout if case.form == "dgrad" else case.cin


def panel_run(k):
    """tiles per workgroup run of the resident-panel kernel at small sizes (its tpb_min)"""
    for kmin, run in tile_constants()["runs"]:
        if k >= kmin:
            return run
    return 1


def tile_regime(case, cls=None):
    """How a case's plane meets the point tiles: the set of
      "whole"    P a multiple of WHOLE: whole tiles in every kernel
      "partial"  P % RAGGED != 0: every sample ends in a partial tile in every kernel
      "p8"       P % 8 == 0 (whole 16-byte vectors of 16-bit elements)
    and for the resident-panel kernel (cls given), whose workgroups take runs of panel_run(K) 128-point tiles:
      "cross"    a run crosses a sample boundary (N >= 2, the per-sample tile count no multiple of the run)
      "short"    the last of several runs is shorter than the others"""
    p = points(case)
    got = set()
    if p % WHOLE == 0:
        got.add("whole")
    if p % RAGGED:
        got.add("partial")
    if p % 8 == 0:
        got.add("p8")
    if cls is not None and is_resident_panel(cls):
        per = -(-p // tile_constants()["PWB_BN"])
        run, tiles = panel_run(gemm_k(case)), per * case.n
        if run >= 2 and any((j * per) % run for j in range(1, case.n)):
            got.add("cross")
        if run >= 2 and tiles > run and tiles % run:
            got.add("short")
    return got


# ---- the committed cases --------------------------------------------------------------------------------------------------------
def _fits(case):
    s = stride_of(case.form, case.val)
    pin = case.t * case.h * case.w
    return points(case) <= MAX_POINTS and case.n * max(case.cin, case.cout) * (pin if s == 2 else points(case)) <= MAX_ELEMS


OFFSET_BOXES = 8      # the offset cases are looked for at the channel corners of a class's first boxes


def _pick(cls, boxes, plane_key, skip_box=None, n=WALK_N, upper=False, k_min=0, want=None, offs=(0,)):
    """The first case of a class in its boxes' order (smallest channel counts first) on the plane that is smallest under
    `plane_key` (None from the key: the plane does not qualify).  upper: at the box's upper channel corner where that stays
    within 48 channels of the lower one, else 13 channels inside.  k_min: a box whose GEMM K reaches it, K at its upper end.
    want(case): a further condition.  offs other than (0,): a case with its activation operands that many elements off their
    alignment (1 before 2), looked for on EVERY walked plane of the form at the corners of the first OFFSET_BOXES boxes -- an
    offset sends planes into a class that its aligned boxes do not hold.  Every candidate is asked of the dry run again."""
    moved = tuple(offs) != (0,)
    for off, box in ((o, b) for o in offs for b in (boxes[:OFFSET_BOXES] if moved else boxes)):
        if box is skip_box:
            continue
        walked = (PLANES_S2 if stride_of(box.form, box.val) == 2 else PLANES) if moved else box.planes
        planes = sorted((plane_key(_plane_points(box.form, box.val, pl)), pl) for pl in walked
                        if plane_key(_plane_points(box.form, box.val, pl)) is not None)
        for _, pl in planes:
            (a0, a1), (b0, b1) = box.cin, box.cout
            up = lambda lo, hi: hi if hi <= lo + 48 else lo + 13
            corners = [(up(a0, a1), up(b0, b1)), (a1, b1), (a0, b0)] if upper else [(a0, b0), (a1, b1)]
            if k_min:
                corners = [(a1, b0), (a1, b1)] if box.form != "dgrad" else [(a0, b1), (a1, b1)]
            for cin, cout in corners:
                case = Case(box.form, box.val, box.dtype, box.panel, n, cin, cout, *pl, off)
                if gemm_k(case) >= k_min and _fits(case) and (want is None or want(case)) and dispatch(case) == cls:
                    return case, box
    return None, None


def class_cases(cls):
    """The committed cases of a class, by fixed rules (no random draws), each inside the size budget and re-checked against the
    dry run:
      1. "ragged": N = 2 in the class's smallest box, on a plane with P % 8 != 0 if the class has one (the smallest with more
         than 128 points, else the largest below), else with P % 32 != 0 -- a partial last tile in every kernel;
      2. "whole": N = 2 in ANOTHER box where the class has several, at the box's upper channel end, on a plane of whole
         256-point tiles if the class has one, else with P % 8 == 0, else any other plane than case 1's.  So a class that takes
         both P % 8 == 0 and P % 8 != 0 (no RAG flag in its name) has one of each;
      3. resident-panel kernel (pw_gemm_bf16_kernel) with K >= 96: N = 3 (5 where every plane of the class is one tile) on a plane
         whose per-sample tile count is no multiple of the kernel's run of 2 / 4 tiles, so that runs cross sample boundaries and
         the last run is short (tile_regime);
      4. offset cases, every activation operand 1 element (2 where 1 does not keep the class and 2 does) off its
         16-byte-aligned allocation, over ALL walked planes at the channel corners of the class's first boxes: one on a ragged
         plane of more than 128 points (P % 32 != 0), one on a plane of whole 256-point tiles, for a resident-panel class with
         K >= 96 one whose runs cross a sample boundary and end short; where the class keeps none of these under an offset, the
         largest plane it does keep.  The scalar kernels (VEC = 1) take aligned launches only below 8 or 16 points; through the
         offset they run the planes of several tiles that the other classes run aligned."""
    boxes = enumerate_classes()[cls]
    ragged = lambda p: (p % 8 == 0, p <= 128, p if p > 128 else -p) if p % RAGGED else None
    c1, b1 = _pick(cls, boxes, ragged)
    if c1 is None:
        c1, b1 = _pick(cls, boxes, lambda p: (p,))
    assert c1 is not None, f"{cls}: no case inside the size budget"
    p1 = points(c1)
    whole = lambda p: (p % WHOLE != 0, p % 8 != 0, p) if p != p1 or p % WHOLE == 0 else None
    c2 = None
    for skip in ((b1, None) if len(boxes) > 1 else (None,)):
        for key in (whole, lambda p: (p,)):
            if c2 is None:
                c2, _ = _pick(cls, boxes, key, skip_box=skip, upper=True, want=lambda c: c != c1)
    cases = [c1] + ([c2] if c2 is not None else [])
    if is_resident_panel(cls):
        aim = {"cross", "short"}
        for n in (3, 5):          # (5: a class whose planes are single tiles, under runs of 4)
            c3, _ = _pick(cls, boxes, lambda p: (-p,), n=n, k_min=96, want=lambda c: aim <= tile_regime(c, cls))
            if c3 is not None:
                cases.append(c3)
                break
    offs = (1, 2)
    moved = [_pick(cls, boxes, lambda p: (p,) if p % RAGGED and p > 128 else None, offs=offs)[0],
             _pick(cls, boxes, lambda p: (p,) if p % WHOLE == 0 else None, upper=True, offs=offs)[0]]
    if is_resident_panel(cls):
        for n in (3, 5):
            c, _ = _pick(cls, boxes, lambda p: (-p,), n=n, k_min=96, want=lambda c: aim <= tile_regime(c, cls), offs=offs)
            if c is not None:
                moved.append(c)
                break
    if not any(moved):
        moved = [_pick(cls, boxes, lambda p: (-p,), offs=offs)[0]]
    return cases + [c for i, c in enumerate(moved) if c is not None and c not in moved[:i]]


def offset_points(cls):
    """{P} of the walked planes that an offset of 1 or 2 elements keeps in (or sends into) the class at the lower channel corner
    of one of its first OFFSET_BOXES boxes -- what rule 4 of class_cases() chooses from."""
    got = set()
    for box in enumerate_classes()[cls][:OFFSET_BOXES]:
        for pl in (PLANES_S2 if stride_of(box.form, box.val) == 2 else PLANES):
            case = Case(box.form, box.val, box.dtype, box.panel, WALK_N, box.cin[0], box.cout[0], *pl, 0)
            if _fits(case) and any(dispatch(case._replace(off=off)) == cls for off in (1, 2)):
                got.add(points(case))
    return got


def has_panel_run(cls):
    """does the resident-panel class hold a box whose GEMM K reaches the kernel's first run threshold?"""
    k = min(kmin for kmin, _ in tile_constants()["runs"])
    return is_resident_panel(cls) and any((b.cout if b.form == "dgrad" else b.cin)[1] >= k for b in enumerate_classes()[cls])


def case_id(case):
    val = case.val if not isinstance(case.val, tuple) else "/".join(str(v) for v in case.val)
    return (f"{case.form}[{val}]-{str(case.dtype)[6:]}{'-panel' if case.panel else ''}-N{case.n}-{case.cin}to{case.cout}-"
            f"T{case.t}-{case.h}x{case.w}" + (f"-off{case.off}" if case.off else ""))


def kernel_calls(case):
    """The kernel tests of tests/test_kernels_gpu.py that check a case against the fp64 restatements:
    [(test function name, positional arguments after `gpu`, keyword arguments)]."""
    from x3d_tf_amd import hip
    shape, kw = case_shape(case), ({"off": case.off} if case.off else {})
    if case.form in ("fwd", "fwd_s2"):
        return [("test_pw_fwd", (case.dtype, shape, case.panel), kw)]
    if case.form == "fwd_tail":
        return [("test_pw_fwd_tail", (case.dtype, shape, case.panel), kw)]
    if case.form == "fwd_infer":
        return [("test_pw_fwd_infer", (case.dtype, shape, case.panel), kw)]
    if case.form == "dgrad":
        return [("test_pw_dgrad", (case.dtype, shape, case.val, case.panel), kw)]
    calls = [("test_pw_wgrad", (case.dtype, shape, False), kw)]
    parts = hip.load().x3d_pw_wgrad_dw_parts
    if parts(C.byref(case_struct(case))) > 0 and parts(C.byref(case_struct(case._replace(off=0)))) > 0:   # (the slab form exists)
        calls.append(("test_pw_wgrad", (case.dtype, shape, True), kw))
    return calls
