"""The class enumeration of x3d_pw_fwd / x3d_pw_dgrad / x3d_pw_wgrad (tests/pw_classes.py) and its committed cases, checked on
the CPU through the library's dry-run dispatch: the enumeration holds everything the registered lists, the fuzz slice, the
full-size plans and the shipped configurations dispatch through these entry points; every class gets its cases by the fixed
rules, inside the size budget, each dispatching to its class; what the walk holds fixed the dispatch does not read; the tile
regimes are met; the "supported" queries and the dispatch do not contradict each other.  tests/test_pw_classes_gpu.py runs the
classes.

The gap this sweep closes (test_gap_report prints it): of the 676 classes, 244 had no case in the registered lists
(tests/shapes.py), the seeded fuzz slice or shapes.PW_FULL before it; a coarser walk had put that at 228 of 646."""
import ctypes as C

import pytest
import torch

from tests import pw_classes as PC
from tests import shapes as S

_ENTRIES = ("x3d_pw_fwd", "x3d_pw_dgrad", "x3d_pw_wgrad")


@pytest.fixture(scope="module")
def classes():
    return PC.enumerate_classes()


@pytest.fixture(scope="module")
def committed(classes):
    """{class: [Case, ...]} as the GPU sweep runs them."""
    return {cls: PC.class_cases(cls) for cls in classes}


def test_enumeration_holds_everything_dispatched_elsewhere(classes):
    """Completeness: what the registered lists, the fuzz slice, the non-`bwd` rows of PW_FULL and the shipped configurations
    (all variants and storage types) dispatch through the three entry points is a subset of the enumeration -- but for the two
    instantiations that only exist at 2 GB, excluded by name."""
    from tests import test_dispatch_coverage as DCOV
    need = dict(PC.listed_names())
    for k, v in PC.full_size_names().items():
        need.setdefault(k, v)
    for k, v in DCOV.shipped_config_kernels().items():
        if k[0] in _ENTRIES:
            need.setdefault(k, v)
    assert len(need) > 300
    missing = {k: v for k, v in need.items() if k not in classes and k not in PC.FULL_SIZE_ONLY}
    print(f"{len(classes)} reachable instantiations, {len(need)} of them dispatched by the lists, the fuzz slice or the plans")
    assert not missing, "dispatched but not enumerated:\n" + "\n".join(f"  {k}   <- {v}" for k, v in sorted(missing.items()))
    assert set(PC.FULL_SIZE_ONLY) <= set(need), "a FULL_SIZE_ONLY instantiation that nothing dispatches any more"
    assert len(classes) >= PC.CLASSES_AT_LEAST, f"{len(classes)} classes: the reachable domain of the pointwise entry points shrank"
    assert {c[0] for c in classes} == set(_ENTRIES)


def test_enumeration_holds_instantiations_the_lists_missed(classes):
    """Instantiations that no registered list or full-size plan ran before this sweep (a fuzz seed at most), by name: ragged weights-stationary
    shapes, the strided add on ragged rows, the weights-streamed data gradient, scalar forms of the resident-panel and generic
    kernels, the fp32 pipelined and resident kernels behind the folded tail, generic weight-gradient groups."""
    for entry, names in (
            ("x3d_pw_fwd", ("pw_gemm_wst_kernel<{h}, 1, 100, 3, 1, 40, 1, 1>", "pw_gemm_wst_kernel<{h}, 1, 100, 5, 1, 20, 1, 1>",
                            "pw_gemm_wst_kernel<{h}, 0, 100, 5, 2, 18, 1, 1>", "pw_f32p_kernel<1, 8, 3, 100, 0>",
                            "pw_f32p_kernel<1, 8, 3, 100, 1>", "pw_f32r_kernel<4, 1, 8, 4, 100>")),
            ("x3d_pw_dgrad", ("pw_gemm_wst_kernel<{h}, 2, 2, 7, 2, 12, 1, 1>", "pw_gemm_ws_kernel<{h}, 2, 0>", "pw_gemm_ws_kernel<{h}, 2, 1>",
                              "pw_gemm_ws_kernel<{h}, 2, 3>", "pw_f32p_kernel<1, 8, 2, 0, 1>", "pw_f32p_kernel<1, 8, 2, 1, 1>",
                              "pw_f32p_kernel<1, 8, 2, 3, 1>")),
            ("x3d_pw_wgrad", tuple(f"pw_wgrad_bf16_kernel<{{h}}, 1, {tpw}, 0, 0>" for tpw in (1, 2, 4, 8))
             + tuple(f"pw_wgrad_kernel<float, 1, {tpw}, 0, 0>" for tpw in (1, 2, 4, 8)))):
        for name in names:
            for h in (("bf16", "f16") if "{h}" in name else ("",)):
                cls = (entry, name.format(h=h))
                assert cls in classes, f"{cls} is not enumerated: a hole in the walked domain"


def test_gap_report(classes):
    """How many classes had no kernel-level case before this sweep: not in the registered lists, not in the fuzz slice, not in
    PW_FULL.  (Recorded in the module docstring; a change of the lists moves it.)"""
    had = set(PC.listed_names()) | set(PC.full_size_names())
    gap = sorted(c for c in classes if c not in had)
    fuzz_only = set(PC.listed_names()) - set(PC.full_size_names()) - _registered_only()
    print(f"{len(gap)} of {len(classes)} classes had no case in tests/shapes.py, the fuzz slice or PW_FULL; "
          f"{len(fuzz_only & set(classes))} more only through the fuzz slice's seeds")
    for entry in _ENTRIES:
        print(f"  {entry}: {sum(1 for c in gap if c[0] == entry)}")
    assert gap, "every class is covered by the lists: the sweep's docstrings are out of date"


def _registered_only():
    return {PC.dispatch(c) for c, what in PC.listed_cases() if not what.startswith("fuzz")} - {None}


def test_every_class_gets_its_cases(classes, committed):
    """Case selection: every class has at least two cases, each dispatches to its class, is within the size budget, runs a
    kernel test, and the list is the same on a second call."""
    from tests import test_kernels_gpu as K
    total = offs = 0
    for cls, cases in committed.items():
        assert 2 <= len(cases) <= 7 and len(set(cases)) == len(cases), (cls, cases)
        assert cases == PC.class_cases(cls), f"{cls}: the case list differs between two calls"
        for case in cases:
            assert PC.dispatch(case) == cls, (cls, case)
            s = PC.stride_of(case.form, case.val)
            elems = case.n * max(case.cin, case.cout) * case.t * case.h * case.w
            assert PC.points(case) <= PC.MAX_POINTS and elems <= PC.MAX_ELEMS and case.n in (2, 3, 5), (cls, case)
            assert s == 1 or case.form in ("fwd_s2", "wgrad")
            assert not (case.panel and case.dtype == torch.float32)
            calls = PC.kernel_calls(case)
            assert calls and all(callable(getattr(K, fn)) for fn, _, _ in calls)
            assert all(kw == ({"off": case.off} if case.off else {}) for _, _, kw in calls)
            total += len(calls)
            offs += bool(case.off)
        assert len({(c.cin, c.cout, c.t, c.h, c.w) for c in cases[:2]}) == 2, (cls, cases)
        if len(classes[cls]) > 1:      # two different boxes where the class has several
            inside = lambda c, b: (b.form, b.val, b.dtype, b.panel) == c[:4] and b.cin[0] <= c.cin <= b.cin[1] and b.cout[0] <= c.cout <= b.cout[1]
            assert not any(inside(cases[0], b) and inside(cases[1], b) for b in classes[cls]), (cls, cases[:2])
    print(f"{len(classes)} classes, {sum(map(len, committed.values()))} cases ({offs} with offset operands), {total} kernel checks")
    assert offs >= 100, "the offset cases went away: does the dry-run struct still carry the offset?"


def test_offset_cases_describe_the_offset_launch(committed):
    """The dry-run struct of an offset case has every activation operand off its 16-byte alignment and nothing else moved; the
    offset is 2 elements only where 1 does not keep the class.  (The aligned launch of the same shape may be in another class:
    the offset is the one route by which planes of 8 points and more reach the scalar kernels.)"""
    seen = 0
    for cls, cases in committed.items():
        for case in cases:
            if case.off:
                seen += 1
                es = 4 if case.dtype == torch.float32 else 2
                st, st0 = PC.case_struct(case), PC.case_struct(case._replace(off=0))
                for name, _ in st._fields_:
                    a, b = getattr(st, name), getattr(st0, name)
                    if name in PC._ACT_FIELDS[cls[0]] and b:
                        assert a % 16 == (case.off * es) % 16 != 0 and b % 16 == 0, (case, name)
                    elif isinstance(b, int) and b > (1 << 32):
                        assert a % 16 == 0, (case, name)
                assert case.off == 1 or (case.off == 2 and PC.dispatch(case._replace(off=1)) != cls), (cls, case)
    assert seen


def test_dispatch_reads_neither_n_nor_the_split_of_the_plane(classes):
    """Dispatch assumptions: on every box of every class (its first plane, its lower channel corner) the name is the same for
    N = 1, 3, 5 as for the walk's N = 2, and for the plane (T Ho, 1, W) as for (T, H, W)."""
    asked = 0
    for cls, boxes in classes.items():
        for b in boxes:
            t, h, w = b.planes[0]
            base = PC.Case(b.form, b.val, b.dtype, b.panel, PC.WALK_N, b.cin[0], b.cout[0], t, h, w, 0)
            assert PC.dispatch(base) == cls, (cls, base)
            for n in (1, 3, 5):
                assert PC.dispatch(base._replace(n=n)) == cls, f"the dispatch reads N: {base} at N = {n}"
            s = PC.stride_of(b.form, b.val)
            flat = base._replace(t=t * (-(-h // s)), h=1)
            assert PC.points(flat) == PC.points(base) and PC.dispatch(flat) == cls, f"the dispatch reads T / H beyond P: {base}"
            asked += 1
    assert asked > 1000


def test_planes_hold_the_edges():
    """the walked planes: P % 8 == 0 and not (odd and even), P < 8, P < 16, both sides of the 32-, 64- and 128-point tile
    boundaries, whole 256-point tiles, 13 frames; stride 2: every gather group with P % 8 == 0 and not"""
    ps = {t * h * w for t, h, w in PC.PLANES}
    assert {3, 8, 12, 25, 34, 66, 98, 128, 129, 130, 256, 325, 392, 1300} <= ps
    assert any(p < 8 for p in ps) and any(8 <= p < 16 for p in ps)
    assert any(p % 8 and p % 2 and p >= 8 for p in ps) and any(p % 8 and p % 2 == 0 and p >= 8 for p in ps)
    groups = {"8k": lambda w: w % 8 == 0, "4k": lambda w: w % 8 == 4, "4k+2": lambda w: w % 4 == 2, "odd": lambda w: w % 2 == 1 and w > 7,
              "7": lambda w: w == 7, "3": lambda w: w == 3}
    for name, ok in groups.items():
        got = {(t * ((h + 1) // 2) * ((w + 1) // 2)) % 8 == 0 for t, h, w in PC.PLANES_S2 if ok(w)}
        assert got == {True, False} or (name == "8k" and True in got), (name, got)
    # 8 k rows of 16 and more give Wo % 8 == 0: P % 8 != 0 there needs W = 8
    assert any(w == 8 and (t * ((h + 1) // 2) * 4) % 8 for t, h, w in PC.PLANES_S2)


def test_tile_constants_and_known_grid():
    """The regime rules read the headers: every point tile divides WHOLE and is a multiple of RAGGED; the resident-panel
    kernel's runs are 2 tiles from K = 96 and 4 from K = 192.  A known grid: (3, 200, 40, 1, 3, 43), P = 129, two 128-point tiles
    per sample, runs of 4 -- [0..3] crosses the first sample boundary, [4, 5] is short."""
    tc = PC.tile_constants()
    assert tc["WS_BN"] == 32 and tc["PWB_BN"] == 128 and tc["runs"] == ((192, 4), (96, 2))
    for tile in (tc["WS_BN"], tc["PWB_BN"], 64, 256):
        assert PC.WHOLE % tile == 0 and tile % PC.RAGGED == 0
    # the fp32 kernels name their point tile: NT tiles of 32 points, NT <= 8
    for entry, name in PC.enumerate_classes():
        if name.startswith(("pw_f32p_kernel<", "pw_f32r_kernel<", "pw_gemm_kernel<")):
            args = [a.strip() for a in name[name.index("<") + 1:-1].split(",")]
            nt = int(args[1] if name.startswith("pw_f32p") else (args[2] if name.startswith("pw_f32r") else args[3]))
            assert nt in (1, 2, 4, 8), name
    assert [PC.panel_run(k) for k in (95, 96, 191, 192, 640)] == [1, 2, 2, 4, 4]
    case = PC.Case("fwd", "swish", torch.bfloat16, False, 3, 200, 40, 1, 3, 43, 0)
    cls = PC.dispatch(case)
    assert cls == ("x3d_pw_fwd", "pw_gemm_bf16_kernel<bf16, 8, 2, 1, 100, 0, 8, 1>")
    assert PC.tile_regime(case, cls) == {"partial", "cross", "short"}
    assert PC.tile_regime(case._replace(n=2), cls) == {"partial", "cross"}      # 4 tiles: one run over both samples, none short
    assert PC.tile_regime(case._replace(cin=100), cls) == {"partial"}           # runs of 2 on 2 tiles per sample
    assert PC.tile_regime(case._replace(cin=100, t=2, h=8, w=8), cls) == {"p8", "cross", "short"}   # one tile per sample, runs of 2
    assert PC.tile_regime(case._replace(t=4, h=8, w=8)) == {"whole", "p8"}


def test_tile_regimes_are_met(classes, committed):
    """Tile regimes, over the aligned planes of a class's boxes AND the walked planes an operand offset keeps in it
    (PC.offset_points): every class has a case with N >= 2 and a partial last tile (P % 32 != 0), one of more than 128 such
    points and one with whole tiles (P % 256 == 0) wherever it holds such planes; a class without the RAG flag in its name that
    takes both P % 8 == 0 and P % 8 != 0 aligned has one of each; a resident-panel class that reaches K >= 96 has a case whose
    runs cross a sample boundary and end short.  Only the generic fp32 kernels of stride 1, which the dispatch takes below 4
    points per sample and nowhere else, are left with cases of fewer than 32 points."""
    crossing, tiny = 0, []
    for cls, cases in committed.items():
        aligned = {PC._plane_points(b.form, b.val, pl) for b in classes[cls] for pl in b.planes}
        have = aligned | PC.offset_points(cls)
        got = [PC.tile_regime(c, cls) for c in cases if c.n >= 2]
        pts = [PC.points(c) for c in cases if c.n >= 2]
        if any(p % PC.RAGGED for p in have):
            assert any("partial" in g for g in got), (cls, cases)
        if any(p % PC.RAGGED and p > 128 for p in have):
            assert any("partial" in g and p > 128 for g, p in zip(got, pts)), (cls, cases)
        if any(p % PC.WHOLE == 0 for p in have):
            assert any("whole" in g for g in got), (cls, cases)
        if any(p % 8 == 0 for p in aligned) and any(p % 8 for p in aligned):
            plain = [PC.tile_regime(c, cls) for c in cases if not c.off]
            assert any("p8" in g for g in plain) and any("p8" not in g for g in plain), (cls, cases)
        if PC.has_panel_run(cls):
            assert any({"cross", "short"} <= g for g in got), (cls, cases)
            crossing += 1
        if max(pts) < 32:
            tiny.append(cls)
            assert max(have) < 4 and cls[1].startswith(("pw_gemm_kernel<float, 1, ", "pw_wgrad_kernel<float, 1, ")) and cls[1].endswith(", 0>"), (cls, cases)
    assert crossing >= 50
    print(f"{len(tiny)} classes run on fewer than 4 points per sample only (the dispatch gives them no other plane)")
    assert len(tiny) <= 32


def test_supported_queries_agree_with_the_dispatch(committed):
    """Class exclusivity: x3d_pw_fwd_tail_supported() is checked against the dispatch on every walked point of the tail forms
    inside enumerate_classes().  x3d_pw_coef_fold_supported() is a function of the instantiation name alone (pw_dgrad.hip: it asks
    the dry run and compares name prefixes), so it is asked once per class and case, not per walked point: on every committed
    dgrad / wgrad case, where it says yes the launch with a coef_fold has a kernel -- the same one -- and where it says no the
    dispatch refuses the fold."""
    from x3d_tf_amd import hip
    lib = hip.load()
    buf = C.create_string_buffer(160)
    seen = set()
    for cls, cases in committed.items():
        if cls[0] == "x3d_pw_fwd":
            continue
        for case in cases:
            st = PC.case_struct(case)
            ref = C.byref(st)
            q = (ref, None, None) if cls[0] == "x3d_pw_dgrad" else (None, ref, None)
            ok = bool(lib.x3d_pw_coef_fold_supported(*q))
            fold = hip.BnBwdFold(S._Addr.new(), 1.0, S._Addr.new(), S._Addr.new(), None, None, None)
            st.coef_fold = hip.fold_address(fold)
            rc = lib.x3d_pw_kernel_name(*PC._slots(case.form, ref), buf, 160)
            assert (rc == 0) == ok, f"x3d_pw_coef_fold_supported() says {ok}, the dispatch {'takes' if rc == 0 else 'refuses'} the fold: {case}"
            if ok:
                assert (cls[0], buf.value.decode()) == cls, (case, buf.value)
            seen.add((cls[0], ok))
    assert seen == {(e, ok) for e in ("x3d_pw_dgrad", "x3d_pw_wgrad") for ok in (True, False)}
