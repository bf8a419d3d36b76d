"""The class enumeration of the fused pointwise backward (tests/pw_bwd_classes.py) and its shape generator, checked on the
CPU through the library's dry-run dispatch: the enumeration holds everything the registered cases and the full-size plans
dispatch, every class gets its committed shapes with (almost) no declined draw, the persistent kernels meet every tile
regime, and the X3D-XL training plan launches nothing outside the classes.  tests/test_pw_bwd_classes_gpu.py runs the
classes."""
import ctypes as C

import pytest
import torch

from tests import pw_bwd_classes as PC
from tests import shapes as S

DECLINE_CAP = 0.02           # of the first draws: a silently shrunk domain shows as declined draws


@pytest.fixture(scope="module")
def classes():
    return PC.enumerate_classes()


@pytest.fixture(scope="module")
def committed(classes):
    """[(class name, [Case, ...], seed, declined first draws)] for the seeds the GPU sweep uses."""
    return [(name,) + PC.class_cases(i, name, boxes) for i, (name, boxes) in enumerate(sorted(classes.items()))]


def _registered():
    """{instantiation: first registered kernel-level case of x3d_pw_bwd that runs it} (tests/shapes.py, as
    tests/test_dispatch_coverage.py reads the lists)."""
    from x3d_tf_amd import hip
    got = {}
    for dt in S.HALF_DTYPES:
        for shp in S.PW_BWD + S.PW_BWD_TAIL:
            got.setdefault(hip.kernel_name(S.pw_bwd_struct(shp, dt)), f"{shp} {dt}")
        for shp in S.PW_BWD_RC:
            got.setdefault(hip.kernel_name(S.pw_bwd_rc_struct(shp, dt)), f"rc {shp} {dt}")
        for shp in S.PW_BWD_RC_STRIDED:
            got.setdefault(hip.kernel_name(S.pw_bwd_rc_strided_struct(shp, dt)), f"rc strided {shp} {dt}")
            n, ci, co, t, xh, xw = shp
            st = S.pw_bwd_rc_struct((n, ci, co, t, (xh + 1) // 2, (xw + 1) // 2, "store", 0), dt)
            if hip.load().x3d_pw_bwd_supported(C.byref(st)):      # (the dense store form on the even-pixel copy)
                got.setdefault(hip.kernel_name(st), f"rc compact {shp} {dt}")
    return got


def test_enumeration_holds_every_registered_and_planned_instantiation(classes):
    """(a) what the registered lists and the full-size dry plans of BASELINE configs 1 - 5 dispatch for x3d_pw_bwd is a subset
    of the enumeration."""
    from x3d_tf_amd import dispatch as D
    need = _registered()
    for index in D.BASELINE_CONFIGS:
        for entry, kern, shape in D.baseline_kernels(index):
            if entry == "x3d_pw_bwd":
                need.setdefault(kern, f"config {index}: {shape}")
    assert need
    missing = {k: v for k, v in need.items() if k not in classes}
    print(f"x3d_pw_bwd: {len(classes)} reachable instantiations, {len(need)} of them registered or planned")
    assert not missing, "dispatched but not enumerated:\n" + "\n".join(f"  {k}   <- {v}" for k, v in sorted(missing.items()))
    assert len(classes) >= PC.CLASSES_AT_LEAST, f"{len(classes)} classes: the admitted domain of x3d_pw_bwd shrank"


def test_every_class_gets_its_committed_shapes(classes, committed):
    """(b) every class gets DRAWS accepted shapes inside its boxes -- the dry run dispatches each to the class, N in 1..5,
    at most MAX_POINTS points, a multiple of 8 -- and at most DECLINE_CAP of the first draws were declined."""
    from tests import test_kernels_gpu as K
    assert len(committed) == len(classes)
    first = declined = 0
    for name, cases, seed, dec in committed:
        assert len(cases) == PC.DRAWS, name
        first += len(cases)
        declined += dec
        for case in cases:
            assert PC.dispatch(*case) == name, (name, case, seed)
            n, cin, cout, t, h, w = case.shape[:6]
            ho, wo = ((h + 1) // 2, (w + 1) // 2) if case.kind == "rcs" else (h, w)
            assert 1 <= n <= 5 and (t * ho * wo) % 8 == 0 and t * ho * wo <= PC.MAX_POINTS, (name, case)
            assert any(b.cin[0] <= cin <= b.cin[1] and b.cout[0] <= cout <= b.cout[1] and w in b.rows for b in classes[name])
            calls = PC.kernel_calls(case)
            assert calls and all(callable(getattr(K, fn)) for fn, _ in calls)
    print(f"{len(classes)} classes, {first} first draws, {declined} declined")
    assert declined <= DECLINE_CAP * first, f"{declined} of {first} first draws declined by the dry run"


def test_draws_reach_the_inside_of_a_class(classes, committed):
    """channel counts anywhere in the tile class: over the committed seeds the draws are not all corners of their boxes"""
    inner = sum(1 for name, cases, _, _ in committed for c in cases
                if not any(c.shape[1] in b.cin and c.shape[2] in b.cout for b in classes[name]))
    assert inner * 4 >= sum(len(cases) for _, cases, _, _ in committed)


@pytest.mark.parametrize("dtype", S.HALF_DTYPES)
def test_persistent_kernels_meet_every_tile_regime(committed, dtype):
    """(c) over the committed seeds the weights-stationary kernels (pw_bwd_wst.hip stages 4 and 5, pw_bwd_wsta.hip) see, per
    storage type: no more tiles than workgroups, runs of >= 2 tiles across a sample boundary, a short last workgroup, a
    partial last tile, and for stage 5 both slices."""
    seen = {}
    for name, cases, _, _ in committed:
        if PC.is_persistent(name):
            for c in cases:
                if c.dtype == dtype:
                    seen.setdefault(name.split("<")[0] + ("/5" if ", 12, 6>" in name else ""), set()).update(PC.tile_regime(c))
    assert set(seen) == {"pw_bwd_wst_kernel", "pw_bwd_wst_kernel/5", "pw_bwd_wsta_kernel"}, seen
    for kern, got in seen.items():
        want = {"few", "cross", "short", "partial"} | ({"slices"} if kern.endswith("/5") else set())
        assert want <= got, f"{kern} ({dtype}): regimes {sorted(want - got)} never drawn"


def test_a_slab_form_exists_only_where_the_reduce_can_add_it_up(committed):
    """x3d_dw_slab_reduce (and the reduce slots of x3d_se_bnb_bwd) add the slabs up in aligned float4s and refuse a job of
    Cout * Cin % 4 != 0 elements: x3d_pw_bwd_dw_parts / x3d_pw_wgrad_dw_parts must say "no slab form" there, so that callers
    (ops.pw_bwd(slab=True), the plan recorder) keep the atomics.  Found by the class sweep on pw_bwd_wst_kernel<f16, 7, 12, 6>
    at (5, 270, 185, 8, 14, 14): the query reported slabs, the reduce refused them."""
    from x3d_tf_amd import hip
    lib = hip.load()
    seen = set()
    for name, cases, _, _ in committed:
        if PC.is_persistent(name):
            for c in cases:
                parts = lib.x3d_pw_bwd_dw_parts(C.byref(PC.case_struct(*c)))
                whole = (c.shape[1] * c.shape[2]) % 4 == 0
                assert (parts > 0) == whole, (name, c, parts)
                seen.add(whole)
    assert seen == {True, False}, "the committed draws should hold layers with and without the slab form"
    assert lib.x3d_pw_bwd_dw_parts(C.byref(S.pw_bwd_struct((5, 270, 185, 8, 14, 14, "swish_bwd"), torch.float16))) == 0
    assert lib.x3d_pw_bwd_dw_parts(C.byref(S.pw_bwd_struct((5, 270, 184, 8, 14, 14, "swish_bwd"), torch.float16))) > 0
    for dt in S.DTYPES:
        assert lib.x3d_pw_wgrad_dw_parts(C.byref(S.pw_wgrad_struct((2, 192, 432, 8, 7, 7, 1, None), dt))) > 0
        assert lib.x3d_pw_wgrad_dw_parts(C.byref(S.pw_wgrad_struct((2, 191, 431, 8, 7, 7, 1, None), dt))) == 0


def test_tile_regime_reads_a_known_grid():
    """(3, 224, 81, 13, 16, 16): 312 tiles on 156 workgroups -- runs of two tiles, 104 tiles per sample"""
    case = PC.Case("plain", torch.bfloat16, (3, 224, 81, 13, 16, 16, "swish_bwd"))
    assert PC.dispatch(*case) == "pw_bwd_wst_kernel<bf16, 7, 6, 3>"
    from x3d_tf_amd import hip
    assert hip.load().x3d_pw_bwd_dw_parts(C.byref(PC.case_struct(*case))) == 156
    assert PC.tile_regime(case) == set()          # (104 % 2 == 0: no run crosses a sample here)
    case = PC.Case("plain", torch.bfloat16, (3, 224, 81, 13, 16, 17, "swish_bwd"))   # 111 tiles per sample, runs of two
    assert "cross" in PC.tile_regime(case)


@pytest.mark.parametrize("dtype", S.HALF_DTYPES)
def test_xl_training_plan_stays_inside_the_classes(classes, dtype):
    """(d) every x3d_pw_bwd launch of the X3D-XL training plan (dry, full-size planes) is one of the classes -- its stage-3 `c`
    conv (162 -> 72) runs pw_bwd_fused_kernel<., 2, 3, 3>, which no registered case reaches."""
    from x3d_tf_amd import dispatch as D
    rows = [r for r in D.config_kernels("XL", 2, 16, 312, dtype, True) if r[0] == "x3d_pw_bwd"]
    assert rows, "the dry plan recorded no fused pointwise backward"
    missing = {k: v for k, v in D.kernel_set(rows).items() if k not in classes}
    assert not missing, "X3D-XL launches outside the enumeration:\n" + "\n".join(f"  {k}   <- {v}" for k, v in sorted(missing.items()))
    tag = "bf16" if dtype == torch.bfloat16 else "f16"
    assert f"pw_bwd_fused_kernel<{tag}, 2, 3, 3>" in {r[1] for r in rows}
