"""shapes.AUX_EDGE stays on the edges of the kernels' tiles (CPU only; tests/test_aux_edges_gpu.py runs the cases).

The head (head.hip), the squeeze-excite path and the slab reducer (se.hip), the plane-wise kernels and the layout converter
(elem.hip) are tiled; AUX_EDGE holds, per entry point, the shapes on both sides of every tile boundary.  This test reads the tile
sizes from the `#define` lines of the sources, holds them against the values the table was built for (shapes.AUX_TILES; the loop
literals that have no #define are restated in shapes.AUX_LITERALS next to their source lines), and asserts that every class of
shape below still has a case.  A retuned tile size therefore fails here, by name, until the table has moved with it.
"""
import pytest
import torch

from tests import shapes as S

F32 = torch.float32
PLANE = ("tail_fwd", "tail_bwd", "relu_bn_bwd_reduce", "pool_fwd")
PLANE_FIELDS = {"tail_fwd": 6, "tail_bwd": 6, "relu_bn_bwd_reduce": 7, "pool_fwd": 5}


def _plane(case):
    """(dtype, N, C, P, element offset, VEC of the launch) of a plane-wise case (elem.hip pick_vec / norm_vec)"""
    dt, n, c, P = case[1:5]
    k = PLANE_FIELDS[case[0]]
    off = case[k] if len(case) > k else 0
    full = S.aux_vec(dt)
    return dt, n, c, P, off, (full if P % full == 0 and off % full == 0 else 1)


def _slab_loops(parts, Lt):
    """(some part group runs the 64-stride loop, some part group runs the 16-stride tail after it) of dw_slab_reduce_block"""
    ran = tail = False
    for pg in range(Lt["SLAB_GROUPS"]):
        p = pg
        looped = False
        while p + Lt["SLAB_STRIDE"] - Lt["SLAB_GROUPS"] < parts:
            p += Lt["SLAB_STRIDE"]
            looped = True
        ran |= looped
        tail |= looped and p < parts
    return ran, tail


def edge_classes(T, Lt):
    """[(entry point, class name, predicate on a case of that entry point)]"""
    W, DX, KB = Lt["LANES"], Lt["DX_BATCH"], Lt["DW_KBLOCK"]
    cls = []
    add = lambda e, name, f: cls.append((e, name, f))
    for e in ("dense_fwd", "dense_bwd"):
        add(e, "K below the lane stride", lambda c: c[2] < W)
        add(e, "K a multiple of the lane stride", lambda c: c[2] % W == 0)
        add(e, "K above the lane stride, no multiple", lambda c: c[2] > W and c[2] % W != 0)
        add(e, "K below the 256-wide k block", lambda c: c[2] < KB)
        add(e, "K at the 256-wide k block", lambda c: c[2] == KB)
        add(e, "K above the 256-wide k block", lambda c: c[2] > KB)
        add(e, "N above 64", lambda c: c[1] > 64)
        add(e, "act off", lambda c: c[4] == 0)
        add(e, "act on", lambda c: c[4] == 1)
        add(e, "mask off", lambda c: c[5] is None)
        add(e, "mask on", lambda c: c[5] is not None)
    add("dense_fwd", "M % DENSE_MT != 0", lambda c: c[3] % T["DENSE_MT"] != 0)
    add("dense_fwd", "M % DENSE_MT == 0", lambda c: c[3] % T["DENSE_MT"] == 0)
    add("dense_fwd", "N % DENSE_NT != 0", lambda c: c[1] % T["DENSE_NT"] != 0)
    add("dense_fwd", "N % DENSE_NT == 0", lambda c: c[1] % T["DENSE_NT"] == 0)
    add("dense_fwd", "bias off", lambda c: not c[6])
    add("dense_fwd", "bias on", lambda c: c[6])
    add("dense_bwd", "M % DENSE_BM != 0", lambda c: c[3] % T["DENSE_BM"] != 0)
    add("dense_bwd", "M % DENSE_BM == 0", lambda c: c[3] % T["DENSE_BM"] == 0)
    add("dense_bwd", "M below the dx batch", lambda c: c[6] and c[3] < DX)
    add("dense_bwd", "M at the dx batch", lambda c: c[6] and c[3] == DX)
    add("dense_bwd", "M above the dx batch, no multiple", lambda c: c[6] and c[3] > DX and c[3] % DX != 0)
    add("dense_bwd", "N % DENSE_BN != 0", lambda c: c[6] and c[1] % T["DENSE_BN"] != 0)
    add("dense_bwd", "N % DENSE_BN == 0", lambda c: c[6] and c[1] % T["DENSE_BN"] == 0)
    add("dense_bwd", "N no multiple of the 8-sample batch", lambda c: c[1] % Lt["DW_NBATCH"] != 0)
    add("dense_bwd", "N a multiple of the 8-sample batch", lambda c: c[1] % Lt["DW_NBATCH"] == 0)
    for i, nm in ((6, "dx"), (7, "db")):
        add("dense_bwd", f"{nm} off", lambda c, i=i: not c[i])
        add("dense_bwd", f"{nm} on", lambda c, i=i: c[i])
    add("dense_bwd_refused", "M one past the LDS limit of dz", lambda c: 4 * T["DENSE_BN"] * (c[3] - 1) == 65536)
    add("dense_bwd_refused", "N one past the LDS limit of dzs", lambda c: 4 * T["DENSE_BM"] * (c[1] - 1) == 65536 and c[3] < 1024)
    for e, se in (("se_fwd", lambda c: True), ("se_bnb_bwd", lambda c: c[5])):
        add(e, "Wd % 8 != 0", lambda c, se=se: se(c) and c[3] % Lt["SE_BATCH"] != 0)
        add(e, "Wd within one 32-row round", lambda c, se=se: se(c) and c[3] <= Lt["SE_ROUND"])
        add(e, "Wd beyond one 32-row round", lambda c, se=se: se(c) and c[3] > Lt["SE_ROUND"])
        add(e, "Wd == SE_MAXW", lambda c, se=se: se(c) and c[3] == T["SE_MAXW"])
        add(e, "C < 64", lambda c, se=se: se(c) and c[2] < 64)
        add(e, "C > 256", lambda c, se=se: se(c) and c[2] > 256)
        add(e, "C == SE_MAXC", lambda c, se=se: se(c) and c[2] == T["SE_MAXC"])
        add(e, "N > 64", lambda c: c[1] > 64)
        add(e, "N % 4 != 0", lambda c: c[1] % 4 != 0)
    add("se_bnb_bwd", "without SE", lambda c: not c[5])
    add("se_bnb_bwd", "without SE, with slab jobs (the 256-thread launch)", lambda c: not c[5] and len(c[6]) > 0)
    add("se_bnb_bwd", "with SE and two slab jobs", lambda c: c[5] and len(c[6]) == 2)
    add("se_fwd_refused", "C == SE_MAXC + 1", lambda c: c[2] == T["SE_MAXC"] + 1 and c[3] <= T["SE_MAXW"])
    add("se_fwd_refused", "Wd == SE_MAXW + 1", lambda c: c[3] == T["SE_MAXW"] + 1 and c[2] <= T["SE_MAXC"])
    jobs = lambda f: (lambda c: any(f(p, e) for p, e in c[1]))
    add("dw_slab_reduce", "parts below the 16 part groups", jobs(lambda p, e: p < Lt["SLAB_GROUPS"]))
    add("dw_slab_reduce", "parts between 16 and 64", jobs(lambda p, e: Lt["SLAB_GROUPS"] < p < Lt["SLAB_STRIDE"]))
    add("dw_slab_reduce", "a 16-stride tail after the 64-stride loop", jobs(lambda p, e: _slab_loops(p, Lt) == (True, True)))
    add("dw_slab_reduce", "the 64-stride loop without a tail", jobs(lambda p, e: _slab_loops(p, Lt) == (True, False)))
    add("dw_slab_reduce", "elems % DWR_EPB != 0", jobs(lambda p, e: e % T["DWR_EPB"] != 0))
    add("dw_slab_reduce", "elems % DWR_EPB == 0", jobs(lambda p, e: e % T["DWR_EPB"] == 0))
    add("dw_slab_reduce", "elems < DWR_EPB", jobs(lambda p, e: e < T["DWR_EPB"]))
    add("dw_slab_reduce", "elems > DWR_EPB", jobs(lambda p, e: e > T["DWR_EPB"]))
    add("dw_slab_reduce", "one job", lambda c: len(c[1]) == 1)
    add("dw_slab_reduce", "two jobs", lambda c: len(c[1]) == 2)
    add("dw_slab_reduce_refused", "elems % 4 != 0", lambda c: c[2] % 4 != 0 and c[3] % 4 == 0)
    add("dw_slab_reduce_refused", "slab not 16-byte aligned", lambda c: c[2] % 4 == 0 and c[3] % 4 != 0)
    blk, its = T["ELEM_BLOCK"], T["ELEM_ITERS"]
    for e in PLANE:
        for dt in (torch.bfloat16, torch.float16, F32):
            d = str(dt)[6:]
            full = S.aux_vec(dt)
            is_ = lambda c, dt=dt: _plane(c)[0] == dt
            add(e, f"{d} vector path", lambda c, is_=is_: is_(c) and _plane(c)[5] > 1)
            add(e, f"{d} scalar path", lambda c, is_=is_: is_(c) and _plane(c)[5] == 1 and _plane(c)[4] == 0)
            for vec, path in ((full, "vector"), (1, "scalar")):
                span = blk * vec * its
                on = lambda c, is_=is_, vec=vec: is_(c) and _plane(c)[5] == vec
                add(e, f"{d} {path} path, P below one workgroup's span", lambda c, on=on, span=span: on(c) and span - 8 <= _plane(c)[3] < span)
                add(e, f"{d} {path} path, P at one workgroup's span", lambda c, on=on, span=span: on(c) and _plane(c)[3] == span)
                add(e, f"{d} {path} path, P above one workgroup's span", lambda c, on=on, span=span: on(c) and span < _plane(c)[3] <= span + 8)
            add(e, f"{d} view not 16-byte aligned with P % VEC == 0",
                lambda c, is_=is_, full=full: is_(c) and _plane(c)[3] % full == 0 and _plane(c)[4] % full != 0)
        add(e, "N * C beyond 16 bits", lambda c: _plane(c)[1] * _plane(c)[2] > Lt["GRID_Y"])
    add("tail_bwd", "N * C beyond 16 bits in gridDim.y (not the small-plane kernel)",
        lambda c: _plane(c)[1] * _plane(c)[2] > Lt["GRID_Y"] and not _small(c, blk))
    for dt in (torch.bfloat16, torch.float16):
        d = str(dt)[6:]
        is_ = lambda c, dt=dt: _plane(c)[0] == dt
        add("tail_bwd", f"{d} small-plane kernel just below its threshold", lambda c, is_=is_: is_(c) and _small(c, blk) and _plane(c)[3] // 8 == blk - 1)
        add("tail_bwd", f"{d} general kernel at the small-plane threshold", lambda c, is_=is_: is_(c) and _plane(c)[5] == 8 and _plane(c)[3] // 8 == blk)
        add("tail_bwd", f"{d} small-plane kernel, partial last sample group", lambda c, is_=is_: is_(c) and _small(c, blk) and _plane(c)[1] % _nb(c, blk) != 0)
        add("tail_bwd", f"{d} small-plane kernel, 16 samples per group", lambda c, is_=is_: is_(c) and _small(c, blk) and _nb(c, blk) == 16)
        add("tail_bwd", f"{d} small-plane kernel, a second round of the 512-vector loop",
            lambda c, is_=is_: is_(c) and _small(c, blk) and _nb(c, blk) * (_plane(c)[3] // 8) > 2 * blk)
    for e, opts in (("tail_bwd", (False, True)), ("tail_fwd", (None, "identity", "conv"))):
        for o in opts:
            add(e, f"option {o}", lambda c, o=o: c[5] == o)
    for o in (("dy", True), ("dy", False), ("dpool", True)):
        add("relu_bn_bwd_reduce", f"form {o[0]}, g written {o[1]}", lambda c, o=o: c[5:7] == o)
    pairs = ((F32, F32), (F32, torch.bfloat16), (torch.bfloat16, torch.bfloat16), (torch.bfloat16, F32), (F32, torch.float16),
             (torch.float16, torch.float16), (torch.float16, F32))
    lay_off = lambda c: c[6] if len(c) > 6 else 0
    fast = lambda c: c[4] == 3 and c[5] % 8 == 0 and lay_off(c) == 0
    for s, d in pairs:
        add("nthwc_to_ncthw", f"{str(s)[6:]} -> {str(d)[6:]}, vector form", lambda c, s=s, d=d: c[1:3] == (s, d) and fast(c))
        add("nthwc_to_ncthw", f"{str(s)[6:]} -> {str(d)[6:]}, one-point form", lambda c, s=s, d=d: c[1:3] == (s, d) and not fast(c))
    add("nthwc_to_ncthw", "C == 3, P % 8 != 0", lambda c: c[4] == 3 and c[5] % 8 != 0)
    add("nthwc_to_ncthw", "C == 3, P % 8 == 0, source not 16-byte aligned", lambda c: c[4] == 3 and c[5] % 8 == 0 and lay_off(c) != 0)
    add("nthwc_to_ncthw", "C != 3", lambda c: c[4] != 3)
    add("nthwc_to_ncthw", "vector form, P8 below / at / above a 256-thread workgroup",
        lambda c: fast(c) and c[5] // 8 in (255, 256, 257))
    for e, cap in (("all_finite", Lt["ALL_FINITE_CAP"]), ("l2_sumsq", Lt["L2_SUMSQ_CAP"])):
        add(e, "n in one workgroup", lambda c: c[1] <= 2048)
        add(e, "n one past a workgroup", lambda c: c[1] == 2049)
        add(e, "n below the grid cap", lambda c, cap=cap: 2048 < c[1] <= 2048 * cap)
        add(e, "n above the grid cap", lambda c, cap=cap: c[1] > 2048 * cap)
    for k in ("none", "+inf", "-inf", "nan", "-nan-payload"):
        add("all_finite", f"{k} above the grid cap", lambda c, k=k: c[2] == k and c[1] > 2048 * Lt["ALL_FINITE_CAP"])
        add("all_finite", f"{k} below the grid cap", lambda c, k=k: c[2] == k and c[1] <= 2048 * Lt["ALL_FINITE_CAP"])
    for ps in ("first", "last", "mid", "trip2"):
        add("all_finite", f"bad value at {ps}", lambda c, ps=ps: c[2] != "none" and c[3] == ps)
    for m in (None, "random", "zeros"):
        add("l2_sumsq", f"mask {m} above the grid cap", lambda c, m=m: c[2] == m and c[1] > 2048 * Lt["L2_SUMSQ_CAP"])
    for m_ in (1, 2, 8, 63, 255, 256, 257, 1000):
        add("softmax_xent", f"M = {m_}, training", lambda c, m_=m_: c[2] == m_ and c[4])
    add("softmax_xent", "M = 1, inference", lambda c: c[2] == 1 and not c[4])
    add("softmax_xent", "M above one 256-thread round, inference", lambda c: c[2] > 256 and not c[4])
    add("softmax_xent", "N = 1", lambda c: c[1] == 1)
    add("view_mean", "M below / at / above the 128-thread workgroup", lambda c: c[3] in (127, 128, 129))
    add("view_mean", "one view", lambda c: c[2] == 1)
    add("view_mean", "M above 256", lambda c: c[3] > 256)
    return cls


def _small(case, blk):
    """tail_bwd takes the small-plane kernel (elem.hip x3d_tail_bwd)"""
    dt, n, c, P, off, vec = _plane(case)
    return case[0] == "tail_bwd" and dt != F32 and vec == 8 and P // 8 < blk


def _nb(case, blk):
    dt, n, c, P, off, vec = _plane(case)
    return min(4 * blk // (P // 8), n, 16)


def missing_classes(edge, T, Lt):
    return [f"{e}: {name}" for e, name, f in edge_classes(T, Lt) if not any(f(c) for c in edge if c[0] == e)]


def test_tile_constants_are_what_the_table_was_built_for():
    """Every tile size is a `#define NAME <integer>` line of its source (a regular expression on the text; a missing one fails
    by name), with the value shapes.AUX_TILES restates: a retuned tile size needs AUX_EDGE, AUX_TILES and the runners' chain
    lengths (tests/aux_checks.py) looked at again."""
    have = S.aux_tile_defines()
    moved = {k: (v, S.AUX_TILES[k]) for k, v in have.items() if v != S.AUX_TILES[k]}
    assert not moved, "tile sizes (source, shapes.AUX_TILES) differ: " + ", ".join(f"{k} {a} != {b}" for k, (a, b) in moved.items())
    assert set(have) == set(S.AUX_TILES)
    from tests import aux_checks as A
    assert (A.ALL_FINITE_CAP, A.L2_SUMSQ_CAP) == (S.AUX_LITERALS["ALL_FINITE_CAP"], S.AUX_LITERALS["L2_SUMSQ_CAP"])


def test_every_class_has_an_edge_case():
    """Per entry point, one case at least in every class of shape, with the class boundaries taken from the sources' tile sizes."""
    miss = missing_classes(S.AUX_EDGE, S.aux_tile_defines(), S.AUX_LITERALS)
    assert not miss, "AUX_EDGE has no case for:\n  " + "\n  ".join(miss)


def test_no_duplicates_and_every_case_has_a_runner():
    from tests.aux_checks import _AUX_CASES
    assert len(set(S.AUX_EDGE)) == len(S.AUX_EDGE), "duplicate AUX_EDGE entries"
    ids = [S.aux_edge_id(c) for c in S.AUX_EDGE]
    assert len(set(ids)) == len(ids), "two AUX_EDGE cases share an id"
    assert not {c[0] for c in S.AUX_EDGE} - set(_AUX_CASES)
    big = [S.aux_edge_id(c) for c in S.AUX_EDGE if c[0] in PLANE and _plane(c)[1] * _plane(c)[2] * _plane(c)[3] > 10 ** 6]
    assert not big, f"plane-wise edge cases above 1e6 elements: {big}"


def test_the_guard_notices_a_lost_class_and_a_moved_tile():
    """The guard itself: without the cases of any one class it names that class; with a tile size moved (DENSE_MT 4 -> 5, the
    vector span doubled) the classes move with it and the table, built for the old size, loses some."""
    T, Lt = S.aux_tile_defines(), S.AUX_LITERALS
    for e, name, f in edge_classes(T, Lt):
        without = [c for c in S.AUX_EDGE if not (c[0] == e and f(c))]
        assert f"{e}: {name}" in missing_classes(without, T, Lt), f"{e}: {name}"
    assert any("workgroup's span" in m for m in missing_classes(S.AUX_EDGE, dict(T, ELEM_ITERS=8), Lt))
    assert any("SE_MAXW" in m for m in missing_classes(S.AUX_EDGE, dict(T, SE_MAXW=128), Lt))
    assert any("DENSE_B" in m for m in missing_classes(S.AUX_EDGE, dict(T, DENSE_BN=2 ** 20, DENSE_BM=2 ** 20), Lt))


@pytest.mark.parametrize("name", ["DENSE_MT", "ELEM_BLOCK", "DWR_EPB"])
def test_a_changed_define_fails_by_name(tmp_path, name):
    """A scratch copy of the sources with one #define changed (DENSE_MT 4 -> 5 ...) is reported by name; one without the line too."""
    import os
    import re
    import shutil
    src = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "x3d-tf_amd", "csrc")
    for f in S.AUX_TILE_SOURCES:
        shutil.copy(os.path.join(src, f), tmp_path / f)
    fname = next(f for f, names in S.AUX_TILE_SOURCES.items() if name in names)
    text = (tmp_path / fname).read_text()
    (tmp_path / fname).write_text(re.sub(rf"^(#define\s+{name}\s+)(\d+)", lambda m: m.group(1) + str(int(m.group(2)) + 1), text, flags=re.M))
    have = S.aux_tile_defines(str(tmp_path))
    assert have[name] == S.AUX_TILES[name] + 1 and {k for k, v in have.items() if v != S.AUX_TILES[k]} == {name}
    (tmp_path / fname).write_text(re.sub(rf"^#define\s+{name}\s.*$", "", text, flags=re.M))
    with pytest.raises(KeyError, match=name):
        S.aux_tile_defines(str(tmp_path))
