"""Every kernel instantiation x3d_pw_bwd can dispatch, as data, and a seeded generator of shapes inside each of them.

tests/shapes.py lists the parity cases of the fused pointwise backward layer by layer, from the BASELINE configurations;
tests/test_dispatch_coverage.py checks "what the configurations dispatch has a case".  This module looks from the other side:
it walks the domain x3d_pw_bwd_supported() admits in dry-run mode (no GPU, nothing launched) and returns every instantiation
(pw_bwd_fused_kernel / pw_bwd_rc_kernel / pw_bwd_wst_kernel / pw_bwd_wsta_kernel <...>) the library can select there -- a
CLASS -- together with the parameter boxes that dispatch to it.  draw() then produces concrete shapes inside one class, so
that a sweep is stratified by class: the classes are discrete tile shapes, uniform sampling of the domain keeps missing them.
tests/test_pw_bwd_classes.py (CPU) checks the enumeration and the generator, tests/test_pw_bwd_classes_gpu.py runs the kernel
tests of tests/test_kernels_gpu.py on two shapes of every class.

The walk knows nothing of the dispatch rules: it asks the library at every (Cin, Cout) of a grid that holds both neighbours of
every multiple of 16 and 32 (in Cin, Cout and Cout + 1: the recomputed-output form carries one extra row), for every launch
form, storage type and row length, and cuts the two channel axes wherever any answer changes.  A box is one cell of that
partition; a draw takes any channel count inside it (checked against the dry run again: a declined draw is counted).
The A/B environment switches of the library are not read here: the enumeration describes the product's dispatch.
"""
import ctypes as C
import functools
import random
from collections import namedtuple

import numpy as np

from tests import shapes as S

CINS = sorted(set(range(8, 513, 8)) | {20, 36, 90, 100} | {16 * k + d for k in range(1, 33) for d in (-1, 1)})
# (Cout + 1 next to a multiple of 16: Cout = 16 k - 2, 16 k)
COUTS = sorted(set(range(8, 225, 8)) | {31, 63, 95, 127, 223} | {16 * k + d for k in range(1, 15) for d in (-2, -1, 1)})
ROWS = (16, 8, 28, 12, 10, 14, 7, 13)                 # row lengths of 8 k, 4 k, 4 k + 2, 7 and odd elements
XROWS = (32, 16, 24, 28, 12, 20, 14, 10, 39, 23, 13, 7)   # input rows of the strided form: gather groups of 4 / 2 / 1, odd rows
_WALK_T, _WALK_H = 8, 2                               # the walk's planes: 16 W points (a multiple of 8 for every W)

# launch forms: (kind, epilogue, tail).  "plain": the conv's raw output is read (S.pw_bwd_struct; tail = folded residual-tail
# backward); "rc": recomputed output (S.pw_bwd_rc_struct; epilogue "store" = the dense shortcut form); "rcs": the strided
# shortcut conv (S.pw_bwd_rc_strided_struct, x_stride = 2)
FORMS = ([("plain", e, t) for e in ("add", "add_strided") for t in (0, 1, 2)] + [("plain", "swish_bwd", 0)] +
         [("rc", e, t) for e in ("add", "add_strided") for t in (0, 1, 2)] + [("rc", "store", 0)] + [("rcs", "store", 0)])

# one box of a class: launch form, storage type, inclusive channel ranges, the row lengths seen to keep the class
Box = namedtuple("Box", "kind dtype epi tail cin cout rows")
# one drawn case: the positional arguments of the kernel tests behind it
Case = namedtuple("Case", "kind dtype shape")


def case_struct(kind, dtype, shape):
    """The argument struct of a case over address-only operands, from the builders of tests/shapes.py."""
    if kind == "plain":
        return S.pw_bwd_struct(shape, dtype)
    if kind == "rc":
        return S.pw_bwd_rc_struct(shape, dtype)
    return S.pw_bwd_rc_strided_struct(shape, dtype)


def case_shape(kind, n, cin, cout, t, h, w, epi, tail):
    """The shape tuple the kernel tests take (h, w: input extents for the strided form)."""
    if kind == "rcs":
        return (n, cin, cout, t, h, w)
    if kind == "plain" and not tail:
        return (n, cin, cout, t, h, w, epi)
    return (n, cin, cout, t, h, w, epi, tail)


def dispatch(kind, dtype, shape):
    """Instantiation name the dry run gives for a case, None where x3d_pw_bwd_supported() declines it."""
    from x3d_tf_amd import hip
    st = case_struct(kind, dtype, shape)
    if not hip.load().x3d_pw_bwd_supported(C.byref(st)):
        return None
    return hip.kernel_name(st)


def _cells(values, breaks):
    """[(lo, hi)] inclusive ranges of walked values between the break positions (a break after index i)."""
    out, lo = [], 0
    for i in range(len(values)):
        if i == len(values) - 1 or breaks[i]:
            out.append((lo, i))
            lo = i + 1
    return out


@functools.lru_cache(maxsize=None)
def enumerate_classes():
    """{kernel instantiation name: [Box, ...]} over the admitted domain of x3d_pw_bwd (dry run, no GPU)."""
    from x3d_tf_amd import hip
    lib = hip.load()
    supported, name_of = lib.x3d_pw_bwd_supported, lib.x3d_pw_kernel_name
    buf = C.create_string_buffer(160)
    ids, mats = {}, {}
    for dtype in S.HALF_DTYPES:
        for kind, epi, tail in FORMS:
            for w in (XROWS if kind == "rcs" else ROWS):
                # one struct per form and row length from the builder; only the two channel counts change along the walk
                h = 2 * _WALK_H if kind == "rcs" else _WALK_H
                st = case_struct(kind, dtype, case_shape(kind, 1, 8, 8, _WALK_T, h, w, epi, tail))
                ref = C.byref(st)
                m = np.full((len(CINS), len(COUTS)), -1, dtype=np.int32)
                for i, cin in enumerate(CINS):
                    st.Cin = cin
                    for j, cout in enumerate(COUTS):
                        st.Cout = cout
                        if supported(ref):
                            rc = name_of(None, None, None, ref, buf, 160)
                            assert rc == 0, (f"x3d_pw_bwd_supported() admits {kind} {epi} tail {tail} {cin}->{cout} W={w} {dtype} but the "
                                             f"dispatch has no kernel for it: {lib.x3d_last_error().decode()}")
                            m[i, j] = ids.setdefault(buf.value.decode(), len(ids))
                if (m >= 0).any():
                    mats[(kind, dtype, epi, tail, w)] = m
    # the channel axes are cut wherever any form's answer changes between two walked neighbours
    bi = np.zeros(len(CINS), dtype=bool)
    bj = np.zeros(len(COUTS), dtype=bool)
    for m in mats.values():
        bi[:-1] |= (m[1:] != m[:-1]).any(axis=1)
        bj[:-1] |= (m[:, 1:] != m[:, :-1]).any(axis=0)
    ci_cells, co_cells = _cells(CINS, bi), _cells(COUTS, bj)
    names = {v: k for k, v in ids.items()}
    rows = {}
    for (kind, dtype, epi, tail, w), m in mats.items():
        for i0, i1 in ci_cells:
            for j0, j1 in co_cells:
                k = int(m[i0, j0])
                assert (m[i0:i1 + 1, j0:j1 + 1] == k).all()
                if k >= 0:
                    rows.setdefault((names[k], kind, dtype, epi, tail, (CINS[i0], CINS[i1]), (COUTS[j0], COUTS[j1])), []).append(w)
    out = {}
    for (name, kind, dtype, epi, tail, cin, cout), ws in sorted(rows.items(), key=lambda kv: (kv[0][0], kv[0][1], kv[0][3], kv[0][4], kv[0][5], kv[0][6])):
        out.setdefault(name, []).append(Box(kind, dtype, epi, tail, cin, cout, tuple(ws)))
    return out


def is_persistent(name):
    """the persistent weights-stationary kernels (pw_bwd_wst.hip / pw_bwd_wsta.hip): one run of tiles per workgroup"""
    return name.startswith(("pw_bwd_wst_kernel", "pw_bwd_wsta_kernel"))


def tile_regime(case):
    """How a persistent kernel cuts a case's 32-point tiles into runs, from x3d_pw_bwd_dw_parts (its grid: one slab per
    workgroup) and ceil(P / 32) * N: the set of
      "few"      no more tiles than workgroups (runs of one tile)
      "cross"    more tiles than workgroups, runs of >= 2 tiles of which one crosses a sample boundary
      "short"    the last workgroup's run is shorter than the others
      "partial"  P % 32 != 0: every sample ends in a partial tile
      "slices"   two slices of row blocks over blockIdx.y (stage 5: more than seven row blocks of input channels)"""
    from x3d_tf_amd import hip
    n, cin, cout, t, h, w = case.shape[:6]
    # (the grid is the slab count; a layer whose Cout * Cin is no multiple of 4 has no slab form and runs the same grid with
    # atomics: asked with Cout rounded up to a multiple of 4, which stays inside the 16-wide k-step that selects the kernel)
    st = case_struct(*case)
    st.Cout = (cout + 3) & ~3
    parts = int(hip.load().x3d_pw_bwd_dw_parts(C.byref(st)))
    assert parts > 0, f"no slab form behind {case}"
    p = t * h * w
    per_sample = -(-p // 32)
    tiles = per_sample * n
    run = -(-tiles // parts)
    got = set()
    if run == 1 and tiles == parts:
        got.add("few")
    if run >= 2 and n >= 2 and per_sample % run:
        got.add("cross")
    if run >= 2 and tiles % run:
        got.add("short")
    if p % 32:
        got.add("partial")
    if -(-cin // 32) > 7:
        got.add("slices")
    return got


# the regimes the two draws of a persistent class aim at (draw 0, draw 1): between them every regime of tile_regime
_AIM = ({"few", "partial"}, {"cross", "short"})

_TS = (1, 2, 3, 4, 5, 8, 13, 16)
_HS = (1, 2, 3, 4, 5, 6, 7, 8, 10, 12, 14, 16, 20, 28)
_XHS = (3, 4, 5, 7, 8, 9, 12, 13, 16, 20, 28, 39)
MAX_POINTS = 3500


def _planes(kind, w):
    """(T, H) choices for a row length: T H W a multiple of 8 (the kernels' domain), at most MAX_POINTS points, and where the
    row allows it at least 256 (several tiles per sample)."""
    wo = (w + 1) // 2 if kind == "rcs" else w
    ok = [(t, h) for t in _TS for h in (_XHS if kind == "rcs" else _HS)
          for p in [t * ((h + 1) // 2 if kind == "rcs" else h) * wo] if p % 8 == 0 and p <= MAX_POINTS]
    big = [(t, h) for t, h in ok if t * ((h + 1) // 2 if kind == "rcs" else h) * wo >= 256]
    return big or ok


def _candidate(box, rng):
    w = rng.choice(box.rows)
    t, h = rng.choice(_planes(box.kind, w))
    n = rng.randint(1, 5)
    cin, cout = rng.randint(*box.cin), rng.randint(*box.cout)
    return Case(box.kind, box.dtype, case_shape(box.kind, n, cin, cout, t, h, w, box.epi, box.tail))


def draw(name, boxes, rng: random.Random, k=0):
    """A concrete case of class `name` inside one of its boxes: (Case, first draws the dry run declined).  Channel counts
    anywhere in the box, N in 1..5, a plane of at most MAX_POINTS points whose row length keeps the class's row form.  k: the
    draw's number within the class -- for the persistent kernels draw k aims at the tile regimes _AIM[k % 2].  A candidate
    the dry run declines (or sends to another class) is counted and redrawn."""
    declined = 0
    for _ in range(50):
        box = rng.choice(boxes)
        case = _candidate(box, rng)
        if is_persistent(name):
            for _ in range(400):          # (the aim is a property of the generator's own choice of N and plane, not a decline)
                if _AIM[k % 2] <= tile_regime(case):
                    break
                case = _candidate(box, rng)
            else:
                raise AssertionError(f"no case of {name} in {box} reaches the tile regimes {_AIM[k % 2]}")
        if dispatch(*case) == name:
            return case, declined
        declined += 1
    raise AssertionError(f"50 draws inside the boxes of {name} were declined by the dry run; last: {case}")


def kernel_calls(case):
    """The kernel tests of tests/test_kernels_gpu.py that check a case against the fp64 restatements:
    [(test function name, positional arguments after `gpu`)]."""
    from x3d_tf_amd import hip
    kind, dtype, shape = case
    if kind == "rc":
        return [("test_pw_bwd_rc", (dtype, shape))]
    if kind == "rcs":
        return [("test_pw_bwd_rc_strided", (dtype, shape))]
    if len(shape) == 8:
        return [("test_pw_bwd_tail", (dtype, shape))]        # (with the slab form inside where the kernel has it)
    calls = [("test_pw_bwd_oracle", (dtype, shape, False))]
    if hip.load().x3d_pw_bwd_dw_parts(C.byref(case_struct(*case))) > 0:
        calls.append(("test_pw_bwd_oracle", (dtype, shape, True)))
    return calls + [("test_pw_bwd_fused", (shape, dtype))]    # dx bit-equal to the x3d_pw_dgrad + x3d_pw_wgrad pair


CLASSES_AT_LEAST = 300   # reachable instantiations when the sweep was written: a narrower dispatch must say so here

SEED = 41000       # the committed seeds: SEED + index of the class in the sorted enumeration
DRAWS = 2


def class_cases(index, name, boxes):
    """The DRAWS committed cases of a class: ([Case, ...], seed, declined first draws)."""
    rng = random.Random(SEED + index)
    got = [draw(name, boxes, rng, k) for k in range(DRAWS)]
    return [c for c, _ in got], SEED + index, sum(min(d, 1) for _, d in got)
