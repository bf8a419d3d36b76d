"""What the launchers and kernels of csrc/roi.hip make of a case of shapes.ROI_EDGE, restated on the host, and the classes of loop
and dispatch forms the table has to contain.  Every line names the line of roi.hip / common.h it follows; the constants are read
from roi.hip's own #define lines (tests/test_roi_head.py fails when one moved away from the values the table was built for).

Outside the class list on purpose: the forward launcher's `if (tc < q) tc = q` cannot be taken while ROI_STAGE / ROI_MAX_HW >= 8
(q <= 8 and H*W <= ROI_MAX_HW give ROI_STAGE / HW >= 8 >= q, so the rounded-down tc is already >= q)."""
import math
import os
import re

ROI = dict(ROI_BLOCK=256, ROI_MAX_HW=1024, ROI_STAGE=8192)      # the values ROI_EDGE was built for
WAVE = 64                                                       # roi.hip: ROI_WAVES = ROI_BLOCK / 64, `b += 64`
DTYPES = ("float32", "bfloat16", "float16")


def roi_defines(csrc=None):
    """{name: value} of ROI's #define lines in roi.hip; KeyError names a missing one"""
    csrc = csrc or os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "x3d-tf_amd", "csrc")
    text = open(os.path.join(csrc, "roi.hip")).read()
    out = {}
    for nm in ROI:
        m = re.search(rf"^#define\s+{nm}\s+(\d+)\b", text, re.M)
        if not m:
            raise KeyError(f"roi.hip: no `#define {nm} <integer>` line")
        out[nm] = int(m.group(1))
    return out


def pick_vec(elem_bytes, extent, *offsets):
    """common.h pick_vec: the widest power-of-two vector of at most 16 bytes that divides `extent` and every pointer's alignment.
    offsets: elements off a 16-byte boundary, one per pointer"""
    v = 16 // elem_bytes
    while v > 1:
        if extent % v == 0 and all((o * elem_bytes) % (v * elem_bytes) == 0 for o in offsets):
            break
        v >>= 1
    return v


def form(case, dtype):
    """the launch of `case` in storage type `dtype` (a name of DTYPES) as a dict"""
    _, (t, h, w), c, k, nb, r, sr, scale_den, boxes, (x_off, y_off, g_off), extra = case
    waves = ROI["ROI_BLOCK"] // WAVE                                   # ROI_WAVES
    hw = h * w
    elem = 4 if dtype == "float32" else 2
    full = 4 if dtype == "float32" else 8                              # x3d_roi_pool_fwd / _bwd: `full = dtype == X3D_F32 ? 4 : 8`
    fwd_vec = pick_vec(elem, t * hw, x_off) >= full                    # x3d_roi_pool_fwd: `vec = pick_vec(.., T * HW, x_raw) >= full`
    bwd_vec = pick_vec(elem, t * hw, y_off, g_off) >= full             # x3d_roi_pool_bwd: `pick_vec(.., T * HW, yraw, g) >= full`
    q = full // math.gcd(hw, full) if fwd_vec else 1                   # `q = vec ? full / roi_gcd(HW, full) : 1`
    tc = ROI["ROI_STAGE"] // hw // q * q                               # `tc = ROI_STAGE / HW / q * q`
    assert tc >= q                                                     # (`if (tc < q) tc = q`: never taken, see the module docstring)
    tc = min(tc, t)                                                    # `if (tc > T) tc = T`
    chunks = -(-t // tc)                                               # roi_pool_fwd_kernel: `for (t0 = 0; t0 < Tn; t0 += tc)`
    last = t - (chunks - 1) * tc
    assert (min(tc, t) * hw) % (full if fwd_vec else 1) == 0 and (last * hw) % (full if fwd_vec else 1) == 0   # `elems % VEC == 0`
    return dict(
        dtype=dtype, hw=hw, elems=t * hw, full=full, fwd_vec=fwd_vec, bwd_vec=bwd_vec, q=q, tc=tc, chunks=chunks, last=last,
        fwd_wrap=fwd_vec and hw % full != 0,                           # a vector of the staging loop crosses a time slice
        bwd_wrap=bwd_vec and hw % full != 0,                           # roi_pool_bwd_kernel: `if (++hw == HW) hw = 0` inside a vector
        pixels=-(-hw // ROI["ROI_BLOCK"]),                             # `hw = threadIdx.x + j * ROI_BLOCK`, j < ROI_PIX
        ragged=hw % ROI["ROI_BLOCK"] != 0,
        fwd_rounds=-(-k // waves),                                     # roi_pool_fwd_kernel: `for (k = wid; k < K; k += ROI_WAVES)`
        bwd_rounds=tuple(-(-min(max(n, 0), k) // waves) for n in nb),  # roi_pool_bwd_kernel: `for (k0 = 0; k0 < nb; k0 += ROI_WAVES)`
        last_round=tuple(min(max(n, 0), k) % waves for n in nb),       # waves with a filled slot in the last round (0: all four)
        bin_trips=-(-(r * r) // WAVE),                                 # `for (b = lane; b < R * R; b += 64)`
        offsets=(x_off, y_off, g_off), nb=tuple(nb), k=k, r=r, sr=sr, thw=(t, h, w), c=c, scale_den=scale_den, boxes=boxes)


def forms(case):
    return {d: form(case, d) for d in DTYPES}


def _all(f, key, want=True):
    return all(f[d][key] == want for d in DTYPES)


def _half(f, key, want=True):
    return all(f[d][key] == want for d in DTYPES[1:])


def _plain(g):
    """nothing but the box rounds leaves its simplest form: one pixel per thread, one bin trip, one chunk, no vector across planes"""
    return g["pixels"] == 1 and g["bin_trips"] == 1 and g["chunks"] == 1 and not g["bwd_wrap"] and not g["fwd_wrap"]


def _default(g):
    return g["k"] == 8 and g["r"] == 7 and g["scale_den"] == 32            # config.py: MAX_BOXES, ROI_XFORM_RESOLUTION, SPATIAL_SCALE_FACTOR


# name -> predicate over forms(case); the rows of the issue's table, each split where it names more than one form
CLASSES = {
    "M plane, shipped default: 16-bit vectors across planes of 49, two box rounds":
        lambda f: f["float32"]["thw"] == (16, 7, 7) and f["float32"]["c"] == 24 and _default(f["float32"]) and f["float32"]["sr"] == 0
        and _half(f, "bwd_wrap") and _half(f, "fwd_wrap") and f["float32"]["q"] == 4 and f["bfloat16"]["q"] == 8
        and max(f["float32"]["bwd_rounds"]) == 2 and f["float32"]["fwd_rounds"] == 2 and 1 in f["float32"]["last_round"],
    "S plane: scalar in every type, two rounds, a sample without boxes":
        lambda f: f["float32"]["thw"] == (13, 5, 5) and _default(f["float32"]) and _all(f, "fwd_vec", False) and _all(f, "bwd_vec", False)
        and sorted(f["float32"]["bwd_rounds"]) == [0, 2],
    "XS plane, sampling_ratio 0: fp32 vectors, 16-bit scalars":
        lambda f: f["float32"]["thw"] == (4, 5, 5) and _default(f["float32"]) and f["float32"]["sr"] == 0 and f["float32"]["bwd_vec"]
        and f["float32"]["fwd_vec"] and _half(f, "fwd_vec", False) and _half(f, "bwd_vec", False) and f["float32"]["fwd_rounds"] == 2,
    "XS plane, sampling_ratio 2":
        lambda f: f["float32"]["thw"] == (4, 5, 5) and _default(f["float32"]) and f["float32"]["sr"] == 2 and f["float32"]["fwd_vec"]
        and _half(f, "fwd_vec", False) and f["float32"]["fwd_rounds"] == 2,
    "L / XL plane, sampling_ratio 0: vectors with H*W % 8 = 4":
        lambda f: f["float32"]["thw"] == (16, 10, 10) and _default(f["float32"]) and f["float32"]["sr"] == 0 and _all(f, "fwd_vec")
        and _all(f, "bwd_vec") and _half(f, "bwd_wrap") and not f["float32"]["bwd_wrap"] and max(f["float32"]["bwd_rounds"]) == 2,
    "L / XL plane, sampling_ratio 2":
        lambda f: f["float32"]["thw"] == (16, 10, 10) and _default(f["float32"]) and f["float32"]["sr"] == 2 and _all(f, "fwd_vec")
        and _half(f, "bwd_wrap") and max(f["float32"]["bwd_rounds"]) == 2,
    "rounds: a second round with one wave at work, all else plain":
        lambda f: all(_plain(g) for g in f.values()) and f["float32"]["bwd_rounds"] == (2, 1) and f["float32"]["last_round"] == (1, 0)
        and f["float32"]["fwd_rounds"] == 2,
    "rounds: sixteen":
        lambda f: 16 in f["float32"]["bwd_rounds"] and f["float32"]["fwd_rounds"] == 16,
    "rounds: num_boxes ends inside a later round of many":
        lambda f: any(r >= 3 and l != 0 for r, l in zip(f["float32"]["bwd_rounds"], f["float32"]["last_round"])),
    "bins: R*R = 64 fills the wave": lambda f: f["float32"]["r"] == 8 and f["float32"]["pixels"] == 1,
    "bins: R*R = 81, two trips": lambda f: f["float32"]["r"] == 9 and f["float32"]["bin_trips"] == 2 and f["float32"]["pixels"] == 1,
    "bins: R*R = 225, four trips": lambda f: f["float32"]["r"] == 15 and f["float32"]["bin_trips"] == 4 and f["float32"]["pixels"] == 1,
    "bins: R*R = 64 on 1024 pixels": lambda f: f["float32"]["r"] == 8 and f["float32"]["hw"] == 1024,
    "bins: R*R = 81 on 1024 pixels": lambda f: f["float32"]["r"] == 9 and f["float32"]["hw"] == 1024,
    "bins: R*R = 225 on 1024 pixels": lambda f: f["float32"]["r"] == 15 and f["float32"]["hw"] == 1024,
    "chunks, q = 1: 8 + 1 slices":
        lambda f: all(g["fwd_vec"] and g["q"] == 1 and (g["tc"], g["chunks"], g["last"]) == (8, 2, 1) for g in f.values()),
    "chunks, q = 4 / 8: fp32 12 + 4, 16-bit 8 + 8":
        lambda f: (f["float32"]["q"], f["float32"]["tc"], f["float32"]["chunks"], f["float32"]["last"]) == (4, 12, 2, 4)
        and all((f[d]["q"], f[d]["tc"], f[d]["chunks"], f[d]["last"]) == (8, 8, 2, 8) for d in DTYPES[1:]),
    "chunks, q = 1 / 2: fp32 9 + 1, 16-bit 8 + 2":
        lambda f: (f["float32"]["q"], f["float32"]["tc"], f["float32"]["chunks"], f["float32"]["last"]) == (1, 9, 2, 1)
        and all((f[d]["q"], f[d]["tc"], f[d]["chunks"], f[d]["last"]) == (2, 8, 2, 2) for d in DTYPES[1:]),
    "chunks, scalar: 8 + 1":
        lambda f: all(not g["fwd_vec"] and g["elems"] % 2 == 1 and (g["tc"], g["chunks"], g["last"]) == (8, 2, 1) for g in f.values()),
    "pixels: 2 per thread, ragged, two box rounds":
        lambda f: f["float32"]["pixels"] == 2 and f["float32"]["ragged"] and max(f["float32"]["bwd_rounds"]) == 2,
    "pixels: 3 per thread, ragged, two box rounds":
        lambda f: f["float32"]["pixels"] == 3 and f["float32"]["ragged"] and max(f["float32"]["bwd_rounds"]) == 2,
    "pixels: 4 per thread, ragged, two box rounds":
        lambda f: f["float32"]["pixels"] == 4 and f["float32"]["ragged"] and max(f["float32"]["bwd_rounds"]) == 2,
    "misaligned: forward x_raw, the extent divisible":
        lambda f: all(g["elems"] % g["full"] == 0 and g["offsets"][0] != 0 and not g["fwd_vec"] for g in f.values()),
    "misaligned: backward yraw alone":
        lambda f: all(g["elems"] % g["full"] == 0 and g["offsets"][1] != 0 and g["offsets"][2] == 0 and not g["bwd_vec"] for g in f.values()),
    "misaligned: backward g alone":
        lambda f: all(g["elems"] % g["full"] == 0 and g["offsets"][1] == 0 and g["offsets"][2] != 0 and not g["bwd_vec"]
                      and g["fwd_vec"] for g in f.values()),
    "geometry: spatial_scale 1/16, boxes off the grid":
        lambda f: f["float32"]["scale_den"] == 16 and f["float32"]["boxes"] == "offgrid",
    "geometry: spatial_scale 1/24 (not a power of two), boxes off the grid":
        lambda f: f["float32"]["scale_den"] == 24 and f["float32"]["boxes"] == "offgrid",
}


def covered(cases):
    """{class name: [labels of the cases that run it]}"""
    fs = [(c[0], forms(c)) for c in cases]
    return {name: [label for label, f in fs if pred(f)] for name, pred in CLASSES.items()}


def missing(cases):
    return [name for name, labels in covered(cases).items() if not labels]


def case_boxes(index, case):
    """boxes [2][K][4] of case number `index` in pixels of its clip: the BOX_KINDS cycle from kind index + 2 (which puts a valid box
    into the second round of the "poison" case)"""
    try:
        from tests import roi_ref
    except ImportError:
        import roi_ref
    _, (t, h, w), c, k, nb, r, sr, scale_den, boxes, _, _ = case
    gen = roi_ref.box_mix if boxes == "grid" else roi_ref.box_mix_offgrid
    return gen(2, k, scale_den * h, scale_den * w, seed=100 + index, first_kind=index + 2)
