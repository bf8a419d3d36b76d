"""x3d_roi_pool_fwd / x3d_roi_pool_bwd on the GPU against tests/roi_ref.py (fp64), the degenerate form against the classification
head's own launches, and the detection head at model and trainer level.

Inputs are drawn in fp32 and pre-rounded to the storage dtype, boxes lie on the 1/8-pixel grid and spatial_scale is 1/32, so
kernel and reference see the same geometry and only the fp32 accumulation separates them.  (test_roi_edge's geometry cases leave
the grid; its docstring says why the bounds hold there too.)

test_parity sweeps features (C, K, R, sampling_ratio) over five planes; test_roi_edge runs shapes.ROI_EDGE, one case per loop and
dispatch class of csrc/roi.hip as tests/roi_classes.py restates them (profiles/roi_classes_mi355x.txt: the measured error / bound
per class, and which cases fail under which seeded wrong value).

Bounds (derived, not fitted).  u = 2^-24, the fp32 unit roundoff.
  forward: a pooled value is a mean of gh*gw samples of four products each, of a map that is a mean over T of relu(s*x + t):
      |err| <= 4 * (T + 4*gh*gw + 8) * u * max|term|,  max|term| = max over the plane of |s*x| + |t|
      (a relu value is bounded by it, and so is the rounding of s*x + t where the two cancel).
  backward: dM/T sums K boxes of dpooled * weight (weight <= 1) the same way, so max|term| = sum_k |dpooled[k][c]| / T, and the stored
      g is that value rounded to the storage dtype: one unit in the last place of the dtype on top.
  sums: 256 threads add 4 * VEC products each and meet in a 6-step wave tree and a 4-term sum: 15 roundings, < 1e-6 of sum |terms|."""
import itertools

import numpy as np
import pytest
import torch

from tests import roi_classes, roi_ref
from tests.shapes import ROI_EDGE, roi_edge_id
from x3d_tf_amd import hip, ops

pytestmark = pytest.mark.gpu

U = 2.0 ** -24
SCALE = 1.0 / 32
DTYPES = [torch.float32, torch.bfloat16, torch.float16]
SHAPES = [(1, 1, 1), (4, 7, 7), (3, 5, 3), (2, 8, 10), (1, 32, 32)]
COMBOS = list(itertools.product([1, 3, 24], [1, 3], [1, 2, 7], [0, 2]))    # C, K, R, sampling_ratio


def _ulp(v, dtype):
    """unit in the last place of |v| in dtype (fp64 tensor in, fp64 out)"""
    mant, emin = {torch.float32: (23, -126), torch.bfloat16: (7, -126), torch.float16: (10, -14)}[dtype]
    e = torch.floor(torch.log2(v.abs().clamp_min(2.0 ** -140))).clamp_min(emin)
    return torch.exp2(e - mant)


def _draw(c, t, h, w, dtype, seed, n=2):
    """x rounded to the storage dtype; scale_shift with t well above the noise of s*x so that few s*x + t sit at zero"""
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(n, c, t, h, w, generator=g).to(dtype)
    ss = torch.stack([(0.5 + torch.rand(c, generator=g)) * torch.where(torch.rand(c, generator=g) < 0.25, -1.0, 1.0),
                      0.25 + torch.rand(c, generator=g)], dim=1).contiguous()
    return x, ss


def _num_boxes(i, k):
    return [k, 0] if i % 2 == 0 else [k - 1, k]


def _counts(boxes, num_boxes, h, w, r, sr, scale=SCALE):
    """gh*gw per row (0 for an empty slot)"""
    n, k = boxes.shape[:2]
    out = np.zeros(n * k)
    for a in range(n):
        for b in range(k):
            geom = roi_ref.box_geometry(boxes[a, b], b < num_boxes[a], scale, h, w, r, sr)
            if geom is not None:
                out[a * k + b] = geom[4] * geom[5]
    return out


def _run_fwd(gpu, x, ss, boxes, nb, r, sr, with_argmax=True):
    n, c = x.shape[:2]
    k = boxes.shape[1]
    pooled = torch.full((n * k, c), 7.0, device=gpu)
    argmax = torch.full((n * k, c), 255, dtype=torch.uint8, device=gpu) if with_argmax else None
    ops.roi_pool_fwd(x.to(gpu), ss.to(gpu), torch.from_numpy(boxes).to(gpu), torch.tensor(nb, dtype=torch.int32, device=gpu),
                     pooled, argmax, resolution=r, sampling_ratio=sr, spatial_scale=SCALE)
    return pooled, argmax


def _run_bwd(gpu, dp, argmax, x, ss, boxes, nb, r, sr):
    c = x.shape[1]
    g = torch.full(x.shape, 3.0, dtype=x.dtype, device=gpu)
    sums = torch.zeros(c, 2, dtype=torch.float64, device=gpu)
    ops.roi_pool_bwd(dp.to(gpu), argmax, torch.from_numpy(boxes).to(gpu), torch.tensor(nb, dtype=torch.int32, device=gpu),
                     x.to(gpu), ss.to(gpu), g, sums, resolution=r, sampling_ratio=sr, spatial_scale=SCALE)
    return g, sums


GUARD = 64                    # elements on each side of a guarded view: a multiple of 16 bytes in every type
SUMS0 = (3.0, -2.0)           # what the edge cases' sums hold before the backward adds to them


def _guarded(gpu, shape, dtype, fill, off=0):
    """(view of `shape`, the whole allocation, (lo, hi)): the view starts `off` elements past a 16-byte boundary inside an
    allocation filled with `fill`, GUARD elements clear of either end"""
    numel = int(np.prod(shape))
    buf = torch.full((GUARD + off + numel + GUARD,), fill, dtype=dtype, device=gpu)
    lo = GUARD + off
    assert (buf.data_ptr() + GUARD * buf.element_size()) % 16 == 0
    return buf[lo:lo + numel].view(shape), buf, (lo, lo + numel)


def _bands_intact(buf, span, fill):
    lo, hi = span
    band = torch.cat([buf[:lo], buf[hi:]])
    return bool(torch.isnan(band).all()) if fill != fill else bool((band == fill).all())


def _place(gpu, t, off):
    """`t` on the device, `off` elements past a 16-byte boundary"""
    view, _, _ = _guarded(gpu, tuple(t.shape), t.dtype, 0, off)
    view.copy_(t)
    return view


class _Edge:
    """how an edge case runs the two launches: operands at element offsets, outputs as guarded views pre-filled with NaN / 255,
    sums from SUMS0.  fwd / bwd return what _run_fwd / _run_bwd do (sums: the increment) after checking the guard bands."""

    def __init__(self, gpu, x, offsets, scale):
        self.gpu, self.scale = gpu, scale
        self.x_off, self.y_off, self.g_off = offsets
        self.x_fwd = _place(gpu, x, self.x_off)
        self.x_bwd = self.x_fwd if self.y_off == self.x_off else _place(gpu, x, self.y_off)

    def fwd(self, x, ss, boxes, nb, r, sr):
        gpu = self.gpu
        n, c, k = x.shape[0], x.shape[1], boxes.shape[1]
        pooled, pbuf, pspan = _guarded(gpu, (n * k, c), torch.float32, float("nan"))
        argmax, abuf, aspan = _guarded(gpu, (n * k, c), torch.uint8, 255)
        ops.roi_pool_fwd(self.x_fwd, ss.to(gpu), torch.from_numpy(boxes).to(gpu), torch.tensor(nb, dtype=torch.int32, device=gpu),
                         pooled, argmax, resolution=r, sampling_ratio=sr, spatial_scale=self.scale)
        assert _bands_intact(pbuf, pspan, float("nan")), "pooled: written outside its rows"
        assert _bands_intact(abuf, aspan, 255), "argmax: written outside its rows"
        assert not torch.isnan(pooled).any(), "pooled: an element was not written"
        return pooled, argmax

    def bwd(self, dp, argmax, x, ss, boxes, nb, r, sr):
        gpu = self.gpu
        c = x.shape[1]
        g, gbuf, gspan = _guarded(gpu, tuple(x.shape), x.dtype, float("nan"), self.g_off)
        sums0 = torch.tensor([SUMS0] * c, dtype=torch.float64, device=gpu)
        sums = sums0.clone()
        ops.roi_pool_bwd(dp.to(gpu), argmax.contiguous(), torch.from_numpy(boxes).to(gpu), torch.tensor(nb, dtype=torch.int32, device=gpu),
                         self.x_bwd, ss.to(gpu), g, sums, resolution=r, sampling_ratio=sr, spatial_scale=self.scale)
        assert _bands_intact(gbuf, gspan, float("nan")), "g: written outside its planes"
        assert not torch.isnan(g).any(), "g: an element was not written"
        return g, sums - sums0


def _g_elementwise(gd, dtype, dp, am, boxes, nb, xn, ssn, r, sr, scale, valid, cnt):
    """g (fp64 copy `gd` of the kernel's) against the fp64 reference rounded to the storage type, element by element: one unit in the
    last place plus the backward bound of the module docstring; an element whose s*x + t lies within 2^-20 |t| of zero may take either
    side of the ReLU.  Returns (ok, ambiguous) masks and the worst error / bound outside the ambiguous elements."""
    n, c, t = xn.shape[:3]
    k = boxes.shape[1]
    dpn = dp.double().numpy()
    ref_g, z = roi_ref.backward(dpn, am, boxes, nb, xn, ssn, r, sr, scale)
    ref_g, z = torch.from_numpy(ref_g), torch.from_numpy(z)
    dpa = dp.double().abs().view(n, k, c) * torch.from_numpy(valid).view(n, k, 1)
    bterm = (dpa.sum(1) / t).view(n, c, 1, 1, 1)
    bbound = 4 * (k + 4 * float(cnt.max()) + 8) * U * bterm
    unmasked = torch.where(z > 0, ref_g, torch.zeros_like(ref_g))
    open_relu = np.stack([0 * ssn[:, 0], 1 + 0 * ssn[:, 1]], 1)
    full = torch.from_numpy(roi_ref.backward(dpn, am, boxes, nb, xn, open_relu, r, sr, scale)[0])          # the gradient with every ReLU open

    def close(ref):
        rr = ref.float().to(dtype).double()
        return (gd - rr).abs() <= _ulp(rr, dtype) + bbound

    amb = z.abs() <= 2.0 ** -20 * torch.from_numpy(ssn[:, 1]).abs().view(1, c, 1, 1, 1)
    ok = torch.where(amb, close(full) | (gd == 0), close(unmasked))
    rr = unmasked.float().to(dtype).double()
    ratio = ((gd - rr).abs() / (_ulp(rr, dtype) + bbound))[~amb]
    return ok, amb, float(ratio.max()) if ratio.numel() else 0.0


def _parity_case(gpu, dtype, thw, x, ss, boxes, nb, r, sr, dp, what, scale=SCALE, edge=None, poison=False):
    """one (shape, C, K, R, sampling_ratio): forward against roi_ref, the kernel's argmax within the bound of the reference maximum,
    and the backward teacher-forced on the kernel's argmax, with the bounds of the module docstring.  edge: an _Edge that runs the
    launches (None: _run_fwd / _run_bwd).  poison: the backward once more with argmax bytes >= R*R in some valid rows, against the
    reference without those rows.  Returns (ambiguous, total, {worst error / bound of the forward, of g, of the sums})."""
    t, h, w = thw
    n, c = x.shape[:2]
    k = boxes.shape[1]
    if edge is None:
        pooled, argmax = _run_fwd(gpu, x, ss, boxes, nb, r, sr)
    else:
        pooled, argmax = edge.fwd(x, ss, boxes, nb, r, sr)
    xn, ssn = x.double().numpy(), ss.double().numpy()
    ref_pooled, ref_bins, _, valid = roi_ref.forward(xn, ssn, boxes, nb, r, sr, scale)
    cnt = _counts(boxes, nb, h, w, r, sr, scale)
    term = (np.abs(ssn[None, :, 0, None, None, None] * xn) + np.abs(ssn[None, :, 1, None, None, None])).max(axis=(2, 3, 4))  # [N][C]
    bound = 4 * (t + 4 * cnt[:, None] + 8) * U * np.repeat(term, k, axis=0)                                                 # [N*K][C]
    got, am = pooled.cpu().double().numpy(), argmax.cpu().numpy().astype(np.int64)
    err = np.abs(got - ref_pooled)
    worst = {"fwd": float((err / bound).max())}
    print(f"{what}: fwd max err / bound = {worst['fwd']:.3f}")
    assert (err <= bound).all(), f"{what}: pooled off by {err.max():.3e} (bound {bound[err > bound].min():.3e})"
    assert (got[~valid] == 0).all() and (am[~valid] == 0).all(), f"{what}: an empty slot is not zero"
    assert (am < r * r).all()
    at_kernel = np.take_along_axis(ref_bins, am[:, :, None], axis=2)[:, :, 0]
    assert (at_kernel >= ref_pooled - bound)[valid].all(), f"{what}: the kernel's argmax is not a maximal bin"
    # backward, teacher-forced
    yd = x.double()
    ambiguous = total = 0
    worst["g"] = worst["sums"] = 0.0

    def backward(argmax_dev, am_ref, dp_ref, label):
        nonlocal ambiguous, total
        if edge is None:
            g, sums = _run_bwd(gpu, dp, argmax_dev, x, ss, boxes, nb, r, sr)
        else:
            g, sums = edge.bwd(dp, argmax_dev, x, ss, boxes, nb, r, sr)
        gd = g.cpu().double()
        ok, amb, ratio = _g_elementwise(gd, dtype, dp_ref, am_ref, boxes, nb, xn, ssn, r, sr, scale, valid, cnt)
        ambiguous += int(amb.sum())
        total += amb.numel()
        worst["g"] = max(worst["g"], ratio)
        assert ok.all(), f"{label}: {int((~ok).sum())} of {ok.numel()} elements of g out of bound, first {torch.nonzero(~ok)[0].tolist()}"
        own = torch.stack([gd.sum(dim=(0, 2, 3, 4)), (gd * yd).sum(dim=(0, 2, 3, 4))], 1)
        scl = torch.stack([gd.abs().sum(dim=(0, 2, 3, 4)), (gd * yd).abs().sum(dim=(0, 2, 3, 4))], 1)
        serr = (sums.cpu() - own).abs()
        worst["sums"] = max(worst["sums"], float((serr / (1e-6 * scl).clamp_min(1e-300))[scl > 0].max()) if (scl > 0).any() else 0.0)
        assert (serr <= 1e-6 * scl).all(), f"{label}: sums {sums.cpu()} vs {own}"
        return gd

    backward(argmax, am, dp, what)
    if poison:
        # "an argmax byte >= R*R is ignored": R*R and 255 alternately in the first valid row and every valid row of a later round
        rows = [i for i in np.nonzero(valid)[0] if i % k >= 4]
        assert rows, "no valid box in a later round: not the case to poison"
        rows = [int(np.nonzero(valid)[0][0])] + [int(i) for i in rows]
        bad = argmax.clone()
        am_ref, dp_ref = am.copy(), dp.clone()
        for j, row in enumerate(rows):
            bad[row] = r * r if j % 2 == 0 else 255
            am_ref[row] = 0
            dp_ref[row] = 0.0
        gd = backward(bad, am_ref, dp_ref, what + f" (argmax of rows {rows} past R*R)")
        assert (gd != 0).any()
    return ambiguous, total, worst


@pytest.mark.parametrize("thw", SHAPES, ids=lambda s: "x".join(map(str, s)))
@pytest.mark.parametrize("dtype", DTYPES, ids=lambda d: str(d).split(".")[-1])
def test_parity(gpu, dtype, thw):
    """forward against roi_ref, the kernel's argmax within the bound of the reference maximum, and the backward teacher-forced on
    the kernel's argmax, for every (C, K, R, sampling_ratio)"""
    t, h, w = thw
    ambiguous = total = 0
    for i, (c, k, r, sr) in enumerate(COMBOS):
        x, ss = _draw(c, t, h, w, dtype, seed=1000 + i)
        boxes = roi_ref.box_mix(2, k, 32 * h, 32 * w, seed=i, first_kind=i)
        nb = _num_boxes(i, k)
        what = f"C={c} K={k} R={r} sr={sr} num_boxes={nb}"
        dp = torch.randn(2 * k, c, generator=torch.Generator().manual_seed(2000 + i))
        a, n, _ = _parity_case(gpu, dtype, thw, x, ss, boxes, nb, r, sr, dp, what)
        ambiguous += a
        total += n
    assert ambiguous < 0.01 * total, f"{ambiguous} of {total} elements within 2^-20 |t| of the ReLU's zero"


@pytest.mark.parametrize("case", ROI_EDGE, ids=roi_edge_id)
@pytest.mark.parametrize("dtype", DTYPES, ids=lambda d: str(d).split(".")[-1])
def test_roi_edge(gpu, dtype, case):
    """shapes.ROI_EDGE: one case per loop and dispatch class of roi.hip (tests/roi_classes.py names them), with test_parity's checks
    and bounds unchanged, and on top of them
      guard bands: pooled, argmax and g are views into larger allocations pre-filled with NaN / 255; the bands on both sides come
          back untouched and no element of the views keeps its pre-fill;
      sums: they start from SUMS0 and the check is on the increment;
      exact ties (R = 9, 15): a plane whose ReLU is closed everywhere gives pooled == 0 and argmax == 0 for every box -- bin 0 wins
          among R*R equal bins, across the lane's trips and across the wave -- and the backward g == 0 and the sums untouched;
      ignored argmax bytes (the "poison" case): rows whose argmax is R*R or 255 drop out of the backward.
    Geometry off the exact grid (spatial_scale 1/24 rounded to fp32, boxes not quantised) needs no new term in the bounds: kernel and
    reference do the geometry in fp64 from the same fp32 inputs in the same order, so they differ at most where the device contracts
    a multiply-add: the last bit of a sample coordinate, 2^-53 relative against the 2^-24 the bounds are written in.  The reference
    receives spatial_scale as the kernel does, rounded to fp32."""
    label, thw, c, k, nb, r, sr, den, kind, offsets, extra = case
    i = ROI_EDGE.index(case)
    t, h, w = thw
    nb = list(nb)
    scale = float(np.float32(1.0 / den))
    x, ss = _draw(c, t, h, w, dtype, seed=3000 + i)
    boxes = roi_classes.case_boxes(i, case)
    dp = torch.randn(2 * k, c, generator=torch.Generator().manual_seed(4000 + i))
    edge = _Edge(gpu, x, offsets, scale)
    what = f"{label} {str(dtype).split('.')[-1]}"
    ambiguous, total, worst = _parity_case(gpu, dtype, thw, x, ss, boxes, nb, r, sr, dp, what, scale=scale, edge=edge,
                                           poison=extra == "poison")
    print(f"{what}: worst error / bound: fwd {worst['fwd']:.3f}  g {worst['g']:.3f}  sums {worst['sums']:.3f}")
    assert ambiguous <= 0.01 * total, f"{ambiguous} of {total} elements within 2^-20 |t| of the ReLU's zero"
    if r in (9, 15):
        closed = ss.clone()
        closed[:, 1] = -(ss[:, 0].abs() * float(x.float().abs().max()) + 1.0)          # s*x + t < 0 everywhere
        assert bool(((closed[:, 0].view(1, c, 1, 1, 1) * x.float() + closed[:, 1].view(1, c, 1, 1, 1)) < 0).all())
        pooled, argmax = edge.fwd(x, closed, boxes, nb, r, sr)
        assert roi_ref.forward(x.double().numpy(), closed.double().numpy(), boxes, nb, r, sr, scale)[3].any()
        assert bool((pooled == 0).all()) and bool((argmax == 0).all()), f"{what}: a tie among zero bins did not go to bin 0"
        g, dsums = edge.bwd(dp, argmax, x, closed, boxes, nb, r, sr)
        assert bool((g == 0).all()) and bool((dsums == 0).all()), f"{what}: a closed ReLU let a gradient through"


@pytest.mark.parametrize("thw", [(4, 7, 7), (2, 8, 10)], ids=lambda s: "x".join(map(str, s)))
@pytest.mark.parametrize("dtype", DTYPES, ids=lambda d: str(d).split(".")[-1])
def test_degenerate_form_is_the_old_head(gpu, dtype, thw):
    """R = 1, sampling_ratio = 0, K = 1, every box the full frame: the samples land on the pixel centres and the two launches are
    x3d_pool_fwd and x3d_relu_bn_bwd_reduce(dpool) up to the order of the fp32 sums"""
    t, h, w = thw
    c, n, p = 24, 2, t * h * w
    x, ss = _draw(c, t, h, w, dtype, seed=5)
    boxes = np.tile(np.array([0, 0, 32 * w, 32 * h], dtype=np.float32), (n, 1, 1))
    pooled, argmax = _run_fwd(gpu, x, ss, boxes, [1, 1], 1, 0)
    old = ops.pool_fwd(x.to(gpu), ss.to(gpu), torch.empty(n, c, device=gpu))
    assert ((pooled.double() - old.double()).abs() <= p * U * old.double().abs()).all()
    dp = torch.randn(n, c, generator=torch.Generator().manual_seed(6))
    g, sums = _run_bwd(gpu, dp, argmax, x, ss, boxes, [1, 1], 1, 0)
    g_old = torch.empty_like(g)
    sums_old = torch.zeros_like(sums)
    ops.relu_bn_bwd_reduce(None, dp.to(gpu), x.to(gpu), ss.to(gpu), g_old, sums_old)
    gd, god = g.double(), g_old.double()
    assert ((gd - god).abs() <= _ulp(god, dtype)).all()
    scale = torch.stack([god.abs().sum(dim=(0, 2, 3, 4)), (god * x.to(gpu).double()).abs().sum(dim=(0, 2, 3, 4))], 1)
    # (the stored g may differ by a unit in the last place: the sums of p such values by that share, plus the 1e-6 of their order)
    ulp_rel = {torch.float32: 2.0 ** -23, torch.bfloat16: 2.0 ** -7, torch.float16: 2.0 ** -10}[dtype]
    assert ((sums - sums_old).abs() <= (ulp_rel + 2e-6) * scale).all()


@pytest.mark.parametrize("dtype", DTYPES, ids=lambda d: str(d).split(".")[-1])
def test_reproducible(gpu, dtype):
    x, ss = _draw(24, 4, 7, 7, dtype, seed=9)
    boxes = roi_ref.box_mix(2, 3, 224, 224, seed=3)
    runs = []
    for _ in range(2):
        pooled, argmax = _run_fwd(gpu, x, ss, boxes, [3, 2], 7, 0)
        dp = torch.randn(6, 24, generator=torch.Generator().manual_seed(4))
        g, _ = _run_bwd(gpu, dp, argmax, x, ss, boxes, [3, 2], 7, 0)
        runs.append((pooled.cpu(), argmax.cpu(), g.cpu()))
    for a, b in zip(*runs):
        assert torch.equal(a.view(torch.uint8), b.view(torch.uint8))
    # the shipped K = 8 on M's plane (two box rounds, 16-bit vectors across planes) with two bin trips
    x, ss = _draw(24, 16, 7, 7, dtype, seed=10)
    boxes = roi_ref.box_mix(2, 8, 224, 224, seed=6)
    runs = []
    for _ in range(2):
        pooled, argmax = _run_fwd(gpu, x, ss, boxes, [8, 5], 9, 0)
        dp = torch.randn(16, 24, generator=torch.Generator().manual_seed(7))
        g, _ = _run_bwd(gpu, dp, argmax, x, ss, boxes, [8, 5], 9, 0)
        runs.append((pooled.cpu(), argmax.cpu(), g.cpu()))
    for a, b in zip(*runs):
        assert torch.equal(a.view(torch.uint8), b.view(torch.uint8))


def test_outputs_left_alone(gpu):
    """argmax == NULL is not written (guard bytes on both sides of pooled stay), and a refused call writes nothing"""
    x, ss = _draw(3, 4, 7, 7, torch.float32, seed=11)
    boxes = roi_ref.box_mix(2, 3, 224, 224, seed=5)
    d_boxes, d_nb = torch.from_numpy(boxes).to(gpu), torch.tensor([3, 1], dtype=torch.int32, device=gpu)
    guard = 64
    buf = torch.full((guard + 6 * 3 + guard,), -5.0, device=gpu)
    pooled = buf[guard:guard + 18].view(6, 3)
    ops.roi_pool_fwd(x.to(gpu), ss.to(gpu), d_boxes, d_nb, pooled, None, resolution=2, sampling_ratio=2, spatial_scale=SCALE)
    ref, _, _, _ = roi_ref.forward(x.double().numpy(), ss.double().numpy(), boxes, [3, 1], 2, 2, SCALE)
    assert (buf[:guard] == -5.0).all() and (buf[guard + 18:] == -5.0).all()
    assert np.abs(pooled.cpu().double().numpy() - ref).max() < 1e-4
    # refused by the library itself (the wrapper's own checks bypassed): R = 16, then H*W > 1024
    xg, sg = x.to(gpu), ss.to(gpu)
    am = torch.full((6, 3), 9, dtype=torch.uint8, device=gpu)
    before = buf.clone()
    g = torch.full(x.shape, 3.0, device=gpu)
    sums = torch.full((3, 2), 2.0, dtype=torch.float64, device=gpu)
    for (hh, ww, r) in ((7, 7, 16), (7, 7, 0), (33, 32, 7)):
        with pytest.raises(hip.X3DHipError):
            hip.call("x3d_roi_pool_fwd", xg.data_ptr(), sg.data_ptr(), d_boxes.data_ptr(), d_nb.data_ptr(), pooled.data_ptr(),
                     am.data_ptr(), 2, 3, 4, hh, ww, 3, r, 0, SCALE, hip.F32)
        with pytest.raises(hip.X3DHipError):
            hip.call("x3d_roi_pool_bwd", pooled.data_ptr(), am.data_ptr(), d_boxes.data_ptr(), d_nb.data_ptr(), xg.data_ptr(),
                     sg.data_ptr(), g.data_ptr(), sums.data_ptr(), 2, 3, 4, hh, ww, 3, r, 0, SCALE, hip.F32)
    torch.cuda.synchronize()
    assert torch.equal(buf, before) and (am == 9).all() and (g == 3.0).all() and (sums == 2.0).all()


# ---- model level ------------------------------------------------------------------------------------------------------------
BASE = ["DATA.TEMP_DURATION", 4, "TEST.NUM_SPATIAL_CROPS", 1, "TEST.NUM_TEMPORAL_VIEWS", 1, "NETWORK.NUM_CLASSES", 11]
KB = 3
DET = ["DETECTION.ENABLE", True, "DETECTION.MAX_BOXES", KB]


def _setup(over):
    import x3d_tf_amd as x
    from x3d_tf_amd.params import init_params, randomize_bn_
    cfg = x.get_config("XS", BASE + over)
    arch = x.build_arch(cfg)
    return cfg, arch, randomize_bn_(init_params(arch, seed=3), seed=4)


def _model(cfg, params, gpu, dtype=torch.float32):
    from x3d_tf_amd.model import X3D
    m = X3D(cfg, dtype=dtype, device=gpu, seed=0)
    m.load_state_dict(params)
    return m


def _clip_boxes(n, size, seed):
    """boxes [n][KB][4] in pixels of a size x size clip: an inside box, a box beyond the frame, the full frame"""
    return roi_ref.box_mix(n, KB, size, size, seed=seed)[:, :, :].copy()


def _rel_l2(a, b):
    return float((a.double() - b.double()).norm() / b.double().norm().clamp_min(1e-30))


# MAX_BOXES 3 on a 64^2 clip (conv5 map 4x2x2), and the shipped MAX_BOXES = 8 -- the section's default, not set here -- on XS's
# 4 x 128^2 (conv5 map 4x4x4: two box rounds, num_boxes [5, 0]) in the three storage types
MODEL_STEPS = [("k3-64", ["DETECTION.ENABLE", True, "DETECTION.MAX_BOXES", KB], 64, [2, 0], torch.float32),
               ("default-128-fp32", ["DETECTION.ENABLE", True], 128, [5, 0], torch.float32),
               ("default-128-bf16", ["DETECTION.ENABLE", True], 128, [5, 0], torch.bfloat16),
               ("default-128-fp16", ["DETECTION.ENABLE", True], 128, [5, 0], torch.float16)]


@pytest.mark.parametrize("multi", [False, True], ids=["softmax", "sigmoid"])
@pytest.mark.parametrize("step", MODEL_STEPS, ids=lambda c: c[0])
def test_model_step_matches_the_head_restated_in_fp64(gpu, multi, step):
    """one forward_backward of the XS model with boxes: the trunk is the plan's own (c5_raw, bn5.ss), the head -- roi_ref pooling on
    the kernel's argmax, fc1, dropout, fc2, the loss as a mean over the filled slots -- is restated in torch fp64; limits as the
    existing head tests' (loss 1e-5, probabilities 1e-4, dlogits 1e-6 of their maximum, gradients 1e-3 relative L2).
    16-bit storage: fc1, fc2 and the loss are fp32 whatever the storage type and the trunk is taken from the plan, so those limits
    hold as they are (dpooled, the last fp32 quantity, at the gradients' 1e-3).  g5 is stored in the storage type, whose rounding
    alone exceeds 1e-3 in bf16: it is compared element by element as the kernel test does -- the fp64 reference of the plan's own
    dpooled rounded to the storage type, one unit in the last place plus the backward bound."""
    _, over, s, nb, dtype = step
    cfg, arch, params = _setup(over + (["DATA.MULTI_LABEL", True] if multi else []))
    kb = cfg.DETECTION.MAX_BOXES
    assert kb == (KB if s == 64 else 8)
    n, t, classes = 2, 4, arch.num_classes
    rows = n * kb
    g = torch.Generator().manual_seed(1)
    clips = torch.randn(n, t, s, s, 3, generator=g)
    boxes = roi_ref.box_mix(n, kb, s, s, seed=2)
    valid = (torch.arange(kb).view(1, kb) < torch.tensor(nb).view(n, 1)).reshape(-1)       # the filled slots
    if multi:
        labels = (torch.rand(n, kb, classes, generator=g) < 0.3).float()
    else:
        labels = torch.randint(0, classes, (n, kb), generator=g)
        labels[1, 2] = -5                                   # an empty slot's label is not used
    mask = (torch.rand(rows, arch.fc1_out, generator=g) >= arch.dropout_rate).float()
    m = _model(cfg, params, gpu, dtype)
    m.set_dropout_mask(mask)
    pl = m.forward_backward(clips.to(gpu), labels, boxes=torch.from_numpy(boxes), num_boxes=nb)
    torch.cuda.synchronize()
    assert pl.rows == rows and tuple(pl.pooled.shape) == (rows, arch.conv5_out) and tuple(pl.dlogits.shape) == (rows, classes)
    c5, ss = pl.c5_raw.cpu().double().numpy(), pl.bn5.ss.cpu().double().numpy()
    am = pl.roi_argmax.cpu().numpy().astype(np.int64)
    h5 = s // 32
    _, bins, _, ref_valid = roi_ref.forward(c5, ss, boxes, nb, 7, 0, SCALE)
    # (a filled slot with a degenerate box pools zeros and still counts: the fifth of the default case is zero-width)
    assert not ref_valid[~valid.numpy()].any() and int(ref_valid.sum()) == (2 if s == 64 else 4)
    pooled = torch.from_numpy(np.take_along_axis(bins, am[:, :, None], 2)[:, :, 0]).requires_grad_(True)
    assert (pl.pooled.cpu().double() - pooled.detach()).abs().max().item() <= 1e-4
    w1 = params["fc1/kernel"].double().reshape(arch.fc1_out, arch.conv5_out).requires_grad_(True)
    w2 = params["fc2/kernel"].double().reshape(classes, arch.fc1_out).requires_grad_(True)
    b2 = params["fc2/bias"].double().requires_grad_(True)
    scale = 1.0 / (1.0 - arch.dropout_rate) if arch.dropout_rate > 0 else 1.0
    z = (torch.relu(pooled @ w1.T) * (mask.double() * scale if arch.dropout_rate > 0 else 1.0)) @ w2.T + b2
    z.retain_grad()
    if multi:
        per_row = (z.clamp(min=0) - z * labels.double().view(rows, classes) + torch.log1p(torch.exp(-z.abs()))).mean(1)
        probs = torch.sigmoid(z)
    else:
        per_row = torch.nn.functional.cross_entropy(z, labels.view(rows).clamp(min=0), reduction="none")
        probs = torch.softmax(z, 1)
    loss = per_row[valid].sum() / int(valid.sum())
    loss.backward()
    got_loss = pl.loss_rows.double().sum().item() / rows
    print(f"loss {got_loss} vs {loss.item()}")
    assert abs(got_loss - loss.item()) <= 1e-5
    assert (pl.probs.cpu().double() - probs.detach()).abs().max().item() <= 1e-4
    dl = pl.dlogits.cpu().double()
    assert (dl - z.grad).abs().max().item() <= 1e-6 * z.grad.abs().max().item() + 1e-30
    assert (dl[~valid] == 0).all() and (dl[:2] != 0).any()
    dpk = pl.backward.dpooled.cpu().double()
    e = _rel_l2(dpk, pooled.grad)
    assert e < 1e-3, f"dpooled: relative L2 error {e:.3e}"
    for name, ref in (("fc1/kernel", w1.grad), ("fc2/kernel", w2.grad), ("fc2/bias", b2.grad)):
        e = _rel_l2(m.grads[name].cpu().reshape(ref.shape), ref)
        assert e < 1e-3, f"grad {name}: relative L2 error {e:.3e}"
    g5_ref, _ = roi_ref.backward(pooled.grad.numpy(), am, boxes, nb, c5, ss, 7, 0, SCALE)
    g5 = pl.backward.g5.cpu().double()
    if dtype == torch.float32:
        assert _rel_l2(g5, torch.from_numpy(g5_ref)) < 1e-3
    else:
        cnt = _counts(boxes, nb, pl.h5, pl.h5, 7, 0)
        ok, amb, ratio = _g_elementwise(g5, dtype, dpk, am, boxes, nb, c5, ss, 7, 0, SCALE, ref_valid, cnt)
        print(f"g5 worst error / bound {ratio:.3f}, {int(amb.sum())} of {amb.numel()} elements at the ReLU's zero")
        assert ok.all(), f"g5: {int((~ok).sum())} of {ok.numel()} elements out of bound, first {torch.nonzero(~ok)[0].tolist()}"
        assert int(amb.sum()) <= 0.01 * amb.numel()
        assert (g5[0] != 0).any()
    assert (g5[1] == 0).all() and h5 == pl.h5               # the sample without boxes sends nothing down
    # call(): [N, K, classes], the empty slots zeroed
    out = m(clips.to(gpu), boxes=torch.from_numpy(boxes), num_boxes=nb)
    torch.cuda.synchronize()
    assert tuple(out.shape) == (n, kb, classes)
    flat = out.reshape(rows, classes).cpu()
    assert (flat[~valid] == 0).all() and (flat[valid] > 0).all() and torch.isfinite(flat).all()
    with pytest.raises(ValueError, match="boxes"):
        m(clips.to(gpu))


def test_switch_off_keeps_the_bits(gpu):
    """DETECTION.ENABLE False and a config without the section: the same logits, bit for bit, and refusal of boxes"""
    import x3d_tf_amd as x
    cfg_off, arch, params = _setup(["DETECTION.ENABLE", False, "DETECTION.MAX_BOXES", KB])
    absent = x.get_config("XS", BASE, freeze=False)
    del absent["DETECTION"]
    clips = torch.randn(2, 4, 64, 64, 3, generator=torch.Generator().manual_seed(3)).to(gpu)
    a = _model(cfg_off, params, gpu).logits(clips).clone()
    b = _model(absent, params, gpu).logits(clips).clone()
    assert torch.equal(a, b) and torch.isfinite(a).all()


def _ap_ref(scores, targets):
    """sklearn's average_precision_score for one class in fp64 (as tests/test_multilabel.py restates it)"""
    s = np.asarray(scores, dtype=np.float64).ravel()
    y = np.asarray(targets, dtype=np.float64).ravel() >= 0.5
    p = int(y.sum())
    if p == 0 or np.isnan(s).any():
        return float("nan")
    order = np.argsort(-s, kind="mergesort")
    s, y = s[order], y[order]
    last = np.r_[np.nonzero(np.diff(s))[0], len(s) - 1]
    tps = np.cumsum(y)[last].astype(np.float64)
    return float(np.sum(np.diff(np.r_[0.0, tps / p]) * (tps / (last + 1))))


def test_trainer_steps_and_validation_over_valid_rows(gpu):
    from x3d_tf_amd.train import Trainer
    cfg, arch, params = _setup(DET + ["DATA.MULTI_LABEL", True, "TRAIN.BATCH_SIZE", 2, "TRAIN.DATASET_SIZE", 4])
    cfg_cls, _, _ = _setup(["DATA.MULTI_LABEL", True, "TRAIN.BATCH_SIZE", 2, "TRAIN.DATASET_SIZE", 4])
    n, t, s, classes = 2, 4, 64, arch.num_classes
    m = _model(cfg, params, gpu)
    tr = Trainer(m, cfg)
    g = torch.Generator().manual_seed(5)
    batches = []
    for i, nb in enumerate(([2, 0], [3, 1])):
        batches.append((torch.randn(n, t, s, s, 3, generator=g).to(gpu), (torch.rand(n, KB, classes, generator=g) < 0.3).float(),
                        torch.from_numpy(_clip_boxes(n, s, seed=10 + i)), torch.tensor(nb)))
    losses = []
    for i in range(3):
        clips, y, bx, nb = batches[i % 2]
        pl = tr.step(clips, y, lr=0.01, boxes=bx, num_boxes=nb)
        losses.append(pl.loss_rows)
    torch.cuda.synchronize()
    assert all(bool(torch.isfinite(l).all()) for l in losses)
    # the step's launch lists are the classification step's but for the two ROI launches: nothing else was added to the replay
    m_cls = _model(cfg_cls, params, gpu)
    pc = m_cls._plan(n, t, s, s, True)
    # (and the head slot, which holds the _w entry point of the same head: the row weights carry the valid-box mean)
    swap = {"x3d_roi_pool_fwd": "x3d_pool_fwd", "x3d_roi_pool_bwd": "x3d_relu_bn_bwd_reduce", "x3d_sigmoid_bce_w": "x3d_sigmoid_bce"}
    for mine, theirs in ((pl.fwd, pc.fwd), (pl.bwd, pc.bwd)):
        assert [swap.get(e[0], e[0]) for e in mine] == [e[0] for e in theirs]
    with pytest.raises(ValueError, match="boxes"):
        tr.step(batches[0][0], batches[0][1], lr=0.01)
    # validate: loss and mAP over the valid rows only, against fp64 from the probabilities call() returns
    r = tr.validate(batches)
    scores, targets = [], []
    for clips, y, bx, nb in batches:
        p = m(clips, boxes=bx, num_boxes=nb).cpu().double().reshape(n * KB, classes)
        keep = (torch.arange(KB).view(1, KB) < nb.view(n, 1)).reshape(-1)
        scores.append(p[keep])
        targets.append(y.reshape(n * KB, classes).double()[keep])
    sc, tg = torch.cat(scores), torch.cat(targets)
    assert r["videos"] == 6 == sc.shape[0]
    q = sc.clamp(1e-7, 1 - 1e-7)
    want_loss = float((-(tg * q.log() + (1 - tg) * (1 - q).log())).mean()) + float(m.regularization_loss().item())
    aps = np.array([_ap_ref(sc[:, c].numpy(), tg[:, c].numpy()) for c in range(classes)])
    want_map = float(np.nanmean(aps))
    print(f"val loss {r['loss']} vs {want_loss}; mAP {r['mAP']} vs {want_map}")
    assert abs(r["loss"] - want_loss) <= 1e-9 * max(1.0, abs(want_loss)) and abs(r["mAP"] - want_map) <= 1e-12


def test_precise_bn_on_a_detection_model_is_the_classification_trunk(gpu):
    """precise_bn.update_bn_stats runs a DETECTION.ENABLE model with every box slot empty (the ROI launch reads no plane): over two
    (clips, labels, boxes, num_boxes) batches it gives the moving statistics of the same parameters and clips with the switch off,
    bn5's included, at the 1 ulp of tests/test_precise_bn_gpu.py's fp64 comparisons (the two runs pool the same fp64 sums of the same
    trunk launches; only the order of the adds into them may differ).  Nothing else of flat_params moves, and the step that follows
    sees its own boxes: the empty-slot call leaves neither box_mask nor num_boxes behind."""
    from tests import precise_bn_ref
    from x3d_tf_amd.precise_bn import update_bn_stats
    n, t, s = 2, 4, 128
    cfg_on, arch, params = _setup(["DETECTION.ENABLE", True])
    cfg_off, _, _ = _setup([])
    kb, classes = cfg_on.DETECTION.MAX_BOXES, arch.num_classes
    g = torch.Generator().manual_seed(21)
    batches = [(torch.randn(n, t, s, s, 3, generator=g).to(gpu), torch.randint(0, classes, (n, kb), generator=g),
                torch.from_numpy(roi_ref.box_mix(n, kb, s, s, seed=30 + i)), torch.tensor(nb)) for i, nb in enumerate(([5, 0], [8, 3]))]
    on, off = _model(cfg_on, params, gpu), _model(cfg_off, params, gpu)
    stats = {}
    for name, m, data in (("on", on, batches), ("off", off, [(b[0], None) for b in batches])):
        m.moving_stats_flat().fill_(12345.0)
        before = m.flat_params[:m.n_trainable_flat].clone()
        assert update_bn_stats(m, data, 2) == 2
        torch.cuda.synchronize()
        assert torch.equal(m.flat_params[:m.n_trainable_flat], before), f"{name}: flat_params moved outside the moving statistics"
        stats[name] = {k: v.detach().cpu().numpy().copy() for k, v in m.params.items() if k.endswith(("/moving_mean", "/moving_variance"))}
    assert stats["on"].keys() == stats["off"].keys() and "conv5/layer_with_weights-1/moving_mean" in stats["on"]
    worst = 0.0
    for k, v in stats["on"].items():
        assert not np.any(v == 12345.0), k
        worst = max(worst, float(precise_bn_ref.ulps(v, stats["off"][k].astype(np.float64)).max()))
    print(f"detection on against off: worst distance {worst} ulp")
    assert worst <= 1.0
    clips, labels, bx, nb = batches[0]
    pl = on.forward_backward(clips, labels, boxes=bx, num_boxes=nb)
    torch.cuda.synchronize()
    assert pl.num_boxes.cpu().tolist() == nb.tolist()
    assert pl.box_mask.cpu().tolist() == (torch.arange(kb).view(1, kb) < nb.view(n, 1)).float().reshape(-1).tolist()
    assert bool(torch.isfinite(pl.loss_rows).all()) and tuple(pl.loss_rows.shape) == (n * kb,)
    g5 = pl.backward.g5
    assert bool(torch.isfinite(g5).all()) and bool((g5[0] != 0).any()) and bool((g5[1] == 0).all())


def test_fit_on_detection_batches(gpu):
    """Trainer.fit over (clips, labels, boxes, num_boxes) batches: one epoch of two steps and a validation pass"""
    from x3d_tf_amd.train import Trainer
    cfg, arch, params = _setup(["DETECTION.ENABLE", True, "TRAIN.BATCH_SIZE", 2, "TRAIN.DATASET_SIZE", 4])
    n, t, s, classes, kb = 2, 4, 64, arch.num_classes, cfg.DETECTION.MAX_BOXES
    g = torch.Generator().manual_seed(8)

    def batch(i, nb):
        return (torch.randn(n, t, s, s, 3, generator=g).to(gpu), torch.randint(0, classes, (n, kb), generator=g),
                torch.from_numpy(roi_ref.box_mix(n, kb, s, s, seed=40 + i)), torch.tensor(nb))
    train = [batch(0, [5, 0]), batch(1, [8, 2])]
    val = [batch(2, [3, 6]), batch(3, [0, 1])]
    tr = Trainer(_model(cfg, params, gpu), cfg)
    seen = []
    real = tr.validate

    def validate(*a, **k):
        seen.append(real(*a, **k))
        return seen[-1]
    tr.validate = validate
    losses = tr.fit(iter(train), epochs=1, validation_data=lambda: val)
    assert tr.opt_step == 2 and tr.epoch == 1 and len(losses) == 1
    assert all(len(v) == 1 and np.isfinite(v[0]) for v in tr.history.values()), tr.history
    assert {"loss", "lr", "val_loss", "val_acc"} <= set(tr.history)
    assert len(seen) == 1 and seen[0]["videos"] == 3 + 6 + 0 + 1
