"""The inputs of the solver tests, shared by tests/test_solver_gpu.py, tests/test_layerwise_gpu.py and tools/solver_digest.py.

Flat kernels: CASES, the seeded host arrays (_host), their placement on the device at a chosen misalignment (_dev), the
hyper-parameters and the raw calls of the plain and the _ex entry points.  Chunk kernels: the segment layout (_fix: built once),
its NaN-padded device copies (_dirty), the hyper-parameters and the sum of squares the launches read (_norm_of)."""
import numpy as np
import torch

U = 2.0 ** -24
F32 = np.float32

# (n, offset of every pointer in elements, with l2 mask): the edges of the vector / one-element paths (n % 4, n < 4), the
# workgroup boundary (256), more than one workgroup, the grid-stride wrap (1024 workgroups x 256 threads x 4 elements =
# 1 048 576 elements per sweep), every pointer misaligned by one float (mask: one byte), and no mask at all
CASES = [(1, 0, True), (3, 0, True), (255, 0, True), (256, 0, True), (257, 0, True), (4100, 0, True), (2_500_003, 0, True),
         (4099, 1, True), (4100, 0, False)]
IDS = [f"n{n}" + ("_misaligned" if off else "") + ("" if mask else "_nomask") for n, off, mask in CASES]
WRAP = 2_000_001                     # an index of the largest case that only a second sweep of the grid reaches


def _host(n, seed, gscale_inv=1024.0):
    """w, v (second slot: >= 0), g (a loss-scaled gradient), l2 mask"""
    rng = np.random.default_rng(seed)
    w = rng.standard_normal(n).astype(F32)
    v = (0.1 * rng.standard_normal(n)).astype(F32)
    g = (gscale_inv * rng.standard_normal(n)).astype(F32)
    mask = (rng.random(n) < 0.7).astype(np.uint8)
    return w, v, g, mask


def _dev(a, gpu, off=0):
    """a copy of `a` on the device whose first element sits `off` elements behind an aligned allocation"""
    if a is None:
        return None
    buf = torch.zeros(a.size + off + 8, dtype=torch.from_numpy(a[:1]).dtype, device=gpu)
    t = buf[off:off + a.size]
    t.copy_(torch.from_numpy(a))
    return t


def _np(t):
    return t.detach().cpu().numpy()


def _bits(a):
    return np.ascontiguousarray(a).view(np.int32 if a.dtype == F32 else np.int64)


def _p(t):
    return None if t is None else t.data_ptr()


def _sumsq(g_dev):
    from x3d_tf_amd import ops
    return ops.grad_sumsq(g_dev)


def _coef(norm0, gs, max_norm):
    """the documented clip rule in fp64 (gs, max_norm: the fp32 values the ABI passes)"""
    gs, max_norm = float(F32(gs)), float(F32(max_norm))
    return gs * min(1.0, max_norm / (np.sqrt(norm0) * gs + 1e-6))

# ---- the flat optimizers: hyper-parameters and the raw calls ------------------------------------------------------------------
SGD = dict(lr=F32(0.1), mom=F32(0.9), wd=F32(5e-5))
ADAM = dict(lr=F32(1e-3), b1=F32(0.9), b2=F32(0.999), eps=F32(1e-7), wd=F32(5e-5), step=3)


def _sgd_plain(w, v, g, mask, gs):
    from x3d_tf_amd import hip
    hip.call("x3d_sgd_nesterov", _p(w), _p(v), _p(g), _p(mask), float(SGD["lr"]), float(SGD["mom"]), float(SGD["wd"]),
             float(gs), w.numel())


def _sgd_ex(w, v, g, mask, gs, norm=None, max_norm=0.0, ema=None, decay=0.0):
    from x3d_tf_amd import hip
    hip.call("x3d_sgd_nesterov_ex", _p(w), _p(v), _p(g), _p(mask), float(SGD["lr"]), float(SGD["mom"]), float(SGD["wd"]),
             float(gs), _p(norm), float(max_norm), _p(ema), float(decay), w.numel())


def _adam_plain(w, m, v, g, mask, gs):
    from x3d_tf_amd import hip
    a = ADAM
    hip.call("x3d_adam", _p(w), _p(m), _p(v), _p(g), _p(mask), float(a["lr"]), float(a["b1"]), float(a["b2"]),
             float(a["eps"]), float(a["wd"]), float(gs), a["step"], w.numel())


def _adam_ex(w, m, v, g, mask, gs, norm=None, max_norm=0.0, ema=None, decay=0.0):
    from x3d_tf_amd import hip
    a = ADAM
    hip.call("x3d_adam_ex", _p(w), _p(m), _p(v), _p(g), _p(mask), float(a["lr"]), float(a["b1"]), float(a["b2"]),
             float(a["eps"]), float(a["wd"]), float(gs), a["step"], _p(norm), float(max_norm), _p(ema), float(decay),
             w.numel())

# ---- the chunk kernels: layout and inputs of tests/test_layerwise_gpu.py ------------------------------------------------------
CHUNK = 1024                                   # X3D_SEG_CHUNK (asserted against the header in _fix)
SWEEP = 1024 * 4 * CHUNK                       # elements the largest grid takes before it strides
LENGTHS = [1, 3, 4, 5, 255, 256, 257, CHUNK - 1, CHUNK, CHUNK + 1, 5 * CHUNK + 77, 37, 41, 2 * SWEEP + 4099]
L2 = [True, False, True, True, False, True, True, True, False, True, True, True, True, True]
ZERO_W, ZERO_G = 11, 12                        # the all-zero w segment and the all-zero g (LAMB: m, v too) segment, both l2
LARS = dict(lr=F32(0.1), mom=F32(0.9), wd=F32(5e-5), eta=F32(0.02), eps=F32(1e-8))
SEG_ADAM = dict(lr=F32(1e-3), b1=F32(0.9), b2=F32(0.999), eps=F32(1e-7), step=3)
LAMB = dict(lr=F32(0.01), b1=F32(0.9), b2=F32(0.999), eps=F32(1e-6), step=3)
GS = F32(1.0 / 1024.0)                         # grad_scale of a loss-scaled gradient, as the flat cases


class _Fix:
    pass


_FIX = {}


def _fix(gpu):
    """the segment layout and the host arrays, built once: clean copies (padding 0) for the fp64 references, `dirty` ones
    (padding NaN) for the device"""
    if _FIX:
        return _FIX["f"]
    from x3d_tf_amd import hip
    from x3d_tf_amd.segments import SegTable
    assert hip.SEG_CHUNK == CHUNK
    f = _Fix()
    rng = np.random.default_rng(7)
    segs, off = [], 4
    for t, (n, l2) in enumerate(zip(LENGTHS, L2)):
        segs.append((off, n, l2))
        off += (n + 3) // 4 * 4 + (4 if t % 2 else 0)          # the model's padding, and a whole vector of it now and then
    f.segs, f.n = segs, off + 8
    f.table = SegTable(segs).to(gpu)
    f.covered = np.zeros(f.n, bool)
    f.l2e = np.zeros(f.n, bool)
    for o, n, l2 in segs:
        f.covered[o:o + n] = True
        f.l2e[o:o + n] = l2
    f.w = rng.standard_normal(f.n).astype(F32)
    for t, (o, n, _) in enumerate(segs):
        if t % 3 == 0:
            f.w[o:o + n] *= F32(10.0)                          # (trust ratios on both sides of lr: LARS_CLIP clips some)
    f.v = (0.1 * rng.standard_normal(f.n)).astype(F32)         # SGD momentum / Adam's first moment
    f.v2 = (np.abs(f.v) * F32(0.01)).astype(F32)               # Adam's second moment (>= 0)
    f.g = (1024.0 * rng.standard_normal(f.n)).astype(F32)
    f.e = (0.5 * f.w + 0.1).astype(F32)
    o, n, _ = segs[ZERO_W]
    f.w[o:o + n] = 0
    o, n, _ = segs[ZERO_G]
    f.g[o:o + n] = 0
    f.v[o:o + n] = 0
    f.v2[o:o + n] = 0
    for a in (f.w, f.v, f.v2, f.g, f.e):
        a[~f.covered] = 0
    f.norm_total = float(np.sqrt(np.sum(f.g.astype(np.float64) ** 2)) * float(GS))     # the unscaled global norm
    _FIX["f"] = f
    return f


def _dirty(f, a, gpu, off=0):
    """`a` with NaN padding on the device; off = 1: the first element one float behind a 16-byte boundary"""
    d = a.copy()
    d[~f.covered] = np.nan
    buf = torch.full((f.n + off + 8,), float("nan"), dtype=torch.float32, device=gpu)
    t = buf[off:off + f.n]
    t.copy_(torch.from_numpy(d))
    return t, d


def _norm_of(g_clean, gpu):
    """x3d_grad_sumsq over the gradient with ZERO padding, as the model's flat_grads has it (NaN padding would count as a
    non-finite gradient): the two doubles the launches read"""
    from x3d_tf_amd import ops
    return ops.grad_sumsq(torch.from_numpy(g_clean).to(gpu))
