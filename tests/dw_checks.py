"""The fp64 runner of the depthwise class sweep (tests/dw_classes.py, tests/test_dw_classes_gpu.py): one committed case of one
kernel instantiation of x3d_dw3d_fwd / x3d_dw3d_bwd against the reference and at the limits of test_dw3d_fwd / test_dw3d_bwd
(tests/test_kernels_gpu.py) -- the vector kernels against the fp64 stencil of the unrounded operands at tol_store, the
matrix-core kernels (asked of the dispatch by name) against the stencil of the operands rounded to the storage type at
tol_gemm / _wtol, statistics, pool and a_sums at _stol, dW with its `+=` pre-fill in the reference.

What differs from those tests: every operand and every output is a view into its own allocation with guard bands
(tests/aux_checks.py _Bands), `off` elements past a 16-byte boundary; y and ga start as NaN, so an element the launch leaves
unwritten is not finite and a write past either end shows in check() (the fp64 sums keep their zero pre-fill, dW its 0.25:
their limits have no term for another start value).  The launch's instantiation is asked of the dispatch over the REAL
pointers before anything runs and must be the case's class.  A forward case runs in every prologue form that keeps it in
its class (DC.case_forms); the "bn" form (the BatchNorm finalize folded into the launch, x3d_bn_fold) is held to the fp64
stencil of x3d_bn_finalize's own table, and must publish that table bit for bit.  The forward's statistics are handed over in
the library's replicated layout, so the kernel writes into the banded view itself.

Every runner returns {compared tensor: worst error as a fraction of its limit}."""
import ctypes as C

import torch
import torch.nn.functional as F

from tests import dw_classes as DC
from tests.aux_checks import _Bands, _frac
from tests.util import rnd, round_to, tol_gemm, tol_store


def _k():
    from tests import test_kernels_gpu as K
    return K


def _real_class(case, entry, **p):
    """The class the dry run gives for the launch over the real device pointers `p` (statistics / pool do not enter)."""
    from x3d_tf_amd import hip
    ptr = lambda t: None if t is None else t.data_ptr()
    code = hip.dtype_code(case.dtype)
    if entry == "bwd":
        st = hip.Dw3dBwdArgs(ptr(p["dv"]), ptr(p["braw"]), ptr(p["coef"]), ptr(p["araw"]), ptr(p["ss"]), ptr(p["w"]), ptr(p["ga"]),
                             ptr(p["a_sums"]), ptr(p["dw"]), case.n, case.c, case.t, case.h, case.w, case.stride, code)
    else:
        fold = p.get("fold")
        st = hip.Dw3dFwdArgs(ptr(p["x"]), ptr(p["w"]), ptr(p["y"]), ptr(p.get("ss")), p["act"], ptr(p.get("stats")), ptr(p.get("pool")),
                             case.n, case.c, case.t, case.h, case.w, case.stride, code, None if fold is None else C.pointer(fold))
    return ("x3d_dw3d_" + entry, hip.dw3d_kernel_name(st))


def run_case(gpu, case, cls):
    """One committed case of class `cls`; {compared tensor: worst error / limit}."""
    assert DC.dispatch(case) == cls, f"{DC.case_id(case)} dispatches {DC.dispatch(case)}, not its class {cls}"
    return (_run_bwd if case.entry == "bwd" else _run_fwd)(gpu, case, cls)


def _run_fwd(gpu, case, cls):
    """The case in every prologue form that keeps it in its class (DC.case_forms); the folded form's ratios carry `_bn`."""
    out = {}
    for pro in DC.case_forms(case, cls):
        form = case._replace(pro=pro)
        assert DC.dispatch(form) == cls, (form, cls)
        for k, v in _run_fwd_form(gpu, form, cls).items():
            out[k + ("_bn" if pro == "bn" else "")] = v
    return out


def _run_fwd_form(gpu, case, cls):
    from x3d_tf_amd import hip, ops
    from oracle import x3d_oracle as O
    K = _k()
    n, c, t, h, w, stride, dtype = case.n, case.c, case.t, case.h, case.w, case.stride, case.dtype
    ho, wo = -(-h // stride), -(-w // stride)
    g = K._gen(2)
    x, xd = rnd((n, c, t, h, w), dtype, g)
    wt = torch.randn((c, 3, 3, 3), generator=g) * 0.3
    B = _Bands(gpu, case.off)
    xg, wg = B.view(x.to(gpu)), B.view(wt.to(gpu))
    y = B((n, c, t, ho, wo), dtype)
    # the statistics in the library's replicated layout, so that the kernel writes into the banded view itself (a plain
    # [C, 2] tensor goes through a temporary of ops._Stats)
    reps, stride_ = hip.stats_layout(c)
    stats_rep = B((reps * stride_,), torch.float64, fill=0.0)
    assert stats_rep.numel() != 2 * c
    pool = B((n, c), torch.float64, fill=0.0)
    mx = "_mx" in cls[1]
    out = {}
    if case.pro == "ss":
        ss = torch.stack([1 + 0.3 * torch.randn(c, generator=g), 0.3 * torch.randn(c, generator=g)], 1)
        ssg = B.view(ss.to(gpu))
        assert _real_class(case, "fwd", x=xg, w=wg, y=y, ss=ssg, act=1, stats=stats_rep, pool=pool) == cls
        ops.dw3d_fwd(xg, wg, stride, y=y, in_ss=ssg, in_act=1, stats=stats_rep, pool=pool)
    else:
        # the BatchNorm statistics of x itself, finalized by x3d_bn_finalize (the reference's table) and inside the launch
        xs = xg.double()
        xstats = torch.stack([xs.sum((0, 2, 3, 4)), (xs * xs).sum((0, 2, 3, 4))], 1).contiguous()
        gamma = B.view((1 + 0.3 * torch.randn(c, generator=g)).to(gpu))
        beta = B.view((0.3 * torch.randn(c, generator=g)).to(gpu))
        count = n * t * h * w
        mm0, mv0 = torch.full((c,), 0.25, device=gpu), torch.full((c,), 1.5, device=gpu)
        ss0, mi0 = torch.zeros((c, 2), device=gpu), torch.zeros((c, 2), device=gpu)
        ops.bn_finalize(xstats, count, gamma, beta, mm0, mv0, 1e-5, 0.9, 1, ss0, mi0)
        mm1, mv1 = B((c,), torch.float32, fill=0.25), B((c,), torch.float32, fill=1.5)
        ss1, mi1 = B((c, 2), torch.float32), B((c, 2), torch.float32)
        fold = ops.bn_fold(xstats, count, gamma, beta, mm1, mv1, 1e-5, 0.9, 1, ss1, mi1)
        assert _real_class(case, "fwd", x=xg, w=wg, y=y, act=1, stats=stats_rep, pool=pool, fold=fold) == cls
        ops.dw3d_fwd(xg, wg, stride, y=y, in_act=1, stats=stats_rep, pool=pool, in_bn=fold)
        torch.cuda.synchronize()
        for name, a_, b_ in (("ss", ss0, ss1), ("mean_invstd", mi0, mi1), ("moving_mean", mm0, mm1), ("moving_var", mv0, mv1)):
            assert torch.equal(a_, b_), f"bn fold: {name} differs from x3d_bn_finalize's"
        assert ss1.abs().sum().item() > 0
        ss = ss0.cpu()
    torch.cuda.synchronize()
    pre = K._affine(xd, ss.double(), None, 1)
    if mx:   # the fp32 prologue's output and the weights are rounded to the storage type first
        ref = O.depthwise3x3x3(round_to(pre.float(), dtype), round_to(wt, dtype), stride)
        rt, at = tol_gemm(dtype)
    else:
        ref = O.depthwise3x3x3(pre, wt.double(), stride)
        rt, at = tol_store(dtype)
    stol = K._stol(dtype)
    out["y"] = _frac("y", y.cpu(), ref, rt, at * ref.abs().max().item())
    ys = y.float().cpu()
    sref = K._stats_ref(ys, dtype)
    out["stats"] = _frac("stats", ops.stats_sum(stats_rep, c).cpu(), sref, stol, stol * max(1.0, sref.abs().max().item()))
    out["pool"] = _frac("pool", pool.cpu(), ys.double().sum((2, 3, 4)), stol, 10 * stol * max(1.0, float(ys[0, 0].numel()) ** 0.5))
    if case.pro == "ss":
        # no prologue, no sums: the same instantiation (tests/test_dw_classes.py), its own absolute scale
        y2 = B((n, c, t, ho, wo), dtype)
        assert _real_class(case, "fwd", x=xg, w=wg, y=y2, act=0) == cls
        ops.dw3d_fwd(xg, wg, stride, y=y2)
        torch.cuda.synchronize()
        ref2 = O.depthwise3x3x3(xd, round_to(wt, dtype) if mx else wt.double(), stride)
        out["y_noprologue"] = _frac("y_noprologue", y2.cpu(), ref2, rt, at * ref2.abs().max().item())
    B.check()
    return out


def _run_bwd(gpu, case, cls):
    from x3d_tf_amd import ops
    from oracle import x3d_oracle as O
    K = _k()
    n, c, t, h, w, stride, dtype = case.n, case.c, case.t, case.h, case.w, case.stride, case.dtype
    ho, wo = -(-h // stride), -(-w // stride)
    g_ = K._gen(5)
    araw, ad = rnd((n, c, t, h, w), dtype, g_)
    dv, dvd = rnd((n, c, t, ho, wo), dtype, g_)
    braw, bd = rnd((n, c, t, ho, wo), dtype, g_)
    coef = torch.randn((n, c, 4), generator=g_) * 0.5
    wt = torch.randn((c, 3, 3, 3), generator=g_) * 0.3
    ss = torch.stack([1 + 0.3 * torch.randn(c, generator=g_), 0.3 * torch.randn(c, generator=g_)], 1)
    cd = coef.double()
    dB = cd[:, :, 0, None, None, None] * dvd + cd[:, :, 1, None, None, None] * bd + cd[:, :, 2, None, None, None]
    z = K._affine(ad, ss.double())
    mx = "_mx" in cls[1]
    if mx:   # dB, A = relu(z) and the weights enter the products rounded to the storage type
        dB = round_to(dB.float(), dtype)
        act = round_to(F.relu(z).float(), dtype).requires_grad_(True)
        wref = round_to(wt, dtype).requires_grad_(True)
    else:
        act = F.relu(z).requires_grad_(True)
        wref = wt.double().requires_grad_(True)
    res = O.depthwise3x3x3(act, wref, stride)
    dA, dWr = torch.autograd.grad((res * dB).sum(), [act, wref])
    ga_ref = dA * (z > 0)
    B = _Bands(gpu, case.off)
    p = dict(dv=B.view(dv.to(gpu)), braw=B.view(braw.to(gpu)), coef=B.view(coef.to(gpu)), araw=B.view(araw.to(gpu)),
             ss=B.view(ss.to(gpu)), w=B.view(wt.to(gpu).view(c, 27)), ga=B((n, c, t, h, w), dtype),
             a_sums=B((c, 2), torch.float64, fill=0.0), dw=B((c, 27), torch.float32, fill=0.25))
    assert _real_class(case, "bwd", **p) == cls
    ops.dw3d_bwd(p["dv"], p["braw"], p["coef"], p["araw"], p["ss"], p["w"], p["ga"], p["a_sums"], p["dw"], stride)
    torch.cuda.synchronize()
    rt, at = tol_gemm(dtype) if mx else tol_store(dtype)
    out = {"ga": _frac("ga", p["ga"].cpu(), ga_ref, rt, at * ga_ref.abs().max().item())}
    wtol = K._wtol(dtype) if mx else 2e-4
    out["dw"] = _frac("dw", p["dw"].cpu(), dWr.view(c, 27) + 0.25, wtol, wtol * dWr.abs().max().item())
    gs = p["ga"].float().cpu().double()
    sref = torch.stack([gs.sum((0, 2, 3, 4)), (gs * ad).sum((0, 2, 3, 4))], 1)
    stol = K._stol(dtype)
    out["a_sums"] = _frac("a_sums", p["a_sums"].cpu(), sref, 10 * stol, 10 * stol * max(1.0, sref.abs().max().item()))
    B.check()
    return out
