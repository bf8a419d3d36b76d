"""The fp64 runner of the stem class sweep (tests/stem_classes.py, tests/test_stem_classes_gpu.py): one committed case of one
kernel instantiation of a stem entry point against fp64 built from torch on the CPU, with the references and at the limits of
test_stem / test_stem_fused (tests/test_kernels_gpu.py):

  x3d_stem_s_fwd    y against F.conv3d (pad (0, 1, 1), stride (1, 2, 2)) at tol_gemm.  The weight set of the reference is chosen
                    from the CLASS NAME, never "either": stem_s_fwd_bf16_kernel (matrix cores) multiplies weights rounded to the
                    storage type, stem_s_fwd_kernel (direct) the fp32 weights.
  x3d_stem_s_wgrad  dW (`+=` on a buffer of 0.25) against autograd, 2e-4 of max |dW|.  Both kernels multiply the stored operands
                    exactly (fp32 products of 16-bit values), so one reference serves both.
  x3d_dwt_fwd       y against the grouped KT x 1 x 1 conv (pad KT // 2) at tol_store; the statistics against sums over the STORED
                    output (rtol 1e-5, atol 1e-4: test_stem's); the inference epilogue with out_act 0 and 1 -- every form on
                    every case (the dispatch does not read the form).
  x3d_dwt_bwd       dx at tol_store and dW_t (`+=` on 0.25) at 2e-4 of max |dW| against autograd through dY = A g + B yraw + C;
                    the masked form (relu_scale_shift) against the mask [s yraw + t > 0] applied to g in fp64 (the exact sign, as the
                    kernel's fused multiply-add gives it).
  x3d_stem_fwd      y against fp64 DIRECTLY: conv_t of conv_s over the weights rounded to storage, the conv_s output rounded to
                    storage as the kernel rounds it on chip, at tol_store plus the tie slack of that rounding
                    (tests.util.tie_slack_t, as test_stem_fused_forward_full_size); and bit for bit against x3d_stem_s_fwd +
                    x3d_dwt_fwd; statistics against the stored output and against the two-kernel path's.
  x3d_stem_bwd      dW_t and dW_s (`+=` on 0.5 / -0.25) against fp64 autograd over the stored tensors at 2e-4 of the maximum (dW_s
                    with the tie slack of the on-chip rounding of ds), and against x3d_dwt_bwd + x3d_stem_s_wgrad at 2e-5.

No class needed a wider limit than those tests use: the bounds come from the output rounding and from fp32 accumulation over
N * T * Ho * Wo points, and neither grows with KT at these sizes (measured worst error / limit per class:
profiles/stem_classes_mi355x.txt).

Every operand and every output is a view into its own allocation with guard bands (tests/aux_checks.py _Bands), `off` elements
past a 16-byte boundary; outputs start as NaN, so an element the launch leaves unwritten is not finite and a write past either
end shows in check() (accumulators keep their pre-fill).  The launch's instantiation is asked of the dispatch over the REAL
pointers before anything runs and must be the case's class.

Every runner returns {compared tensor: worst error as a fraction of its limit}."""
import torch
import torch.nn.functional as F

from tests import stem_classes as SC
from tests.aux_checks import _Bands, _frac
from tests.util import _tie_ulps, rnd, round_to, tie_slack_t, tol_gemm, tol_store


def _k():
    from tests import test_kernels_gpu as K
    return K


def conv_s64(x, w):
    """conv_s in the dtype of its operands: x [N, Cin, T, H, W], w [Cout, Cin, 3, 3]"""
    return F.conv3d(F.pad(x, (1, 1, 1, 1, 0, 0)), w.unsqueeze(2), stride=(1, 2, 2))


def conv_t64(s, wt):
    """conv_t: s [N, C, T, H, W], wt [C, KT]"""
    kt = wt.shape[1]
    return F.conv3d(F.pad(s, (0, 0, 0, 0, kt // 2, kt // 2)), wt.view(-1, 1, kt, 1, 1), groups=wt.shape[0])


def _ch(v):
    return v.view(1, -1, 1, 1, 1)


def _within(name, got, ref, rtol, atol, slack):
    """|got - ref| <= atol + rtol |ref| + slack element-wise; the worst error as a fraction of that limit"""
    got, ref = got.double().cpu(), ref.double().cpu()
    lim = atol + rtol * ref.abs() + slack.double().cpu()
    err = (got - ref).abs()
    assert torch.isfinite(got).all(), f"{name}: non-finite values"
    bad = err > lim
    assert not bad.any(), (f"{name}: {int(bad.sum())}/{bad.numel()} out of tolerance (rtol {rtol}, atol {atol:.3e}, tie slack on "
                           f"{int((slack > 0).sum())} elements); max err {err.max().item():.3e}, max |ref| {ref.abs().max().item():.3e}")
    return (err / lim.clamp_min(1e-300)).max().item()


def _is_class(cls, entry, *args):
    """the dry run over the launch's real arguments (C ABI order, no stream) gives the case's class"""
    from x3d_tf_amd import hip
    ptr = lambda a: a.data_ptr() if isinstance(a, torch.Tensor) else a
    got = (entry, hip.stem_kernel_name(entry, *[ptr(a) for a in args]))
    assert got == cls, f"the launch over the real pointers dispatches {got}, not {cls}"


def run_case(gpu, case, cls):
    """One committed case of class `cls` in every launch form that keeps it there; {compared tensor: worst error / limit}."""
    assert SC.dispatch(case) == cls, f"{SC.case_id(case)} dispatches {SC.dispatch(case)}, not its class {cls}"
    forms = SC.case_forms(case, cls)
    for f in forms:
        assert SC.dispatch(case._replace(form=f)) == cls, (case, f)
    return _RUN[case.entry](gpu, case, cls, forms)


def _clip(case, g):
    """the clip batch of a case: (planar fp64 copy, the tensor in the case's layout on the CPU)"""
    x, xd = rnd((case.n, case.cin, case.t, case.h, case.w), case.dtype, g)
    return xd, (x.permute(0, 2, 3, 4, 1).contiguous() if case.layout else x)


def _run_s_fwd(gpu, case, cls, forms):
    from x3d_tf_amd import hip, ops
    n, t, h, w, cout, dtype = case.n, case.t, case.h, case.w, case.cout, case.dtype
    ho, wo = SC.out_hw(h, w)
    g = _k()._gen(6)
    xd, xk = _clip(case, g)
    ws = torch.randn((cout, case.cin, 3, 3), generator=g) * 0.3
    B = _Bands(gpu, case.off)
    xg, wg = B.view(xk.to(gpu)), B.view(ws.to(gpu))
    y = B((n, cout, t, ho, wo), dtype)
    _is_class(cls, case.entry, xg, wg, y, n, case.cin, t, h, w, cout, hip.dtype_code(dtype), case.layout)
    ops.stem_s_fwd(xg, wg, y=y, channels_last=bool(case.layout))
    torch.cuda.synchronize()
    # the reference's weights by the kernel that ran: the matrix-core kernel rounds them to the storage type
    assert cls[1].startswith(("stem_s_fwd_bf16_kernel<", "stem_s_fwd_kernel<")), cls
    ref_s = conv_s64(xd, ws.double())
    ref = conv_s64(xd, round_to(ws, dtype)) if cls[1].startswith("stem_s_fwd_bf16_kernel<") else ref_s
    rt, at = tol_gemm(dtype)
    out = {"y": _frac("conv_s", y.cpu(), ref, rt, at * ref_s.abs().max().item())}
    B.check()
    return out


def _run_s_wgrad(gpu, case, cls, forms):
    from x3d_tf_amd import hip, ops
    n, cin, t, h, w, cout, dtype = case.n, case.cin, case.t, case.h, case.w, case.cout, case.dtype
    ho, wo = SC.out_hw(h, w)
    g = _k()._gen(7)
    xd, xk = _clip(case, g)
    dy, dyd = rnd((n, cout, t, ho, wo), dtype, g)
    B = _Bands(gpu, case.off)
    xg, dyg = B.view(xk.to(gpu)), B.view(dy.to(gpu))
    dw = B((cout, cin, 3, 3), torch.float32, fill=0.25)
    _is_class(cls, case.entry, xg, dyg, dw, n, cin, t, h, w, cout, hip.dtype_code(dtype), case.layout)
    ops.stem_s_wgrad(xg, dyg, dw, channels_last=bool(case.layout))
    torch.cuda.synchronize()
    wz = torch.zeros((cout, cin, 3, 3), dtype=torch.float64, requires_grad=True)
    (ref,) = torch.autograd.grad((conv_s64(xd, wz) * dyd).sum(), [wz])
    out = {"dw_s": _frac("stem_s_dw", dw.cpu(), ref + 0.25, 2e-4, 2e-4 * ref.abs().max().item())}
    B.check()
    return out


def _dwt_fwd_forms(gpu, B, forms, c, dtype, launch, ref_t, g, tag=""):
    """Launch a conv_t-bearing forward in each of `forms` through launch(y, stats, out_ss, out_act) and check y (and the
    statistics) against ref_t [, slack]; returns ({name: fraction}, {form: y})."""
    from x3d_tf_amd import hip, ops
    K = _k()
    ref_t, slack = ref_t
    rs, as_ = tol_store(dtype)
    oss = torch.stack([1 + 0.3 * torch.randn(c, generator=g), 0.3 * torch.randn(c, generator=g)], 1)
    ossg = B.view(oss.to(gpu))
    aff = _ch(oss[:, 0].double()) * ref_t + _ch(oss[:, 1].double())
    ref_i = F.relu(aff)
    out, ys = {}, {}
    for form in forms:
        y = B(tuple(ref_t.shape), dtype)
        if form == "stats":
            reps, stride = hip.stats_layout(c)
            st = B((reps * stride,), torch.float64, fill=0.0)       # the library's replicated layout: the kernel adds into the banded view
            assert st.numel() != 2 * c
            launch(y, st, None, 0)
        elif form == "plain":
            launch(y, None, None, 0)
        else:
            launch(y, None, ossg, int(form[-1]))
        torch.cuda.synchronize()
        if form in ("stats", "plain"):
            out["y_" + form] = _within(f"conv_t{tag} ({form})", y, ref_t, rs, as_ * ref_t.abs().max().item(), slack)
        else:
            ref = ref_i if form == "infer1" else aff
            out["y_" + form] = _within(f"conv_t{tag} + bn{' + relu' if form == 'infer1' else ''}", y, ref, rs,
                                       as_ * max(1.0, ref_i.abs().max().item()), slack * _ch(oss[:, 0].double().abs()))
        if form == "stats":
            out["stats"] = _frac("stats", ops.stats_sum(st, c).cpu(), K._stats_ref(y.float().cpu(), dtype), 1e-5, 1e-4)
        ys[form] = (y, ops.stats_sum(st, c) if form == "stats" else None, ossg)
    return out, ys


def _run_dwt_fwd(gpu, case, cls, forms):
    from x3d_tf_amd import hip
    n, t, c, kt, dtype = case.n, case.t, case.cout, case.kt, case.dtype
    ho, wo = SC.out_hw(case.h, case.w)
    g = _k()._gen(8)
    x, xd = rnd((n, c, t, ho, wo), dtype, g)
    wt = torch.randn((c, kt), generator=g) * 0.4
    B = _Bands(gpu, case.off)
    xg, wg = B.view(x.to(gpu)), B.view(wt.to(gpu))
    code = hip.dtype_code(dtype)

    def launch(y, st, oss, act):
        _is_class(cls, case.entry, xg, wg, y, st, oss, act, n, c, t, ho * wo, kt, code)
        hip.call("x3d_dwt_fwd", xg.data_ptr(), wg.data_ptr(), y.data_ptr(), hip.ptr(st), hip.ptr(oss), act, n, c, t, ho * wo, kt, code)
    ref_t = conv_t64(xd, wt.double())
    out, _ = _dwt_fwd_forms(gpu, B, forms, c, dtype, launch, (ref_t, torch.zeros_like(ref_t)), g)
    B.check()
    return out


def _dy64(gd, yd, coef, rss):
    """dY = A g' + B yraw + C in fp64, g' = g masked by [s yraw + t > 0] when rss is given"""
    cf = coef.double()
    if rss is not None:
        gd = torch.where(_ch(rss[:, 0].double()) * yd + _ch(rss[:, 1].double()) > 0, gd, torch.zeros_like(gd))
    return _ch(cf[:, 0]) * gd + _ch(cf[:, 1]) * yd + _ch(cf[:, 2])


def _run_dwt_bwd(gpu, case, cls, forms):
    from x3d_tf_amd import hip, ops
    n, t, c, kt, dtype = case.n, case.t, case.cout, case.kt, case.dtype
    ho, wo = SC.out_hw(case.h, case.w)
    g_ = _k()._gen(9)
    shape = (n, c, t, ho, wo)
    g, gd = rnd(shape, dtype, g_)
    yr, yd = rnd(shape, dtype, g_)
    x, xd = rnd(shape, dtype, g_)
    coef = torch.randn((c, 4), generator=g_) * 0.5
    wt = torch.randn((c, kt), generator=g_) * 0.4
    rss = torch.stack([1 + 0.3 * torch.randn(c, generator=g_), 0.3 * torch.randn(c, generator=g_)], 1)
    B = _Bands(gpu, case.off)
    gg, yg, xg = B.view(g.to(gpu)), B.view(yr.to(gpu)), B.view(x.to(gpu))
    cg, wg, rg = B.view(coef.to(gpu)), B.view(wt.to(gpu)), B.view(rss.to(gpu))
    rs, as_ = tol_store(dtype)
    out = {}
    for form in forms:
        masked = form == "masked"
        dx = B(shape, dtype)
        dw = B((c, kt), torch.float32, fill=0.25)
        _is_class(cls, case.entry, gg, yg, rg if masked else None, cg, xg, wg, dx, dw, n, c, t, ho * wo, kt, hip.dtype_code(dtype))
        ops.dwt_bwd(gg, yg, cg, xg, wg, dx, dw, relu_ss=rg if masked else None)
        torch.cuda.synchronize()
        dY = _dy64(gd, yd, coef, rss if masked else None)
        xs = xd.clone().requires_grad_(True)
        wtr = wt.double().requires_grad_(True)
        dxs, dwt_ref = torch.autograd.grad((conv_t64(xs, wtr) * dY).sum(), [xs, wtr])
        out["dx_" + form] = _frac(f"dwt_dx ({form})", dx.cpu(), dxs, rs, as_ * dxs.abs().max().item())
        out["dw_t_" + form] = _frac(f"dwt_dw ({form})", dw.cpu(), dwt_ref + 0.25, 2e-4, 2e-4 * dwt_ref.abs().max().item())
    B.check()
    return out


def _fused_inputs(gpu, case, seed):
    g = _k()._gen(seed)
    xd, xk = _clip(case, g)
    ws = torch.randn((case.cout, 3, 3, 3), generator=g) * 0.3
    wt = torch.randn((case.cout, case.kt), generator=g) * 0.4
    return g, xd, xk, ws, wt


def _run_stem_fwd(gpu, case, cls, forms):
    from x3d_tf_amd import hip, ops
    n, t, h, w, c, kt, dtype = case.n, case.t, case.h, case.w, case.cout, case.kt, case.dtype
    assert case.layout == 1 and case.cin == 3
    g, xd, xk, ws, wt = _fused_inputs(gpu, case, 11)
    B = _Bands(gpu, case.off)
    xg, wsg, wtg = B.view(xk.to(gpu)), B.view(ws.to(gpu)), B.view(wt.to(gpu))
    code = hip.dtype_code(dtype)

    def launch(y, st, oss, act):
        _is_class(cls, case.entry, xg, wsg, wtg, y, st, oss, act, n, 3, t, h, w, c, kt, code, 1)
        hip.call("x3d_stem_fwd", xg.data_ptr(), wsg.data_ptr(), wtg.data_ptr(), y.data_ptr(), hip.ptr(st), hip.ptr(oss), act,
                 n, 3, t, h, w, c, kt, code, 1)
    # fp64, directly: conv_s over the weights rounded to storage, its output rounded to storage as on chip, then conv_t
    s64 = conv_s64(xd, round_to(ws, dtype))
    ref_t = conv_t64(round_to(s64, dtype), wt.double())
    out, ys = _dwt_fwd_forms(gpu, B, forms, c, dtype, launch, (ref_t, tie_slack_t(s64, dtype, wt.abs())), g, " of conv_s")
    # ... and bit for bit against the two-kernel path (aligned tensors of its own)
    s2 = ops.stem_s_fwd(xk.to(gpu), ws.to(gpu), channels_last=True)
    for form, (y, st, ossg) in ys.items():
        st2 = torch.zeros((c, 2), dtype=torch.float64, device=gpu) if form == "stats" else None
        y2 = ops.dwt_fwd(s2, wt.to(gpu), stats=st2, out_ss=ossg if form.startswith("infer") else None,
                         out_act=int(form[-1]) if form.startswith("infer") else 0)
        torch.cuda.synchronize()
        assert torch.equal(y, y2), f"fused stem forward ({form}) differs from conv_s + conv_t: {(y.float() - y2.float()).abs().max().item()}"
        if st2 is not None:
            out["stats_vs_two_kernels"] = _frac("stats vs two kernels", st.cpu(), st2.cpu(), 1e-5, 1e-5 * max(1.0, st2.abs().max().item()))
    B.check()
    return out


def _run_stem_bwd(gpu, case, cls, forms):
    from x3d_tf_amd import hip, ops
    n, t, h, w, c, kt, dtype = case.n, case.t, case.h, case.w, case.cout, case.kt, case.dtype
    assert case.layout == 1 and case.cin == 3
    g_, xd, xk, ws, wt = _fused_inputs(gpu, case, 12)
    # the stored tensors of the forward pass, from the two-kernel path (x3d_stem_fwd is bit-identical to it: _run_stem_fwd)
    xa, wsa, wta = xk.to(gpu), ws.to(gpu), wt.to(gpu)
    s2 = ops.stem_s_fwd(xa, wsa, channels_last=True)
    yt = ops.dwt_fwd(s2, wta)
    gq, gd = rnd(tuple(yt.shape), dtype, g_)
    coef = torch.randn((c, 4), generator=g_) * 0.5
    rss = torch.stack([1 + 0.3 * torch.randn(c, generator=g_), 0.3 * torch.randn(c, generator=g_)], 1)
    B = _Bands(gpu, case.off)
    xg, wsg, wtg = B.view(xa), B.view(wsa), B.view(wta)
    gg, yg, cg, rg = B.view(gq.to(gpu)), B.view(yt), B.view(coef.to(gpu)), B.view(rss.to(gpu))
    ysd, ytd = s2.float().cpu().double(), yt.float().cpu().double()
    code = hip.dtype_code(dtype)
    out = {}
    for form in forms:
        masked = form == "masked"
        dwt = B((c, kt), torch.float32, fill=0.5)               # += on what is there
        dws = B((c, 3, 3, 3), torch.float32, fill=-0.25)
        _is_class(cls, case.entry, gg, yg, rg if masked else None, cg, xg, wsg, wtg, dws, dwt, n, 3, t, h, w, c, kt, code, 1)
        ops.stem_bwd(gg, yg, cg, xg, wsg, wtg, dws, dwt, relu_ss=rg if masked else None)
        # the two-kernel path on the same operands
        ds = torch.empty_like(s2)
        dwt2 = torch.zeros((c, kt), dtype=torch.float32, device=gpu)
        dws2 = torch.zeros((c, 3, 3, 3), dtype=torch.float32, device=gpu)
        ops.dwt_bwd(gg, yg, cg, s2, wta, ds, dwt2, relu_ss=rg if masked else None)
        ops.stem_s_wgrad(xa, ds, dws2, channels_last=True)
        torch.cuda.synchronize()
        dwt_, dws_ = dwt.cpu() - 0.5, dws.cpu() + 0.25
        out["dw_t_vs_two_" + form] = _frac("dw_t vs two kernels", dwt_, dwt2.cpu(), 2e-5, 2e-5 * dwt2.abs().max().item())
        out["dw_s_vs_two_" + form] = _frac("dw_s vs two kernels", dws_, dws2.cpu(), 2e-5, 2e-5 * dws2.abs().max().item())
        # fp64 autograd over the stored tensors: dY -> conv_t^T -> ds rounded to storage -> conv_s weight gradient
        dY = _dy64(gd, ytd, coef, rss if masked else None)
        xs = ysd.clone().requires_grad_(True)
        wtr = wt.double().requires_grad_(True)
        dxs, dwt64 = torch.autograd.grad((conv_t64(xs, wtr) * dY).sum(), [xs, wtr])
        out["dw_t_" + form] = _frac("dw_t vs fp64", dwt_, dwt64, 2e-4, 2e-4 * dwt64.abs().max().item())
        wz = torch.zeros((c, 3, 3, 3), dtype=torch.float64, requires_grad=True)
        (dws64,) = torch.autograd.grad((conv_s64(xd, wz) * round_to(dxs.float(), dtype)).sum(), [wz])
        # where ds sits on a rounding midpoint the kernel's fp32 sum may take the other neighbour: one ulp of ds times |x| per tap
        (slack,) = torch.autograd.grad((conv_s64(xd.abs(), wz) * _tie_ulps(dxs, dtype, 2e-4)).sum(), [wz])
        out["dw_s_" + form] = _within("dw_s vs fp64", dws_, dws64, 2e-4, 2e-4 * dws64.abs().max().item(), slack)
    B.check()
    return out


_RUN = {"x3d_stem_s_fwd": _run_s_fwd, "x3d_stem_s_wgrad": _run_s_wgrad, "x3d_dwt_fwd": _run_dwt_fwd, "x3d_dwt_bwd": _run_dwt_bwd,
        "x3d_stem_fwd": _run_stem_fwd, "x3d_stem_bwd": _run_stem_bwd}
