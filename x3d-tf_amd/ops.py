"""Tensor-level wrappers over the C ABI: shape inference + pointer plumbing, nothing else.

Every function launches hand-written HIP kernels from libx3d_hip.so on the current stream.  Tensors
are NCTHW activations (fp32 or bf16) and fp32 parameters / coefficient vectors, all on the GPU.
"""
import ctypes

import torch

from . import hip
from .hip import (ACT_NONE, ACT_RELU, ACT_SWISH, EPI_ADD, EPI_ADD_STRIDED, EPI_STORE,  # noqa: F401
                  EPI_SWISH_BWD, ptr)
from .solver import RULES, SLOT_NAMES


def _chk(*ts):
    for t in ts:
        if t is not None:
            if not t.is_cuda:
                raise hip.X3DHipError("x3d ops need GPU tensors (no CPU fallback)")
            if not t.is_contiguous():
                raise hip.X3DHipError("x3d ops need contiguous tensors")


def _out_hw(h, w, stride):
    return -(-h // stride), -(-w // stride)


# ---- stem ---------------------------------------------------------------------------------------
def stem_s_fwd(x, w, y=None, channels_last=False):
    """channels_last: x is the clip batch [N, T, H, W, Cin] as the reference's model takes it (X3D_LAYOUT_NTHWC)."""
    _chk(x, w, y)
    if channels_last:
        n, t, h, ww, cin = x.shape
    else:
        n, cin, t, h, ww = x.shape
    cout = w.shape[0]
    ho, wo = (h - 1) // 2 + 1, (ww - 1) // 2 + 1
    if y is None:
        y = torch.empty((n, cout, t, ho, wo), dtype=x.dtype, device=x.device)
    hip.call("x3d_stem_s_fwd", ptr(x), ptr(w), ptr(y), n, cin, t, h, ww, cout, hip.dtype_code(x.dtype), int(channels_last))
    return y


def stem_s_wgrad(x, dy, dw, channels_last=False):
    _chk(x, dy, dw)
    if channels_last:
        n, t, h, ww, cin = x.shape
    else:
        n, cin, t, h, ww = x.shape
    hip.call("x3d_stem_s_wgrad", ptr(x), ptr(dy), ptr(dw), n, cin, t, h, ww, dy.shape[1],
             hip.dtype_code(x.dtype), int(channels_last))


# ---- replicated statistics accumulators (include/x3d_hip.h) ----------------------------------------
def stats_buffer(c, device):
    """Zeroed accumulator in the library's replicated layout for c channels."""
    r, stride = hip.stats_layout(c)
    return torch.zeros(r * stride, dtype=torch.float64, device=device)


def stats_sum(buf, c):
    """[c, 2] totals of a replicated accumulator."""
    r, stride = hip.stats_layout(c)
    return buf.view(r, stride)[:, :2 * c].sum(0).view(c, 2)


_KEEP = []


class _Stats:
    """Producers called with a plain [C, 2] tensor (tests, tools) run on a temporary replicated accumulator whose
    totals are added to the tensor afterwards; a tensor already in the replicated layout is passed through."""

    def __init__(self, user, c):
        self.user, self.c, self.tmp = user, c, None
        if user is not None and user.numel() == 2 * c:
            self.tmp = stats_buffer(c, user.device)

    def arg(self):
        return self.user if self.tmp is None else self.tmp

    def done(self):
        if self.tmp is not None:
            self.user += stats_sum(self.tmp, self.c).view_as(self.user)


def _expand_stats(stats, c):
    """Consumers called with plain [C, 2] totals: replica 0 holds them, the others are zero."""
    if stats.numel() != 2 * c:
        return stats
    buf = stats_buffer(c, stats.device)
    buf[:2 * c] = stats.reshape(-1)
    return buf


def dwt_fwd(x, w, y=None, stats=None, out_ss=None, out_act=ACT_NONE):
    """out_ss [C][2]: the inference epilogue y = out_act(s*conv + t) (no statistics)."""
    _chk(x, w, y, stats, out_ss)
    n, c, t, h, ww = x.shape
    if y is None:
        y = torch.empty_like(x)
    st = _Stats(stats, c)
    hip.call("x3d_dwt_fwd", ptr(x), ptr(w), ptr(y), ptr(st.arg()), ptr(out_ss), out_act, n, c, t, h * ww, w.shape[1],
             hip.dtype_code(x.dtype))
    st.done()
    return y


def dwt_bwd(g, yraw, coef, x, w, dx, dw, relu_ss=None):
    """relu_ss [C][2]: g is the unmasked gradient, the ReLU mask of bn(yraw) is applied inside the kernel."""
    _chk(g, yraw, coef, x, w, dx, dw, relu_ss)
    n, c, t, h, ww = x.shape
    hip.call("x3d_dwt_bwd", ptr(g), ptr(yraw), ptr(relu_ss), ptr(coef), ptr(x), ptr(w), ptr(dx), ptr(dw), n, c, t,
             h * ww, w.shape[1], hip.dtype_code(x.dtype))


def stem_fused_supported(x, cout, kt=5):
    """x: the channels-last clip batch [N, T, H, W, Cin].  x3d_stem_fused_supported: bit 0 = stem_fwd takes the shape, bit 1 =
    stem_bwd takes it and is the faster backward."""
    n, t, h, ww, cin = x.shape
    code = hip.dtype_code(x.dtype)
    return int(hip.load().x3d_stem_fused_supported(cin, cout, kt, n, t, h, ww, code, 1))


def stem_fwd(x, w_s, w_t, y=None, stats=None, out_ss=None, out_act=ACT_NONE):
    """conv_s -> conv_t in one launch (x3d_stem_fwd): x is the channels-last clip batch [N, T, H, W, 3]; the conv_s output
    never reaches HBM.  stats / out_ss / out_act as in dwt_fwd."""
    _chk(x, w_s, w_t, y, stats, out_ss)
    n, t, h, ww, cin = x.shape
    cout = w_s.shape[0]
    ho, wo = (h - 1) // 2 + 1, (ww - 1) // 2 + 1
    if y is None:
        y = torch.empty((n, cout, t, ho, wo), dtype=x.dtype, device=x.device)
    st = _Stats(stats, cout)
    hip.call("x3d_stem_fwd", ptr(x), ptr(w_s), ptr(w_t), ptr(y), ptr(st.arg()), ptr(out_ss), out_act, n, cin, t, h, ww, cout,
             w_t.shape[1], hip.dtype_code(x.dtype), 1)
    st.done()
    return y


def stem_bwd(g, yraw, coef, x, w_s, w_t, dw_s, dw_t, relu_ss=None):
    """Backward of the fused stem (x3d_stem_bwd): dw_s, dw_t += ; the conv_s output is recomputed, its gradient stays on chip."""
    _chk(g, yraw, coef, x, w_s, w_t, dw_s, dw_t, relu_ss)
    n, t, h, ww, cin = x.shape
    hip.call("x3d_stem_bwd", ptr(g), ptr(yraw), ptr(relu_ss), ptr(coef), ptr(x), ptr(w_s), ptr(w_t), ptr(dw_s), ptr(dw_t),
             n, cin, t, h, ww, w_s.shape[0], w_t.shape[1], hip.dtype_code(x.dtype), 1)


# ---- batch norm ---------------------------------------------------------------------------------
def bn_finalize(stats, count, gamma, beta, mmean, mvar, eps, momentum, update, ss, mi):
    _chk(stats, gamma, beta, mmean, mvar, ss, mi)
    stats = _expand_stats(stats, gamma.numel())
    hip.call("x3d_bn_finalize", ptr(stats), float(count), ptr(gamma), ptr(beta), ptr(mmean), ptr(mvar),
             float(eps), float(momentum), int(update), ptr(ss), ptr(mi), gamma.numel())


def bn_fold(stats, count, gamma, beta, mmean, mvar, eps, momentum, update, ss, mi):
    """x3d_bn_fold for a consumer that runs the finalize itself (x3d_dw3d_fwd in_bn / x3d_tail_fwd_bn)."""
    _chk(stats, gamma, beta, mmean, mvar, ss, mi)
    stats = _expand_stats(stats, gamma.numel())
    _KEEP.append(stats)   # the struct holds a raw pointer
    del _KEEP[:-64]
    return hip.BnFold(ptr(stats), float(count), ptr(gamma), ptr(beta), ptr(mmean), ptr(mvar), float(eps), float(momentum),
                      int(update), ptr(ss), ptr(mi))


def bn_eval_coef(gamma, beta, mmean, mvar, eps, ss, mi):
    _chk(gamma, beta, mmean, mvar, ss, mi)
    item = hip.BnEvalItem(ptr(gamma), ptr(beta), ptr(mmean), ptr(mvar), ptr(ss), ptr(mi), gamma.numel())
    table = torch.frombuffer(bytearray(bytes(item)), dtype=torch.uint8).to(gamma.device)   # (the item table lives in device memory)
    hip.call("x3d_bn_eval_coef_batched", table.data_ptr(), 1, float(eps))
    torch.cuda.current_stream().synchronize()     # `table` is freed on return


def bn_bwd_finalize(sums, count, mi, gamma, coef, dgamma, dbeta):
    _chk(sums, mi, gamma, coef, dgamma, dbeta)
    hip.call("x3d_bn_bwd_finalize", ptr(sums), float(count), ptr(mi), ptr(gamma), ptr(coef),
             ptr(dgamma), ptr(dbeta), gamma.numel())


# ---- pointwise ----------------------------------------------------------------------------------
def pw_pack_weights(weights, dgrad=True, dtype=torch.bfloat16):
    """fp32 [Cout, Cin] weights -> list of (fwd_panel, dgrad_panel) LDS-image panels of the 16-bit storage type `dtype`,
    one launch (x3d_pw_pack_weights)."""
    lib = hip.load()
    items = (hip.PwPackItem * len(weights))()
    out = []
    for i, w in enumerate(weights):
        _chk(w)
        cout, cin = w.shape
        fp = torch.empty(lib.x3d_pw_panel_elems(cout, cin), dtype=dtype, device=w.device)
        dp = torch.empty(lib.x3d_pw_panel_elems(cin, cout), dtype=dtype, device=w.device) if dgrad else None
        items[i] = hip.PwPackItem(ptr(w), ptr(fp), ptr(dp), cout, cin)
        out.append((fp, dp))
    table = torch.frombuffer(bytearray(bytes(items)), dtype=torch.uint8).to(weights[0].device)
    hip.call("x3d_pw_pack_weights", table.data_ptr(), len(weights), hip.dtype_code(dtype))
    torch.cuda.current_stream().synchronize()   # `table` must outlive the launch
    return out


def pw_fwd(x, w, y=None, stats=None, in_ss=None, in_gate=None, in_act=ACT_NONE, stride=1, w_panel=None,
           out_ss=None, out_add=None, out_add_ss=None, out_act=ACT_NONE, in_add=None, in_add_ss=None, in_store=None):
    """out_ss [Cout][2]: the inference epilogue y = out_act(s_o*acc + t_o [+ s_r*out_add + t_r]) (no statistics).
    in_add / in_add_ss / in_store: the residual tail of the block below folded into the prologue (x = its raw c output)."""
    _chk(x, w, y, stats, in_ss, in_gate, w_panel, out_ss, out_add, out_add_ss, in_add, in_add_ss, in_store)
    n, cin, t, h, ww = x.shape
    cout = w.shape[0]
    ho, wo = _out_hw(h, ww, stride)
    if y is None:
        y = torch.empty((n, cout, t, ho, wo), dtype=x.dtype, device=x.device)
    st = _Stats(stats, cout)
    a = hip.PwFwdArgs(ptr(x), ptr(w), ptr(y), ptr(st.arg()), ptr(in_ss), ptr(in_gate), in_act, n, cin,
                      cout, t, h, ww, stride, hip.dtype_code(x.dtype), ptr(w_panel), in_add=ptr(in_add),
                      in_add_scale_shift=ptr(in_add_ss), in_store=ptr(in_store), out_scale_shift=ptr(out_ss),
                      out_add=ptr(out_add), out_add_scale_shift=ptr(out_add_ss), out_act=out_act)
    hip.call_struct("x3d_pw_fwd", a)
    st.done()
    return y


def bn_bwd_fold(sums, count, mi, gamma, dgamma=None, dbeta=None, coef_out=None):
    """x3d_bn_bwd_fold for the `coef_fold` argument of pw_dgrad / pw_wgrad / pw_bwd: the consumer derives its coefficient table
    from the BatchNorm-backward sums; dgamma / dbeta / coef_out: this launch also publishes them (one launch per BatchNorm)."""
    _chk(sums, mi, gamma, dgamma, dbeta, coef_out)
    f = hip.BnBwdFold(ptr(sums), float(count), ptr(mi), ptr(gamma), ptr(dgamma), ptr(dbeta), ptr(coef_out))
    _KEEP.append((f, sums, mi, gamma, dgamma, dbeta, coef_out))
    del _KEEP[:-64]
    return f


def pw_dgrad(g, yraw, coef, w, dx, epi=EPI_STORE, add=None, braw=None, b_ss=None, gate=None,
             nc_sums=None, w_panel=None, coef_fold=None):
    """g/yraw: [N,Cout,T,H,W]; dx: [N,Cin,T,H,W]."""
    _chk(g, yraw, coef, w, dx, add, braw, b_ss, gate, nc_sums)
    n, cout, t, h, ww = g.shape
    cin = w.shape[1]
    a = hip.PwDgradArgs(ptr(g), ptr(yraw), ptr(coef), ptr(w), ptr(dx), epi, ptr(add), ptr(braw),
                        ptr(b_ss), ptr(gate), ptr(nc_sums), n, cin, cout, t, h, ww,
                        hip.dtype_code(g.dtype), ptr(w_panel))
    if coef_fold is not None:
        a.coef_fold = hip.fold_address(coef_fold)
    hip.call_struct("x3d_pw_dgrad", a)
    return dx


def pw_bwd(g, yraw, coef, w_panel, dx, dw, epi, x=None, add=None, braw=None, b_ss=None, gate=None, nc_sums=None,
           tail_c=None, tail_r=None, tail_sums_c=None, tail_sums_r=None, slab=False, coef_fold=None):
    """Fused dgrad + wgrad (x3d_pw_bwd).  g/yraw: [N,Cout,T,H,W]; dx: [N,Cin,T,H,W]; dw: [Cout,Cin] +=.
    tail_c (/ tail_r) + their [Cin, 2] fp64 sums: the folded Add + ReLU backward of the block whose output is x.
    slab: the weight gradient through per-workgroup partial slabs + x3d_dw_slab_reduce instead of fp32 atomics (None is
    returned when the kernel behind the call has no slab form).
    Returns False (nothing launched) when the fused kernel does not cover the call."""
    _chk(g, yraw, coef, w_panel, dx, dw, x, add, braw, b_ss, gate, nc_sums, tail_c, tail_r, tail_sums_c, tail_sums_r)
    n, cout, t, h, ww = g.shape
    cin = dx.shape[1]
    a = hip.PwBwdArgs(ptr(g), ptr(yraw), ptr(coef), ptr(w_panel), ptr(dx), epi, ptr(add), ptr(braw), ptr(b_ss),
                      ptr(gate), ptr(nc_sums), ptr(x), ptr(dw), n, cin, cout, t, h, ww, hip.dtype_code(g.dtype),
                      ptr(tail_c), ptr(tail_r), ptr(tail_sums_c), ptr(tail_sums_r))
    if coef_fold is not None:
        a.coef_fold = hip.fold_address(coef_fold)
    if not hip.load().x3d_pw_bwd_supported(ctypes.byref(a)):
        return False
    if slab:
        parts = int(hip.load().x3d_pw_bwd_dw_parts(ctypes.byref(a)))
        if parts <= 0:
            return None
        buf = torch.full((parts * cout * cin,), float("nan"), dtype=torch.float32, device=g.device)   # (every slab element must be written)
        a.dw_slab, a.dw_slab_parts = ptr(buf), parts
        hip.call_struct("x3d_pw_bwd", a)
        dw_slab_reduce([(buf, dw, parts)])
        return True
    hip.call_struct("x3d_pw_bwd", a)
    return True


def dw_reduce_jobs(jobs):
    """[(slab [parts * elems] fp32, dw [elems...] fp32, parts), ...] -> a ctypes array of x3d_dw_reduce_job"""
    arr = (hip.DwReduceJob * max(len(jobs), 1))()
    for i, (slab_, dw_, parts) in enumerate(jobs):
        _chk(slab_, dw_)
        assert slab_.numel() == parts * dw_.numel()
        arr[i] = hip.DwReduceJob(ptr(slab_), ptr(dw_), parts, dw_.numel())
    return arr


def dw_slab_reduce(jobs):
    """dw += sum of its partial slabs (x3d_dw_slab_reduce): one or two jobs."""
    arr = dw_reduce_jobs(jobs)
    hip.call("x3d_dw_slab_reduce", arr, len(jobs))


def pw_bwd_rc(g, x, w, coef, dx, dw, epi, add, tail_c=None, tail_r=None, tail_sums_c=None, tail_sums_r=None, x_stride=1):
    """Fused dgrad + wgrad of an `a` conv WITHOUT its raw output (x3d_pw_bwd with rc_panel: the conv output y = W x is
    folded algebraically into the BatchNorm backward dY = A g + B y + C).  Three launches: x3d_pw_bwd_rc_prepare (per-step panel
    [W^T diag(A) | W^T diag(B) W] and c0 = W^T C from the fp32 weights w [Cout, Cin] and coef [Cout, 4]), x3d_pw_bwd (streams
    g and x only), x3d_pw_bwd_rc_finish (dw += from the moment sums).  x_stride = 2: the strided shortcut conv (x is the
    block input, g / dx live at the sampled pixels; epi = EPI_STORE, add = None).  Returns False (nothing launched) when the
    shape is not covered."""
    _chk(g, x, w, coef, dx, dw, add, tail_c, tail_r, tail_sums_c, tail_sums_r)
    n, cout, t, h, ww = g.shape
    cin = dx.shape[1]
    lib = hip.load()
    pe = int(lib.x3d_pw_bwd_rc_panel_elems(cout, cin))
    if pe == 0:
        return False
    panel = torch.empty(pe, dtype=g.dtype, device=g.device)
    c0 = torch.empty(cin, dtype=torch.float32, device=g.device)
    sums = torch.zeros(int(lib.x3d_pw_bwd_rc_sums_elems(cout, cin)), dtype=torch.float32, device=g.device)
    a = hip.PwBwdArgs(ptr(g), None, None, None, ptr(dx), epi, ptr(add), None, None, None, None, ptr(x), None, n, cin, cout,
                      t, h, ww, hip.dtype_code(g.dtype), ptr(tail_c), ptr(tail_r), ptr(tail_sums_c), ptr(tail_sums_r),
                      ptr(panel), ptr(c0), ptr(sums), x_stride, x.shape[3], x.shape[4])
    if not lib.x3d_pw_bwd_supported(ctypes.byref(a)):
        return False
    dt = hip.dtype_code(g.dtype)
    hip.call("x3d_pw_bwd_rc_prepare", ptr(w), ptr(coef), ptr(panel), ptr(c0), cout, cin, dt)
    hip.call_struct("x3d_pw_bwd", a)
    hip.call("x3d_pw_bwd_rc_finish", ptr(sums), ptr(w), ptr(coef), ptr(dw), cout, cin, dt)
    return True


def bn_bwd_finalize_rc(sums, count, mi, gamma, coef, dgamma, dbeta, dtype, prep=None, fin=None):
    """x3d_bn_bwd_finalize_rc: the BatchNorm-backward finalize + (prep = (w, panel, c0)) the recomputed-output panel of the conv
    in front of this BatchNorm + (fin = (sums, w, coef, dw)) the pending dW of an earlier x3d_pw_bwd, one launch."""
    w, panel, c0 = prep if prep is not None else (None, None, None)
    fs, fw, fc, fdw = fin if fin is not None else (None, None, None, None)
    _chk(sums, mi, gamma, coef, dgamma, dbeta, w, panel, c0, fs, fw, fc, fdw)
    hip.call("x3d_bn_bwd_finalize_rc", ptr(sums), float(count), ptr(mi), ptr(gamma), ptr(coef), ptr(dgamma), ptr(dbeta),
             gamma.numel(), ptr(w), ptr(panel), ptr(c0), 0 if w is None else w.shape[1], ptr(fs), ptr(fw), ptr(fc), ptr(fdw),
             0 if fw is None else fw.shape[0], 0 if fw is None else fw.shape[1], hip.dtype_code(dtype))


def pw_wgrad(g, yraw, coef, x, dw, in_ss=None, in_gate=None, in_act=ACT_NONE, stride=1, slab=False, coef_fold=None):
    """x: conv input [N,Cin,T,H,W] (input extents); g/yraw at the output points.  slab: through partial slabs +
    x3d_dw_slab_reduce (returns None, nothing launched, when the kernel behind the call has no slab form)."""
    _chk(g, yraw, coef, x, dw, in_ss, in_gate)
    n, cin, t, h, ww = x.shape
    cout = g.shape[1]
    a = hip.PwWgradArgs(ptr(g), ptr(yraw), ptr(coef), ptr(x), ptr(in_ss), ptr(in_gate), in_act, ptr(dw),
                        n, cin, cout, t, h, ww, stride, hip.dtype_code(x.dtype))
    if coef_fold is not None:
        a.coef_fold = hip.fold_address(coef_fold)
    if slab:
        parts = int(hip.load().x3d_pw_wgrad_dw_parts(ctypes.byref(a)))
        if parts <= 0:
            return None
        buf = torch.full((parts * cout * cin,), float("nan"), dtype=torch.float32, device=g.device)   # (every slab element must be written)
        a.dw_slab, a.dw_slab_parts = ptr(buf), parts
        hip.call_struct("x3d_pw_wgrad", a)
        dw_slab_reduce([(buf, dw, parts)])
        return True
    hip.call_struct("x3d_pw_wgrad", a)
    return True


# ---- depthwise ----------------------------------------------------------------------------------
def dw3d_fwd(x, w, stride, y=None, in_ss=None, in_act=ACT_NONE, stats=None, pool=None, in_bn=None, dilation=1):
    """in_bn: an ops.bn_fold(...) struct -- the prologue's BatchNorm finalize runs inside the kernel (in_ss unused).
    dilation >= 2: the dilated form, x3d_dw3d_fwd_dil (stride 1, padding `dilation`: y has x's extents)."""
    _chk(x, w, y, in_ss, stats, pool)
    n, c, t, h, ww = x.shape
    ho, wo = _out_hw(h, ww, stride)
    if y is None:
        y = torch.empty((n, c, t, ho, wo), dtype=x.dtype, device=x.device)
    st = _Stats(stats, c)
    a = hip.Dw3dFwdArgs(ptr(x), ptr(w), ptr(y), ptr(in_ss), in_act, ptr(st.arg()), ptr(pool), n, c, t, h,
                        ww, stride, hip.dtype_code(x.dtype), None if in_bn is None else ctypes.pointer(in_bn))
    if int(dilation) in (0, 1):
        hip.call_struct("x3d_dw3d_fwd", a)
    else:
        hip.call_struct_dil("x3d_dw3d_fwd_dil", a, dilation)
    st.done()
    return y


def dw3d_bwd(dv, braw, coef_nc, araw, a_ss, w, ga, a_sums, dw, stride, dilation=1):
    _chk(dv, braw, coef_nc, araw, a_ss, w, ga, a_sums, dw)
    n, c, t, h, ww = araw.shape
    a = hip.Dw3dBwdArgs(ptr(dv), ptr(braw), ptr(coef_nc), ptr(araw), ptr(a_ss), ptr(w), ptr(ga),
                        ptr(a_sums), ptr(dw), n, c, t, h, ww, stride, hip.dtype_code(araw.dtype))
    if int(dilation) in (0, 1):
        hip.call_struct("x3d_dw3d_bwd", a)
    else:
        hip.call_struct_dil("x3d_dw3d_bwd_dil", a, dilation)


# ---- squeeze-excite -----------------------------------------------------------------------------
def se_fwd(pool_sums, P, b_ss, w1, b1, w2, b2, gate, hidden):
    _chk(pool_sums, b_ss, w1, b1, w2, b2, gate, hidden)
    n, c = gate.shape
    hip.call("x3d_se_fwd", ptr(pool_sums), float(P), ptr(b_ss), ptr(w1), ptr(b1), ptr(w2), ptr(b2),
             ptr(gate), ptr(hidden), n, c, w1.shape[0])


def se_bnb_bwd(nc_sums, pool_sums, P, b_ss, b_mi, gamma_b, dgamma_b, dbeta_b, coef_nc, N, C,
               w1=None, b1=None, w2=None, b2=None, gate=None, hidden=None, dw1=None, db1=None,
               dw2=None, db2=None, scratch=None, reduce=()):
    """reduce: up to two (slab, dw, parts) weight-gradient slab jobs added up by extra workgroups of the launch."""
    _chk(nc_sums, pool_sums, b_ss, b_mi, gamma_b, dgamma_b, dbeta_b, coef_nc, w1, b1, w2, b2, gate,
         hidden, dw1, db1, dw2, db2, scratch)
    a = hip.SeBnbBwdArgs(ptr(nc_sums), ptr(pool_sums), float(P), ptr(b_ss), ptr(b_mi), ptr(gamma_b),
                         ptr(w1), ptr(b1), ptr(w2), ptr(b2), ptr(gate), ptr(hidden), ptr(dw1),
                         ptr(db1), ptr(dw2), ptr(db2), ptr(dgamma_b), ptr(dbeta_b), ptr(coef_nc),
                         ptr(scratch), N, C, 0 if w1 is None else w1.shape[0])
    for i, job in enumerate(dw_reduce_jobs(list(reduce))[:len(reduce)]):
        a.reduce[i] = job
    hip.call_struct("x3d_se_bnb_bwd", a)


# ---- residual tail / reductions -----------------------------------------------------------------
def tail_fwd(c_raw, c_ss, shortcut, r_ss, y):
    _chk(c_raw, c_ss, shortcut, r_ss, y)
    n, c = c_raw.shape[:2]
    hip.call("x3d_tail_fwd", ptr(c_raw), ptr(c_ss), ptr(shortcut), ptr(r_ss), ptr(y), n, c,
             c_raw[0, 0].numel(), hip.dtype_code(c_raw.dtype))
    return y


def tail_fwd_bn(c_raw, c_bn, shortcut, r_bn, y):
    """tail_fwd with the finalize of bn_c (and bn_r) folded in; c_bn / r_bn: ops.bn_fold(...) structs."""
    _chk(c_raw, shortcut, y)
    n, c = c_raw.shape[:2]
    hip.call("x3d_tail_fwd_bn", ptr(c_raw), ctypes.byref(c_bn), ptr(shortcut), None if r_bn is None else ctypes.byref(r_bn),
             ptr(y), n, c, c_raw[0, 0].numel(), hip.dtype_code(c_raw.dtype))
    return y


def tail_bwd(dy_g, y, c_raw, r_raw, sums_c, sums_r):
    _chk(dy_g, y, c_raw, r_raw, sums_c, sums_r)
    n, c = y.shape[:2]
    hip.call("x3d_tail_bwd", ptr(dy_g), ptr(y), ptr(c_raw), ptr(r_raw), ptr(sums_c), ptr(sums_r), n, c,
             y[0, 0].numel(), hip.dtype_code(y.dtype))


def tail_fwd_dp(c_raw, c_ss, shortcut, r_ss, keep, y):
    """tail_fwd with stochastic depth: y = relu(keep[n] * bn_c(c_raw) + shortcut); keep [N] fp32 (x3d_tail_fwd_dp)."""
    _chk(c_raw, c_ss, shortcut, r_ss, keep, y)
    n, c = c_raw.shape[:2]
    if keep.dtype != torch.float32 or keep.numel() != n:
        raise ValueError(f"tail_fwd_dp: keep must be {n} float32, got {keep.numel()} {keep.dtype}")
    hip.call("x3d_tail_fwd_dp", ptr(c_raw), ptr(c_ss), ptr(shortcut), ptr(r_ss), ptr(keep), ptr(y), n, c,
             c_raw[0, 0].numel(), hip.dtype_code(c_raw.dtype))
    return y


def tail_bwd_dp(dy_g, g_branch, y, c_raw, r_raw, keep, sums_c, sums_r):
    """tail_bwd with stochastic depth: g = dy * [y > 0] in place, g_branch = keep[n] * g (x3d_tail_bwd_dp)."""
    _chk(dy_g, g_branch, y, c_raw, r_raw, keep, sums_c, sums_r)
    n, c = y.shape[:2]
    if keep.dtype != torch.float32 or keep.numel() != n:
        raise ValueError(f"tail_bwd_dp: keep must be {n} float32, got {keep.numel()} {keep.dtype}")
    hip.call("x3d_tail_bwd_dp", ptr(dy_g), ptr(g_branch), ptr(y), ptr(c_raw), ptr(r_raw), ptr(keep), ptr(sums_c), ptr(sums_r),
             n, c, y[0, 0].numel(), hip.dtype_code(y.dtype))


def drop_path_state(seed, step=0, device="cuda"):
    """The device state of x3d_drop_path_draw: int32 [4] holding the uint32 words (seed_lo, seed_hi, step_lo, step_hi)."""
    seed, step = int(seed) & (2 ** 64 - 1), int(step) & (2 ** 64 - 1)
    words = [seed & 0xFFFFFFFF, seed >> 32, step & 0xFFFFFFFF, step >> 32]
    return torch.tensor([w - (1 << 32) if w >= (1 << 31) else w for w in words], dtype=torch.int32, device=device)


def drop_path_step(state):
    """The 64-bit step counter a drop-path state holds (synchronises)."""
    w = [int(v) & 0xFFFFFFFF for v in state.tolist()]
    return w[2] | (w[3] << 32)


def drop_path_draw(keep, rates, state):
    """keep [L][N] fp32 <- the table of the step `state` holds; the step advances by one on the device (x3d_drop_path_draw)."""
    _chk(keep, rates, state)
    nl, n = keep.shape
    if keep.dtype != torch.float32 or rates.dtype != torch.float32 or rates.numel() != nl:
        raise ValueError(f"drop_path_draw: keep [L][N] and rates [L] must be float32, got {keep.dtype} / {rates.numel()} {rates.dtype}")
    if state.dtype != torch.int32 or state.numel() != 4:
        raise ValueError("drop_path_draw: state must be the int32 [4] tensor of drop_path_state()")
    hip.call("x3d_drop_path_draw", ptr(keep), ptr(rates), ptr(state), nl, n)
    return keep


def relu_bn_bwd_reduce(dy, dpool, yraw, ss, g, sums):
    _chk(dy, dpool, yraw, ss, g, sums)
    n, c = yraw.shape[:2]
    hip.call("x3d_relu_bn_bwd_reduce", ptr(dy), ptr(dpool), ptr(yraw), ptr(ss), ptr(g), ptr(sums), n, c,
             yraw[0, 0].numel(), hip.dtype_code(yraw.dtype))


def pool_fwd(x_raw, ss, pooled):
    _chk(x_raw, ss, pooled)
    n, c = x_raw.shape[:2]
    hip.call("x3d_pool_fwd", ptr(x_raw), ptr(ss), ptr(pooled), n, c, x_raw[0, 0].numel(),
             hip.dtype_code(x_raw.dtype))
    return pooled


ROI_MAX_HW, ROI_MAX_R, ROI_MAX_K, ROI_MAX_ROWS = 1024, 15, 64, 2048   # the limits of x3d_roi_pool_fwd / _bwd (include/x3d_hip.h)


def roi_limits(name, n, hw, k, r, sampling_ratio, spatial_scale):
    """The refusals of x3d_roi_pool_fwd / x3d_roi_pool_bwd as ValueErrors that name the argument (config.py and the plan
    recorder state them through this too, before anything is allocated or launched)."""
    if not 1 <= int(r) <= ROI_MAX_R:
        raise ValueError(f"{name}: resolution R = {r} must be in 1..{ROI_MAX_R}")
    if not 1 <= int(k) <= ROI_MAX_K:
        raise ValueError(f"{name}: boxes holds K = {k} slots per clip, must be in 1..{ROI_MAX_K}")
    if int(n) * int(k) > ROI_MAX_ROWS:
        raise ValueError(f"{name}: boxes gives N*K = {int(n) * int(k)} rows, at most {ROI_MAX_ROWS}")
    if hw is not None and int(hw) > ROI_MAX_HW:
        raise ValueError(f"{name}: the feature map has H*W = {hw} pixels, at most {ROI_MAX_HW}")
    if int(sampling_ratio) < 0:
        raise ValueError(f"{name}: sampling_ratio = {sampling_ratio} must be >= 0")
    if not 0.0 < float(spatial_scale) < float("inf"):
        raise ValueError(f"{name}: spatial_scale = {spatial_scale} must be positive and finite")


def _roi_args(name, fmap, ss, boxes, num_boxes, rows, argmax, resolution, sampling_ratio, spatial_scale):
    """the tensor checks both ROI wrappers make; rows: {what: fp32 [N*K, C] tensor}.  Returns (N, C, T, H, W, K)."""
    if fmap.dim() != 5:
        raise ValueError(f"{name}: the feature map must be [N, C, T, H, W], got {tuple(fmap.shape)}")
    n, c, t, h, w = fmap.shape
    if boxes.dtype != torch.float32 or boxes.dim() != 3 or boxes.shape[0] != n or boxes.shape[2] != 4:
        raise ValueError(f"{name}: boxes must be [{n}, K, 4] float32, got {tuple(boxes.shape)} {boxes.dtype}")
    k = boxes.shape[1]
    if num_boxes.dtype != torch.int32 or tuple(num_boxes.shape) != (n,):
        raise ValueError(f"{name}: num_boxes must be [{n}] int32, got {tuple(num_boxes.shape)} {num_boxes.dtype}")
    roi_limits(name, n, h * w, k, resolution, sampling_ratio, spatial_scale)
    if ss.dtype != torch.float32 or ss.numel() != 2 * c:
        raise ValueError(f"{name}: scale_shift must be [{c}, 2] float32, got {tuple(ss.shape)} {ss.dtype}")
    for what, r in rows.items():
        _f32_2d(name, what, r, (n * k, c))
    if argmax is not None and (argmax.dtype != torch.uint8 or tuple(argmax.shape) != (n * k, c)):
        raise ValueError(f"{name}: argmax must be [{n * k}, {c}] uint8, got {tuple(argmax.shape)} {argmax.dtype}")
    return n, c, t, h, w, k


def roi_pool_fwd(x_raw, ss, boxes, num_boxes, pooled, argmax=None, resolution=7, sampling_ratio=0, spatial_scale=1.0 / 32):
    """pooled [N*K, C] fp32 = per box, the spatial max over resolution^2 ROIAlign bins of mean_t relu(s*x_raw + t)
    (x3d_roi_pool_fwd: the rules are in include/x3d_hip.h).  boxes [N, K, 4] fp32 in pixels of the clip, num_boxes [N] int32;
    argmax [N*K, C] uint8 receives the winning bin (None: inference).  One launch, does not synchronise."""
    n, c, t, h, w, k = _roi_args("roi_pool_fwd", x_raw, ss, boxes, num_boxes, dict(pooled=pooled), argmax, resolution,
                                 sampling_ratio, spatial_scale)
    _chk(x_raw, ss, boxes, num_boxes, pooled, argmax)
    hip.call("x3d_roi_pool_fwd", ptr(x_raw), ptr(ss), ptr(boxes), ptr(num_boxes), ptr(pooled), ptr(argmax), n, c, t, h, w, k,
             int(resolution), int(sampling_ratio), float(spatial_scale), hip.dtype_code(x_raw.dtype))
    return pooled


def roi_pool_bwd(dpooled, argmax, boxes, num_boxes, yraw, ss, g, sums, resolution=7, sampling_ratio=0,
                 spatial_scale=1.0 / 32):
    """g [N, C, T, H, W] = the gradient of roi_pool_fwd's input through the ReLU of s*yraw + t, given dpooled [N*K, C] and the
    forward's argmax; sums [C, 2] fp64 += (sum g, sum g*yraw) (x3d_roi_pool_bwd).  One launch, does not synchronise."""
    n, c, t, h, w, k = _roi_args("roi_pool_bwd", yraw, ss, boxes, num_boxes, dict(dpooled=dpooled), argmax, resolution,
                                 sampling_ratio, spatial_scale)
    if argmax is None:
        raise ValueError("roi_pool_bwd: argmax is required")
    if g.dtype != yraw.dtype or tuple(g.shape) != tuple(yraw.shape):
        raise ValueError(f"roi_pool_bwd: g must be {tuple(yraw.shape)} {yraw.dtype}, got {tuple(g.shape)} {g.dtype}")
    if sums.dtype != torch.float64 or sums.numel() != 2 * c:
        raise ValueError(f"roi_pool_bwd: sums must be [{c}, 2] float64, got {tuple(sums.shape)} {sums.dtype}")
    _chk(dpooled, argmax, boxes, num_boxes, yraw, ss, g, sums)
    hip.call("x3d_roi_pool_bwd", ptr(dpooled), ptr(argmax), ptr(boxes), ptr(num_boxes), ptr(yraw), ptr(ss), ptr(g), ptr(sums),
             n, c, t, h, w, k, int(resolution), int(sampling_ratio), float(spatial_scale), hip.dtype_code(yraw.dtype))


# ---- head ---------------------------------------------------------------------------------------
def dense_fwd(x, w, b, y, act=ACT_NONE, mask=None, mask_scale=1.0):
    _chk(x, w, b, y, mask)
    n, k = x.shape
    hip.call("x3d_dense_fwd", ptr(x), ptr(mask), float(mask_scale), ptr(w), ptr(b), ptr(y), act, n, k,
             w.shape[0])
    return y


def dense_bwd(dy, y, act, x, w, dx, dw, db, mask=None, mask_scale=1.0):
    _chk(dy, y, x, w, dx, dw, db, mask)
    n, k = x.shape
    hip.call("x3d_dense_bwd", ptr(dy), ptr(y), act, ptr(x), ptr(mask), float(mask_scale), ptr(w),
             ptr(dx), ptr(dw), ptr(db), n, k, w.shape[0])


def softmax_xent(logits, labels, probs, loss_rows=None, dlogits=None, grad_scale=1.0):
    _chk(logits, labels, probs, loss_rows, dlogits)
    n, m = logits.shape
    hip.call("x3d_softmax_xent", ptr(logits), ptr(labels), ptr(probs), ptr(loss_rows), ptr(dlogits),
             float(grad_scale), n, m)
    return probs


def view_mean(probs, out, views):
    _chk(probs, out)
    hip.call("x3d_view_mean", ptr(probs), ptr(out), out.shape[0], views, probs.shape[1])
    return out


def topk_metrics(probs, labels, acc, k=5):
    """acc [4] fp64 += (sum of loss rows, top-1 hits, top-k hits, rows) of probs [N, M] fp32 against labels [N] int32 |
    int64 (x3d_topk_metrics: the rules are in include/x3d_hip.h).  Launches one kernel, does not synchronise."""
    _chk(probs, labels, acc)
    if probs.dtype != torch.float32 or probs.dim() != 2:
        raise ValueError(f"topk_metrics: probs must be [N, M] float32, got {tuple(probs.shape)} {probs.dtype}")
    if labels.dtype not in (torch.int32, torch.int64) or labels.dim() != 1 or labels.shape[0] != probs.shape[0]:
        raise ValueError(f"topk_metrics: labels must be [{probs.shape[0]}] int32 or int64, got {tuple(labels.shape)} "
                         f"{labels.dtype}")
    if acc.dtype != torch.float64 or acc.numel() != 4:
        raise ValueError(f"topk_metrics: acc must be 4 float64 counters, got {acc.numel()} {acc.dtype}")
    if not probs.device == labels.device == acc.device:
        raise ValueError("topk_metrics: probs, labels and acc must be on one device")
    if int(k) < 1:
        raise ValueError(f"topk_metrics: k = {k} (k >= 1)")
    hip.call("x3d_topk_metrics", ptr(probs), ptr(labels), labels.element_size(), ptr(acc), probs.shape[0],
             probs.shape[1], int(k))
    return acc



def _f32_2d(name, what, t, shape=None):
    if t.dtype != torch.float32 or t.dim() != 2 or (shape is not None and tuple(t.shape) != tuple(shape)):
        want = f"[{shape[0]}, {shape[1]}]" if shape is not None else "[N, M]"
        raise ValueError(f"{name}: {what} must be {want} float32, got {tuple(t.shape)} {t.dtype}")


def _loss_args(name, logits, probs, mats, rows):
    """the tensor checks of the loss wrappers (all but softmax_xent's): logits and probs [N, M] float32, every tensor given in
    `mats` ({what: tensor or None}) the same, every one in `rows` N float32; returns (N, M)"""
    _f32_2d(name, "logits", logits)
    n, m = logits.shape
    _f32_2d(name, "probs", probs, (n, m))
    for what, t in mats.items():
        if t is not None:
            _f32_2d(name, what, t, (n, m))
    for what, t in rows.items():
        if t is not None and (t.dtype != torch.float32 or t.numel() != n):
            raise ValueError(f"{name}: {what} must be {n} float32, got {t.numel()} {t.dtype}")
    return n, m


def sigmoid_bce(logits, targets, probs, loss_rows=None, dlogits=None, grad_scale=1.0):
    """probs = sigmoid(logits); with targets [N, M] fp32 in [0, 1]: loss_rows [N] = Keras BinaryCrossentropy per row,
    dlogits = grad_scale * (probs - targets) / M (x3d_sigmoid_bce: the rules are in include/x3d_hip.h).  targets=None
    computes probs only.  One launch, does not synchronise."""
    _chk(logits, targets, probs, loss_rows, dlogits)
    if targets is None and (loss_rows is not None or dlogits is not None):
        raise ValueError("sigmoid_bce: loss_rows / dlogits need targets")
    n, m = _loss_args("sigmoid_bce", logits, probs, dict(targets=targets, dlogits=dlogits), dict(loss_rows=loss_rows))
    hip.call("x3d_sigmoid_bce", ptr(logits), ptr(targets), ptr(probs), ptr(loss_rows), ptr(dlogits),
             float(grad_scale), n, m)
    return probs


def view_max(probs, out, views):
    """out[v] = element-wise max of probs[v * views : (v + 1) * views] (NaN propagates)."""
    _chk(probs, out)
    _f32_2d("view_max", "probs", probs)
    if probs.shape[0] % int(views) or int(views) < 1:
        raise ValueError(f"view_max: {probs.shape[0]} rows are not a multiple of views = {views}")
    _f32_2d("view_max", "out", out, (probs.shape[0] // int(views), probs.shape[1]))
    hip.call("x3d_view_max", ptr(probs), ptr(out), out.shape[0], int(views), probs.shape[1])
    return out


def multilabel_ap(scores, targets, ap=None, npos=None, check=True):
    """Per-class average precision of scores [N, M] fp32 against targets [N, M] fp32 (>= 0.5 = positive):
    (ap [M] float64, npos [M] int32), x3d_multilabel_ap (the rules are in include/x3d_hip.h).  A class without positives
    or with a NaN score has ap NaN.  One launch; it synchronises only when N > AP_MAX_POSITIVES and `check` is set, to
    raise if a class has more positives than the kernel holds (npos < 0: never truncated)."""
    _chk(scores, targets, ap, npos)
    _f32_2d("multilabel_ap", "scores", scores)
    n, m = scores.shape
    _f32_2d("multilabel_ap", "targets", targets, (n, m))
    if n < 1 or m < 1:
        raise ValueError(f"multilabel_ap: empty [{n}, {m}]")
    if n * m >= 2 ** 31:
        raise ValueError(f"multilabel_ap: N * M = {n * m} >= 2^31")
    if scores.device != targets.device:
        raise ValueError("multilabel_ap: scores and targets must be on one device")
    if ap is None:
        ap = torch.empty(m, dtype=torch.float64, device=scores.device)
    if npos is None:
        npos = torch.empty(m, dtype=torch.int32, device=scores.device)
    if ap.dtype != torch.float64 or ap.numel() != m or npos.dtype != torch.int32 or npos.numel() != m:
        raise ValueError(f"multilabel_ap: ap must be {m} float64 and npos {m} int32")
    hip.call("x3d_multilabel_ap", ptr(scores), ptr(targets), n, m, ptr(ap), ptr(npos))
    if check and n > hip.AP_MAX_POSITIVES:
        over = npos < 0
        if bool(over.any()):
            cls = over.nonzero().flatten().tolist()
            raise ValueError(f"multilabel_ap: classes {cls[:5]} have more than {hip.AP_MAX_POSITIVES} positives")
    return ap, npos


FRAME_MAX_BOXES = 64   # K and G of x3d_frame_match (include/x3d_hip.h)


def _frame_tensor(name, what, t, dtype, shape, device):
    if not torch.is_tensor(t) or t.dtype != dtype or tuple(t.shape) != tuple(shape):
        got = f"{tuple(t.shape)} {t.dtype}" if torch.is_tensor(t) else type(t).__name__
        raise ValueError(f"{name}: {what} must be {list(shape)} {str(dtype).replace('torch.', '')}, got {got}")
    if t.device != device:
        raise ValueError(f"{name}: {what} is on {t.device}, scores on {device}: all tensors must be on one device")


def frame_match(scores, boxes, num_boxes, gt_boxes, gt_labels, num_gt, iou_threshold=0.5, tp=None, det_scores=None, ngt=None):
    """The frame-mAP matching of a batch of images (x3d_frame_match: the rules are in include/x3d_hip.h): scores [I*K, C] fp32,
    boxes [I, K, 4] fp32 with num_boxes [I] int32 (the proposals), gt_boxes [I, G, 4] fp32 with num_gt [I] int32 and gt_labels
    [I, G, C] uint8 (the annotated boxes and the classes each carries).  Returns (tp [I*K, C] uint8, det_scores [I*K, C] fp32,
    ngt [C] int32); a given ngt is INCREMENTED, a missing one starts at zero.  One launch, does not synchronise."""
    name = "frame_match"
    if not torch.is_tensor(scores) or scores.dtype != torch.float32 or scores.dim() != 2:
        got = f"{tuple(scores.shape)} {scores.dtype}" if torch.is_tensor(scores) else type(scores).__name__
        raise ValueError(f"{name}: scores must be [I*K, C] float32, got {got}")
    rows, c = scores.shape
    if not torch.is_tensor(boxes) or boxes.dim() != 3 or boxes.shape[2] != 4:
        raise ValueError(f"{name}: boxes must be [I, K, 4] float32, got {tuple(boxes.shape) if torch.is_tensor(boxes) else boxes}")
    i, k = int(boxes.shape[0]), int(boxes.shape[1])
    if not torch.is_tensor(gt_boxes) or gt_boxes.dim() != 3 or gt_boxes.shape[2] != 4:
        raise ValueError(f"{name}: gt_boxes must be [I, G, 4] float32, got "
                         f"{tuple(gt_boxes.shape) if torch.is_tensor(gt_boxes) else gt_boxes}")
    g = int(gt_boxes.shape[1])
    if i < 1:
        raise ValueError(f"{name}: boxes holds I = {i} images, must be >= 1")
    if not 1 <= k <= FRAME_MAX_BOXES:
        raise ValueError(f"{name}: boxes holds K = {k} slots per image, must be in 1..{FRAME_MAX_BOXES}")
    if not 1 <= g <= FRAME_MAX_BOXES:
        raise ValueError(f"{name}: gt_boxes holds G = {g} slots per image, must be in 1..{FRAME_MAX_BOXES}")
    if c < 1:
        raise ValueError(f"{name}: scores has C = {c} classes, must be >= 1")
    if rows != i * k:
        raise ValueError(f"{name}: scores has {rows} rows, boxes gives I*K = {i * k}")
    if i * k * c >= 2 ** 31:
        raise ValueError(f"{name}: scores has I*K*C = {i * k * c} elements, must be < 2^31")
    thr = float(iou_threshold)
    if not 0.0 < thr <= 1.0:     # (false for NaN)
        raise ValueError(f"{name}: iou_threshold = {iou_threshold} must be in (0, 1]")
    dev = scores.device
    _frame_tensor(name, "boxes", boxes, torch.float32, (i, k, 4), dev)
    _frame_tensor(name, "num_boxes", num_boxes, torch.int32, (i,), dev)
    _frame_tensor(name, "gt_boxes", gt_boxes, torch.float32, (i, g, 4), dev)
    _frame_tensor(name, "gt_labels", gt_labels, torch.uint8, (i, g, c), dev)
    _frame_tensor(name, "num_gt", num_gt, torch.int32, (i,), dev)
    if tp is not None:
        _frame_tensor(name, "tp", tp, torch.uint8, (rows, c), dev)
    if det_scores is not None:
        _frame_tensor(name, "det_scores", det_scores, torch.float32, (rows, c), dev)
    if ngt is not None:
        _frame_tensor(name, "ngt", ngt, torch.int32, (c,), dev)
    _chk(scores, boxes, num_boxes, gt_boxes, gt_labels, num_gt, tp, det_scores, ngt)
    if tp is None:
        tp = torch.empty((rows, c), dtype=torch.uint8, device=dev)
    if det_scores is None:
        det_scores = torch.empty((rows, c), dtype=torch.float32, device=dev)
    if ngt is None:
        ngt = torch.zeros(c, dtype=torch.int32, device=dev)
    hip.call("x3d_frame_match", ptr(scores), ptr(boxes), ptr(num_boxes), ptr(gt_boxes), ptr(gt_labels), ptr(num_gt), i, k, g, c,
             thr, ptr(tp), ptr(det_scores), ptr(ngt))
    return tp, det_scores, ngt


def frame_ap(tp, det_scores, ngt, order=None, ap=None, ntp=None):
    """Per-class PASCAL VOC average precision over the N rows of an evaluation set (x3d_frame_ap: the rules are in
    include/x3d_hip.h): tp [N, C] uint8 and det_scores [N, C] fp32 as frame_match wrote them, ngt [C] int32.  order [N, C] int64:
    every class's rows by score descending, stable; None: torch.sort(det_scores, dim=0, descending=True, stable=True).
    Returns (ap [C] float64, ntp [C] int32).  A class without ground truth or with a NaN score has ap NaN.  Does not
    synchronise."""
    name = "frame_ap"
    if not torch.is_tensor(det_scores) or det_scores.dtype != torch.float32 or det_scores.dim() != 2:
        got = f"{tuple(det_scores.shape)} {det_scores.dtype}" if torch.is_tensor(det_scores) else type(det_scores).__name__
        raise ValueError(f"{name}: det_scores must be [N, C] float32, got {got}")
    n, c = det_scores.shape
    if n < 1:
        raise ValueError(f"{name}: det_scores has N = {n} rows, must be >= 1")
    if c < 1:
        raise ValueError(f"{name}: det_scores has C = {c} classes, must be >= 1")
    if n * c >= 2 ** 31:
        raise ValueError(f"{name}: det_scores has N*C = {n * c} elements, must be < 2^31")
    dev = det_scores.device
    _frame_tensor(name, "tp", tp, torch.uint8, (n, c), dev)
    _frame_tensor(name, "ngt", ngt, torch.int32, (c,), dev)
    if order is not None:
        _frame_tensor(name, "order", order, torch.int64, (n, c), dev)
    if ap is not None:
        _frame_tensor(name, "ap", ap, torch.float64, (c,), dev)
    if ntp is not None:
        _frame_tensor(name, "ntp", ntp, torch.int32, (c,), dev)
    _chk(tp, det_scores, ngt, order, ap, ntp)
    if order is None:
        order = torch.sort(det_scores, dim=0, descending=True, stable=True).indices
    if ap is None:
        ap = torch.empty(c, dtype=torch.float64, device=dev)
    if ntp is None:
        ntp = torch.empty(c, dtype=torch.int32, device=dev)
    hip.call("x3d_frame_ap", ptr(tp), ptr(det_scores), ptr(order), ptr(ngt), n, c, ptr(ap), ptr(ntp))
    return ap, ntp


def softmax_xent_soft(logits, targets, probs, loss_rows=None, dlogits=None, grad_scale=1.0):
    """probs = softmax(logits); with dense target rows [N, M] fp32 (label smoothing, mixup / CutMix): loss_rows [N] = Keras
    CategoricalCrossentropy on the probabilities and its gradient (x3d_softmax_xent_soft: the rules are in
    include/x3d_hip.h; a one-hot row gives softmax_xent's result).  targets=None computes probs only.  One launch, does not
    synchronise."""
    _chk(logits, targets, probs, loss_rows, dlogits)
    if targets is None and (loss_rows is not None or dlogits is not None):
        raise ValueError("softmax_xent_soft: loss_rows / dlogits need targets")
    n, m = _loss_args("softmax_xent_soft", logits, probs, dict(targets=targets, dlogits=dlogits), dict(loss_rows=loss_rows))
    hip.call("x3d_softmax_xent_soft", ptr(logits), ptr(targets), ptr(probs), ptr(loss_rows), ptr(dlogits),
             float(grad_scale), n, m)
    return probs


def softmax_xent_kd(logits, teacher_logits, probs, labels=None, targets=None, loss_rows=None, kd_rows=None, dlogits=None,
                    grad_scale=1.0, alpha=0.5, temperature=1.0):
    """Distillation loss of the softmax head (x3d_softmax_xent_kd: the rules are in include/x3d_hip.h): loss_rows [N] =
    (1 - alpha) * hard + alpha * kd, with the hard term of softmax_xent on `labels` [N] int32 or of softmax_xent_soft on
    `targets` [N, M] fp32 (exactly one of the two), kd = T^2 * KL(softmax(teacher / T) || softmax(logits / T)) in kd_rows,
    and the gradient of the sum in dlogits.  probs is softmax(logits), as those kernels write it.  alpha = 0 does not read
    the teacher (teacher_logits may be None).  The scalars are the library's to check.  One launch, does not synchronise."""
    _chk(logits, teacher_logits, labels, targets, probs, loss_rows, kd_rows, dlogits)
    n, m = _loss_args("softmax_xent_kd", logits, probs, dict(teacher_logits=teacher_logits, targets=targets, dlogits=dlogits),
                      dict(loss_rows=loss_rows, kd_rows=kd_rows))
    if (labels is None) == (targets is None):
        raise ValueError("softmax_xent_kd: exactly one of labels / targets must be given")
    if labels is not None and (labels.dtype != torch.int32 or labels.numel() != n):
        raise ValueError(f"softmax_xent_kd: labels must be {n} int32, got {labels.numel()} {labels.dtype}")
    hip.call("x3d_softmax_xent_kd", ptr(logits), ptr(teacher_logits), ptr(labels), ptr(targets), ptr(probs), ptr(loss_rows),
             ptr(kd_rows), ptr(dlogits), float(grad_scale), float(alpha), float(temperature), n, m)
    return probs


def sigmoid_bce_kd(logits, teacher_logits, targets, probs, loss_rows=None, kd_rows=None, dlogits=None, grad_scale=1.0,
                   alpha=0.5, temperature=1.0):
    """Distillation loss of the multi-label head (x3d_sigmoid_bce_kd: the rules are in include/x3d_hip.h): loss_rows [N] =
    (1 - alpha) * sigmoid_bce's row + alpha * kd, kd = T^2 * the mean Bernoulli KL of sigmoid(logits / T) from
    sigmoid(teacher / T) in kd_rows, and the gradient of the sum in dlogits.  probs is sigmoid(logits).  alpha = 0 does not
    read the teacher (teacher_logits may be None).  One launch, does not synchronise."""
    _chk(logits, teacher_logits, targets, probs, loss_rows, kd_rows, dlogits)
    if targets is None:
        raise ValueError("sigmoid_bce_kd: targets must be given")
    n, m = _loss_args("sigmoid_bce_kd", logits, probs, dict(teacher_logits=teacher_logits, targets=targets, dlogits=dlogits),
                      dict(loss_rows=loss_rows, kd_rows=kd_rows))
    hip.call("x3d_sigmoid_bce_kd", ptr(logits), ptr(teacher_logits), ptr(targets), ptr(probs), ptr(loss_rows), ptr(kd_rows),
             ptr(dlogits), float(grad_scale), float(alpha), float(temperature), n, m)
    return probs


def _weight_args(name, n, m, tables, row_w):
    """the weight tensors of the _w wrappers: every table in `tables` ({what: tensor or None}) M float32, row_w N float32"""
    for what, t in list(tables.items()) + [("row_w", row_w)]:
        want = n if what == "row_w" else m
        if t is not None and (t.dtype != torch.float32 or t.dim() != 1 or t.numel() != want or not t.is_contiguous()):
            raise ValueError(f"{name}: {what} must be {want} contiguous float32, got {tuple(t.shape)} {t.dtype}")


def softmax_xent_w(logits, probs, labels=None, targets=None, class_w=None, row_w=None, teacher_logits=None, loss_rows=None,
                   kd_rows=None, dlogits=None, grad_scale=1.0, gamma=0.0, alpha=0.0, temperature=1.0):
    """The softmax head's loss with class weights class_w [M], sample weights row_w [N] (fp32; None = all ones) and the focal
    exponent gamma on the hard term (x3d_softmax_xent_w: the rules are in include/x3d_hip.h), on `labels` [N] int32 or dense
    `targets` [N, M] fp32 (exactly one of the two): loss_rows = (1 - alpha) * hard + alpha * row_w * kd, the gradient in dlogits.
    alpha = 0 does not read the teacher (teacher_logits may be None).  With nothing set the results have the bits of
    softmax_xent_kd.  The scalars are the library's to check.  One launch, does not synchronise."""
    _chk(logits, teacher_logits, labels, targets, class_w, row_w, probs, loss_rows, kd_rows, dlogits)
    n, m = _loss_args("softmax_xent_w", logits, probs, dict(teacher_logits=teacher_logits, targets=targets, dlogits=dlogits),
                      dict(loss_rows=loss_rows, kd_rows=kd_rows))
    if (labels is None) == (targets is None):
        raise ValueError("softmax_xent_w: exactly one of labels / targets must be given")
    if labels is not None and (labels.dtype != torch.int32 or labels.numel() != n):
        raise ValueError(f"softmax_xent_w: labels must be {n} int32, got {labels.numel()} {labels.dtype}")
    _weight_args("softmax_xent_w", n, m, dict(class_w=class_w), row_w)
    hip.call("x3d_softmax_xent_w", ptr(logits), ptr(teacher_logits), ptr(labels), ptr(targets), ptr(class_w), ptr(row_w),
             ptr(probs), ptr(loss_rows), ptr(kd_rows), ptr(dlogits), float(grad_scale), float(gamma), float(alpha),
             float(temperature), n, m)
    return probs


def sigmoid_bce_w(logits, targets, probs, class_w=None, pos_w=None, row_w=None, teacher_logits=None, loss_rows=None,
                  kd_rows=None, dlogits=None, grad_scale=1.0, gamma_pos=0.0, gamma_neg=0.0, alpha=0.0, temperature=1.0):
    """The multi-label head's loss with class weights class_w [M], positive weights pos_w [M], sample weights row_w [N] (fp32;
    None = all ones) and the focal exponents of the positive and the negative term (x3d_sigmoid_bce_w: the rules are in
    include/x3d_hip.h): loss_rows = (1 - alpha) * hard + alpha * row_w * kd, the gradient in dlogits.  alpha = 0 does not read
    the teacher.  With nothing set the results have the bits of sigmoid_bce_kd.  One launch, does not synchronise."""
    _chk(logits, teacher_logits, targets, class_w, pos_w, row_w, probs, loss_rows, kd_rows, dlogits)
    if targets is None:
        raise ValueError("sigmoid_bce_w: targets must be given")
    n, m = _loss_args("sigmoid_bce_w", logits, probs, dict(teacher_logits=teacher_logits, targets=targets, dlogits=dlogits),
                      dict(loss_rows=loss_rows, kd_rows=kd_rows))
    _weight_args("sigmoid_bce_w", n, m, dict(class_w=class_w, pos_w=pos_w), row_w)
    hip.call("x3d_sigmoid_bce_w", ptr(logits), ptr(teacher_logits), ptr(targets), ptr(class_w), ptr(pos_w), ptr(row_w),
             ptr(probs), ptr(loss_rows), ptr(kd_rows), ptr(dlogits), float(grad_scale), float(gamma_pos), float(gamma_neg),
             float(alpha), float(temperature), n, m)
    return probs


def class_hits(probs, labels, hits, counts):
    """counts[y] += rows with label y, hits[y] += those that are top-1 hits, for probs [N, M] fp32 against labels [N] int32 |
    int64; hits, counts: int64 [M] device counters (x3d_class_hits: the rules are in include/x3d_hip.h).  One launch, does
    not synchronise."""
    _chk(probs, labels, hits, counts)
    _f32_2d("class_hits", "probs", probs)
    n, m = probs.shape
    if labels.dtype not in (torch.int32, torch.int64) or labels.dim() != 1 or labels.shape[0] != n:
        raise ValueError(f"class_hits: labels must be [{n}] int32 or int64, got {tuple(labels.shape)} {labels.dtype}")
    for what, t in (("hits", hits), ("counts", counts)):
        if t.dtype != torch.int64 or t.dim() != 1 or t.numel() != m or not t.is_contiguous():
            raise ValueError(f"class_hits: {what} must be {m} contiguous int64 counters, got {tuple(t.shape)} {t.dtype}")
    if not probs.device == labels.device == hits.device == counts.device:
        raise ValueError("class_hits: probs, labels, hits and counts must be on one device")
    hip.call("x3d_class_hits", ptr(probs), ptr(labels), labels.element_size(), ptr(hits), ptr(counts), n, m)
    return hits, counts


MIX_MODES = {"mixup": hip.MIX_MIXUP, "cutmix": hip.MIX_CUTMIX}


def mix_clips(x, mode, lam, box=(0, 0, 0, 0), out=None):
    """Mixes the channels-last clip batch x [N, T, H, W, C] (fp32 / bf16 / fp16) with its own reverse, clip i with clip
    N-1-i (x3d_mix_clips: the rules are in include/x3d_hip.h).  mode "mixup": out_i = lam * x_i + (1 - lam) * x_{N-1-i};
    "cutmix": box = (y0, y1, x0, x1) of every frame is swapped between the two clips.  out=None allocates, out=x mixes in
    place.  One or two launches, does not synchronise."""
    if mode not in MIX_MODES:
        raise ValueError(f"mix_clips: mode must be one of {sorted(MIX_MODES)}, not {mode!r}")
    if out is None:
        out = torch.empty_like(x)
    _chk(x, out)
    if x.dim() != 5:
        raise ValueError(f"mix_clips: expected a clip batch [N, T, H, W, C], got {tuple(x.shape)}")
    if out.shape != x.shape or out.dtype != x.dtype or out.device != x.device:
        raise ValueError(f"mix_clips: out must be {tuple(x.shape)} {x.dtype} on {x.device}")
    n, t, h, w, c = x.shape
    y0, y1, x0, x1 = (int(v) for v in box)
    hip.call("x3d_mix_clips", ptr(x), ptr(out), MIX_MODES[mode], float(lam), y0, y1, x0, x1, n, t, h, w, c,
             hip.dtype_code(x.dtype))
    return out


def mix_targets(labels, num_classes, lam, eps=0.0, out=None, hard=None):
    """Soft targets [N, M] fp32 of a batch mixed with its own reverse (x3d_mix_targets: the rules are in include/x3d_hip.h).
    labels [N] int32: smoothed one-hot rows mixed with weight lam; `hard` [N] int32, when given, receives the class the
    training metrics count against.  labels [N, M] float32 (multi-hot / soft targets): the rows mixed, eps must be 0; out
    may be the targets themselves.  One launch, does not synchronise."""
    _chk(labels, out, hard)
    n, m = labels.shape[0], int(num_classes)
    if out is None:
        out = torch.empty((n, m), dtype=torch.float32, device=labels.device)
    _f32_2d("mix_targets", "out", out, (n, m))
    if hard is not None and (hard.dtype != torch.int32 or hard.numel() != n):
        raise ValueError(f"mix_targets: hard must be {n} int32, got {hard.numel()} {hard.dtype}")
    if labels.dim() == 1:
        if labels.dtype != torch.int32:
            raise ValueError(f"mix_targets: class labels must be int32, got {labels.dtype}")
        hip.call("x3d_mix_targets", ptr(labels), None, ptr(out), ptr(hard), float(lam), float(eps), n, m)
    else:
        _f32_2d("mix_targets", "targets", labels, (n, m))
        hip.call("x3d_mix_targets", None, ptr(labels), ptr(out), ptr(hard), float(lam), float(eps), n, m)
    return out

def randaug_clips(videos, randaug_list, t, rate=1, starts=None, fill=(0, 0, 0)):
    """RandAugment on uint8 GPU videos [F_i, H_i, W_i, 3] (x3d_randaug_clips; the rules are in include/x3d_hip.h): clip i =
    frames (starts[i] + j * rate) mod F_i, j < t, through the ops randaug_list[i] (a tuple of aug.RandAugOp, one per layer).
    Returns one uint8 tensor [t, H_i, W_i, 3] per clip; a clip no layer touches whose video already is its t frames comes
    back as videos[i] itself."""
    from . import views
    videos = list(videos)
    if not videos:
        raise ValueError("randaug_clips: empty batch")
    views._check_videos("randaug_clips", videos)
    if len(randaug_list) != len(videos):
        raise ValueError(f"{len(videos)} videos but {len(randaug_list)} op tuples")
    starts = [0] * len(videos) if starts is None else [int(v) for v in starts]
    return views.randaug_clips(videos, randaug_list, int(t), int(rate), starts, fill)[0]


def _f32_flat(op, name, t, n=None):
    if t.dtype != torch.float32 or not t.is_contiguous() or (n is not None and t.numel() != n):
        raise ValueError(f"{op}: {name} must be contiguous float32" + (f" of {n} elements" if n is not None else "")
                         + f", got {t.numel()} {t.dtype}")


def _f64_scratch(op, name, t, need, device, exact=False):
    """the `out` / `partials` / `scratch` of the sum-of-squares launches: checked (contiguous float64 of `need` elements when
    `exact`, of at least that many otherwise), or allocated when None"""
    if t is None:
        return torch.empty(need, dtype=torch.float64, device=device)
    if t.dtype != torch.float64 or not t.is_contiguous() or (t.numel() != need if exact else t.numel() < need):
        raise ValueError(f"{op}: {name} must {'be' if exact else 'hold'} {need} float64, got {t.numel()} {t.dtype}")
    return t


def grad_sumsq(g, out=None, scratch=None):
    """out [2] fp64 = (sum of squares of g in fp64, number of non-finite entries) (x3d_grad_sumsq: the rules are in
    include/x3d_hip.h).  The same bits on every run.  out / scratch=None allocate.  Two launches, does not synchronise."""
    _chk(g, out, scratch)
    _f32_flat("grad_sumsq", "g", g)
    n = g.numel()
    scratch = _f64_scratch("grad_sumsq", "scratch", scratch, int(hip.load().x3d_grad_sumsq_scratch(n)), g.device)
    out = _f64_scratch("grad_sumsq", "out", out, 2, g.device, exact=True)
    hip.call("x3d_grad_sumsq", ptr(g), n, ptr(scratch), ptr(out))
    return out


def ema_update(ema, w, decay, norm=None):
    """ema = decay * ema + (1 - decay) * w in place (x3d_ema_update); norm: the [2] fp64 result of grad_sumsq, the update
    is skipped on the device when its second entry is not 0.  One launch, does not synchronise."""
    _chk(ema, w, norm)
    _f32_flat("ema_update", "ema", ema)
    _f32_flat("ema_update", "w", w, ema.numel())
    if not 0.0 <= float(decay) < 1.0:
        raise ValueError(f"ema_update: decay must lie in [0, 1), not {decay}")
    hip.call("x3d_ema_update", ptr(ema), ptr(w), float(decay), ptr(norm), ema.numel())
    return ema


def grad_accum(acc, g, first=False):
    """acc = g (first) or acc += g, exact fp32 (x3d_grad_accum); acc may be g.  One launch, does not synchronise."""
    _chk(acc, g)
    _f32_flat("grad_accum", "acc", acc)
    _f32_flat("grad_accum", "g", g, acc.numel())
    hip.call("x3d_grad_accum", ptr(acc), ptr(g), acc.numel(), 1 if first else 0)
    return acc


def _covered(op, end, what, *buffers):
    """every (name, tensor) of `buffers` is contiguous float32 and holds the first `end` elements"""
    for name, t in buffers:
        if t is not None:
            _f32_flat(op, name, t)
            if t.numel() < end:
                raise ValueError(f"{op}: {name} holds {t.numel()} elements, {what} {end}")


def _seg_table(op, table, *buffers):
    """the table is on the device and covers nothing outside any of `buffers` (contiguous float32, same device)"""
    if table.d_chunks is None:
        raise ValueError(f"{op}: the chunk table is not on a device yet (SegTable.to(device))")
    _covered(op, table.end, "the chunk table covers up to", *buffers)
    _chk(table.d_chunks, table.d_segs, *[t for _, t in buffers])


def seg_sumsq(a, table, out=None, partials=None):
    """out [nseg] fp64 = per-segment sum of squares of `a` (squared and added in fp64, a fixed order: the same bits on every
    run; x3d_seg_sumsq).  table: segments.SegTable on a's device.  Two launches, does not synchronise."""
    _seg_table("seg_sumsq", table, ("a", a))
    _chk(partials, out)
    partials = _f64_scratch("seg_sumsq", "partials", partials, table.nchunk, a.device)
    out = _f64_scratch("seg_sumsq", "out", out, table.nseg, a.device, exact=True)
    hip.call("x3d_seg_sumsq", ptr(a), ptr(table.d_chunks), table.nchunk, ptr(table.d_segs), table.nseg, ptr(partials), ptr(out))
    return out


def seg_grad_sumsq(g, table, out=None, partials=None):
    """out [2] fp64 = (sum of squares of the finite entries of g inside the table's chunks, number of non-finite ones):
    grad_sumsq restricted to the segments of `table` (x3d_seg_grad_sumsq), the `norm=` of the launches over a table of tuned
    segments.  The same bits on every run.  Two launches, does not synchronise."""
    _seg_table("seg_grad_sumsq", table, ("g", g))
    partials = _f64_scratch("seg_grad_sumsq", "partials", partials, 2 * table.nchunk, g.device)
    out = _f64_scratch("seg_grad_sumsq", "out", out, 2, g.device, exact=True)
    _chk(partials, out)
    hip.call("x3d_seg_grad_sumsq", ptr(g), ptr(table.d_chunks), table.nchunk, ptr(table.d_segs), table.nseg, ptr(partials),
             ptr(out))
    return out


# ---- the fp16 loss scaler on the device (include/x3d_hip.h: X3D_LOSS_SCALE_STATE) ----------------------------------------------
LOSS_SCALE_STATE = hip.LOSS_SCALE_STATE
LS_SCALE, LS_INV, LS_GOOD, LS_SKIPPED, LS_APPLIED, LS_LAST_SKIPPED = range(6)     # the slots of the state


def loss_scale_value(scale) -> float:
    """`scale` as the float a loss-scaler state may hold: a power of two >= 1, ValueError else"""
    import math
    s = float(scale)
    if not (s >= 1.0 and math.isfinite(s) and math.frexp(s)[0] == 0.5):
        raise ValueError(f"the loss scale must be a power of two >= 1, not {scale!r}")
    return s


def loss_scale_state(scale, device, applied=0, skipped=0):
    """The device state of the loss scaler: [LOSS_SCALE_STATE] fp64 = (scale, 1 / scale, 0 finite steps in a row, `skipped`,
    `applied`, 0, 0, 0).  scale: a power of two >= 1 (what makes every product with it exact)."""
    s = loss_scale_value(scale)
    return torch.tensor([s, 1.0 / s, 0.0, float(skipped), float(applied), 0.0, 0.0, 0.0], dtype=torch.float64).to(device)


def _ls_state(op, state):
    if not torch.is_tensor(state) or state.dtype != torch.float64 or state.numel() != LOSS_SCALE_STATE or not state.is_cuda \
            or not state.is_contiguous():
        raise ValueError(f"{op}: state must be the device [{LOSS_SCALE_STATE}] float64 tensor of loss_scale_state")


def loss_scale_apply(x, state):
    """x *= scale in place, the scale read from the device state (x3d_loss_scale_apply).  One launch, does not synchronise."""
    _ls_state("loss_scale_apply", state)
    _chk(x, state)
    _f32_flat("loss_scale_apply", "x", x)
    hip.call("x3d_loss_scale_apply", ptr(x), x.numel(), ptr(state))
    return x


def unscale_sumsq(g, state, out=None, scratch=None):
    """grad_sumsq with g *= 1 / scale written back in the same pass (x3d_unscale_sumsq): out [2] fp64 = (sum of squares of the
    finite unscaled entries, number of non-finite ones).  Two launches, does not synchronise."""
    _ls_state("unscale_sumsq", state)
    _chk(g, state, out, scratch)
    _f32_flat("unscale_sumsq", "g", g)
    n = g.numel()
    scratch = _f64_scratch("unscale_sumsq", "scratch", scratch, int(hip.load().x3d_grad_sumsq_scratch(n)), g.device)
    out = _f64_scratch("unscale_sumsq", "out", out, 2, g.device, exact=True)
    hip.call("x3d_unscale_sumsq", ptr(g), n, ptr(state), ptr(scratch), ptr(out))
    return out


def seg_unscale_sumsq(g, table, state, out=None, partials=None):
    """seg_grad_sumsq with g *= 1 / scale written back inside the table's chunks, and nowhere else (x3d_seg_unscale_sumsq).  Two
    launches, does not synchronise."""
    _ls_state("seg_unscale_sumsq", state)
    _seg_table("seg_unscale_sumsq", table, ("g", g))
    partials = _f64_scratch("seg_unscale_sumsq", "partials", partials, 2 * table.nchunk, g.device)
    out = _f64_scratch("seg_unscale_sumsq", "out", out, 2, g.device, exact=True)
    _chk(g, state, partials, out)
    hip.call("x3d_seg_unscale_sumsq", ptr(g), ptr(table.d_chunks), table.nchunk, ptr(table.d_segs), table.nseg, ptr(state),
             ptr(partials), ptr(out))
    return out


def loss_scale_update(state, norm, growth_steps):
    """Keras' DynamicLossScale on the device state, from norm = the [2] fp64 result the step's update launches read
    (x3d_loss_scale_update): halve and count a skip when norm[1] != 0, else count an applied step and double after
    `growth_steps` finite ones in a row.  One launch, does not synchronise."""
    _ls_state("loss_scale_update", state)
    if norm is None or norm.dtype != torch.float64 or norm.numel() != 2 or not norm.is_cuda:
        raise ValueError("loss_scale_update: norm must be the device [2] float64 result of unscale_sumsq")
    if int(growth_steps) < 1:
        raise ValueError(f"loss_scale_update: growth_steps must be >= 1, not {growth_steps}")
    _chk(state, norm)
    hip.call("x3d_loss_scale_update", ptr(state), ptr(norm), int(growth_steps))
    return state


# ---- the update rules (solver.RULES): one assembler makes every launch, the public wrappers bind their arguments to it -------
def solver_extras(op, norm, max_norm, ema, ema_decay, n):
    """The norm / max_norm / ema / ema_decay arguments of the _ex and the chunk-table launches: norm is grad_sumsq's device result
    and brings a positive max_norm, ema is a flat device buffer of at least n elements and brings a decay in [0, 1)."""
    if norm is not None and (norm.dtype != torch.float64 or norm.numel() != 2 or not norm.is_cuda):
        raise ValueError(f"{op}: norm must be the device [2] float64 result of grad_sumsq")
    if norm is not None and not float(max_norm) > 0.0:
        raise ValueError(f"{op}: max_norm must be positive with norm, not {max_norm}")
    if ema is not None and (ema.dtype != torch.float32 or ema.numel() < n or not ema.is_cuda or not ema.is_contiguous()):
        raise ValueError(f"{op}: ema must be a contiguous device float32 buffer of at least {n} elements")
    if ema is not None and not 0.0 <= float(ema_decay) < 1.0:
        raise ValueError(f"{op}: ema_decay must lie in [0, 1), not {ema_decay}")


_AS_C = {float: float, int: int, bool: lambda flag: 1 if flag else 0}
_OUTSIDE = {"> 0": lambda v: not v > 0, ">= 0": lambda v: v < 0, ">= 1": lambda v: v < 1}      # the bounds solver.RULES names


def solver_launch(op, rule, w, slots, g, *, mask=None, n=None, table=None, pt=False, lr_scale=None, norm=None, max_norm=0.0,
                  ema=None, ema_decay=0.0, partials=None, q=None, **scalars):
    """One update of rule `rule` (a key of solver.RULES) on the weights w, its slot buffers `slots` and the gradient g: every
    argument checked, then exactly one hip.call.  `op` is the caller's name, for the messages.
      where     mask (byte mask of the L2-regularised elements, or None) and n: the first n elements, by the rule's flat entry
                point -- the plain one when neither norm nor ema is given, else _ex.  table (a segments.SegTable on the device):
                its segments, by the chunk-table entry point; pt: its _pt form, at lr * lr_scale[segment] (lr_scale None: all 1)
      scalars   by the names of RULES[rule].scalars; the record's defaults for those not given
      extras    norm (grad_sumsq's / seg_grad_sumsq's result) + max_norm: clip to that global L2 norm, skip the update on a
                non-finite gradient; ema + ema_decay: the weight average kept in the same pass (solver_extras)
      scratch   partials [2 * nchunk] fp64 and q [nseg] fp32 of a rule with trust ratios, allocated when None (ignored by the
                other rules).  Returns q for such a rule, else None."""
    r = RULES[rule]
    buffers = (("w", w), *zip(SLOT_NAMES[r.slot_kind], slots, strict=True), ("g", g))
    ex = table is not None or norm is not None or ema is not None          # the entry point takes the extras
    entry = r.table[bool(pt)] if table is not None else r.flat and r.flat[ex]
    if not entry:
        raise ValueError(f"{op}: {rule} has no {'chunk-table entry point without lr_scale' if table is not None else 'flat form'}")
    if table is None:
        n = int(n)
        _chk(mask, *[t for _, t in buffers])
        _covered(op, n, "the update covers", *buffers)
        if mask is not None and mask.numel() < n:
            raise ValueError(f"{op}: l2_mask holds {mask.numel()} elements, the update covers {n}")
        where = (ptr(mask),)
    else:
        _seg_table(op, table, *buffers, ("ema", ema))
        n = table.end
        where = (ptr(table.d_chunks), table.nchunk, ptr(table.d_segs), table.nseg)
    solver_extras(op, norm, max_norm, ema, ema_decay, n)
    values = {}
    for name, default in r.scalars.items():
        v = scalars.pop(name, default)
        if isinstance(v, type):
            raise TypeError(f"{op}: {rule} needs {name}")
        values[name] = _AS_C[default if isinstance(default, type) else type(default)](v)
    if scalars:
        raise TypeError(f"{op}: {rule} takes no {sorted(scalars)}")
    if table is not None and any(_OUTSIDE[b](values[k]) for k, b in r.bounds.items()):    # (the flat forms take what they are given)
        raise ValueError(f"{op}: " + ", ".join(f"{k} must be {b}" for k, b in r.bounds.items()) + ", not "
                         + ", ".join(str(values[k]) for k in r.bounds))
    if pt:
        if lr_scale is not None:
            if lr_scale.dtype != torch.float32 or lr_scale.numel() != table.nseg or not lr_scale.is_contiguous() \
                    or not lr_scale.is_cuda:
                raise ValueError(f"{op}: lr_scale must be a contiguous device float32 tensor of {table.nseg} elements (one per "
                                 f"segment of the table), got {lr_scale.numel()} {lr_scale.dtype}")
            _chk(table.d_chunks, lr_scale)
        where += (ptr(lr_scale),)
    tail = (ptr(norm), float(max_norm), ptr(ema), float(ema_decay)) if ex else ()
    if table is None:
        tail += (n,)
    if r.trust:
        partials = _f64_scratch(op, "partials", partials, 2 * table.nchunk, w.device)
        if q is None:
            q = torch.ones(table.nseg, dtype=torch.float32, device=w.device)
        elif q.dtype != torch.float32 or q.numel() != table.nseg or not q.is_contiguous():
            raise ValueError(f"{op}: q must be {table.nseg} float32, got {q.numel()} {q.dtype}")
        _chk(partials, q)
        tail += (ptr(partials), ptr(q))
    hip.call(entry, *map(ptr, (w, *slots, g)), *where, *values.values(), *tail)
    return q if r.trust else None


def _bound(op, rule, a):
    """The launch of a public wrapper from its locals(): the wrappers' parameter names are those of the rule's slots (v | m, v)
    and scalars and solver_launch's keywords; a wrapper with an lr_scale parameter is the _pt form."""
    keys = ("table", "lr_scale", "norm", "max_norm", "ema", "ema_decay", "partials", "q", *RULES[rule].scalars)
    return solver_launch(op, rule, a["w"], [a[k] for k in SLOT_NAMES[RULES[rule].slot_kind]], a["g"], pt="lr_scale" in a,
                         **{k: a[k] for k in keys if k in a})


def sgd_nesterov(w, v, g, l2_mask, lr, momentum, weight_decay, grad_scale=1.0):
    solver_launch("sgd_nesterov", "sgd", w, (v,), g, mask=l2_mask, n=w.numel(), lr=lr, momentum=momentum,
                  weight_decay=weight_decay, grad_scale=grad_scale)


def lars(w, v, g, table, lr, momentum, weight_decay, trust_coef=0.001, eps=1e-8, clip=False, grad_scale=1.0, norm=None,
         max_norm=0.0, ema=None, ema_decay=0.0, partials=None, q=None):
    """LARS on the segments of `table` (x3d_lars: the rule is in include/x3d_hip.h); returns q [nseg] fp32, the trust ratios,
    on the device.  Three launches, does not synchronise; g is not written."""
    return _bound("lars", "lars", locals())


def adamw(w, m, v, g, table, lr, step, beta1=0.9, beta2=0.999, eps=1e-7, decay=0.0, grad_scale=1.0, norm=None, max_norm=0.0,
          ema=None, ema_decay=0.0):
    """Adam with decoupled weight decay on the l2 segments of `table` (x3d_adamw).  One launch, does not synchronise."""
    _bound("adamw", "adamw", locals())


def lamb(w, m, v, g, table, lr, step, beta1=0.9, beta2=0.999, eps=1e-6, decay=0.0, grad_scale=1.0, norm=None, max_norm=0.0,
         ema=None, ema_decay=0.0, partials=None, q=None):
    """LAMB on the segments of `table` (x3d_lamb); returns q [nseg] fp32, the trust ratios, on the device.  Three launches, does
    not synchronise; g is not written."""
    return _bound("lamb", "lamb", locals())


# fine-tuning: the same rules on a table of the TUNED segments, lr * lr_scale[segment] per segment (finetune.py; lr_scale None: all 1)
def sgd_pt(w, v, g, table, lr_scale, lr, momentum, weight_decay, grad_scale=1.0, norm=None, max_norm=0.0, ema=None,
           ema_decay=0.0):
    """SGD(momentum, nesterov) + L2 on the segments of `table` at lr * lr_scale[t] (x3d_sgd_pt; the l2 flag is the segment's).
    One launch, does not synchronise."""
    _bound("sgd_pt", "sgd", locals())


def adam_pt(w, m, v, g, table, lr_scale, lr, step, beta1=0.9, beta2=0.999, eps=1e-7, weight_decay=0.0, grad_scale=1.0, norm=None,
            max_norm=0.0, ema=None, ema_decay=0.0):
    """Adam + L2 on the segments of `table` at lr * lr_scale[t] (x3d_adam_pt).  One launch, does not synchronise."""
    _bound("adam_pt", "adam", locals())


def lars_pt(w, v, g, table, lr_scale, lr, momentum, weight_decay, trust_coef=0.001, eps=1e-8, clip=False, grad_scale=1.0,
            norm=None, max_norm=0.0, ema=None, ema_decay=0.0, partials=None, q=None):
    """lars at lr * lr_scale[t] per segment (x3d_lars_pt); q [nseg] in the order of the table's segments."""
    return _bound("lars_pt", "lars", locals())


def adamw_pt(w, m, v, g, table, lr_scale, lr, step, beta1=0.9, beta2=0.999, eps=1e-7, decay=0.0, grad_scale=1.0, norm=None,
             max_norm=0.0, ema=None, ema_decay=0.0):
    """adamw at lr * lr_scale[t] per segment (x3d_adamw_pt)."""
    _bound("adamw_pt", "adamw", locals())


def lamb_pt(w, m, v, g, table, lr_scale, lr, step, beta1=0.9, beta2=0.999, eps=1e-6, decay=0.0, grad_scale=1.0, norm=None,
            max_norm=0.0, ema=None, ema_decay=0.0, partials=None, q=None):
    """lamb at lr * lr_scale[t] per segment (x3d_lamb_pt); q [nseg] in the order of the table's segments."""
    return _bound("lamb_pt", "lamb", locals())


def l2_sumsq(w, l2_mask, out):
    _chk(w, l2_mask, out)
    hip.call("x3d_l2_sumsq", ptr(w), ptr(l2_mask), ptr(out), w.numel())


def nthwc_to_ncthw(src, dst):
    """src [N,T,H,W,C] -> dst [N,C,T,H,W] (with dtype conversion)."""
    _chk(src, dst)
    n, t, h, w, c = src.shape
    hip.call("x3d_nthwc_to_ncthw", ptr(src), hip.dtype_code(src.dtype), ptr(dst),
             hip.dtype_code(dst.dtype), n, c, t * h * w)
    return dst


def subsample2(x, out=None):
    """Even-pixel copy x[..., ::2, ::2] of an NCTHW tensor (x3d_subsample2): what a stride-(1,2,2) shortcut conv samples."""
    _chk(x, out)
    n, c, t, h, w = x.shape
    if out is None:
        out = torch.empty((n, c, t, (h + 1) // 2, (w + 1) // 2), dtype=x.dtype, device=x.device)
    hip.call("x3d_subsample2", ptr(x), ptr(out), n * c * t, h, w, hip.dtype_code(x.dtype))
    return out
