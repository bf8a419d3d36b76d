import torch


def report(name, got, ref, rtol, atol):
    got = got.detach().double().cpu()
    ref = ref.detach().double().cpu()
    assert got.shape == ref.shape, f"{name}: shape {tuple(got.shape)} vs {tuple(ref.shape)}"
    err = (got - ref).abs()
    tol = atol + rtol * ref.abs()
    bad = err > tol
    if bad.any() or not torch.isfinite(got).all():
        idx = torch.nonzero(bad | ~torch.isfinite(got))[0].tolist() if (bad | ~torch.isfinite(got)).any() else None
        raise AssertionError(
            f"{name}: {int(bad.sum())}/{bad.numel()} elements out of tolerance (rtol={rtol}, atol={atol}); "
            f"max abs err {err.max().item():.3e}, max |ref| {ref.abs().max().item():.3e}; first bad index {idx}: "
            f"got {got[tuple(idx)].item() if idx is not None else None} ref {ref[tuple(idx)].item() if idx is not None else None}")
    return err.max().item()


def tie_slack(v, dtype, w_abs, eps_ulps=2e-4):
    """Extra absolute tolerance [N, M, T, H, W] for a GEMM whose operand `v` ([N, K, T, H, W], the fp32 output of a prologue)
    is rounded to the 16-bit `dtype` before the product.  Where a value sits within `eps_ulps` of the midpoint between two
    neighbouring `dtype` values, fp32 arithmetic in another order (the kernel's folded swish against torch's) may round it to
    the other neighbour: one ulp of the operand, so every output at that point may move by ulp * |w[m, k]|.  Zero almost
    everywhere.  (Found by the fuzz sweep, seed 20261004: a prologue value 2.1e-6 bf16-ulps off a midpoint under a weight
    of 0.66 moved 15 outputs of one point by up to 1.2e-2, five times the flat atol.)"""
    amb = _tie_ulps(v.detach().double().cpu(), dtype, eps_ulps)      # [N, K, T, H, W]
    return torch.einsum("mk,nkthw->nmthw", w_abs.detach().double().cpu(), amb)


def _tie_ulps(v64, dtype, eps_ulps):
    """ulp(v) in `dtype` where the fp64 value v sits within `eps_ulps` of a rounding midpoint, 0 elsewhere (on v's device)."""
    r = v64.float().to(dtype).double()
    mant = 7 if dtype == torch.bfloat16 else 10
    ulp = torch.exp2(torch.floor(torch.log2(r.abs().clamp_min(1e-30))) - mant)
    if dtype == torch.float16:
        ulp = ulp.clamp_min(2.0 ** -24)               # (subnormals: a fixed spacing)
    d = (v64 - r).abs() / ulp                         # 0 .. 0.5 (0.5 = a tie)
    return ((0.5 - d) < eps_ulps).double() * ulp


def tie_slack_t(v, dtype, w_abs, eps_ulps=2e-4):
    """The temporal analogue of tie_slack, for a depthwise conv along T (the stem's conv_t, "same" padding KT // 2) whose
    input `v` ([N, C, T, H, W], fp64: the conv_s output before the kernel rounds it to the 16-bit `dtype` on chip) is such a
    rounded operand: where v sits within `eps_ulps` of a midpoint, the kernel's fp32 sum may round to the other neighbour
    than the fp64 reference did, and every output that reads that point, out[t] = sum_k w[c, k] v[t + k - KT // 2], may move
    by |w[c, k]| * ulp.  Returns that extra absolute tolerance [N, C, T, H, W] on v's device (the full-size tests stay on the
    GPU).  w_abs: [C, KT]."""
    kt = w_abs.shape[1]
    amb = torch.nn.functional.pad(_tie_ulps(v.detach().double(), dtype, eps_ulps), (0, 0, 0, 0, kt // 2, kt // 2))
    t = v.shape[2]
    wa = w_abs.detach().double().to(v.device)
    out = torch.zeros(v.shape, dtype=torch.float64, device=v.device)
    for k in range(kt):
        out += wa[:, k].view(1, -1, 1, 1, 1) * amb[:, :, k:k + t]
    return out


def tie_slack_pw(v, dtype, w_abs, eps_ulps=2e-4):
    """tie_slack on v's device, for any sample chunk of v ([n, K, T, H, W], the fp32 / fp64 prologue output before the
    rounding): the full-size pointwise tests keep it on the GPU.  w_abs [M, K]; returns [n, M, T, H, W] fp64."""
    return torch.einsum("mk,nkthw->nmthw", w_abs.detach().double().to(v.device), _tie_ulps(v.detach().double(), dtype, eps_ulps))


def pw_prologue64(x, ss=None, gate=None, act=0, dtype=None):
    """The input prologue of x3d_pw_fwd / x3d_pw_wgrad, v = act(gate[n, c] (s x + t)) (act 0 none, 1 ReLU, 2 swish), as the
    16-bit GEMM operand: evaluated in fp32 like the kernels and rounded to `dtype` (tests.util.round_to); dtype None: the
    fp64 value.  x [N, C, T, H, W]; ss [C, 2]; gate [N, C]."""
    f = torch.float64 if dtype is None else torch.float32
    v = x.to(f)
    if ss is not None:
        v = v * ss[:, 0].to(f).view(1, -1, 1, 1, 1) + ss[:, 1].to(f).view(1, -1, 1, 1, 1)
    if gate is not None:
        v = v * gate.to(f)[:, :, None, None, None]
    if act == 1:
        v = torch.relu(v)
    elif act == 2:
        v = v * torch.sigmoid(v)
    return v.double() if dtype is None else round_to(v, dtype)


def pw_gemm64(v, w, stride=1):
    """The pointwise conv y[n, o] = sum_c w[o, c] v[n, c] (oracle.x3d_oracle.pointwise; stride 2 samples the even pixels) in
    fp64 on v's device."""
    if stride != 1:
        v = v[:, :, :, ::stride, ::stride]
    return torch.einsum("oc,ncthw->nothw", w.double().to(v.device), v.double())


def pw_infer_epi64(acc, oss, add=None, add_ss=None, act=0):
    """x3d_pw_fwd's inference epilogue y = act(s_o acc + t_o [+ s_r add + t_r | + add]) in fp64 (act 1: ReLU)."""
    c = lambda t, j: t[:, j].double().view(1, -1, 1, 1, 1)
    y = acc * c(oss, 0) + c(oss, 1)
    if add is not None:
        y = y + (add.double() * c(add_ss, 0) + c(add_ss, 1) if add_ss is not None else add.double())
    return torch.relu(y) if act == 1 else y


def bn_bwd_coef_sums(m, sy, syy, sg, sgy, gamma):
    """[C][4] fp32 coefficients (A, B, C, 0) of the training-mode BatchNorm backward dY = A g + B y + C over m points per
    channel, from the fp64 sums of y, y^2, g and g y (x3d_bn_finalize / x3d_bn_bwd_finalize arithmetic)."""
    mean = sy / m
    var = syy / m - mean * mean
    invstd = 1.0 / torch.sqrt(var + 1e-5)
    dbe = sg
    dga = (sgy - mean * dbe) * invstd
    k1 = gamma * invstd
    b = -k1 * invstd * dga / m
    c = -k1 * dbe / m - b * mean
    return torch.stack([k1, b, c, torch.zeros_like(c)], 1).float()


def bn_bwd_fold64(sums, count, mi, gamma):
    """What a publishing x3d_bn_bwd_fold derives from its operands, in fp64: (coef [C][4], dgamma, dbeta) from sums [C][2] =
    (sum g, sum g y), mean_invstd [C][2] and gamma (common.h bn_bwd_coefs)."""
    mean, invstd, g = mi[:, 0].double(), mi[:, 1].double(), gamma.double()
    dbe = sums[:, 0].double()
    dga = (sums[:, 1].double() - mean * dbe) * invstd
    k1 = g * invstd
    b = -k1 * invstd * dga / count
    c = -k1 * dbe / count - b * mean
    return torch.stack([k1, b, c, torch.zeros_like(c)], 1), dga, dbe


def dw_same_pads(n, stride):
    """(output extent, pad before, pad after) of a 3-tap TF-SAME window along an extent of n at `stride` (156 -> 78: 0 / 1,
    39 -> 20: 1 / 1, 56 -> 56: 1 / 1)."""
    out = -(-n // stride)
    tot = max((out - 1) * stride + 3 - n, 0)
    return out, tot // 2, tot - tot // 2


def dw_stencil64(a, w, stride, dy=None):
    """The channelwise 3x3x3 convolution (strides (1, s, s), TF-SAME padding: oracle.x3d_oracle.depthwise3x3x3) as 27
    shifted-slice products in the dtype and on the device of `a` [N, C, T, H, W]; w [C, 3, 3, 3].  Without `dy`: the output
    [N, C, T, Ho, Wo].  With `dy` (an output gradient): (dA, dW), the gradients with respect to `a` and `w`.  Test side only:
    the full-size tests run it in fp64 on the GPU, sample chunk by sample chunk."""
    n, c, t, h, wd = a.shape
    ho, hb, ha = dw_same_pads(h, stride)
    wo, wb, wa = dw_same_pads(wd, stride)
    ap = torch.nn.functional.pad(a, (wb, wa, hb, ha, 1, 1))
    wv = lambda k: w[:, k[0], k[1], k[2]].view(1, -1, 1, 1, 1)
    sl = lambda kt, kh, kw: (slice(None), slice(None), slice(kt, kt + t), slice(kh, kh + stride * (ho - 1) + 1, stride),
                             slice(kw, kw + stride * (wo - 1) + 1, stride))
    taps = [(kt, kh, kw) for kt in range(3) for kh in range(3) for kw in range(3)]
    if dy is None:
        out = torch.zeros((n, c, t, ho, wo), dtype=a.dtype, device=a.device)
        for k in taps:
            out += wv(k) * ap[sl(*k)]
        return out
    dap = torch.zeros_like(ap)
    dw = torch.zeros((c, 3, 3, 3), dtype=a.dtype, device=a.device)
    for k in taps:
        dap[sl(*k)] += wv(k) * dy
        dw[:, k[0], k[1], k[2]] = (dy * ap[sl(*k)]).sum((0, 2, 3, 4))
    return dap[:, :, 1:1 + t, hb:hb + h, wb:wb + wd], dw


def relu_mask_mismatch(masks, oracle_taps_masks):
    """Fraction of ReLU sites whose sign differs between the device (hip_relu_masks) and a free-running oracle forward."""
    bad = tot = 0
    for k, m in oracle_taps_masks.items():
        d = masks[k]
        bad += int((d != m).sum())
        tot += m.numel()
    return bad / max(tot, 1), bad, tot


def hip_relu_masks(pl):
    """Sign patterns of every ReLU in a training plan of the HIP model, keyed like the oracle's ReLU sites.
    Computed in fp64 from the stored fp32 tensors/coefficients: the kernels evaluate s*x+t with one fused
    rounding, which preserves the sign of the exact value."""
    def affine_mask(raw, ss):
        ss = ss.detach().double().cpu()
        z = raw.detach().double().cpu() * ss[:, 0].view(1, -1, 1, 1, 1) + ss[:, 1].view(1, -1, 1, 1, 1)
        return z > 0

    masks = {"conv1": pl.y0.detach().float().cpu() > 0,
             "conv5": affine_mask(pl.c5_raw, pl.bn5.ss),
             "fc1": pl.h1.detach().cpu() > 0}
    for B in pl.blocks:
        s = B.spec
        pre = f"stages/{s.stage}/stage/layer_with_weights-{s.index}"
        masks[pre + "/a"] = affine_mask(B.a_raw, B.bn_a.ss)
        masks[pre + "/out"] = B.y.detach().float().cpu() > 0
        if s.has_se:
            masks[pre + "/se"] = B.hidden.detach().cpu() > 0
    return masks


def rel_l2(got, ref):
    got, ref = got.detach().double().cpu(), ref.detach().double().cpu()
    return ((got - ref).norm() / (ref.norm() + 1e-30)).item()


def round_to(x, dtype):
    """x (fp32 / fp64) rounded to the storage type `dtype`, as fp64: what a 16-bit GEMM operand holds after the kernel's
    fp32 prologue.  float32: unchanged (the fp32 kernels feed the exact-fp32 matrix instruction)."""
    if dtype == torch.float32:
        return x.double()
    return x.float().to(dtype).double()


def tol_gemm(dtype):
    """(rtol, atol-per-unit-of-scale) for the pointwise (matrix-core) kernels against an fp64 GEMM whose OPERANDS were
    rounded to the storage type first (weights; the fp32 prologue's output -- round_to), so that what is left is the
    rounding of the stored output (rtol, as tol_store), fp32 accumulation order, and the rare operand whose fp32
    prologue value sits on a rounding boundary and lands on the other side in the reference's arithmetic (one product
    off by an operand ulp: << 1e-3 of the tensor's scale).  Round 2 compared with UNROUNDED operands at 1.6e-2 of the
    tensor maximum, which a dropped k-element of a K = 432 GEMM (1.2 %) passed."""
    if dtype == torch.float32:
        return (2e-5, 2e-5)
    return (4e-3, 1e-3) if dtype == torch.bfloat16 else (1e-3, 2.5e-4)


def tol_store(dtype):
    """(rtol, atol-per-unit-of-scale) for kernels whose ONLY error source against the fp64 reference is the rounding of
    the stored output (depthwise convs, residual tails, stem temporal conv: inputs are pre-rounded, arithmetic fp32):
    half an ulp of the storage type relative (2^-9 bf16, 2^-12 fp16... 2^-11 as fp16 has 11 significand bits) plus fp32
    accumulation noise."""
    if dtype == torch.float32:
        return (2e-5, 2e-5)
    return (4e-3, 2e-4) if dtype == torch.bfloat16 else (1e-3, 1e-4)


def rnd(shape, dtype, gen, scale=1.0):
    """random tensor representable in `dtype`, returned as (device-dtype tensor on cpu, fp64 copy)"""
    t = (torch.randn(shape, generator=gen, dtype=torch.float32) * scale).to(dtype)
    return t, t.double()


def dev_at(t, gpu, off=0):
    """t on the device; off > 0: as a contiguous view `off` elements into a larger allocation, so that the kernel sees an
    operand `off` elements past a 16-byte boundary (torch's device allocations are aligned to far more).  None stays None."""
    if t is None or not off:
        return None if t is None else t.to(gpu)
    v = torch.empty(t.numel() + off, dtype=t.dtype, device=gpu)[off:].view(t.shape)
    v.copy_(t)
    assert v.is_contiguous() and v.data_ptr() % 16 == (off * v.element_size()) % 16
    return v


def out_at(shape, dtype, gpu, off=0, fill=None):
    """A caller-provided output on the device, uninitialised or filled, placed like dev_at()."""
    import math
    v = torch.empty(math.prod(shape) + off, dtype=dtype, device=gpu)[off:].view(shape)
    return v if fill is None else v.fill_(fill)


class AltBackward:
    """A second backward pass (`rec`: x3d_tf_amd.plan.Backward) recorded over the SAME forward buffers of a training plan with
    other plan options (record_alternate_backward).  run() replays it from the forward state `snapshot` captured."""

    def __init__(self, model, pl, rec, extra):
        self.model, self.pl, self.rec, self.lst, self.extra = model, pl, rec, rec.launches, extra
        self.info = dict(tail_folded=[r.tail_folded for r in rec.blocks], a_bwd_rc=[r.a_bwd_rc for r in rec.blocks],
                         stem_bwd_folded=rec.stem_bwd_folded)

    def run(self):
        self.extra.zero_()
        self.pl.run(self.lst)


def record_alternate_backward(model, pl, x, **options):
    """Differential tests: record the backward pass of `pl` AGAIN with `options` overriding the model's plan options, against
    the forward tensors the plan already owns -- so that two backward variants (e.g. pw_bwd_rc on / off) can be compared on
    bit-identical forward state, where the backward pass is a LINEAR map of the upstream gradient and differences do not
    amplify.  New fp64 accumulators of the second list live in their own zeroed buffer; x = the bound input batch (the
    stem's weight-gradient launch of the new list is bound to it).  The plan's own backward pass is left as it is: the
    record (`.rec`) owns the second list's scratch buffers."""
    from x3d_tf_amd.model import PLAN_DEFAULTS
    from x3d_tf_amd.plan import record_backward
    assert all(k in PLAN_DEFAULTS for k in options)
    first = len(pl._zero_chunks)
    rec = record_backward(model, pl, dict(model.opt, **{k: bool(v) for k, v in options.items()}))
    extra = pl.carve(first)           # the accumulators the new list added
    pl.resolve()
    pl.input_slots += rec.input_slots
    model._bind_input(pl, x)          # (the input slots now include the new list's stem launch)
    return AltBackward(model, pl, rec, extra)
