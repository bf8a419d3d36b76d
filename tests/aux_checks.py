"""fp64 runners with derived limits for every launch outside the pointwise / depthwise / stem families: BatchNorm bookkeeping,
the residual tail, squeeze-excite and its slab reductions, the head, the loss, the plane-wise reductions and the layout
converter.  tests/test_full_size_gpu.py runs them at the full-size plans' shapes (shapes.AUX_FULL), tests/test_aux_edges_gpu.py at
the edges of the kernels' tiles (shapes.AUX_EDGE)."""
import torch

from tests.util import tol_store


def _check(name, got, ref, rtol, atol):
    got, ref = got.double(), ref.double()
    err = (got - ref).abs()
    bad = err > atol + rtol * ref.abs()
    assert torch.isfinite(got).all(), f"{name}: non-finite values"
    assert not bad.any(), (f"{name}: {int(bad.sum())}/{bad.numel()} out of tolerance (rtol {rtol}, atol {atol:.3e}); max err "
                           f"{err.max().item():.3e}, max |ref| {ref.abs().max().item():.3e}")
    return (err.max() / (ref.abs().max() + 1e-300)).item()


def _frac(name, got, ref, rtol, atol):
    """_check, returning the worst error as a fraction of its limit atol + rtol |ref|."""
    _check(name, got, ref, rtol, atol)
    got, ref = got.double(), ref.double()
    return ((got - ref).abs() / (atol + rtol * ref.abs()).clamp_min(1e-300)).max().item()


# ---- every other launch of the full-size plans (tests/shapes.py AUX_FULL: BatchNorm bookkeeping, residual-tail backward,
# squeeze-excite and its slab reductions, head, loss) ----------------------------------------------------------------------
# fp32 sums are held to the probabilistic bound of test_stem_fp32_full_size, lambda sqrt(L) u sum |terms| (lambda = 6,
# u = 2^-24), plus 2^-50 sum |terms| for the fp64 atomics that combine the workgroups' partial sums.  BatchNorm finalize
# arithmetic against fp64 of the same operands, to _AUX_ULPS fp32 roundings of the magnitude of each result's terms.
_LAM, _U = 6.0, 2.0 ** -24
_AUX_ULPS = 8
_GRAD_FILL = 0.5        # pre-fill of the squeeze-excite / BatchNorm_b gradient accumulators in the edge cases


def _sum_lim(L, absum):
    import math
    return _LAM * math.sqrt(L) * _U * absum + 2.0 ** -50 * absum


def _within(name, got, ref, lim):
    """|got - ref| <= lim element-wise; returns the worst error as a fraction of its limit."""
    got, ref = got.double(), ref.double()
    err = (got - ref).abs()
    lim = torch.as_tensor(lim, dtype=torch.float64, device=err.device).expand_as(err)
    assert torch.isfinite(got).all(), f"{name}: non-finite values"
    bad = err > lim
    assert not bad.any(), (f"{name}: {int(bad.sum())}/{bad.numel()} beyond the limit; worst err / limit "
                           f"{(err / lim.clamp_min(1e-300)).max().item():.3e}, max err {err.max().item():.3e}, "
                           f"max |ref| {ref.abs().max().item():.3e}")
    return (err / lim.clamp_min(1e-300)).max().item()


_BAND = 64
_SENTINEL = {1: 0x5A, 2: 0x7FA5, 4: 0x7FC0A5A5, 8: 0x7FF8A5A5A5A5A5A5}     # a NaN in bf16, fp16, fp32 and fp64
_BITS = {1: torch.uint8, 2: torch.int16, 4: torch.int32, 8: torch.int64}


class _Bands:
    """Tensors as views into larger allocations: _BAND elements of a sentinel bit pattern (a NaN in every float type) on
    each side, and `off` more elements in front (a view that is not 16-byte aligned; with off = 0 the view is).  An output
    starts as the sentinel as well unless `fill` (an accumulator's pre-fill) or `init` (its input values) is given, so an
    element the launch leaves unwritten is not finite.  check(): after the launch every band still holds its pattern."""

    def __init__(self, gpu, off=0):
        self.gpu, self.off, self.items = gpu, off, []

    def __call__(self, shape, dtype, fill=None, init=None):
        import math
        n, es = math.prod(shape), torch.empty((), dtype=dtype).element_size()
        lo = _BAND + self.off
        raw = torch.full((lo + n + _BAND,), _SENTINEL[es], dtype=_BITS[es], device=self.gpu)
        v = raw.view(dtype)[lo:lo + n].view(shape)
        if fill is not None:
            v.fill_(fill)
        if init is not None:
            v.copy_(init)
        assert v.is_contiguous() and (v.data_ptr() % 16 == 0) == ((self.off * es) % 16 == 0)
        self.items.append((raw, lo, lo + n, _SENTINEL[es]))
        return v

    def view(self, t):
        """t (an input) moved into a banded allocation at the same offset; None stays None"""
        return None if t is None else self(tuple(t.shape), t.dtype, init=t)

    def check(self):
        torch.cuda.synchronize()
        for i, (raw, lo, hi, s) in enumerate(self.items):
            assert bool((raw[:lo] == s).all()) and bool((raw[hi:] == s).all()), f"tensor {i}: written outside its {hi - lo} elements"


def _with_off(case, k):
    """(the first k fields of a case, its optional trailing element offset)"""
    assert len(case) in (k, k + 1), case
    return case[:k], (case[k] if len(case) > k else 0)


def _elem_vec(dtype, P, off=0):
    """VEC of elem.hip's launchers: 16-byte vectors when P is a multiple of one and every tensor is 16-byte aligned (pick_vec,
    norm_vec; torch allocations are 256-byte aligned, so P and the views' element offset decide), else scalar loads."""
    full = 4 if dtype == torch.float32 else 8
    return full if P % full == 0 and off % full == 0 else 1


def _aux_fp32_chain(entry, dtype, n, P, off=0):
    """L, the longest chain of fp32 roundings a term of the launch's per-channel sum passes through (elem.hip):
      tail_bwd_kernel / relu_bn_bwd_reduce_kernel: ELEM_ITERS = 4 rounds of VEC terms per thread, the product (1), the
          256-thread block_sum (8 levels); one fp64 atomic per workgroup;
      tail_bwd_small_kernel (16-bit, VEC 8, P / 8 < 256): NB samples of one channel per workgroup, NB = min(1024 / (P / 8),
          N, 16), so ceil(NB P / 8 / 256) vectors of 8 terms per thread, the product, 8 levels;
      pool_fwd_kernel: one workgroup per (n, c), ceil(P / (256 VEC)) vectors of VEC terms per thread, the fma and the max,
          8 levels, the division by P."""
    vec = _elem_vec(dtype, P, off)
    if entry == "pool_fwd":
        return -(-P // (256 * vec)) * vec + 2 + 8 + 1
    if entry == "tail_bwd" and dtype != torch.float32 and vec == 8 and P // 8 < 256:
        nb = min(1024 // (P // 8), n, 16)
        return -(-(nb * (P // 8)) // 256) * 8 + 1 + 8
    return 4 * vec + 1 + 8


def _aux_rn(gpu, seed):
    g_ = torch.Generator(device=gpu)
    g_.manual_seed(seed)
    return (lambda *s: torch.randn(*s, generator=g_, device=gpu, dtype=torch.float32)), g_


def _aux_raw(rn, n, c, P, dtype):
    """A raw conv output [N, C, P] with non-zero channel means, several standard deviations in some channels."""
    mu, sd = 3 * rn(c), 0.5 + rn(c).abs()
    return (rn(n, c, P) * sd.view(1, -1, 1) + mu.view(1, -1, 1)).to(dtype)


_PROJECT_MIN = 16


def _project_out(d, mask, basis):
    """d * mask minus its per-channel least-squares fit on mask * basis_k (fp64, [N, C, P]): the result's sums against each
    basis tensor vanish per channel, as the BatchNorm-backward sums (sum g, sum g y) do in a training step.  With a handful of
    active points the 2 x 2 / 3 x 3 system is singular: when a channel has fewer than _PROJECT_MIN, the case keeps the plain
    d * mask (the cancellation matters at full size, where every channel has thousands)."""
    if int(mask.sum((0, 2)).min()) < _PROJECT_MIN:
        return d * mask
    B = [mask * b for b in basis]
    G = torch.stack([torch.stack([(bi * bj).sum((0, 2)) for bj in B], -1) for bi in B], -2)
    r = torch.stack([(d * mask * b).sum((0, 2)) for b in B], -1)
    a = torch.linalg.solve(G, r.unsqueeze(-1)).squeeze(-1)
    return d * mask - sum(a[:, k].view(1, -1, 1) * B[k] for k in range(len(B)))


def _moment_checks(tag, got, gd, vals, L, count, gpu, rn):
    """The kernel's (sum g, sum g v) per channel against fp64, and what they do after the BatchNorm-backward finalize:
    both sums through tests.util.bn_bwd_fold64 with v's own statistics, dgamma and B = coef[:, 1] against the same fold of the
    fp64 sums, as a fraction of the bound the sum limits imply (|d dgamma| <= (lim1 + |mean| lim0) invstd, |d B| <=
    |gamma| invstd^2 |d dgamma| / count)."""
    from tests.util import bn_bwd_fold64
    vd = vals.double()
    ref = torch.stack([gd.sum((0, 2)), (gd * vd).sum((0, 2))], 1)
    lim = torch.stack([_sum_lim(L, gd.abs().sum((0, 2))), _sum_lim(L, (gd * vd).abs().sum((0, 2)))], 1)
    e = _within(f"{tag} sums", got, ref, lim)
    mean = vd.sum((0, 2)) / count
    inv = 1.0 / torch.sqrt((vd * vd).sum((0, 2)) / count - mean * mean + 1e-5)
    mi = torch.stack([mean, inv], 1).float()
    gamma = 1 + 0.3 * rn(got.shape[0])
    c_got, dga_got, _ = bn_bwd_fold64(got, count, mi, gamma)
    c_ref, dga_ref, _ = bn_bwd_fold64(ref, count, mi, gamma)
    mi64 = mi.double()
    lim_dg = (lim[:, 1] + mi64[:, 0].abs() * lim[:, 0]) * mi64[:, 1] * (1 + 1e-9) + 1e-300
    lim_b = gamma.double().abs() * mi64[:, 1] ** 2 * lim_dg / count * (1 + 1e-9) + 1e-300
    e_dg = _within(f"{tag} dgamma", dga_got, dga_ref, lim_dg)
    e_b = _within(f"{tag} B", c_got[:, 1], c_ref[:, 1], lim_b)
    return f"{tag} sums {e:.2e} (L {L}), dgamma {e_dg:.2e}, B {e_b:.2e}"


def _aux_tail_bwd(gpu, case, rn, g_, edge=False):
    """g = dy [y > 0] bit for bit; (sum g, sum g c_raw) and (sum g, sum g r_raw) at the fp32 summation bound, with dy built so
    that both sums cancel per channel."""
    from x3d_tf_amd import ops
    (_, dtype, n, c, P, has_r), off = _with_off(case, 6)
    B = _Bands(gpu, off)
    craw = B.view(_aux_raw(rn, n, c, P, dtype))
    rraw = B.view(_aux_raw(rn, n, c, P, dtype)) if has_r else None
    y = B.view(torch.relu(rn(n, c, P)).to(dtype))
    mask = (y > 0).double()
    d0 = rn(n, c, P).double()
    basis = [torch.ones_like(d0), craw.double()] + ([rraw.double()] if has_r else [])
    g = _project_out(d0, mask, basis)
    dy = torch.where(y > 0, g, d0).to(dtype)
    del g, d0, basis
    dyg = B((n, c, P), dtype, init=dy)
    sc = B((c, 2), torch.float64, fill=0.0)
    sr = B((c, 2), torch.float64, fill=0.0) if has_r else None
    ops.tail_bwd(dyg, y, craw, rraw, sc, sr)
    B.check()
    assert torch.equal(dyg, torch.where(y > 0, dy, torch.zeros_like(dy))), "tail_bwd: g differs from dy [y > 0]"
    gd = dy.double() * mask
    L = _aux_fp32_chain("tail_bwd", dtype, n, P, off)
    msg = "g exact, " + _moment_checks("c", sc, gd, craw, L, n * P, gpu, rn)
    if has_r:
        msg += ", " + _moment_checks("r", sr, gd, rraw, L, n * P, gpu, rn)
    return msg


def _aux_relu_bn_bwd_reduce(gpu, case, rn, g_, edge=False):
    """g = (dy | dpool / P) [s yraw + t > 0]: the dy form (g not written in the plans: sums only) and the dpool form (g at
    tol_store: the only arithmetic is dpool / P and the stored rounding).  Points whose z lies within 4 fp32 roundings of 0
    may take either side of the mask; they are left out of the g check and their |terms| added to the sum limits.  The dpool
    form's sums add the rounding of the stored g, which has one sign per (n, c): u_T sum |terms| on top of the fp32 bound."""
    from x3d_tf_amd import ops
    (_, dtype, n, c, P, form, g_written), off = _with_off(case, 7)
    B = _Bands(gpu, off)
    yraw = B.view(_aux_raw(rn, n, c, P, dtype))
    yd = yraw.double()
    mean = yd.mean((0, 2))
    sd = (yd * yd).mean((0, 2)) - mean * mean
    k = (1 + 0.3 * rn(c)).double() / torch.sqrt(sd + 1e-5)
    ss = B.view(torch.stack([k, 0.3 * rn(c).double() - mean * k], 1).float())
    s64, t64 = ss[:, 0].double().view(1, -1, 1), ss[:, 1].double().view(1, -1, 1)
    z = s64 * yd + t64
    amb = z.abs() <= 4 * _U * ((s64 * yd).abs() + t64.abs())
    mask = (z > 0).double()
    del z
    if form == "dy":
        d0 = rn(n, c, P).double()
        dy = B.view(torch.where(mask > 0, _project_out(d0, mask, [torch.ones_like(d0), yd]), d0).to(dtype))
        del d0
        dpool, gd = None, dy.double() * mask
    else:
        d0 = rn(n, c).double()
        A = torch.stack([mask.sum(2), (mask * yd).sum(2)], -1).transpose(0, 1)          # [C, N, 2]
        if n >= _PROJECT_MIN and int(mask.sum((0, 2)).min()) >= _PROJECT_MIN:          # (else singular: see _project_out)
            coef = torch.linalg.solve(A.transpose(1, 2) @ A, A.transpose(1, 2) @ d0.t().unsqueeze(-1))
            d0 = (d0.t() - (A @ coef).squeeze(-1)).t()                                  # sum_n dpool cnt = sum_n dpool sy = 0
        dpool = B.view(d0.float().contiguous())
        dy, gd = None, (dpool.double() / P).unsqueeze(-1) * mask
    gbuf = B((n, c, P), dtype) if g_written else None
    sums = B((c, 2), torch.float64, fill=0.0)
    ops.relu_bn_bwd_reduce(dy, dpool, yraw, ss, gbuf, sums)
    B.check()
    assert not edge or int(amb.sum()) <= 2, f"{int(amb.sum())} points at the mask boundary (expected < 0.1 per case)"
    msg = ""
    if g_written:
        keep = ~amb
        rt, at = tol_store(dtype)
        msg = f"g {_frac('g', gbuf[keep], gd[keep], rt, at * gd.abs().max().item()):.2e}, "
    L = _aux_fp32_chain("relu_bn_bwd_reduce", dtype, n, P, off)
    uT = {torch.float32: _U, torch.bfloat16: 2.0 ** -8, torch.float16: 2.0 ** -11}[dtype] if form == "dpool" else 0.0
    ref = torch.stack([gd.sum((0, 2)), (gd * yd).sum((0, 2))], 1)
    ga = (dy.double().abs() if dy is not None else (dpool.double().abs() / P).unsqueeze(-1).expand_as(yd)) * amb
    t0, t1 = gd.abs().sum((0, 2)), (gd * yd).abs().sum((0, 2))
    lim = torch.stack([_sum_lim(L, t0) + uT * t0 + ga.sum((0, 2)), _sum_lim(L, t1) + uT * t1 + (ga * yd.abs()).sum((0, 2))], 1)
    e = _within("sums", sums, ref, lim)
    return msg + f"sums {e:.2e} (L {L}, {int(amb.sum())} points at the mask boundary)"


def _aux_pool_fwd(gpu, case, rn, g_, edge=False):
    """pooled = mean_p relu(s x + t) at the fp32 summation bound over sum |relu| / P, and the rounding of the quotient."""
    from x3d_tf_amd import ops
    (_, dtype, n, c, P), off = _with_off(case, 5)
    B = _Bands(gpu, off)
    x = B.view(_aux_raw(rn, n, c, P, dtype))
    xd = x.double()
    mean = xd.mean((0, 2))
    k = 1.0 / torch.sqrt((xd * xd).mean((0, 2)) - mean * mean + 1e-5)
    ss = B.view(torch.stack([k, 0.2 * rn(c).double() - mean * k], 1).float())
    a = torch.relu(ss[:, 0].double().view(1, -1, 1) * xd + ss[:, 1].double().view(1, -1, 1))
    ref = a.mean(2)
    pooled = B((n, c), torch.float32)
    ops.pool_fwd(x, ss, pooled)
    B.check()
    L = _aux_fp32_chain("pool_fwd", dtype, n, P, off)
    e = _within("pooled", pooled, ref, _sum_lim(L, a.sum(2)) / P + 2 * _U * ref.abs())
    return f"pooled {e:.2e} (L {L})"


def _aux_subsample2(gpu, case, rn, g_, edge=False):
    from x3d_tf_amd import ops
    _, dtype, planes, h, w = case
    x = rn(1, planes, 1, h, w).to(dtype)
    B = _Bands(gpu)
    out = ops.subsample2(x, B((1, planes, 1, (h + 1) // 2, (w + 1) // 2), dtype))
    B.check()
    assert torch.equal(out, x[..., ::2, ::2]), "subsample2: not the even-pixel copy"
    return "exact"


def _aux_se_params(rn, c, wd):
    return (rn(wd, c) / c ** 0.5, 0.1 * rn(wd), rn(c, wd) / wd ** 0.5, 0.1 * rn(c))


def _aux_se_fwd(gpu, case, rn, g_, edge=False):
    """hidden = relu(W1 pooled + b1), gate = sigmoid(W2 hidden + b2), pooled = s pool_sums / P + t.  Limits: pooled carries 4
    fp32 roundings of |s pool_sums / P| + |t|; each GEMV the fp32 bound with L = K + 8 (any summation tree of K terms has
    a chain of at most K - 1, plus the product, the bias and the lane reduction), hidden's error through |W2|, and the
    sigmoid (slope <= 1/4) plus 4 roundings of the gate."""
    from x3d_tf_amd import ops
    _, n, c, wd, P = case
    mu, sd = 3 * rn(c).double(), (0.5 + rn(c).abs()).double()
    ps = P * mu.view(1, -1) + P ** 0.5 * sd.view(1, -1) * rn(n, c).double()
    k = (1 + 0.3 * rn(c)).double() / torch.sqrt(sd * sd / P + 1e-5)
    bss = torch.stack([k, 0.3 * rn(c).double() - mu * k], 1).float()
    w1, b1, w2, b2 = _aux_se_params(rn, c, wd)
    B = _Bands(gpu)
    gate, hidden = B((n, c), torch.float32), B((n, wd), torch.float32)
    ops.se_fwd(ps, float(P), bss, w1, b1, w2, b2, gate, hidden)
    B.check()
    s64, t64 = bss[:, 0].double(), bss[:, 1].double()
    pooled = s64 * ps / P + t64
    e_p = 4 * _U * ((s64 * ps / P).abs() + t64.abs())
    w1d, w2d = w1.double(), w2.double()
    h = torch.relu(pooled @ w1d.t() + b1.double())
    lim_h = e_p @ w1d.abs().t() + _sum_lim(c + 8, pooled.abs() @ w1d.abs().t() + b1.double().abs())
    z2 = h @ w2d.t() + b2.double()
    lim_z = lim_h @ w2d.abs().t() + _sum_lim(wd + 8, h.abs() @ w2d.abs().t() + b2.double().abs())
    gref = torch.sigmoid(z2)
    e_h = _within("hidden", hidden, h, lim_h)
    e_g = _within("gate", gate, gref, 0.25 * lim_z + 4 * _U * gref)
    return f"hidden {e_h:.2e}, gate {e_g:.2e}"


def _aux_se_bnb_bwd(gpu, case, rn, g_, edge=False):
    """BN_b backward through the SE gate from per-(n, c) sums: the fp64 restatement is autograd over the SUM-level graph
    L = sum_{n,c} gate (k (S2 - mean S1) + beta S1), with the batch statistics from pool_sums and Q = sum b_raw^2, so that
    dL/db_raw = A dv + B b_raw + C with A = dL/dS2, B = 2 dL/dQ (the same for every sample), C = dL/dpool_sums: coef_nc must reproduce that gradient
    (error of A rms(dv) + B rms(b_raw) + C within 2e-4 of its scale, test_se_bnb_bwd's tolerance) and the parameter
    gradients fp64 autograd (2e-4 of each one's maximum).  The slab jobs: the same bits as x3d_dw_slab_reduce on the same
    slabs, and the fp64 sum at the fp32 bound with L = parts + 8."""
    from x3d_tf_amd import ops
    _, n, c, wd, P, has_se, jobs = case
    mu, sd = 3 * rn(c), 0.5 + rn(c).abs()
    S1 = torch.empty((n, c), dtype=torch.float64, device=gpu)
    S2, ps, Q, Qd = torch.empty_like(S1), torch.empty_like(S1), torch.empty_like(S1), torch.empty_like(S1)
    for i in range(n):
        b = (rn(c, P) * sd.view(-1, 1) + mu.view(-1, 1)).double()
        dv = rn(c, P).double()
        S1[i], S2[i], ps[i], Q[i], Qd[i] = dv.sum(1), (dv * b).sum(1), b.sum(1), (b * b).sum(1), (dv * dv).sum(1)
    del b, dv
    m = n * P
    gam = (1 + 0.3 * rn(c)).double().requires_grad_(True)
    bet = (0.3 * rn(c)).double().requires_grad_(True)
    prm = [t.double().requires_grad_(True) for t in _aux_se_params(rn, c, wd)] if has_se else []
    lv = [S2.clone().requires_grad_(True), ps.clone().requires_grad_(True), Q.clone().requires_grad_(True)]
    mean = lv[1].sum(0) / m
    inv = 1.0 / torch.sqrt(lv[2].sum(0) / m - mean * mean + 1e-5)
    k = gam * inv
    gate = hid = None
    G = 1.0
    if has_se:
        pooled = k * (lv[1] / P - mean) + bet
        hid = torch.relu(pooled @ prm[0].t() + prm[1])
        gate = torch.sigmoid(hid @ prm[2].t() + prm[3])
        G = gate
    Lsum = (G * (k * (lv[0] - mean * S1) + bet * S1)).sum()
    grads = torch.autograd.grad(Lsum, lv + [gam, bet] + prm)
    A, Bq, Cp = grads[0], 2 * grads[2], grads[1]
    f32 = lambda t: t.detach().float().contiguous()
    bss = torch.stack([k, bet - mean * k], 1)
    bmi = torch.stack([mean, inv], 1)
    Bd = _Bands(gpu)
    fill = _GRAD_FILL if edge else 0.0
    coef = Bd((n, c, 4), torch.float32)
    dgam = Bd((c,), torch.float32, fill=fill)
    dbet = Bd((c,), torch.float32, fill=fill)
    kw = {}
    if has_se:
        kw = dict(w1=f32(prm[0]), b1=f32(prm[1]), w2=f32(prm[2]), b2=f32(prm[3]), gate=f32(gate), hidden=f32(hid),
                  dw1=Bd((wd, c), torch.float32, fill=fill), db1=Bd((wd,), torch.float32, fill=fill),
                  dw2=Bd((c, wd), torch.float32, fill=fill), db2=Bd((c,), torch.float32, fill=fill),
                  scratch=Bd((n * (2 * c + wd),), torch.float32))
    red = []
    for parts, elems in jobs:
        red.append((rn(parts * elems), Bd((elems,), torch.float32, fill=0.5), parts))
    ops.se_bnb_bwd(torch.stack([S1, S2], -1).contiguous(), ps if has_se else None, float(P), f32(bss), f32(bmi), f32(gam), dgam,
                   dbet, coef, n, c, reduce=red, **kw)
    Bd.check()
    msgs = []
    for j, (slab, dwj, parts) in enumerate(red):
        alone = Bd(tuple(dwj.shape), torch.float32, fill=0.5)
        ops.dw_slab_reduce([(slab, alone, parts)])
        Bd.check()
        assert torch.equal(alone, dwj), "the reduce slots of x3d_se_bnb_bwd and x3d_dw_slab_reduce add in the same order"
        sv = slab.double().view(parts, -1)
        ref = sv.sum(0) + 0.5
        msgs.append(f"slab{j} {_within(f'slab {j}', dwj, ref, _sum_lim(parts + 8, sv.abs().sum(0) + 0.5) + _U * ref.abs()):.2e}")
    rdv, rb = (Qd / P).sqrt(), (Q / P).sqrt()
    cf = coef.double()
    scale = (A.abs() * rdv + Bq.abs() * rb + Cp.abs()).max()
    err = (cf[:, :, 0] - A).abs() * rdv + (cf[:, :, 1] - Bq).abs() * rb + (cf[:, :, 2] - Cp).abs()
    e_c = _within("coef_nc (dL/db_raw)", err, torch.zeros_like(err), 2e-4 * scale)
    out = [("dgamma_b", dgam, grads[3]), ("dbeta_b", dbet, grads[4])]
    if has_se:
        out += [(nm, kw[nm], gr) for nm, gr in zip(("dw1", "db1", "dw2", "db2"), grads[5:])]
    # (edge cases: onto a pre-fill of _GRAD_FILL, whose sum with the gradient is rounded once more)
    pre = _U * (fill != 0.0)
    e_p = max(_within(nm, got, gr + fill, 2e-4 * gr.abs().max() + pre * (gr + fill).abs() + 1e-300) for nm, got, gr in out)
    return ", ".join([f"coef {e_c:.2e}", f"param grads {e_p:.2e}"] + msgs)


def _aux_dense_fwd(gpu, case, rn, g_, edge=False):
    """y = act(sum_k x m s w + b) at the fp32 bound, L = K + 8 (see _aux_se_fwd); the dropout mask scale (2.0, keep 0 / 1)
    is exact."""
    from x3d_tf_amd import ops
    _, n, kk, mm, act, mscale, bias = case
    x = torch.relu(rn(n, kk)) + 0.05
    w = rn(mm, kk) / kk ** 0.5
    b = 0.1 * rn(mm) if bias else None
    mask = (torch.rand((n, kk), generator=g_, device=gpu) >= 0.5).float() if mscale is not None else None
    B = _Bands(gpu)
    y = B((n, mm), torch.float32)
    ops.dense_fwd(x, w, b, y, act=act, mask=mask, mask_scale=1.0 if mscale is None else mscale)
    B.check()
    xm = x.double() * (mask.double() * mscale if mask is not None else 1.0)
    ref = xm @ w.double().t() + (b.double() if bias else 0.0)
    lim = _sum_lim(kk + 8, xm.abs() @ w.double().abs().t() + (b.double().abs() if bias else 0.0))
    if act == 1:
        ref = torch.relu(ref)
    return f"y {_within('y', y, ref, lim):.2e}"


def _aux_dense_bwd(gpu, case, rn, g_, edge=False):
    """dz = dy [y > 0]; dx = (W^T dz) m s (L = M + 8), dw += dz^T (x m s) and db += sum_n dz (L = N + 8), at the fp32 bound
    (+ the rounding of the pre-filled accumulators)."""
    from x3d_tf_amd import ops
    _, n, kk, mm, act, mscale, has_dx, has_db = case
    x = torch.relu(rn(n, kk)) + 0.05
    w = rn(mm, kk) / kk ** 0.5
    dy = rn(n, mm) / n
    y = torch.relu(rn(n, mm)) if act == 1 else None
    mask = (torch.rand((n, kk), generator=g_, device=gpu) >= 0.5).float() if mscale is not None else None
    B = _Bands(gpu)
    dx = B((n, kk), torch.float32) if has_dx else None
    dw = B((mm, kk), torch.float32, fill=0.25)
    db = B((mm,), torch.float32, fill=-0.5) if has_db else None
    ops.dense_bwd(dy, y, act, x, w, dx, dw, db, mask=mask, mask_scale=1.0 if mscale is None else mscale)
    B.check()
    ms = mask.double() * mscale if mask is not None else torch.ones((n, kk), dtype=torch.float64, device=gpu)
    dz = dy.double() * ((y > 0).double() if act == 1 else 1.0)
    xm, wd = x.double() * ms, w.double()
    msg = []
    if has_dx:
        ref = (dz @ wd) * ms
        msg.append(f"dx {_within('dx', dx, ref, _sum_lim(mm + 8, dz.abs() @ wd.abs()) * ms + 1e-300):.2e}")
    ref = dz.t() @ xm + 0.25
    msg.append(f"dw {_within('dw', dw, ref, _sum_lim(n + 8, dz.abs().t() @ xm.abs() + 0.25) + _U * ref.abs()):.2e}")
    if has_db:
        ref = dz.sum(0) - 0.5
        msg.append(f"db {_within('db', db, ref, _sum_lim(n + 8, dz.abs().sum(0) + 0.5) + _U * ref.abs()):.2e}")
    return ", ".join(msg)


def _aux_softmax_xent(gpu, case, rn, g_, edge=False):
    """probs, loss rows and dlogits = grad_scale d(sum loss)/dlogits (Keras' clipped cross-entropy on probabilities) against
    fp64 autograd; row 0 is in the clipped regime (one logit 40 above the rest at index min(3, M - 1), the label min(7, M - 1):
    elsewhere for M > 4; at M = 1 p = 1 is clipped, loss 0 and no gradient, and clamp has the same sub-gradient).  Limits: rho = (lambda
    sqrt(M + 8) + 8) u relative on every probability (the exponentials, the fp32 row sum, the division); loss rows 2 rho +
    4 u |loss|; dlogits grad_scale 4 rho (p_j + |ref| / grad_scale + 1e-7)."""
    import math
    from x3d_tf_amd import ops
    _, n, mm, gs, train = case
    logits = 3 * rn(n, mm)
    logits[0, min(3, mm - 1)] = 40.0
    labels = torch.randint(0, mm, (n,), generator=g_, device=gpu, dtype=torch.int32)
    labels[0] = min(7, mm - 1)
    B = _Bands(gpu)
    probs = B((n, mm), torch.float32)
    loss = B((n,), torch.float32) if train else None
    dl = B((n, mm), torch.float32) if train else None
    ops.softmax_xent(logits, labels if train else None, probs, loss, dl, gs)
    B.check()
    ld = logits.double().requires_grad_(True)
    p = torch.softmax(ld, -1)
    q = p.clamp(1e-7, 1 - 1e-7)
    rows = -torch.log(q.gather(1, labels.long().view(-1, 1)).squeeze(1)) + torch.log(q.sum(1))
    rho = (_LAM * math.sqrt(mm + 8) + 8) * _U
    pd = p.detach()
    msg = f"probs {_within('probs', probs, pd, rho * pd + 1e-300):.2e}"
    if train:
        (g,) = torch.autograd.grad(rows.sum() * gs, [ld])
        msg += f", loss {_within('loss rows', loss, rows.detach(), 2 * rho + 4 * _U * rows.detach().abs()):.2e}"
        msg += f", dlogits {_within('dlogits', dl, g, gs * 4 * rho * (pd + g.abs() / gs + 1e-7)):.2e}"
    return msg


def _aux_view_mean(gpu, case, rn, g_, edge=False):
    from x3d_tf_amd import ops
    _, videos, views, mm = case
    probs = torch.softmax(3 * rn(videos * views, mm), -1)
    B = _Bands(gpu)
    out = B((videos, mm), torch.float32)
    ops.view_mean(probs, out, views)
    B.check()
    pv = probs.double().view(videos, views, mm)
    ref = pv.mean(1)
    return f"out {_within('view mean', out, ref, _sum_lim(views + 8, pv.sum(1)) / views + 2 * _U * ref):.2e}"


def _aux_bn_stats(rn, c, count):
    """fp64 (sum, sum of squares) of `count` points per channel with means up to several standard deviations."""
    mu, sd = 3 * rn(c).double(), (0.5 + rn(c).abs()).double()
    mean = mu + sd * rn(c).double() / count ** 0.5
    var = sd * sd * (1 + 0.01 * rn(c).double())
    return count * mean, count * (var + mean * mean)


def _aux_bn_finalize(gpu, case, rn, g_, edge=False):
    """x3d_bn_finalize reading the replicated statistics layout (every copy holds a random share of the totals) against fp64
    of the same fp64 copies: scale / shift, mean / invstd and the moving statistics (momentum 0.9, unbiased variance), each to
    _AUX_ULPS fp32 roundings of the magnitude of its terms."""
    from x3d_tf_amd import hip, ops
    _, c, count, upd = case
    s1, s2 = _aux_bn_stats(rn, c, count)
    r, stride = hip.stats_layout(c)
    share = torch.rand((r, c), generator=g_, device=gpu).double()
    share = share / share.sum(0, keepdim=True)
    buf = torch.zeros(r * stride, dtype=torch.float64, device=gpu)
    bv = buf.view(r, stride)[:, :2 * c].view(r, c, 2)
    bv[:, :, 0], bv[:, :, 1] = share * s1, share * s2
    gamma, beta = 1 + 0.3 * rn(c), 0.3 * rn(c)
    mmv, mvv = rn(c), 0.5 + rn(c).abs()
    mm_, mv_ = mmv.clone(), mvv.clone()
    ss = torch.empty((c, 2), device=gpu)
    mi = torch.empty((c, 2), device=gpu)
    ops.bn_finalize(buf, count, gamma, beta, mm_, mv_, 1e-5, 0.9, upd, ss, mi)
    torch.cuda.synchronize()
    S1, S2 = bv[:, :, 0].sum(0), bv[:, :, 1].sum(0)
    mean = S1 / count
    var = S2 / count - mean * mean
    inv = 1.0 / torch.sqrt(var + 1e-5)
    g64, b64 = gamma.double(), beta.double()
    sc = g64 * inv
    u = _AUX_ULPS * _U
    e = [_within("scale", ss[:, 0], sc, u * sc.abs()), _within("shift", ss[:, 1], b64 - mean * sc, u * (b64.abs() + (mean * sc).abs())),
         _within("mean", mi[:, 0], mean, u * mean.abs()), _within("invstd", mi[:, 1], inv, u * inv)]
    if upd:
        a, b = 0.9 * mmv.double(), 0.1 * mean
        e.append(_within("moving_mean", mm_, a + b, u * (a.abs() + b.abs())))
        a, b = 0.9 * mvv.double(), 0.1 * var * count / (count - 1)
        e.append(_within("moving_var", mv_, a + b, u * (a.abs() + b.abs())))
    return f"worst {max(e):.2e}"


def _aux_bwd_fin_inputs(rn, c, count):
    """(sums [C][2] = (sum g, sum g y) of a training step -- sum g near 0, sum g y of sqrt(count) size --, mean_invstd, gamma)."""
    s1, s2 = _aux_bn_stats(rn, c, count)
    mean = s1 / count
    inv = 1.0 / torch.sqrt(s2 / count - mean * mean + 1e-5)
    sums = torch.stack([0.01 * count ** 0.5 * rn(c).double(), count ** 0.5 * rn(c).double() / inv], 1)
    return sums, torch.stack([mean, inv], 1).float(), 1 + 0.3 * rn(c)


def _aux_bwd_fin_check(sums, count, mi, gamma, coef, dg, db):
    """coef, dgamma (+= onto 0.25), dbeta (+= onto -0.5) against tests.util.bn_bwd_fold64 of the same operands, to _AUX_ULPS
    fp32 roundings of the magnitude of each result's terms."""
    from tests.util import bn_bwd_fold64
    ref, dga, dbe = bn_bwd_fold64(sums, count, mi, gamma)
    mean, inv, g = mi[:, 0].double(), mi[:, 1].double(), gamma.double()
    u = _AUX_ULPS * _U
    mdg = (sums[:, 1].abs() + (mean * sums[:, 0]).abs()) * inv
    k1 = g * inv
    mb = k1.abs() * inv * mdg / count
    mc = k1.abs() * sums[:, 0].abs() / count + mb * mean.abs()
    return max(_within("coef A", coef[:, 0], ref[:, 0], u * k1.abs()), _within("coef B", coef[:, 1], ref[:, 1], u * mb),
               _within("coef C", coef[:, 2], ref[:, 2], u * mc + 1e-300),
               _within("dgamma", dg, dga + 0.25, u * (mdg + 0.25)), _within("dbeta", db, dbe - 0.5, u * (dbe.abs() + 0.5)))


def _aux_bn_bwd_finalize(gpu, case, rn, g_, edge=False):
    from x3d_tf_amd import ops
    _, c, count = case
    sums, mi, gamma = _aux_bwd_fin_inputs(rn, c, count)
    coef = torch.empty((c, 4), device=gpu)
    dg, db = torch.full((c,), 0.25, device=gpu), torch.full((c,), -0.5, device=gpu)
    ops.bn_bwd_finalize(sums, count, mi, gamma, coef, dg, db)
    torch.cuda.synchronize()
    return f"worst {_aux_bwd_fin_check(sums, count, mi, gamma, coef, dg, db):.2e}"


def _aux_bn_bwd_finalize_rc(gpu, case, rn, g_, edge=False):
    """x3d_bn_bwd_finalize_rc in the plan's form writes the same bits as x3d_bn_bwd_finalize + x3d_pw_bwd_rc_prepare +
    x3d_pw_bwd_rc_finish one after the other, and its finalize outputs match fp64 as in _aux_bn_bwd_finalize."""
    from x3d_tf_amd import hip, ops
    _, dtype, c, count, cin, fin = case
    lib = hip.load()
    sums, mi, gamma = _aux_bwd_fin_inputs(rn, c, count)
    w = 0.2 * rn(c, cin) if cin else None
    pe = int(lib.x3d_pw_bwd_rc_panel_elems(c, cin)) if cin else 0
    if fin:
        fco, fci = fin
        fw, fcoef = 0.2 * rn(fco, fci), 0.5 * rn(fco, 4)
        fsums = 30 * rn((fco + 1 + fci) * fci)

    def fresh():
        return (torch.zeros((c, 4), device=gpu), torch.full((c,), 0.25, device=gpu), torch.full((c,), -0.5, device=gpu),
                torch.zeros(max(pe, 1), dtype=dtype, device=gpu), torch.zeros(max(cin, 1), device=gpu),
                torch.full(fin or (1,), 0.5, device=gpu))
    dt = hip.dtype_code(dtype)
    coef0, dg0, db0, pan0, c00, dw0 = fresh()
    ops.bn_bwd_finalize(sums, count, mi, gamma, coef0, dg0, db0)
    if cin:
        hip.call("x3d_pw_bwd_rc_prepare", w.data_ptr(), coef0.data_ptr(), pan0.data_ptr(), c00.data_ptr(), c, cin, dt)
    if fin:
        hip.call("x3d_pw_bwd_rc_finish", fsums.data_ptr(), fw.data_ptr(), fcoef.data_ptr(), dw0.data_ptr(), fco, fci, dt)
    coef1, dg1, db1, pan1, c01, dw1 = fresh()
    ops.bn_bwd_finalize_rc(sums, count, mi, gamma, coef1, dg1, db1, dtype, prep=(w, pan1, c01) if cin else None,
                           fin=(fsums, fw, fcoef, dw1) if fin else None)
    torch.cuda.synchronize()
    assert torch.equal(coef0, coef1) and torch.equal(dg0, dg1) and torch.equal(db0, db1), "finalize outputs differ"
    assert torch.equal(pan0, pan1) and torch.equal(c00, c01), "prepare outputs differ"
    assert torch.equal(dw0, dw1), "finish output differs"
    return f"same bits as the three launches; finalize worst {_aux_bwd_fin_check(sums, count, mi, gamma, coef1, dg1, db1):.2e}"


def _aux_bn_eval_coef_batched(gpu, case, rn, g_, edge=False):
    """The whole X3D-XL inference BatchNorm table in one launch: scale = gamma invstd, shift = beta - mean scale, mean /
    invstd from the moving statistics, every item against fp64 to _AUX_ULPS fp32 roundings of its terms' magnitude."""
    from x3d_tf_amd import hip
    _, chans = case
    rows, items = [], []
    for c in chans:
        g, b, m_, v = 1 + 0.3 * rn(c), 0.3 * rn(c), 3 * rn(c), 0.05 + rn(c).abs()
        ss, mi = torch.empty((c, 2), device=gpu), torch.empty((c, 2), device=gpu)
        rows.append((g, b, m_, v, ss, mi))
        items.append(hip.BnEvalItem(g.data_ptr(), b.data_ptr(), m_.data_ptr(), v.data_ptr(), ss.data_ptr(), mi.data_ptr(), c))
    arr = (hip.BnEvalItem * len(items))(*items)
    table = torch.frombuffer(bytearray(bytes(arr)), dtype=torch.uint8).to(gpu)
    hip.call("x3d_bn_eval_coef_batched", table.data_ptr(), len(items), 1e-5)
    torch.cuda.synchronize()
    u, worst = _AUX_ULPS * _U, 0.0
    for i, (g, b, m_, v, ss, mi) in enumerate(rows):
        inv = 1.0 / torch.sqrt(v.double() + 1e-5)
        sc = g.double() * inv
        worst = max(worst, _within(f"item {i} scale", ss[:, 0], sc, u * sc.abs()),
                    _within(f"item {i} shift", ss[:, 1], b.double() - m_.double() * sc, u * (b.double().abs() + (m_.double() * sc).abs())),
                    _within(f"item {i} mean", mi[:, 0], m_.double(), 0.0), _within(f"item {i} invstd", mi[:, 1], inv, u * inv))
    return f"worst {worst:.2e}"


def _aux_tail_fwd(gpu, case, rn, g_, edge=False):
    """y = relu(s_c c + t_c + (s_r r + t_r)) against fp64 at tol_store (the stored rounding and a few fp32 roundings, as
    test_bn_tail_pool); shortcut None (BN + ReLU of the stem), "identity" (s_r = 1, t_r = 0) or "conv"."""
    from x3d_tf_amd import ops
    (_, dtype, n, c, P, shortcut), off = _with_off(case, 6)
    assert shortcut in (None, "identity", "conv")
    B = _Bands(gpu, off)
    craw = B.view(_aux_raw(rn, n, c, P, dtype))
    sh = B.view(_aux_raw(rn, n, c, P, dtype)) if shortcut else None
    ssc = B.view(torch.stack([1 + 0.3 * rn(c), 0.3 * rn(c)], 1))
    ssr = B.view(torch.stack([1 + 0.3 * rn(c), 0.3 * rn(c)], 1)) if shortcut == "conv" else None
    y = B((n, c, P), dtype)
    ops.tail_fwd(craw, ssc, sh, ssr, y)
    B.check()
    col = lambda s, j: s[:, j].double().view(1, -1, 1)
    z = col(ssc, 0) * craw.double() + col(ssc, 1)
    if shortcut:
        z = z + (col(ssr, 0) * sh.double() + col(ssr, 1) if ssr is not None else sh.double())
    ref = torch.relu(z)
    rt, at = tol_store(dtype)
    return f"y {_frac('y', y, ref, rt, at * ref.abs().max().item()):.2e}"


def _aux_dw_slab_reduce(gpu, case, rn, g_, edge=False):
    """x3d_dw_slab_reduce alone, one or two jobs: dw (pre-filled with 0.5) against the fp64 sum of the parts at the fp32 bound
    with L = parts + 8 (as the slots of _aux_se_bnb_bwd), and a second run on the same slabs gives the same bits."""
    from x3d_tf_amd import ops
    _, jobs = case
    B = _Bands(gpu)
    slabs = [rn(parts * elems) for parts, elems in jobs]
    runs = []
    for _ in range(2):
        dws = [B((elems,), torch.float32, fill=0.5) for _, elems in jobs]
        ops.dw_slab_reduce([(s, d, parts) for s, d, (parts, _) in zip(slabs, dws, jobs)])
        runs.append(dws)
    B.check()
    msgs = []
    for j, (slab, (parts, elems)) in enumerate(zip(slabs, jobs)):
        assert torch.equal(runs[0][j], runs[1][j]), f"job {j}: two runs on the same slabs differ"
        sv = slab.double().view(parts, elems)
        ref = sv.sum(0) + 0.5
        msgs.append(f"slab{j} {_within(f'slab {j}', runs[0][j], ref, _sum_lim(parts + 8, sv.abs().sum(0) + 0.5) + _U * ref.abs()):.2e}")
    return ", ".join(msgs + ["two runs the same bits"])


_BAD_BITS = {"none": None, "+inf": 0x7F800000, "-inf": 0xFF800000 - (1 << 32), "nan": 0x7FC00000, "-nan-payload": 0xFF800001 - (1 << 32)}
ALL_FINITE_CAP, L2_SUMSQ_CAP = 2048, 1024         # workgroups of x3d_all_finite / x3d_l2_sumsq at most (head.hip), 2048 elements each


def _aux_all_finite(gpu, case, rn, g_, edge=False):
    """The flag (set to 1 by the caller) is cleared exactly when one of the n values is inf / nan.  The background holds FLT_MAX,
    -FLT_MAX, a denormal and -0.0: values next to the exponent mask that are finite.  pos: "first", "last", "mid", or "trip2",
    an index past workgroups * 256 that only the second trip of the grid-stride loop reads."""
    from x3d_tf_amd import hip
    _, n, kind, pos = case
    fmax = 3.4028234663852886e38
    bg = torch.tensor([fmax, -fmax, 1e-40, -0.0, 1.0, -2.5, 0.0], device=gpu)
    g = bg.repeat(-(-n // bg.numel()))[:n].contiguous()
    if kind != "none":
        stride = min(-(-n // 2048), ALL_FINITE_CAP) * 256
        i = {"first": 0, "last": n - 1, "mid": n // 2, "trip2": stride + 7}[pos]
        assert 0 <= i < n and (pos != "trip2" or n > stride + 7)
        g.view(torch.int32)[i] = _BAD_BITS[kind]
        assert not bool(torch.isfinite(g[i]))
    assert int(torch.isfinite(g).sum()) == n - (kind != "none")
    B = _Bands(gpu)
    flag = B((1,), torch.int32, fill=1)
    hip.call("x3d_all_finite", g.data_ptr(), n, flag.data_ptr())
    B.check()
    want = 1 if kind == "none" else 0
    assert int(flag) == want, f"all_finite: flag {int(flag)}, expected {want}"
    return f"flag {want} exact"


def _aux_l2_sumsq(gpu, case, rn, g_, edge=False):
    """out (fp64, pre-filled with 0.5) += sum of w^2 over the mask: every workgroup sums ceil(n / (workgroups 256)) squares per
    thread in fp32, then the 256-thread block_sum (8 levels) and one fp64 atomic: L = that + 1 (the square) + 8."""
    from x3d_tf_amd import ops
    _, n, mask = case
    w = rn(n)
    m = {None: None, "random": (torch.rand(n, generator=g_, device=gpu) > 0.5).to(torch.uint8),
         "zeros": torch.zeros(n, dtype=torch.uint8, device=gpu)}[mask]
    B = _Bands(gpu)
    out = B((1,), torch.float64, fill=0.5)
    ops.l2_sumsq(w, m, out)
    B.check()
    wg = min(-(-n // 2048), L2_SUMSQ_CAP)
    L = -(-n // (wg * 256)) + 1 + 8
    sq = (w.double() ** 2 * (m.double() if m is not None else 1.0)).sum()
    ref = sq + 0.5
    return f"out {_within('l2', out, ref.view(1), _sum_lim(L, sq.item()) + _U * ref.abs().item()):.2e} (L {L})"


def _aux_nthwc_to_ncthw(gpu, case, rn, g_, edge=False):
    """dst [N, C, P] = src [N, P, C] converted, bit for bit permute().to(); `off` moves the source off 16-byte alignment."""
    from x3d_tf_amd import ops
    (_, sdt, ddt, n, c, P), off = _with_off(case, 6)
    src = _Bands(gpu, off).view((3 * rn(n, P, 1, 1, c)).to(sdt))
    B = _Bands(gpu)
    dst = B((n, c, P, 1, 1), ddt)
    ops.nthwc_to_ncthw(src, dst)
    B.check()
    assert torch.equal(dst, src.permute(0, 4, 1, 2, 3).to(ddt)), "nthwc_to_ncthw: not permute().to()"
    return "exact"


def _refused(fn, outs):
    """fn() fails with X3D_ERR_INVALID and leaves every tensor of outs as it was, bit for bit."""
    import pytest
    from x3d_tf_amd import hip
    bits = lambda v: v.view(_BITS[v.element_size()])
    before = [bits(v).clone() for v in outs]
    with pytest.raises(hip.X3DHipError, match=r"failed \(1\)"):
        fn()
    torch.cuda.synchronize()
    assert all(torch.equal(bits(v), b) for v, b in zip(outs, before)), "a refused call wrote to an output"
    return "refused, outputs untouched"


def _aux_dense_bwd_refused(gpu, case, rn, g_, edge=False):
    """The host limits of x3d_dense_bwd (64 KiB of LDS for dz [DENSE_BN][M] and for dzs [N rounded up to 8][DENSE_BM]) are
    checked before the first of its two launches."""
    from x3d_tf_amd import ops
    _, n, kk, mm = case
    B = _Bands(gpu)
    dx, dw, db = B((n, kk), torch.float32), B((mm, kk), torch.float32, fill=0.25), B((mm,), torch.float32, fill=-0.5)
    return _refused(lambda: ops.dense_bwd(rn(n, mm), None, 0, rn(n, kk), rn(mm, kk), dx, dw, db), [dx, dw, db])


def _aux_se_fwd_refused(gpu, case, rn, g_, edge=False):
    from x3d_tf_amd import ops
    _, n, c, wd = case
    B = _Bands(gpu)
    gate, hidden = B((n, c), torch.float32), B((n, wd), torch.float32)
    w1, b1, w2, b2 = _aux_se_params(rn, c, wd)
    return _refused(lambda: ops.se_fwd(rn(n, c).double(), 8.0, rn(c, 2), w1, b1, w2, b2, gate, hidden), [gate, hidden])


def _aux_dw_slab_reduce_refused(gpu, case, rn, g_, edge=False):
    """elems % 4 != 0, or a slab view that is not 16-byte aligned (off floats into its allocation)"""
    from x3d_tf_amd import ops
    _, parts, elems, off = case
    B = _Bands(gpu)
    dw = B((elems,), torch.float32, fill=0.5)
    slab = rn(parts * elems + off)[off:]
    assert elems % 4 != 0 or slab.data_ptr() % 16 != 0
    return _refused(lambda: ops.dw_slab_reduce([(slab, dw, parts)]), [dw])


_AUX_CASES = {"tail_bwd": _aux_tail_bwd, "relu_bn_bwd_reduce": _aux_relu_bn_bwd_reduce, "pool_fwd": _aux_pool_fwd,
              "subsample2": _aux_subsample2, "se_fwd": _aux_se_fwd, "se_bnb_bwd": _aux_se_bnb_bwd, "dense_fwd": _aux_dense_fwd,
              "dense_bwd": _aux_dense_bwd, "softmax_xent": _aux_softmax_xent, "view_mean": _aux_view_mean,
              "bn_finalize": _aux_bn_finalize, "bn_bwd_finalize": _aux_bn_bwd_finalize,
              "bn_bwd_finalize_rc": _aux_bn_bwd_finalize_rc, "bn_eval_coef_batched": _aux_bn_eval_coef_batched,
              "tail_fwd": _aux_tail_fwd, "dw_slab_reduce": _aux_dw_slab_reduce, "all_finite": _aux_all_finite,
              "l2_sumsq": _aux_l2_sumsq, "nthwc_to_ncthw": _aux_nthwc_to_ncthw, "dense_bwd_refused": _aux_dense_bwd_refused,
              "se_fwd_refused": _aux_se_fwd_refused, "dw_slab_reduce_refused": _aux_dw_slab_reduce_refused}

