"""Single layers at BASELINE config 3's FULL size (X3D-M, 64 clips of 16 x 224^2, bf16 / fp16 storage) against fp64 on the GPU.

The kernel-level parity cases (tests/test_kernels_gpu.py) run shapes a CPU finishes in seconds: at most 150 k points per
channel.  Three kernels of the headline step reduce over 3.2 - 12.8 M points in fp32 (MFMA accumulators, per-thread partial
sums, fp32 atomics), one of them -- the recomputed-output `a` backward, pw_bwd_rc.hip -- through a CANCELLING expression
(dW = diag(A)(sum g x^T) + diag(B) W (sum x x^T) + C (sum x)^T with a post-ReLU x of positive mean: the C term removes the mean
part of the first).  "Finite and linear in the upstream gradient" (test_full_size_plan_properties) passes for any amount of
cancellation error, so here the same launches are compared with the fp64 definition at the real reduction length.

The stem (conv_s -> conv_t, one launch each way for 16-bit clips: stem_fused.hip) reduces its weight gradients over the
same 12.8 M points, from inputs with the non-zero channel means of a normalised clip, so that sum dY = 0 cancels their mean
part as in a real step; its BatchNorm sums go through replicated fp64 atomics.  Those cases run here as well, with the
two-kernel plans (stem.hip) that the fp32 model and X3D-XL training use.

Every depthwise launch (tests/shapes.py DW_FULL) and every pointwise launch (PW_FULL: the `a` / `c` / shortcut convs and conv5,
x3d_pw_fwd / _dgrad / _wgrad / _bwd, each in its plan's form -- prologue, residual-tail fold, inference epilogue, weight-gradient
slabs, the folded BatchNorm-backward finalize and its publishing) of BASELINE configs 2 - 5 and config 3 in fp16 run here too,
at their real grids, and so does every other launch of those plans (AUX_FULL: BatchNorm bookkeeping, residual-tail backward,
squeeze-excite, slab reductions, head, loss): tests/test_dispatch_coverage.py keeps the three lists complete.

The fp64 side is torch on the GPU (einsum / shifted slices), TEST SIDE ONLY, chunked over samples; it restates the same
definitions the small cases check against the CPU oracle (test_pw_bwd_rc, test_pw_wgrad, test_dw3d_bwd), with the
BatchNorm-backward coefficients DERIVED from the data (sum dY = 0 and sum dY * yhat = 0 per channel, as in a real step) instead
of drawn at random -- that is what makes the moment sums cancel.
"""
import pytest
import torch

from tests import shapes as S
from tests.aux_checks import (_AUX_CASES, _AUX_ULPS, _LAM, _U, _aux_fp32_chain, _aux_raw, _aux_rn, _check, _elem_vec,  # noqa: F401
                              _frac, _moment_checks, _project_out, _sum_lim, _within)
from tests.util import bn_bwd_coef_sums as _bn_bwd_coef_sums, round_to, tie_slack_t, tol_gemm, tol_store

pytestmark = pytest.mark.gpu
HALF = [torch.bfloat16, torch.float16]


def _wtol(dtype):
    return 1e-3 if dtype == torch.bfloat16 else 4e-4      # as tests/test_kernels_gpu.py::_wtol


def _bn_bwd_coef(g, y, gamma):
    """[C][4] fp32 coefficients (A, B, C, 0) of dY = A g + B y + C for training-mode BatchNorm over (N, T, H, W), from the
    tensors themselves: fp64 statistics, as x3d_bn_finalize / x3d_bn_bwd_finalize produce them."""
    m = y.shape[0] * y.shape[2] * y.shape[3] * y.shape[4]
    return _bn_bwd_coef_sums(m, y.sum((0, 2, 3, 4)), (y * y).sum((0, 2, 3, 4)), g.sum((0, 2, 3, 4)), (g * y).sum((0, 2, 3, 4)), gamma)



@pytest.mark.parametrize("dtype", HALF)
def test_block0_a_backward_recomputed_output_full_size(gpu, dtype):
    """x3d_pw_bwd, rc form, block 0 of X3D-M at batch 64: 24 <-> 54 channels on 16 x 112 x 112 points (12.8 M per channel), the
    strided shortcut-gradient add and the stem-fold tail, post-ReLU x with mean/std ~ 1.  dx against the fold with its panel
    operands rounded (tol_gemm), dW against the DEFINITION dY x^T in fp64 (_wtol: 1e-3 / 4e-4 of its maximum)."""
    from x3d_tf_amd import ops
    n, cin, cout, t, h, w = 64, 24, 54, 16, 112, 112
    g_ = torch.Generator(device=gpu)
    g_.manual_seed(41)
    rn = lambda *s: torch.randn(*s, generator=g_, device=gpu, dtype=torch.float32)
    t_raw = (rn(n, cin, t, h, w) + 0.6).to(dtype)                       # the stem's conv_t output; x = relu(.) = y0
    x = torch.relu(t_raw.float()).to(dtype)
    wt = rn(cout, cin) * 0.2
    gamma = 1 + 0.3 * rn(cout)
    beta = 0.3 * rn(cout)
    wr = round_to(wt.cpu(), dtype).to(gpu)
    # upstream gradient = what the depthwise backward emits: masked by the ReLU behind bn_a
    g = torch.empty((n, cout, t, h, w), dtype=dtype, device=gpu)
    CH = 8
    s1 = torch.zeros(cout, dtype=torch.float64, device=gpu)
    s2 = torch.zeros(cout, dtype=torch.float64, device=gpu)
    for i in range(0, n, CH):        # statistics of y = Wr x
        y = torch.einsum("oc,ncthw->nothw", wr, x[i:i + CH].double())
        s1 += y.sum((0, 2, 3, 4))
        s2 += (y * y).sum((0, 2, 3, 4))
        del y
    m = n * t * h * w
    mean = s1 / m
    invstd = 1.0 / torch.sqrt(s2 / m - mean * mean + 1e-5)
    dbe = torch.zeros(cout, dtype=torch.float64, device=gpu)
    dgy = torch.zeros(cout, dtype=torch.float64, device=gpu)
    for i in range(0, n, CH):
        y = torch.einsum("oc,ncthw->nothw", wr, x[i:i + CH].double())
        z = (y - mean.view(1, -1, 1, 1, 1)) * (gamma.double() * invstd).view(1, -1, 1, 1, 1) + beta.double().view(1, -1, 1, 1, 1)
        gi = (rn(CH, cout, t, h, w) * (z > 0)).to(dtype)
        g[i:i + CH] = gi
        dbe += gi.double().sum((0, 2, 3, 4))
        dgy += (gi.double() * y).sum((0, 2, 3, 4))
        del y, z, gi
    dga = (dgy - mean * dbe) * invstd
    k1 = gamma.double() * invstd
    bb = -k1 * invstd * dga / m
    cc = -k1 * dbe / m - bb * mean
    coef = torch.stack([k1, bb, cc, torch.zeros_like(cc)], 1).float()
    add = rn(n, cin, t, h // 2, w // 2).to(dtype)                        # the strided shortcut conv's data gradient
    dx = torch.empty((n, cin, t, h, w), dtype=dtype, device=gpu)
    dw = torch.full((cout, cin), 0.5, dtype=torch.float32, device=gpu)
    sums_c = torch.zeros((cin, 2), dtype=torch.float64, device=gpu)
    ok = ops.pw_bwd_rc(g, x, wt, coef, dx, dw, ops.EPI_ADD_STRIDED, add, tail_c=t_raw, tail_sums_c=sums_c)
    torch.cuda.synchronize()
    assert ok, "the recomputed-output form should cover block 0 of X3D-M"
    # ---- fp64 definition, chunked
    c = coef.double()
    w1 = round_to((wr.cpu() * c[:, 0:1].cpu()).float(), dtype).to(gpu)
    mm = round_to(torch.einsum("oc,o,od->cd", wr, c[:, 1], wr).float().cpu(), dtype).to(gpu)
    c0 = (wr * c[:, 2:3]).sum(0)
    dw_ref = torch.zeros((cout, cin), dtype=torch.float64, device=gpu)
    rt, at = tol_gemm(dtype)
    worst_dx, scale = 0.0, 0.0
    ts1 = torch.zeros(cin, dtype=torch.float64, device=gpu)
    ts2 = torch.zeros(cin, dtype=torch.float64, device=gpu)
    refs = []
    for i in range(0, n, CH):
        xd, gd = x[i:i + CH].double(), g[i:i + CH].double()
        y = torch.einsum("oc,ncthw->nothw", wr, xd)
        dy = c[:, 0].view(1, -1, 1, 1, 1) * gd + c[:, 1].view(1, -1, 1, 1, 1) * y + c[:, 2].view(1, -1, 1, 1, 1)
        dw_ref += torch.einsum("nothw,ncthw->oc", dy, xd)
        del y, dy
        ref = (torch.einsum("oc,nothw->ncthw", w1, gd) + torch.einsum("cd,ndthw->ncthw", mm, xd) + c0.view(1, -1, 1, 1, 1))
        ref[:, :, :, ::2, ::2] += add[i:i + CH].double()
        ref = ref * (xd > 0)
        scale = max(scale, ref.abs().max().item())
        refs.append((i, ref))
        dxs = dx[i:i + CH].double()
        ts1 += dxs.sum((0, 2, 3, 4))
        ts2 += (dxs * t_raw[i:i + CH].double()).sum((0, 2, 3, 4))
        if len(refs) == 2 or i + CH >= n:      # (two chunks at a time in memory)
            for j, rf in refs:
                worst_dx = max(worst_dx, _check(f"dx[{j}:{j + CH}]", dx[j:j + CH], rf, rt, at * max(scale, 1e-30)))
            refs = []
    # (measured: 2.5e-6 / 1.9e-6 of the maximum -- profiles/r05_full_size_fp64_checks.txt -- although the sum cancels to 1e-3 of
    # its terms; the kernel tests' limit for this quantity is 1e-3 / 4e-4, here a tenth of it)
    tol = 0.1 * _wtol(dtype)
    e_dw = _check("dw", dw.double() - 0.5, dw_ref, tol, tol * dw_ref.abs().max().item())
    st = 3e-3 if dtype == torch.bfloat16 else 5e-4
    sref = torch.stack([ts1, ts2], 1)
    _check("tail_sums_c", sums_c, sref, 10 * st, 10 * st * max(1.0, sref.abs().max().item()))
    print(f"full-size block-0 `a` backward {dtype}: dx err {worst_dx:.2e} of max, dW err {e_dw:.2e} of max (limit {tol:.0e}); "
          f"|dW| max {dw_ref.abs().max().item():.3e}, term scale {(c[:, 0].abs().max() * g.double().abs().mean() * x.double().mean() * m).item():.3e}")


@pytest.mark.parametrize("dtype", HALF)
@pytest.mark.parametrize("which", ["c", "a"])
def test_stage5_weight_gradient_full_size(gpu, dtype, which):
    """x3d_pw_wgrad of stage 5 at batch 64 (50 176 points per channel, 7 x 7 planes): `c` conv 192 x 432 with the
    BN_b * gate -> swish prologue, `a` conv 432 x 192 on the block input; coefficients derived from the data."""
    from x3d_tf_amd import ops
    n, t, h, w = 64, 16, 7, 7
    cin, cout = (432, 192) if which == "c" else (192, 432)
    g_ = torch.Generator(device=gpu)
    g_.manual_seed(43)
    rn = lambda *s: torch.randn(*s, generator=g_, device=gpu, dtype=torch.float32)
    x = rn(n, cin, t, h, w).to(dtype)
    if which == "a":
        x = torch.relu(x.float() + 0.3).to(dtype)
    yraw = (rn(n, cout, t, h, w) * 0.8 + 0.2).to(dtype)
    g = rn(n, cout, t, h, w).to(dtype)
    coef = _bn_bwd_coef(g.double(), yraw.double(), (1 + 0.3 * rn(cout)).double())
    ss = gate = None
    act = 0
    xin = x.double()
    if which == "c":
        ss = torch.stack([1 + 0.3 * rn(cin), 0.3 * rn(cin)], 1)
        gate = torch.rand((n, cin), generator=g_, device=gpu)
        act = 2
        u = (x.float() * ss[:, 0].view(1, -1, 1, 1, 1) + ss[:, 1].view(1, -1, 1, 1, 1)) * gate[:, :, None, None, None]
        xin = (u * torch.sigmoid(u)).to(dtype).double()
    cf = coef.float()
    dy = (cf[:, 0].view(1, -1, 1, 1, 1) * g.float() + cf[:, 1].view(1, -1, 1, 1, 1) * yraw.float() + cf[:, 2].view(1, -1, 1, 1, 1)).to(dtype).double()
    ref = torch.einsum("nothw,ncthw->oc", dy, xin)
    dw = torch.full((cout, cin), 0.5, dtype=torch.float32, device=gpu)
    ops.pw_wgrad(g, yraw, coef, x, dw, in_ss=ss, in_gate=gate, in_act=act)
    torch.cuda.synchronize()
    tol = 0.3 * _wtol(dtype)        # (measured 6.3e-5 / 1.4e-5 of the maximum)
    e = _check("dw", dw.double() - 0.5, ref, tol, tol * ref.abs().max().item())
    print(f"full-size stage-5 `{which}` weight gradient {dtype}: err {e:.2e} of max (limit {tol:.0e})")


@pytest.mark.parametrize("dtype", HALF)
def test_depthwise_56_backward_full_size(gpu, dtype):
    """x3d_dw3d_bwd of the stage-2 stride-1 layers at batch 64: 54 channels of 16 x 56 x 56 (3.2 M points per channel and
    weight tap), fused data + weight gradient with the BN_b / SE backward on load and the ReLU mask + BN_a sums in the
    epilogue, against the fp64 stencil (shifted slices)."""
    from x3d_tf_amd import hip, ops
    from tests import shapes as S
    n, c, t, h, w = 64, 54, 16, 56, 56
    g_ = torch.Generator(device=gpu)
    g_.manual_seed(47)
    rn = lambda *s: torch.randn(*s, generator=g_, device=gpu, dtype=torch.float32)
    araw = rn(n, c, t, h, w).to(dtype)
    dv = rn(n, c, t, h, w).to(dtype)
    braw = rn(n, c, t, h, w).to(dtype)
    coef = rn(n, c, 4) * 0.5
    wt = rn(c, 3, 3, 3) * 0.3
    ss = torch.stack([1 + 0.3 * rn(c), 0.3 * rn(c)], 1)
    ga = torch.empty((n, c, t, h, w), dtype=dtype, device=gpu)
    a_sums = torch.zeros((c, 2), dtype=torch.float64, device=gpu)
    dw = torch.full((c, 27), 0.25, dtype=torch.float32, device=gpu)
    ops.dw3d_bwd(dv, braw, coef, araw, ss, wt.view(c, 27), ga, a_sums, dw, 1)
    torch.cuda.synchronize()
    mx = "_mx" in hip.kernel_name(S.dw_bwd_struct((n, c, t, h, w, 1), dtype))
    wd = round_to(wt.cpu(), dtype).to(gpu) if mx else wt.double()
    dw_ref = torch.zeros((c, 3, 3, 3), dtype=torch.float64, device=gpu)
    worst, CH = 0.0, 8
    s1 = torch.zeros(c, dtype=torch.float64, device=gpu)
    s2 = torch.zeros(c, dtype=torch.float64, device=gpu)
    rt, at = tol_gemm(dtype) if mx else tol_store(dtype)
    for i in range(0, n, CH):
        cd = coef[i:i + CH].double()
        dB = cd[:, :, 0, None, None, None] * dv[i:i + CH].double() + cd[:, :, 1, None, None, None] * braw[i:i + CH].double() + cd[:, :, 2, None, None, None]
        z = araw[i:i + CH].double() * ss[:, 0].double().view(1, -1, 1, 1, 1) + ss[:, 1].double().view(1, -1, 1, 1, 1)
        act = torch.relu(z)
        if mx:
            dB = dB.float().to(dtype).double()
            act = act.float().to(dtype).double()
        pa = torch.nn.functional.pad(act, (1, 1, 1, 1, 1, 1))
        pb = torch.nn.functional.pad(dB, (1, 1, 1, 1, 1, 1))
        dA = torch.zeros_like(act)
        for kt in range(3):
            for kh in range(3):
                for kw in range(3):
                    # out[p] = sum_k w[k] a[p + k - 1]  =>  dA[q] = sum_k w[k] dB[q - k + 1],  dW[k] = sum_p dB[p] a[p + k - 1]
                    dA += wd[:, kt, kh, kw].view(1, -1, 1, 1, 1) * pb[:, :, 2 - kt:2 - kt + t, 2 - kh:2 - kh + h, 2 - kw:2 - kw + w]
                    dw_ref[:, kt, kh, kw] += (dB * pa[:, :, kt:kt + t, kh:kh + h, kw:kw + w]).sum((0, 2, 3, 4))
        ref = dA * (z > 0)
        worst = max(worst, _check(f"ga[{i}:{i + CH}]", ga[i:i + CH], ref, rt, at * ref.abs().max().item()))
        gs = ga[i:i + CH].double()
        s1 += gs.sum((0, 2, 3, 4))
        s2 += (gs * araw[i:i + CH].double()).sum((0, 2, 3, 4))
        del dB, z, act, pa, pb, dA, ref, gs
    wtol = _wtol(dtype) if mx else 2e-5        # (vector kernel, fp32 products: measured 5.6e-7 of the maximum)
    e = _check("dw", dw.double().view(c, 3, 3, 3) - 0.25, dw_ref, wtol, wtol * dw_ref.abs().max().item())
    st = 3e-3 if dtype == torch.bfloat16 else 5e-4
    sref = torch.stack([s1, s2], 1)
    _check("a_sums", a_sums, sref, 10 * st, 10 * st * max(1.0, sref.abs().max().item()))
    print(f"full-size 56^2 depthwise backward {dtype} ({'matrix-core' if mx else 'vector'} kernel): ga err {worst:.2e} of max, dW err {e:.2e} of max (limit {wtol:.0e})")


@pytest.mark.parametrize("dtype", HALF)
def test_depthwise_112_stride2_backward_full_size(gpu, dtype):
    """x3d_dw3d_bwd of the first block's stride-2 layer at batch 64: 54 channels of 16 x 112 x 112 -> 56 x 56 (the launch with the
    largest total of the train step; dw3d_bwd_s2r_kernel for 16-bit storage), against the fp64 stencil written as strided slices
    (TF-SAME for an even extent at stride 2: no pad in front, one behind)."""
    from x3d_tf_amd import hip, ops
    from tests import shapes as S
    n, c, t, h, w = 64, 54, 16, 112, 112
    ho, wo = h // 2, w // 2
    g_ = torch.Generator(device=gpu)
    g_.manual_seed(53)
    rn = lambda *s: torch.randn(*s, generator=g_, device=gpu, dtype=torch.float32)
    araw = rn(n, c, t, h, w).to(dtype)
    dv = rn(n, c, t, ho, wo).to(dtype)
    braw = rn(n, c, t, ho, wo).to(dtype)
    coef = rn(n, c, 4) * 0.5
    wt = rn(c, 3, 3, 3) * 0.3
    ss = torch.stack([1 + 0.3 * rn(c), 0.3 * rn(c)], 1)
    ga = torch.empty((n, c, t, h, w), dtype=dtype, device=gpu)
    a_sums = torch.zeros((c, 2), dtype=torch.float64, device=gpu)
    dw = torch.full((c, 27), 0.25, dtype=torch.float32, device=gpu)
    ops.dw3d_bwd(dv, braw, coef, araw, ss, wt.view(c, 27), ga, a_sums, dw, 2)
    torch.cuda.synchronize()
    name = hip.kernel_name(S.dw_bwd_struct((n, c, t, h, w, 2), dtype))
    assert "s2r" in name, name
    wd = wt.double()
    dw_ref = torch.zeros((c, 3, 3, 3), dtype=torch.float64, device=gpu)
    worst, CH = 0.0, 4
    s1 = torch.zeros(c, dtype=torch.float64, device=gpu)
    s2 = torch.zeros(c, dtype=torch.float64, device=gpu)
    rt, at = tol_store(dtype)
    for i in range(0, n, CH):
        cd = coef[i:i + CH].double()
        dB = cd[:, :, 0, None, None, None] * dv[i:i + CH].double() + cd[:, :, 1, None, None, None] * braw[i:i + CH].double() + cd[:, :, 2, None, None, None]
        z = araw[i:i + CH].double() * ss[:, 0].double().view(1, -1, 1, 1, 1) + ss[:, 1].double().view(1, -1, 1, 1, 1)
        pa = torch.nn.functional.pad(torch.relu(z), (0, 1, 0, 1, 1, 1))
        dAp = torch.zeros_like(pa)
        for kt in range(3):
            for kh in range(3):
                for kw in range(3):
                    # out[t, ho, wo] = sum_k w[k] a[t + kt - 1, 2 ho + kh, 2 wo + kw]
                    sl = (slice(None), slice(None), slice(kt, kt + t), slice(kh, kh + 2 * ho, 2), slice(kw, kw + 2 * wo, 2))
                    dAp[sl] += wd[:, kt, kh, kw].view(1, -1, 1, 1, 1) * dB
                    dw_ref[:, kt, kh, kw] += (dB * pa[sl]).sum((0, 2, 3, 4))
        ref = dAp[:, :, 1:1 + t, :h, :w] * (z > 0)
        worst = max(worst, _check(f"ga[{i}:{i + CH}]", ga[i:i + CH], ref, rt, at * ref.abs().max().item()))
        gs = ga[i:i + CH].double()
        s1 += gs.sum((0, 2, 3, 4))
        s2 += (gs * araw[i:i + CH].double()).sum((0, 2, 3, 4))
        del dB, z, pa, dAp, ref, gs
    e = _check("dw", dw.double().view(c, 3, 3, 3) - 0.25, dw_ref, 2e-5, 2e-5 * dw_ref.abs().max().item())
    st = 3e-3 if dtype == torch.bfloat16 else 5e-4
    sref = torch.stack([s1, s2], 1)
    _check("a_sums", a_sums, sref, 10 * st, 10 * st * max(1.0, sref.abs().max().item()))
    print(f"full-size 112^2 -> 56^2 depthwise backward {dtype} ({name}): ga err {worst:.2e} of max, dW err {e:.2e} of max (limit 2e-05)")


# ---- the stem: conv_s (1 x 3 x 3, stride 2, 3 -> C1 channels) then conv_t (KT x 1 x 1 depthwise), reference model.py:202-206 ----
# Shapes and channel counts come from the named variant's config; the clip counts are BASELINE's (configs 2 - 5).
STEM_MU = (0.5, 0.4, 0.3)        # per-channel means of the normalised clip: every RGB channel of a real one has one


def _stol(dtype):
    return 1e-5 if dtype == torch.float32 else (3e-3 if dtype == torch.bfloat16 else 5e-4)     # as tests/test_kernels_gpu.py::_stol


def _stem_inputs(gpu, variant, n, dtype, seed):
    """(x [n, T, S, S, 3] channels-last in `dtype`, w_s [C1, 3, 3, 3], w_t [C1, KT], generator): x = randn * 0.5 + mu_c."""
    import x3d_tf_amd as x3d
    cfg = x3d.get_config(variant)
    arch = x3d.build_arch(cfg)
    c1, kt, t, s = arch.c1, arch.c1_temp_filter, cfg.DATA.TEMP_DURATION, cfg.DATA.TRAIN_CROP_SIZE
    g_ = torch.Generator(device=gpu)
    g_.manual_seed(seed)
    rn = lambda *sh: torch.randn(*sh, generator=g_, device=gpu, dtype=torch.float32)
    x = (rn(n, t, s, s, 3) * 0.5 + torch.tensor(STEM_MU, device=gpu)).to(dtype)
    return x, rn(c1, 3, 3, 3) * 0.3, rn(c1, kt) * 0.4, rn


def _im2col_taps(xc):
    """The nine (kh, kw) taps of conv_s over a channels-last fp64 chunk [n, T, H, W, 3]: tap[..., ho, wo, ci] =
    x[..., 2 ho + kh - 1, 2 wo + kw - 1, ci], zero outside the image."""
    n, t, h, w, _ = xc.shape
    ho, wo = (h - 1) // 2 + 1, (w - 1) // 2 + 1
    xp = torch.nn.functional.pad(xc, (0, 0, 1, 2 * wo - w, 1, 2 * ho - h))
    return [((kh, kw), xp[:, :, kh:kh + 2 * ho:2, kw:kw + 2 * wo:2, :]) for kh in range(3) for kw in range(3)]


def _conv_s64(taps, ws):
    return sum(torch.einsum("oc,nthwc->nothw", ws[:, :, kh, kw], tap) for (kh, kw), tap in taps)


def _conv_t64(s, wt):
    """out[t] = sum_k w[c, k] s[t + k - KT // 2], zero outside [0, T)."""
    kt, t = wt.shape[1], s.shape[2]
    sp = torch.nn.functional.pad(s, (0, 0, 0, 0, kt // 2, kt // 2))
    out = torch.zeros_like(s)
    for k in range(kt):
        out += wt[:, k].view(1, -1, 1, 1, 1) * sp[:, :, k:k + t]
    return out


def _check_slack(name, got, ref, rtol, atol, slack):
    """_check with a per-element tie slack on top of atol + rtol |ref|: returns (worst err / its limit, elements that needed
    the slack)."""
    got, ref = got.double(), ref.double()
    err = (got - ref).abs()
    base = atol + rtol * ref.abs()
    lim = base + slack
    bad = err > lim
    assert torch.isfinite(got).all(), f"{name}: non-finite values"
    assert not bad.any(), (f"{name}: {int(bad.sum())}/{bad.numel()} out of tolerance (rtol {rtol}, atol {atol:.3e} + tie slack); "
                           f"max err {err.max().item():.3e}, max |ref| {ref.abs().max().item():.3e}")
    return (err / lim).max().item(), int((err > base).sum())


STEM_FWD = [("M", 64, torch.bfloat16), ("M", 64, torch.float16),    # config 3: Wo = 112 = 64 + 48 columns
            ("L", 16, torch.bfloat16),                               # config 4: Wo = 156, the third segment 28 of 64 columns
            ("XL", 30, torch.float16)]                               # config 5 (30 views of one video): 32 channels, inference


@pytest.mark.parametrize("variant,n,dtype", STEM_FWD, ids=[f"{v}-{str(d)[6:]}" for v, _, d in STEM_FWD])
def test_stem_fused_forward_full_size(gpu, variant, n, dtype):
    """x3d_stem_fwd at full size against fp64: t_raw = conv_t(s) with s = conv_s over the weights rounded to storage, then
    rounded to storage as the kernel does on chip (tol_store plus the conv_t tie slack, tests.util.tie_slack_t; fewer than
    1e-4 of the elements may need that slack); the BatchNorm sums (replicated fp64 atomics) against an fp64 reduction of
    the stored t_raw; for X3D-XL the inference epilogue act(s * conv + b) as well, act in {none, ReLU}.  (Measured: worst
    err / limit 0.61 - 0.99, the store's half ulp against tol_store's rtol; 3e-8 - 7e-7 of the outputs needed the slack;
    the sums 1.1e-8 - 1.6e-8 of their maximum.)"""
    from x3d_tf_amd import ops
    x, ws, wt, rn = _stem_inputs(gpu, variant, n, dtype, 61)
    c1 = ws.shape[0]
    infer = c1 > 24
    assert ops.stem_fused_supported(x, c1) == (1 if infer else 3)       # (forward only with 32 channels)
    st = torch.zeros((c1, 2), dtype=torch.float64, device=gpu)
    y = ops.stem_fwd(x, ws, wt, stats=st)
    outs = [("t_raw", y, None)]
    if infer:
        oss = torch.stack([1 + 0.3 * rn(c1), 0.3 * rn(c1)], 1)
        outs += [(f"inference epilogue act {act}", ops.stem_fwd(x, ws, wt, out_ss=oss, out_act=act), act) for act in (0, 1)]
    torch.cuda.synchronize()
    wsr, wt64, wabs = round_to(ws, dtype), wt.double(), wt.abs()
    rt, at = tol_store(dtype)
    worst = {name: 0.0 for name, _, _ in outs}
    needed = 0
    s1 = torch.zeros(c1, dtype=torch.float64, device=gpu)
    s2 = torch.zeros(c1, dtype=torch.float64, device=gpu)
    CH = 8
    for i in range(0, n, CH):
        s64 = _conv_s64(_im2col_taps(x[i:i + CH].double()), wsr)
        slack = tie_slack_t(s64, dtype, wabs)
        tref = _conv_t64(round_to(s64, dtype), wt64)
        del s64
        for name, got, act in outs:
            ref, sl = tref, slack
            if act is not None:
                ref = oss[:, 0].double().view(1, -1, 1, 1, 1) * tref + oss[:, 1].double().view(1, -1, 1, 1, 1)
                ref = torch.relu(ref) if act == 1 else ref
                sl = slack * oss[:, 0].double().abs().view(1, -1, 1, 1, 1)
            e, nd = _check_slack(f"{name}[{i}:{i + CH}]", got[i:i + CH], ref, rt, at * ref.abs().max().item(), sl)
            worst[name] = max(worst[name], e)
            needed += nd
            del ref, sl
        yd = y[i:i + CH].double()
        s1 += yd.sum((0, 2, 3, 4))
        s2 += (yd * yd).sum((0, 2, 3, 4))
        del slack, tref, yd
    frac = needed / (y.numel() * len(outs))
    assert frac < 1e-4, f"{frac:.2e} of the outputs needed the tie slack: a systematic error, not ties"
    sref = torch.stack([s1, s2], 1)
    stol = _stol(dtype)
    e_st = _check("stats", st, sref, stol, stol * max(1.0, sref.abs().max().item()))
    print(f"full-size stem forward X3D-{variant} {dtype} {tuple(y.shape)}: worst err / limit "
          + ", ".join(f"{k} {v:.2e}" for k, v in worst.items()) + f"; {frac:.1e} needed the tie slack; stats err {e_st:.2e} of max "
          f"(limit {stol:.0e})")


def _stem_backward_case(gpu, variant, n, dtype, seed, fused):
    """Shared body of the full-size stem backward tests.  A training step's inputs: the stored t_raw of the forward pass, a
    random upstream gradient g (unmasked: the ReLU behind conv1/bn is applied inside the kernels), relu_ss from the actual
    BatchNorm of t_raw (random gamma / beta), and coef derived from the masked g and t_raw (sum dY = 0 per channel, so both
    weight gradients lose the mean part of s and x to cancellation).  Runs x3d_stem_bwd when `fused`, and always the
    two-kernel plan (x3d_dwt_bwd, then x3d_stem_s_wgrad on the conv_t input gradient ds); returns the launches' results with
    the fp64 definitions: dW_t[c, k] = sum dY[t + 2 - k] s[t], ds = conv_t^T dY, dW_s = sum round_to(ds) im2col(x); for fp32
    also sum |terms| of both (what an fp32 summation bound scales with)."""
    from x3d_tf_amd import ops
    x, ws, wt, rn = _stem_inputs(gpu, variant, n, dtype, seed)
    c1 = ws.shape[0]
    cl = dtype != torch.float32             # fp32 storage: the planar batch and the scalar kernels (config 2's plan)
    xk = x if cl else x.permute(0, 4, 1, 2, 3).contiguous()
    if cl:
        assert ops.stem_fused_supported(x, c1) == (3 if fused else 1)
        assert x.shape[3] % 8 == 0       # x3d_stem_s_wgrad takes stem_s_wgrad_bf16_kernel (16-bit, W % 8 == 0)
    s = ops.stem_s_fwd(xk, ws, channels_last=cl)
    t_raw = ops.dwt_fwd(s, wt)
    torch.cuda.synchronize()
    CH = 8
    m = t_raw.numel() // c1
    s1 = torch.zeros(c1, dtype=torch.float64, device=gpu)
    s2 = torch.zeros(c1, dtype=torch.float64, device=gpu)
    for i in range(0, n, CH):
        yd = t_raw[i:i + CH].double()
        s1 += yd.sum((0, 2, 3, 4))
        s2 += (yd * yd).sum((0, 2, 3, 4))
        del yd
    gamma = (1 + 0.3 * rn(c1)).double()
    beta = (0.3 * rn(c1)).double()
    mean = s1 / m
    k1 = gamma / torch.sqrt(s2 / m - mean * mean + 1e-5)
    rss = torch.stack([k1, beta - mean * k1], 1).float()
    g = rn(*t_raw.shape).to(dtype)
    v = lambda a: a.double().view(1, -1, 1, 1, 1)
    mask = lambda i: (v(rss[:, 0]) * t_raw[i:i + CH].double() + v(rss[:, 1])) > 0       # (exact sign, as the kernels' fma)
    sg = torch.zeros(c1, dtype=torch.float64, device=gpu)
    sgy = torch.zeros(c1, dtype=torch.float64, device=gpu)
    for i in range(0, n, CH):
        gm = g[i:i + CH].double() * mask(i)
        sg += gm.sum((0, 2, 3, 4))
        sgy += (gm * t_raw[i:i + CH].double()).sum((0, 2, 3, 4))
        del gm
    coef = _bn_bwd_coef_sums(m, s1, s2, sg, sgy, gamma)
    res = {}
    if fused:
        dwt = torch.full((c1, wt.shape[1]), 0.5, dtype=torch.float32, device=gpu)      # += on what is there
        dws = torch.full((c1, 3, 3, 3), -0.25, dtype=torch.float32, device=gpu)
        ops.stem_bwd(g, t_raw, coef, x, ws, wt, dws, dwt, relu_ss=rss)
        res["fused"] = (dwt, 0.5, dws, -0.25)
    ds = torch.empty_like(s)
    dwt2 = torch.full((c1, wt.shape[1]), 0.5, dtype=torch.float32, device=gpu)
    dws2 = torch.full((c1, 3, 3, 3), -0.25, dtype=torch.float32, device=gpu)
    ops.dwt_bwd(g, t_raw, coef, s, wt, ds, dwt2, relu_ss=rss)
    ops.stem_s_wgrad(xk, ds, dws2, channels_last=cl)
    res["two-kernel"] = (dwt2, 0.5, dws2, -0.25)
    torch.cuda.synchronize()
    # ---- fp64 definitions, chunked
    wsr, wt64, cf = round_to(ws, dtype), wt.double(), coef.double()
    kt, t = wt.shape[1], t_raw.shape[2]
    dwt_ref = torch.zeros((c1, kt), dtype=torch.float64, device=gpu)
    dws_ref = torch.zeros((c1, 3, 3, 3), dtype=torch.float64, device=gpu)
    abs_t = torch.zeros_like(dwt_ref)
    abs_s = torch.zeros_like(dws_ref)
    rt, at = tol_store(dtype)
    e_ds = 0.0
    for i in range(0, n, CH):
        taps = _im2col_taps(x[i:i + CH].double())
        sp = torch.nn.functional.pad(round_to(_conv_s64(taps, wsr), dtype), (0, 0, 0, 0, kt // 2, kt // 2))
        yd = t_raw[i:i + CH].double()
        gm = g[i:i + CH].double() * mask(i)
        dy = v(cf[:, 0]) * gm + v(cf[:, 1]) * yd + v(cf[:, 2])
        dyp = torch.nn.functional.pad(dy, (0, 0, 0, 0, kt // 2, kt // 2))
        dsr = torch.zeros_like(dy)
        for k in range(kt):
            dwt_ref[:, k] += (dy * sp[:, :, k:k + t]).sum((0, 2, 3, 4))
            dsr += v(wt64[:, k]) * dyp[:, :, kt - 1 - k:kt - 1 - k + t]          # ds[t] = sum_k w[k] dY[t + 2 - k]
        e_ds = max(e_ds, _check(f"ds[{i}:{i + CH}]", ds[i:i + CH], dsr, rt, at * dsr.abs().max().item()))
        dsr = round_to(dsr, dtype)
        for (kh, kw), tap in taps:
            dws_ref[:, :, kh, kw] += torch.einsum("nothw,nthwc->oc", dsr, tap)
        if dtype == torch.float32:       # |terms|, with |dY| bounded by |A g| + |B y| + |C| (its own fp32 rounding scales with those)
            mag = v(cf[:, 0].abs()) * gm.abs() + v(cf[:, 1].abs()) * yd.abs() + v(cf[:, 2].abs())
            magp = torch.nn.functional.pad(mag, (0, 0, 0, 0, kt // 2, kt // 2))
            mds = torch.zeros_like(mag)
            for k in range(kt):
                abs_t[:, k] += (mag * sp[:, :, k:k + t].abs()).sum((0, 2, 3, 4))
                mds += v(wt64[:, k].abs()) * magp[:, :, kt - 1 - k:kt - 1 - k + t]
            for (kh, kw), tap in taps:
                abs_s[:, :, kh, kw] += torch.einsum("nothw,nthwc->oc", mds, tap.abs())
            del mag, magp, mds
        del taps, sp, yd, gm, dy, dyp, dsr
    return res, dwt_ref, dws_ref, abs_t, abs_s, e_ds, tuple(x.shape)


@pytest.mark.parametrize("dtype", HALF)
def test_stem_backward_full_size(gpu, dtype):
    """Config 3's stem backward at full size (X3D-M, 64 x 16 x 224^2: 14 336 row segments, 12.8 M points per channel):
    x3d_stem_bwd, and the two-kernel plan of X3D_NO_STEM_FUSED (x3d_dwt_bwd + the 16-bit stem_s_wgrad_bf16_kernel),
    against the fp64 definitions (_stem_backward_case) at _wtol (1e-3 / 4e-4 of the maximum), accumulators pre-filled;
    the two-kernel plan's ds against fp64 at tol_store.  (Measured: 1.3e-2 - 1.5e-2 of the limit for bf16, 4.0e-2 - 5.4e-2
    for fp16, both plans.)"""
    res, dwt_ref, dws_ref, _, _, e_ds, shape = _stem_backward_case(gpu, "M", 64, dtype, 67, fused=True)
    tol = _wtol(dtype)
    msg = []
    for name, (dwt, ft, dws, fs) in res.items():
        e_t = _check(f"{name} dW_t", dwt.double() - ft, dwt_ref, tol, tol * dwt_ref.abs().max().item())
        e_s = _check(f"{name} dW_s", dws.double() - fs, dws_ref, tol, tol * dws_ref.abs().max().item())
        msg.append(f"{name}: dW_t {e_t / tol:.2e}, dW_s {e_s / tol:.2e}")
    print(f"full-size stem backward X3D-M {dtype} {shape}: worst err / limit " + "; ".join(msg) + f"; ds err {e_ds:.2e} of max")


def test_stem_two_kernel_backward_xl_full_rows(gpu):
    """The stem backward X3D-XL training runs (x3d_stem_fused_supported refuses its 32 channels for the backward pass):
    x3d_dwt_bwd + stem_s_wgrad_bf16_kernel on full 312^2 rows of 16 frames, fp16, a reduced batch of 4 clips; fp64
    definitions at _wtol.  (Measured: dW_t 3.8e-2, dW_s 2.7e-2 of the limit.)"""
    res, dwt_ref, dws_ref, _, _, e_ds, shape = _stem_backward_case(gpu, "XL", 4, torch.float16, 71, fused=False)
    tol = _wtol(torch.float16)
    dwt, ft, dws, fs = res["two-kernel"]
    e_t = _check("dW_t", dwt.double() - ft, dwt_ref, tol, tol * dwt_ref.abs().max().item())
    e_s = _check("dW_s", dws.double() - fs, dws_ref, tol, tol * dws_ref.abs().max().item())
    print(f"full-row stem backward X3D-XL fp16 {shape}: worst err / limit dW_t {e_t / tol:.2e}, dW_s {e_s / tol:.2e}; ds err {e_ds:.2e} of max")


def test_stem_fp32_full_size(gpu):
    """Config 2's stem at full size (X3D-S, 32 x 13 x 160^2, fp32 storage, planar batch: two kernels each way, the only
    full-size case of stem_s_wgrad_rows_kernel).  Forward: s_raw and t_raw against fp64 at tol_store(float32), the
    BatchNorm sums at _stol.  Backward (_stem_backward_case): ds at tol_store(float32); the two weight gradients against an
    fp32 summation bound.  A sum of L fp32 roundings over terms a_i is off by at most lambda sqrt(L) u sum |a_i| with
    probability >= 1 - 2 exp(-lambda^2 / 2) when the rounding errors are independent (Higham & Mary, SIAM J. Sci. Comput.
    41 (2019), the probabilistic form of gamma_L); u = 2^-24, lambda = 6 (1.5e-8 per element).  L is the longest chain a
    term passes through in the launch:
      dW_t (x3d_dwt_bwd, <= 2 points per thread): 2 T products per thread, <= 8 levels of the workgroup sum, one atomic per
           workgroup of the channel (N ceil(HW / 256)), and the 3 roundings of dY = A g + B y + C;
      dW_s (stem_s_wgrad_rows_kernel): 16 points per wave and segment over the workgroup's spb segments, 3 adds across the
           four waves, one atomic per workgroup (gx), and the 8 roundings of ds (dY, then 5 taps);
    spb / gx as the launcher sets them (ceil(segments / (3 CUs)), at least 8).  |a_i| uses |A g| + |B y| + |C| for |dY|.
    (Measured on 256 CUs: dW_t 2.4e-3 and dW_s 5.6e-4 of these limits, which are 6e-3 and 1.1e-2 of the maxima.)"""
    import math
    from x3d_tf_amd import ops
    n, dtype = 32, torch.float32
    x, ws, wt, _ = _stem_inputs(gpu, "S", n, dtype, 73)
    c1 = ws.shape[0]
    xp = x.permute(0, 4, 1, 2, 3).contiguous()
    s = ops.stem_s_fwd(xp, ws)
    st = torch.zeros((c1, 2), dtype=torch.float64, device=gpu)
    y = ops.dwt_fwd(s, wt, stats=st)
    torch.cuda.synchronize()
    rt, at = tol_store(dtype)
    e_s = e_y = 0.0
    s1 = torch.zeros(c1, dtype=torch.float64, device=gpu)
    s2 = torch.zeros(c1, dtype=torch.float64, device=gpu)
    CH = 8
    for i in range(0, n, CH):
        s64 = _conv_s64(_im2col_taps(x[i:i + CH].double()), ws.double())
        e_s = max(e_s, _check(f"s_raw[{i}:{i + CH}]", s[i:i + CH], s64, rt, at * s64.abs().max().item()))
        t64 = _conv_t64(s64, wt.double())
        e_y = max(e_y, _check(f"t_raw[{i}:{i + CH}]", y[i:i + CH], t64, rt, at * t64.abs().max().item()))
        yd = y[i:i + CH].double()
        s1 += yd.sum((0, 2, 3, 4))
        s2 += (yd * yd).sum((0, 2, 3, 4))
        del s64, t64, yd
    sref = torch.stack([s1, s2], 1)
    e_st = _check("stats", st, sref, _stol(dtype), _stol(dtype) * max(1.0, sref.abs().max().item()))
    res, dwt_ref, dws_ref, abs_t, abs_s, e_ds, shape = _stem_backward_case(gpu, "S", n, dtype, 73, fused=False)
    _, t, h, w, _ = shape
    ho, wo = (h - 1) // 2 + 1, (w - 1) // 2 + 1
    segs = n * t * ho * -(-wo // 64)
    spb = max(8, -(-segs // (3 * torch.cuda.get_device_properties(gpu).multi_processor_count)))
    l_t = 2 * t + 8 + n * -(-(ho * wo) // 256) + 3
    l_s = 16 * spb + 3 + -(-segs // spb) + 8
    lam, u = 6.0, 2.0 ** -24
    dwt, ft, dws, fs = res["two-kernel"]
    got_t, got_s = dwt.double() - ft, dws.double() - fs
    lim_t = lam * math.sqrt(l_t) * u * abs_t + 2 * u * abs(ft)           # (+ the rounding of the pre-filled accumulator)
    lim_s = lam * math.sqrt(l_s) * u * abs_s + 2 * u * abs(fs)
    e_t, _ = _check_slack("dW_t", got_t, dwt_ref, 0.0, 0.0, lim_t)
    e_w, _ = _check_slack("dW_s", got_s, dws_ref, 0.0, 0.0, lim_s)
    print(f"full-size stem X3D-S fp32 {shape}: s_raw err {e_s:.2e}, t_raw err {e_y:.2e} of max (limit {at:.0e}), stats "
          f"{e_st:.2e}, ds {e_ds:.2e}; dW_t err / limit {e_t:.2e} (L {l_t}, limit {(lim_t / dwt_ref.abs().max()).max().item():.1e} "
          f"of max), dW_s err / limit {e_w:.2e} (L {l_s}, limit {(lim_s / dws_ref.abs().max()).max().item():.1e} of max)")


# ---- every depthwise launch of the full-size plans (tests/shapes.py DW_FULL: BASELINE configs 2 - 5, config 3 in fp16 too) ----

def _dw_chunk(case):
    """Samples per fp64 chunk: about 48 M input elements (0.4 GB in fp64) at a time."""
    _, _, n, c, t, h, w = case[:7]
    return max(1, min(n, 48_000_000 // (c * t * h * w)))


def _dw_fp32_chain(name, n, t, h, w, stride):
    """L, the longest chain of fp32 roundings a product of the fp32 weight gradient passes through in the vector kernels of
    config 2 (one thread owns a strip of SW outputs of one row: T SW products per tap; the wave's DPP tree, 6 levels; the
    sum over the workgroup's waves; one atomic per workgroup of the channel; the 4 roundings of dB = A dv + B b + C and of
    the prologue).  dw3d_bwd_kernel / dw3d_bwd_pd_kernel: dw_geom's partition (workgroups of 64 / 128 / 256 threads, one
    per (n, c, H-tile)); dw3d_bwd_pk_kernel: one plane per strip set, at most 8 waves and N workgroups per channel."""
    args = name[name.index("<") + 1:-1].split(", ")
    ho, wo = -(-h // stride), -(-w // stride)
    if name.startswith("dw3d_bwd_pk_kernel<"):
        sw, waves, atomics = int(args[1]), 8, n
    elif name.startswith(("dw3d_bwd_kernel<", "dw3d_bwd_pd_kernel<")):
        sw = int(args[2])
        nstrips = -(-wo // sw)
        items = ho * nstrips
        bd = 64 if items <= 64 else (128 if items <= 128 else 256)
        th = min(bd // nstrips, ho)
        waves, atomics = bd // 64, n * -(-ho // th)
    else:
        raise AssertionError(f"no fp32 summation bound for {name}")
    return t * sw + 6 + waves + atomics + 4


def _dw_inputs(gpu, case, seed):
    """a_raw (the `a` conv's raw output, [N, C, T, H, W] in the storage type) with non-zero channel means, the depthwise
    weights, and BN_a over the whole batch as the prologue sees it: (gamma, beta, fp64 sums of a_raw, scale / shift)."""
    _, dtype, n, c, t, h, w = case[:7]
    g_ = torch.Generator(device=gpu)
    g_.manual_seed(seed)
    rn = lambda *s: torch.randn(*s, generator=g_, device=gpu, dtype=torch.float32)
    mu, sd = 1.0 + rn(c), 0.5 + rn(c).abs()
    araw = torch.empty((n, c, t, h, w), dtype=dtype, device=gpu)
    for i in range(n):
        araw[i] = (rn(c, t, h, w) * sd.view(-1, 1, 1, 1) + mu.view(-1, 1, 1, 1)).to(dtype)
    wt = rn(c, 3, 3, 3) * 0.3
    gamma, beta = 1 + 0.3 * rn(c), 0.3 * rn(c)
    s1 = torch.zeros(c, dtype=torch.float64, device=gpu)
    s2 = torch.zeros(c, dtype=torch.float64, device=gpu)
    for i in range(n):
        ad = araw[i].double()
        s1 += ad.sum((1, 2, 3))
        s2 += (ad * ad).sum((1, 2, 3))
    m = n * t * h * w
    mean = s1 / m
    k = gamma.double() / torch.sqrt(s2 / m - mean * mean + 1e-5)
    ss = torch.stack([k, beta.double() - mean * k], 1).float()
    return araw, wt, gamma, beta, torch.stack([s1, s2], 1), ss, rn, g_


def _dw_forward_case(gpu, case, seed):
    """x3d_dw3d_fwd in the plan's form: y against the fp64 stencil of act = relu(s a_raw + t) at tol_store, or -- matrix-core
    kernels, which round act and the weights to the storage type -- over those rounded operands at tol_gemm plus a tie slack:
    where act sits within 2e-4 ulps of a rounding midpoint the kernel's fp32 prologue may round it to the other neighbour, so
    every output reading it may move by ulp |w| per such tap (at most 1e-4 of the outputs may need that); stats and pool
    against fp64 sums of the stored y at _stol."""
    from x3d_tf_amd import hip, ops
    from tests import shapes as S
    from tests.util import _tie_ulps, dw_stencil64
    _, dtype, n, c, t, h, w, stride, pro, want_stats, want_pool = case
    araw, wt, gamma, beta, sums, ss, _, _ = _dw_inputs(gpu, case, seed)
    stats = torch.zeros((c, 2), dtype=torch.float64, device=gpu) if want_stats else None
    pool = torch.zeros((n, c), dtype=torch.float64, device=gpu) if want_pool else None
    fold = None
    if pro == "bn":        # the prologue's finalize inside the launch: it writes the scale / shift the reference then reads
        ss = torch.zeros((c, 2), dtype=torch.float32, device=gpu)
        fold = ops.bn_fold(sums, n * t * h * w, gamma, beta, torch.zeros(c, device=gpu), torch.ones(c, device=gpu), 1e-5, 0.9,
                           1, ss, torch.zeros((c, 2), device=gpu))
    y = ops.dw3d_fwd(araw, wt, stride, in_ss=ss if fold is None else None, in_act=1, stats=stats, pool=pool, in_bn=fold)
    torch.cuda.synchronize()
    name = hip.kernel_name(S.dw_full_struct(case))
    mx = "_mx" in name
    rt, at = tol_gemm(dtype) if mx else tol_store(dtype)
    wd = round_to(wt, dtype) if mx else wt.double()
    sc, sh = ss[:, 0].double().view(1, -1, 1, 1, 1), ss[:, 1].double().view(1, -1, 1, 1, 1)
    worst, needed, CH = 0.0, 0, _dw_chunk(case)
    y1 = torch.zeros(c, dtype=torch.float64, device=gpu)
    y2 = torch.zeros(c, dtype=torch.float64, device=gpu)
    pref = torch.zeros((n, c), dtype=torch.float64, device=gpu)
    for i in range(0, n, CH):
        act = torch.relu(araw[i:i + CH].double() * sc + sh)
        slack = 0.0
        if mx:
            slack = dw_stencil64(_tie_ulps(act, dtype, 2e-4), wd.abs(), stride)
            act = round_to(act, dtype)
        ref = dw_stencil64(act, wd, stride)
        del act
        e, nd = _check_slack(f"y[{i}:{i + CH}]", y[i:i + CH], ref, rt, at * ref.abs().max().item(), slack)
        worst, needed = max(worst, e), needed + nd
        del ref, slack
        yd = y[i:i + CH].double()
        y1 += yd.sum((0, 2, 3, 4))
        y2 += (yd * yd).sum((0, 2, 3, 4))
        pref[i:i + CH] = yd.sum((2, 3, 4))
        del yd
    frac = needed / y.numel()
    assert frac < 1e-4, f"{frac:.2e} of the outputs needed the tie slack: a systematic error, not ties"
    stol = _stol(dtype)
    msg = f"y {worst:.2e}"
    if want_stats:
        sref = torch.stack([y1, y2], 1)
        msg += f", stats {_frac('stats', stats, sref, stol, stol * max(1.0, sref.abs().max().item())):.2e}"
    if want_pool:
        msg += f", pool {_frac('pool', pool, pref, stol, stol * max(1.0, pref.abs().max().item())):.2e}"
    return name, msg + (f" ({frac:.1e} needed the tie slack)" if mx else "")


def _dw_backward_case(gpu, case, seed):
    """x3d_dw3d_bwd with the coefficients of a real step: dB = A[n, c] dv + B[c] b_raw + C[c], A = k1[c] times a positive
    per-sample SE gate, and B, C solved so that sum dB = 0 and sum dB b_raw = 0 per channel over the whole batch (what BN_b's
    backward guarantees).  dW = sum dB shift(relu(z)) then cancels the positive mean of the post-ReLU activation at the real
    reduction length.  ga against the fp64 stencil (tol_gemm on matrix-core kernels, over operands rounded as they round them;
    tol_store on vector kernels), a_sums at 10 _stol, dW (accumulator pre-filled with 0.25) at _wtol on matrix-core kernels,
    2e-5 of its maximum on vector kernels with 16-bit storage, and for fp32 (config 2) at the probabilistic fp32 summation
    bound of test_stem_fp32_full_size, lambda sqrt(L) u sum |dB act| with lambda = 6, L from the launcher's partition
    (_dw_fp32_chain)."""
    import math
    from x3d_tf_amd import hip, ops
    from tests import shapes as S
    from tests.util import dw_stencil64
    _, dtype, n, c, t, h, w, stride = case[:8]
    araw, wt, _, _, _, ss, rn, g_ = _dw_inputs(gpu, case, seed)
    ho, wo = -(-h // stride), -(-w // stride)
    dv = rn(n, c, t, ho, wo).to(dtype)
    braw = (rn(n, c, t, ho, wo) * 0.8 + 0.5 * rn(c).view(1, -1, 1, 1, 1)).to(dtype)
    gate = 0.2 + 0.8 * torch.rand((n, c), generator=g_, device=gpu)
    m = n * t * ho * wo
    red = lambda v: v.sum((2, 3, 4))                         # [n, c]
    bd, dvd = braw.double(), dv.double()
    sb, sbb = red(bd).sum(0), red(bd * bd).sum(0)
    mean_b = sb / m
    k1 = (1 + 0.3 * rn(c)).double() / torch.sqrt(sbb / m - mean_b * mean_b + 1e-5)
    cA = (k1.view(1, -1) * gate.double()).float()
    sa, sab = (cA.double() * red(dvd)).sum(0), (cA.double() * red(dvd * bd)).sum(0)
    det = sb * sb - m * sbb
    cB, cC = ((m * sab - sa * sb) / det).float(), ((sbb * sa - sb * sab) / det).float()
    del bd, dvd
    coef = torch.stack([cA, cB.expand(n, c), cC.expand(n, c), torch.zeros_like(cA)], 2).contiguous()
    ga = torch.empty_like(araw)
    a_sums = torch.zeros((c, 2), dtype=torch.float64, device=gpu)
    dw = torch.full((c, 27), 0.25, dtype=torch.float32, device=gpu)
    ops.dw3d_bwd(dv, braw, coef, araw, ss, wt.view(c, 27), ga, a_sums, dw, stride)
    torch.cuda.synchronize()
    name = hip.kernel_name(S.dw_full_struct(case))
    mx = "_mx" in name
    fp32 = dtype == torch.float32
    wd = round_to(wt, dtype) if mx else wt.double()
    rt, at = tol_gemm(dtype) if mx else tol_store(dtype)
    sc, sh = ss[:, 0].double().view(1, -1, 1, 1, 1), ss[:, 1].double().view(1, -1, 1, 1, 1)
    dw_ref = torch.zeros((c, 3, 3, 3), dtype=torch.float64, device=gpu)
    dw_abs = torch.zeros_like(dw_ref)
    s1 = torch.zeros(c, dtype=torch.float64, device=gpu)
    s2 = torch.zeros(c, dtype=torch.float64, device=gpu)
    worst, CH = 0.0, _dw_chunk(case)
    for i in range(0, n, CH):
        cd = coef[i:i + CH].double()
        terms = [cd[:, :, j, None, None, None] * v for j, v in ((0, dv[i:i + CH].double()), (1, braw[i:i + CH].double()))]
        dB = terms[0] + terms[1] + cd[:, :, 2, None, None, None]
        ad = araw[i:i + CH].double()
        z = ad * sc + sh
        act = torch.relu(z)
        if fp32:        # sum |terms| of dW, with |dB| bounded by |A dv| + |B b| + |C|
            mag = terms[0].abs() + terms[1].abs() + cd[:, :, 2, None, None, None].abs()
            dw_abs += dw_stencil64(act, wd.abs(), stride, dy=mag)[1]
            del mag
        del terms
        if mx:
            dB, act = round_to(dB, dtype), round_to(act, dtype)
        dA, dwc = dw_stencil64(act, wd, stride, dy=dB)
        dw_ref += dwc
        del dB, act
        ref = dA * (z > 0)
        del dA, z
        worst = max(worst, _frac(f"ga[{i}:{i + CH}]", ga[i:i + CH], ref, rt, at * ref.abs().max().item()))
        del ref
        gs = ga[i:i + CH].double()
        s1 += gs.sum((0, 2, 3, 4))
        s2 += (gs * ad).sum((0, 2, 3, 4))
        del gs, ad
    stol = _stol(dtype)
    sref = torch.stack([s1, s2], 1)
    e_s = _frac("a_sums", a_sums, sref, 10 * stol, 10 * stol * max(1.0, sref.abs().max().item()))
    got = dw.double().view(c, 3, 3, 3) - 0.25
    if fp32:
        L = _dw_fp32_chain(name, n, t, h, w, stride)
        lim = 6.0 * math.sqrt(L) * 2.0 ** -24 * dw_abs + 2 * 2.0 ** -24 * 0.25
        e_w, _ = _check_slack("dw", got, dw_ref, 0.0, 0.0, lim)
        wmsg = f"dW {e_w:.2e} (L {L}, limit {(lim / dw_ref.abs().max()).max().item():.1e} of max)"
    else:
        wtol = _wtol(dtype) if mx else 2e-5
        e_w = _frac("dw", got, dw_ref, wtol, wtol * dw_ref.abs().max().item())
        wmsg = f"dW {e_w:.2e} (limit {wtol:.0e} of max)"
    return name, f"ga {worst:.2e}, a_sums {e_s:.2e}, {wmsg}"


@pytest.mark.parametrize("case", S.DW_FULL, ids=[S.dw_full_id(c) for c in S.DW_FULL])
def test_depthwise_full_size(gpu, case):
    """One depthwise launch of a full-size plan (tests/shapes.py DW_FULL; tests/test_dispatch_coverage.py keeps the list
    complete), in its launch form, against the fp64 stencil (tests.util.dw_stencil64) on the GPU, sample chunk by sample
    chunk: _dw_forward_case / _dw_backward_case.  Prints the kernel and each check's worst error as a fraction of its limit."""
    import time
    t0 = time.time()
    seed = 1000 + S.DW_FULL.index(case)
    name, msg = (_dw_forward_case if case[0] == "fwd" else _dw_backward_case)(gpu, case, seed)
    torch.cuda.synchronize()
    print(f"full-size depthwise {S.dw_full_id(case)} {name}: worst err / limit {msg}; {time.time() - t0:.1f} s")


# ---- every pointwise launch of the full-size plans (tests/shapes.py PW_FULL: BASELINE configs 2 - 5, config 3 in fp16 too) ----
def _pw_chunk(case):
    """Samples per fp64 chunk: about 48 M elements of the wider side at a time."""
    n, ci, co, t, h, w = case[2:8]
    return max(1, min(n, 48_000_000 // (max(ci, co) * t * h * w)))


def _pw_act(rn, shape, dtype, kind, gpu):
    """An activation as a real step has it, sample by sample: "relu" a block output (post-ReLU, positive channel means), "raw"
    a raw conv / depthwise output (channel means and scales of their own)."""
    c = shape[1]
    mu, sd = 0.5 * rn(c), 0.5 + 0.5 * rn(c).abs()
    if kind == "relu":
        mu = mu + 0.3
    out = torch.empty(shape, dtype=dtype, device=gpu)
    for i in range(shape[0]):
        v = rn(*shape[1:]) * sd.view(-1, 1, 1, 1) + mu.view(-1, 1, 1, 1)
        out[i] = (torch.relu(v) if kind == "relu" else v).to(dtype)
    return out


def _pw_ss(rn, c):
    return torch.stack([1 + 0.3 * rn(c), 0.3 * rn(c)], 1)


def _v(t, j=None):
    return (t if j is None else t[:, j]).double().view(1, -1, 1, 1, 1)


def _pw_bn_bwd(rn, g, yraw, ch):
    """The BatchNorm-backward operands of a real step, from the data: mean / invstd of yraw (fp32, as x3d_bn_finalize keeps
    them), the fp64 sums (sum g, sum g yraw) and gamma; coef = what x3d_bn_bwd_finalize / a coef_fold derives from them, so
    sum dY = 0 and sum dY yraw = 0 per channel.  Returns (coef fp32 [C][4], sums, mi, gamma, count)."""
    from tests.util import bn_bwd_fold64
    co = g.shape[1]
    m = g.numel() // co
    acc = torch.zeros((4, co), dtype=torch.float64, device=g.device)
    for i in range(0, g.shape[0], ch):
        yd, gd = yraw[i:i + ch].double(), g[i:i + ch].double()
        acc += torch.stack([yd.sum((0, 2, 3, 4)), (yd * yd).sum((0, 2, 3, 4)), gd.sum((0, 2, 3, 4)), (gd * yd).sum((0, 2, 3, 4))])
    mean = acc[0] / m
    mi = torch.stack([mean, 1.0 / torch.sqrt(acc[1] / m - mean * mean + 1e-5)], 1).float()
    sums = torch.stack([acc[2], acc[3]], 1).contiguous()
    gamma = 1 + 0.3 * rn(co)
    return bn_bwd_fold64(sums, m, mi, gamma)[0].float(), sums, mi, gamma, m


def _pw_dy32(coef, gd, yd):
    """dYraw = A g + B yraw + C evaluated in fp32, as the kernels' coefficient prologue does (before any storage rounding)."""
    c = coef.float()
    return c[:, 0].view(1, -1, 1, 1, 1) * gd.float() + c[:, 1].view(1, -1, 1, 1, 1) * yd.float() + c[:, 2].view(1, -1, 1, 1, 1)


def _pw_fold(ops, form, sums, m, mi, gamma, gpu):
    """(coef_fold for the launch or None, its publishing outputs (dgamma, dbeta, coef_out) pre-filled, or None)."""
    if "fold" not in form:
        return None, None
    if "pub" not in form:
        return ops.bn_bwd_fold(sums, m, mi, gamma), None
    co = gamma.numel()
    pub = (torch.full((co,), 0.25, device=gpu), torch.full((co,), -0.5, device=gpu), torch.full((co, 4), 7.0, device=gpu))
    return ops.bn_bwd_fold(sums, m, mi, gamma, *pub), pub


def _pw_check_pub(pub, sums, m, mi, gamma):
    """A publishing fold added dgamma / dbeta exactly once and wrote the coefficient table: against the fp64 formula from the
    same operands, to 1e-6 of the magnitudes involved (the fp32 roundings of the value and of the += on the pre-filled
    accumulator; a second publisher doubles the gradients)."""
    from tests.util import bn_bwd_fold64
    if pub is None:
        return ""
    cf, dga, dbe = bn_bwd_fold64(sums, m, mi, gamma)
    e = max(_check_slack("dgamma", pub[0], dga + 0.25, 0.0, 0.0, 1e-6 * (dga.abs() + 0.25))[0],
            _check_slack("dbeta", pub[1], dbe - 0.5, 0.0, 0.0, 1e-6 * (dbe.abs() + 0.5))[0],
            _check_slack("coef_out", pub[2], cf, 0.0, 0.0, 1e-6 * cf.abs() + 1e-30)[0])
    return f", fold publishing {e:.2e}"


def _pw_fp32_chain(name, n, ci, co, p, cus):
    """L of the fp32 weight-gradient kernels of config 2 (the probabilistic summation bound of test_stem_fp32_full_size): a
    workgroup sums 32 points per step over its run of spb steps (MFMA accumulators, exact fp32 products), then one atomic or
    slab per (sample, point chunk) of the channel pair; + the roundings of dY = A g + B y + C and of the prologue.
    pw_wgrad_f32p_kernel / pw_wgrad_f32r_kernel: about two workgroups per CU (pw_wgrad_f32p.h wgrad_f32p_launch);
    pw_wgrad_kernel: spb = total steps / 1024 in [4, 64] (pw_wgrad.hip pw_wgrad_launch)."""
    args = [int(a) for a in name[name.index("<") + 1:-1].split(", ") if a.isdigit()]
    steps = -(-p // 32)
    if name.startswith(("pw_wgrad_f32p_kernel<", "pw_wgrad_f32r_kernel<")):
        groups = -(-(-(-co // 32)) // args[0]) * -(-(-(-ci // 32)) // args[1])
        per_n = max(max((2 * cus) // groups, n) // n, 1)
        spb = min(max(-(-steps // per_n), 4), steps)
    elif name.startswith("pw_wgrad_kernel<float"):
        spb = min(max(min(steps * n // 1024, 64), 4), steps)
    else:
        raise AssertionError(f"no fp32 summation bound for {name}")
    return 32 * spb + -(-steps // spb) * n + 8


def _pw_dw_check(name, dtype, dw, fill, ref, absum, case, gpu):
    """The weight gradient (accumulator pre-filled with `fill`): _wtol of its maximum for 16-bit storage; for fp32 the
    probabilistic summation bound lambda sqrt(L) u sum |terms| (lambda = 6, L = _pw_fp32_chain), capped at 2e-5 of the
    maximum.  (Measured on an MI355X: the bound is 2e-4 - 4e-4 of the maximum, the errors at most 6.3e-6 of it.)"""
    import math
    got = dw.double() - fill
    if dtype != torch.float32:
        tol = _wtol(dtype)
        return f"dW {_frac('dw', got, ref, tol, tol * ref.abs().max().item()):.2e} (limit {tol:.0e} of max)"
    e, dt, n, ci, co, t, h, w, s = case[:9]
    p = t * -(-h // (s or 1)) * -(-w // (s or 1))
    L = _pw_fp32_chain(name, n, ci, co, p, torch.cuda.get_device_properties(gpu).multi_processor_count)
    lim = 6.0 * math.sqrt(L) * 2.0 ** -24 * absum + 2 * 2.0 ** -24 * abs(fill)
    lim = lim.clamp_max(2e-5 * ref.abs().max().item())      # (2e-5 of the maximum, fp32 tol_gemm, where that is the tighter)
    err, _ = _check_slack("dw", got, ref, 0.0, 0.0, lim)
    return f"dW {err:.2e} (L {L}, limit {(lim / ref.abs().max()).max().item():.1e} of max)"


def _pw_forward_case(gpu, case, seed):
    """x3d_pw_fwd in the plan's form.  Inputs: the tail fold reads the raw `c` output of the block below (+ its shortcut: the
    block input, or a raw shortcut conv output with bn_r) and stores relu(s x + t + [s_r] add + [t_r]); the `c` conv reads a
    raw depthwise output through BN_b [* SE gate] -> swish; plain launches read a block output (post-ReLU).  y against the fp64
    GEMM over the operands as the kernel rounds them (tol_gemm; the tail fold's operand is the stored in_store, the swish
    prologue's output rounded to storage with the tie slack of tests.util.tie_slack_pw, at most 1e-4 of the outputs may need
    it), through the inference epilogue where the case has it; in_store at tol_store; stats against fp64 sums of the stored y
    at _stol."""
    from x3d_tf_amd import hip, ops
    from tests.util import pw_gemm64, pw_infer_epi64, pw_prologue64, tie_slack_pw
    _, dtype, n, ci, co, t, h, w, stride, _, ia, oa, form = case
    f = set(form)
    g_ = torch.Generator(device=gpu)
    g_.manual_seed(seed)
    rn = lambda *s: torch.randn(*s, generator=g_, device=gpu, dtype=torch.float32)
    ho, wo = -(-h // stride), -(-w // stride)
    wt = rn(co, ci) * (2.0 / ci) ** 0.5
    kw = dict(in_act=ia)
    if "store" in f:
        x = _pw_act(rn, (n, ci, t, h, w), dtype, "raw", gpu)
        kw.update(in_ss=_pw_ss(rn, ci), in_store=torch.full(x.shape, 7.0, dtype=dtype, device=gpu))
        if "add" in f:
            kw["in_add"] = _pw_act(rn, x.shape, dtype, "raw" if "add_ss" in f else "relu", gpu)
            kw["in_add_ss"] = _pw_ss(rn, ci) if "add_ss" in f else None
    elif "ss" in f:
        x = _pw_act(rn, (n, ci, t, h, w), dtype, "raw", gpu)
        kw.update(in_ss=_pw_ss(rn, ci), in_gate=0.2 + 0.8 * torch.rand((n, ci), generator=g_, device=gpu) if "gate" in f else None)
    else:
        x = _pw_act(rn, (n, ci, t, h, w), dtype, "relu", gpu)
    if "oss" in f:
        kw.update(out_ss=_pw_ss(rn, co), out_act=oa)
        if "oadd" in f:
            kw["out_add"] = _pw_act(rn, (n, co, t, ho, wo), dtype, "raw" if "oadd_ss" in f else "relu", gpu)
            kw["out_add_ss"] = _pw_ss(rn, co) if "oadd_ss" in f else None
    stats = torch.zeros((co, 2), dtype=torch.float64, device=gpu) if "stats" in f else None
    wp = ops.pw_pack_weights([wt], dgrad=False, dtype=dtype)[0][0] if dtype != torch.float32 else None
    y = ops.pw_fwd(x, wt, stats=stats, stride=stride, w_panel=wp, **kw)
    torch.cuda.synchronize()
    name = hip.kernel_name(S.pw_full_struct(case))
    wr = round_to(wt, dtype)
    rt, at = tol_gemm(dtype)
    rs, as_ = tol_store(dtype)
    worst = dict(y=0.0, in_store=0.0)
    needed, CH = 0, _pw_chunk(case)
    y1 = torch.zeros(co, dtype=torch.float64, device=gpu)
    y2 = torch.zeros(co, dtype=torch.float64, device=gpu)
    for i in range(0, n, CH):
        sl = slice(i, i + CH)
        slack = 0.0
        if "store" in f:
            v = _v(kw["in_ss"], 0) * x[sl].double() + _v(kw["in_ss"], 1)
            if "add" in f:
                a = kw["in_add"][sl].double()
                v = v + (a * _v(kw["in_add_ss"], 0) + _v(kw["in_add_ss"], 1) if "add_ss" in f else a)
            v = torch.relu(v)
            worst["in_store"] = max(worst["in_store"], _frac(f"in_store[{i}]", kw["in_store"][sl], v, rs, as_ * v.abs().max().item()))
            op = kw["in_store"][sl].double()            # (the GEMM operand is the stored block output)
            del v
        elif "ss" in f:
            gate = None if kw["in_gate"] is None else kw["in_gate"][sl]
            op = pw_prologue64(x[sl], kw["in_ss"], gate, ia, dtype)
            if dtype != torch.float32:
                slack = tie_slack_pw(pw_prologue64(x[sl], kw["in_ss"], gate, ia), dtype, wr.abs())
        else:
            op = x[sl].double()
        ref = pw_gemm64(op, wr, stride)
        del op
        if "oss" in f:
            ref = pw_infer_epi64(ref, kw["out_ss"], None if "oadd" not in f else kw["out_add"][sl], kw.get("out_add_ss"), oa)
            slack = slack * kw["out_ss"][:, 0].double().abs().view(1, -1, 1, 1, 1)
        e, nd = _check_slack(f"y[{i}:{i + CH}]", y[sl], ref, rt, at * max(ref.abs().max().item(), 1e-30), slack)
        worst["y"], needed = max(worst["y"], e), needed + nd
        del ref, slack
        if stats is not None:
            yd = y[sl].double()
            y1 += yd.sum((0, 2, 3, 4))
            y2 += (yd * yd).sum((0, 2, 3, 4))
            del yd
    frac = needed / y.numel()
    assert frac < 1e-4, f"{frac:.2e} of the outputs needed the tie slack: a systematic error, not ties"
    msg = f"y {worst['y']:.2e} ({frac:.1e} needed the tie slack)"
    if "store" in f:
        msg += f", in_store {worst['in_store']:.2e}"
    if stats is not None:
        sref = torch.stack([y1, y2], 1)
        stol = _stol(dtype)
        msg += f", stats {_frac('stats', stats, sref, stol, stol * max(1.0, sref.abs().max().item())):.2e}"
    return name, msg


def _pw_backward_case(gpu, case, seed):
    """x3d_pw_dgrad / x3d_pw_wgrad / x3d_pw_bwd in the plan's form, with a real step's BatchNorm backward (_pw_bn_bwd: the
    coefficient table, or the coef_fold that derives it from the same sums).  Conv inputs: a block output (post-ReLU) for the
    `a` / shortcut convs, a raw depthwise output through BN_b [* SE gate] -> swish for the `c` convs (stride 2: the even
    pixels).  dx against Wr^T dY with dY evaluated in fp32 and rounded to storage (tol_gemm + the dY tie slack, x 1.1 through
    swish'), then its epilogue: add / strided add, swish' with the per-(n, c) sums (10 _stol), the tail fold's [x > 0] mask with
    tail_sums_c / _r (10 _stol).  dW (accumulator pre-filled, slabs through x3d_dw_slab_reduce from a NaN-filled buffer) against
    sum dY x^T over the operands as rounded (_pw_dw_check).  The recomputed-output form (rc) goes through ops.pw_bwd_rc
    (prepare -> launch -> finish): y = Wr x, dx against the fold with its two panel operands rounded, dW against the
    definition.  A publishing fold's dgamma / dbeta / table: _pw_check_pub."""
    from x3d_tf_amd import hip, ops
    from tests.util import pw_prologue64, tie_slack_pw
    e, dtype, n, ci, co, t, h, w, s, epi, ia, _, form = case
    f = set(form)
    g_ = torch.Generator(device=gpu)
    g_.manual_seed(seed)
    rn = lambda *sh: torch.randn(*sh, generator=g_, device=gpu, dtype=torch.float32)
    stride = 2 if s == 2 else 1
    ho, wo = -(-h // stride), -(-w // stride)
    half = dtype != torch.float32
    wt = rn(co, ci) * (2.0 / ci) ** 0.5
    wr = round_to(wt, dtype)
    CH = _pw_chunk(case)
    swish = epi == 3 or "ss" in f
    # the conv input (as stored) and, for the `c` conv, its prologue
    x = _pw_act(rn, (n, ci, t, h, w), dtype, "raw" if swish else "relu", gpu)
    bss = _pw_ss(rn, ci) if swish else None
    gate = 0.2 + 0.8 * torch.rand((n, ci), generator=g_, device=gpu) if "gate" in f else None
    g = rn(n, co, t, ho, wo).to(dtype)
    dx = torch.empty((n, ci, t, ho, wo), dtype=dtype, device=gpu) if e != "wgrad" else None
    dw = torch.full((co, ci), 0.5, dtype=torch.float32, device=gpu)
    add = None
    if epi in (1, 2):
        add = (rn(n, ci, t, ho, wo) if epi == 1 else rn(n, ci, t, -(-ho // 2), -(-wo // 2))).to(dtype)
    nc = torch.zeros((n, ci, 2), dtype=torch.float64, device=gpu) if epi == 3 else None
    tails = {k: (_pw_act(rn, (n, ci, t, ho, wo), dtype, "raw", gpu), torch.zeros((ci, 2), dtype=torch.float64, device=gpu))
             for k in ("tail_c", "tail_r") if k in f}
    pub = None
    if "rc" in f:
        yraw = None             # y = Wr x, recomputed: its statistics and the coefficients from an fp64 pass
        xs = lambda sl: x[sl].double()[:, :, :, ::stride, ::stride]
        acc = torch.zeros((4, co), dtype=torch.float64, device=gpu)
        for i in range(0, n, CH):
            yd, gd = torch.einsum("oc,ncthw->nothw", wr, xs(slice(i, i + CH))), g[i:i + CH].double()
            acc[:2] += torch.stack([yd.sum((0, 2, 3, 4)), (yd * yd).sum((0, 2, 3, 4))])
            del yd
        m = n * t * ho * wo
        mean = acc[0] / m
        invstd = 1.0 / torch.sqrt(acc[1] / m - mean * mean + 1e-5)
        for i in range(0, n, CH):
            yd, gd = torch.einsum("oc,ncthw->nothw", wr, xs(slice(i, i + CH))), g[i:i + CH].double()
            acc[2:] += torch.stack([gd.sum((0, 2, 3, 4)), (gd * yd).sum((0, 2, 3, 4))])
            del yd, gd
        coef = _bn_bwd_coef_sums(m, acc[0], acc[1], acc[2], acc[3], (1 + 0.3 * rn(co)).double())
        tc, tr = tails.get("tail_c", (None, None)), tails.get("tail_r", (None, None))
        assert ops.pw_bwd_rc(g, x, wt, coef, dx, dw, epi, add, tail_c=tc[0], tail_r=tr[0], tail_sums_c=tc[1], tail_sums_r=tr[1],
                             x_stride=stride), "the recomputed-output form should cover this launch"
    else:
        yraw = _pw_act(rn, (n, co, t, ho, wo), dtype, "raw", gpu)
        coef, sums, mi, gamma, m = _pw_bn_bwd(rn, g, yraw, CH)
        fold, pub = _pw_fold(ops, f, sums, m, mi, gamma, gpu)
        dp = ops.pw_pack_weights([wt], dtype=dtype)[0][1] if half and e != "wgrad" else None
        swk = dict(braw=x, b_ss=bss, gate=gate, nc_sums=nc) if epi == 3 else {}
        if e == "dgrad":
            ops.pw_dgrad(g, yraw, coef, wt, dx, epi, add=add, w_panel=dp, coef_fold=fold, **swk)
        elif e == "wgrad":
            assert ops.pw_wgrad(g, yraw, coef, x, dw, in_ss=bss, in_gate=gate, in_act=ia, stride=stride, slab="slab" in f,
                                coef_fold=fold), "the plan's slab form should be there"
        else:
            tc = tails.get("tail_c", (None, None))
            assert ops.pw_bwd(g, yraw, coef, dp, dx, dw, epi, x=None if epi == 3 else x, add=add, tail_c=tc[0],
                              tail_sums_c=tc[1], slab="slab" in f, coef_fold=fold, **swk), "the fused kernel should cover this launch"
    torch.cuda.synchronize()
    name = hip.kernel_name(S.pw_full_struct(case))
    rt, at = tol_gemm(dtype)
    cd = coef.double()
    dw_ref = torch.zeros((co, ci), dtype=torch.float64, device=gpu)
    dw_abs = torch.zeros_like(dw_ref)
    worst, needed = 0.0, 0
    tsum = {k: torch.zeros((ci, 2), dtype=torch.float64, device=gpu) for k in tails}
    ncref = torch.zeros((n, ci, 2), dtype=torch.float64, device=gpu)
    if "rc" in f:
        w1 = round_to((wr * cd[:, 0:1]).float(), dtype)
        mm = round_to(torch.einsum("oc,o,od->cd", wr, cd[:, 1], wr).float(), dtype)
        c0 = (wr * cd[:, 2:3]).sum(0).view(1, -1, 1, 1, 1)
    for i in range(0, n, CH):
        sl = slice(i, i + CH)
        gd = g[sl].double()
        if "rc" in f:
            xd = xs(sl)
            dy = _v(cd, 0) * gd + _v(cd, 1) * torch.einsum("oc,ncthw->nothw", wr, xd) + _v(cd, 2)     # the definition
            ref = torch.einsum("oc,nothw->ncthw", w1, gd) + torch.einsum("cd,ndthw->ncthw", mm, xd) + c0
            slack = 0.0
        else:
            dy32 = _pw_dy32(coef, gd, yraw[sl].double())
            dy = round_to(dy32, dtype)
            xd = pw_prologue64(x[sl], bss, None if gate is None else gate[sl], 2, dtype) if swish else x[sl].double()
            xd = xd[:, :, :, ::stride, ::stride]
            if dtype == torch.float32:
                mag = _v(cd[:, 0].abs()) * gd.abs() + _v(cd[:, 1].abs()) * yraw[sl].double().abs() + _v(cd[:, 2].abs())
                dw_abs += torch.einsum("nothw,ncthw->oc", mag, xd.abs())
                del mag
            if e != "wgrad":
                ref = torch.einsum("oc,nothw->ncthw", wr, dy)
                slack = tie_slack_pw(dy32, dtype, wr.abs().t()) * (1.1 if epi == 3 else 1.0) if half else 0.0
            del dy32
        dw_ref += torch.einsum("nothw,ncthw->oc", dy, xd)
        del dy, xd
        if e != "wgrad":
            if epi == 1:
                ref += add[sl].double()
            elif epi == 2:
                ref[:, :, :, ::2, ::2] += add[sl].double()
            elif epi == 3:
                vb = (_v(bss, 0) * x[sl].double() + _v(bss, 1)) * (1.0 if gate is None else gate[sl].double()[:, :, None, None, None])
                sg = torch.sigmoid(vb)
                ref = ref * (sg * (1 + vb * (1 - sg)))
                del vb, sg
            if tails:
                keep = x[sl] > 0
                ref = ref * keep
                slack = slack * keep if torch.is_tensor(slack) else slack
                assert not bool((dx[sl][~keep] != 0).any()), "gradient leaked through a closed ReLU"
            ew, nd = _check_slack(f"dx[{i}:{i + CH}]", dx[sl], ref, rt, at * max(ref.abs().max().item(), 1e-30), slack)
            worst, needed = max(worst, ew), needed + nd
            del ref, slack
            ds = dx[sl].double()
            if epi == 3:
                ncref[sl] = torch.stack([ds.sum((2, 3, 4)), (ds * x[sl].double()).sum((2, 3, 4))], -1)
            for k, (tt, _) in tails.items():
                tsum[k] += torch.stack([ds.sum((0, 2, 3, 4)), (ds * tt[sl].double()).sum((0, 2, 3, 4))], 1)
            del ds
        del gd
    msgs = []
    st10 = 10 * _stol(dtype)
    if e != "wgrad":
        frac = needed / dx.numel()
        assert frac < 1e-4, f"{frac:.2e} of the outputs needed the tie slack: a systematic error, not ties"
        msgs.append(f"dx {worst:.2e} ({frac:.1e} needed the tie slack)")
        if epi == 3:
            msgs.append(f"nc_sums {_frac('nc_sums', nc, ncref, st10, st10 * max(1.0, ncref.abs().max().item())):.2e}")
        for k, (_, got) in tails.items():
            msgs.append(f"{k} sums {_frac(k, got, tsum[k], st10, st10 * max(1.0, tsum[k].abs().max().item())):.2e}")
    if e != "dgrad":
        msgs.append(_pw_dw_check(name, dtype, dw, 0.5, dw_ref, dw_abs, case, gpu))
    else:
        assert float((dw - 0.5).abs().max()) == 0.0
    msg = ", ".join(msgs)
    if pub is not None:
        msg += _pw_check_pub(pub, sums, m, mi, gamma)
    return name, msg


@pytest.mark.parametrize("case", S.PW_FULL, ids=[S.pw_full_id(c) for c in S.PW_FULL])
def test_pointwise_full_size(gpu, case):
    """One pointwise launch of a full-size plan (tests/shapes.py PW_FULL; tests/test_dispatch_coverage.py keeps the list
    complete), in its launch form, against fp64 on the GPU (tests.util.pw_gemm64 and its prologue / epilogue restatements),
    sample chunk by sample chunk: _pw_forward_case / _pw_backward_case.  Prints the kernel, each check's worst error as a
    fraction of its limit, and the seconds the case took."""
    import time
    t0 = time.time()
    seed = 2000 + S.PW_FULL.index(case)
    name, msg = (_pw_forward_case if case[0] == "fwd" else _pw_backward_case)(gpu, case, seed)
    torch.cuda.synchronize()
    print(f"full-size pointwise {S.pw_full_id(case)} {name}: worst err / limit {msg}; {time.time() - t0:.1f} s")


@pytest.mark.parametrize("dtype", HALF)
def test_pw_wgrad_generic_kernel_refuses_a_slab(gpu, dtype):
    """x3d_pw_wgrad's 16-bit generic kernel (an odd point count on a row-misaligned x: pw_wgrad_bf16_kernel) has no slab form:
    given a dw_slab it must refuse before any launch, not add into dw by atomics and leave the slabs unwritten."""
    import ctypes as C
    from x3d_tf_amd import hip
    n, ci, co, t, h, w = 1, 48, 108, 13, 5, 5
    g_ = torch.Generator(device=gpu)
    g_.manual_seed(5)
    xb = torch.randn(n * ci * t * h * w + 1, generator=g_, device=gpu).to(dtype)
    g = torch.randn((n, co, t, h, w), generator=g_, device=gpu).to(dtype)
    yraw = torch.randn((n, co, t, h, w), generator=g_, device=gpu).to(dtype)
    coef = torch.randn((co, 4), generator=g_, device=gpu) * 0.5
    dw = torch.full((co, ci), 0.5, device=gpu)
    slab = torch.full((4 * co * ci,), float("nan"), device=gpu)
    a = hip.PwWgradArgs(g.data_ptr(), yraw.data_ptr(), coef.data_ptr(), xb.data_ptr() + xb.element_size(), None, None, 0,
                        dw.data_ptr(), n, ci, co, t, h, w, 1, hip.dtype_code(dtype))
    assert hip.kernel_name(a).startswith("pw_wgrad_bf16_kernel<") and hip.load().x3d_pw_wgrad_dw_parts(C.byref(a)) == 0
    a.dw_slab, a.dw_slab_parts = slab.data_ptr(), 4
    with pytest.raises(hip.X3DHipError, match="slab"):
        hip.call_struct("x3d_pw_wgrad", a)
    torch.cuda.synchronize()
    assert float((dw - 0.5).abs().max()) == 0.0 and bool(slab.isnan().all())


# ---- every other launch of the full-size plans (tests/shapes.py AUX_FULL; the runners and their limits: tests/aux_checks.py) ----

@pytest.mark.parametrize("case", S.AUX_FULL, ids=[S.aux_full_id(c) for c in S.AUX_FULL])
def test_aux_full_size(gpu, case):
    """One launch of a full-size plan outside the pointwise / depthwise / stem families (tests/shapes.py AUX_FULL;
    tests/test_dispatch_coverage.py keeps the list complete), at its real size and in its launch form, against fp64 on the
    GPU.  Prints each check's worst error as a fraction of its limit."""
    import time
    t0 = time.time()
    rn, g_ = _aux_rn(gpu, 3000 + S.AUX_FULL.index(case))
    msg = _AUX_CASES[case[0]](gpu, case, rn, g_)
    torch.cuda.synchronize()
    print(f"full-size {S.aux_full_id(case)}: worst err / limit {msg}; {time.time() - t0:.1f} s")
