"""The dilated channelwise kernels (csrc/dw_dil.hip, x3d_dw3d_fwd_dil / x3d_dw3d_bwd_dil) against the fp64 stencil of
tests/dilated_ref.py, and a model with NETWORK.RES5_DILATION = 2 against the oracle with the dilation applied (DilatedStorage).

Kernel parity: the limits of the dense vector kernels (tests/dw_checks.py, tests/test_kernels_gpu.py) -- y / ga at tol_store of
the unrounded operands' stencil, statistics and pool at _stol, a_sums at 10 _stol, dW at 2e-4 of its maximum -- on guarded
views (tests/aux_checks.py _Bands) with NaN-prefilled outputs; the `+=` outputs start from non-zero values.  N = 2, C = 3
everywhere.  Model level: the comparisons of tests/test_model_gpu.py at their own limits, run over the dilated model."""
import ctypes as C

import pytest
import torch

from tests import dilated_ref as R
from tests import shapes as S
from tests.aux_checks import _Bands, _frac
from tests.util import report, rnd, round_to, tol_gemm, tol_store

pytestmark = pytest.mark.gpu

N, CH = 2, 3
DTYPES = [torch.float32, torch.bfloat16, torch.float16]
_id = lambda d: str(d).split(".")[-1]

# (T, H, W, d, off): what each exercises is in the comment; off = elements past 16-byte alignment of EVERY operand
CASES = [
    (1, 3, 3, 2, 0),      # T = 1: the ring never fills (no t-1, no t+1)
    (2, 3, 3, 2, 0),      # T = 2: a ring shorter than itself
    (5, 3, 3, 2, 0),      # T = 5: the ring wraps; 3 x 3 at d = 2: every off-centre tap of the centre pixel in the halo
    (3, 1, 1, 2, 0),      # 1 x 1: every spatial tap but the centre in the halo
    (3, 2, 3, 2, 0),      # 2 x 3: taps partly in the halo
    (3, 5, 7, 2, 0),      # non-square
    (3, 10, 10, 2, 0),    # 16-bit plane of 200 bytes: plane starts 8 bytes off 16-byte alignment
    (3, 14, 14, 2, 0),    # 392-byte planes; the M / S / XS plane of a dilated res5
    (3, 14, 14, 3, 0),    # each dilation once (d = 1: test_dilation_one_is_the_dense_entry)
    (3, 14, 14, 4, 0),
    (2, 16, 16, 2, 0),    # exactly 256 pixels: every thread owns one
    (2, 17, 19, 2, 0),    # two pixels per thread, the second round ragged (323 pixels)
    (2, 20, 20, 2, 0),    # the L / XL plane
    (2, 23, 24, 2, 0),    # past 512 pixels: the direct-staging instantiation (NP = 0)
    (3, 14, 14, 2, 1),    # every operand one element past alignment
    (2, 17, 19, 3, 1),
]
_case_id = lambda c: f"T{c[0]}-{c[1]}x{c[2]}-d{c[3]}" + (f"-off{c[4]}" if c[4] else "")
PREFILL = 0.5             # start value of stats / pool / a_sums; dW starts at 0.25 as in tests/dw_checks.py


def _k():
    from tests import test_kernels_gpu as K
    return K


def _name(st):
    from x3d_tf_amd import hip
    return hip.dw3d_kernel_name(st)


def _np(h, w):
    return 1 if h * w <= 256 else (2 if h * w <= 512 else 0)


def _tname(dtype):
    return {torch.float32: "float", torch.bfloat16: "bf16", torch.float16: "f16"}[dtype]


def _fwd_forms(gpu, dtype, t, h, w, d, off):
    """the forward of one case in its three forms -- scale/shift + ReLU with both sums, scale/shift without activation and without
    sums, the BatchNorm fold -- each against the stencil; {name: worst error / limit}"""
    from x3d_tf_amd import hip, ops
    K = _k()
    g = K._gen(2)
    x, xd = rnd((N, CH, t, h, w), dtype, g)
    wt = torch.randn((CH, 3, 3, 3), generator=g) * 0.3
    ss = torch.stack([1 + 0.3 * torch.randn(CH, generator=g), 0.3 * torch.randn(CH, generator=g)], 1)
    B = _Bands(gpu, off)
    xg, wg, ssg = B.view(x.to(gpu)), B.view(wt.to(gpu)), B.view(ss.to(gpu))
    code = hip.dtype_code(dtype)
    rt, at = tol_store(dtype)
    stol = K._stol(dtype)
    out = {}

    def struct(y, ssp, act, stats, pool, fold=None, dil=d):
        return hip.dilated(hip.Dw3dFwdArgs(xg.data_ptr(), wg.data_ptr(), y.data_ptr(), ssp, act, stats, pool, N, CH, t, h, w, 1, code,
                                           None if fold is None else C.pointer(fold)), dil)

    want = f"dw3d_dil_fwd_kernel<{_tname(dtype)}, {_np(h, w)}, {2 if d == 2 else 0}>"
    # ---- scale/shift + ReLU, statistics (replicated layout) and pool on a non-zero start
    reps, rstride = hip.stats_layout(CH)
    stats_rep = B((reps * rstride,), torch.float64, fill=0.0)
    stats_rep[:2 * CH] = PREFILL
    pool = B((N, CH), torch.float64, fill=PREFILL)
    y = B((N, CH, t, h, w), dtype)
    assert _name(struct(y, ssg.data_ptr(), 1, stats_rep.data_ptr(), pool.data_ptr())) == want
    ops.dw3d_fwd(xg, wg, 1, y=y, in_ss=ssg, in_act=1, stats=stats_rep, pool=pool, dilation=d)
    torch.cuda.synchronize()
    ref = R.fwd_ref(xd, wt, d, ss, 1)
    out["y"] = _frac("y", y.cpu(), ref, rt, at * ref.abs().max().item())
    ys = y.float().cpu()
    sref = K._stats_ref(ys, dtype) + PREFILL
    out["stats"] = _frac("stats", ops.stats_sum(stats_rep, CH).cpu(), sref, stol, stol * max(1.0, sref.abs().max().item()))
    out["pool"] = _frac("pool", pool.cpu(), ys.double().sum((2, 3, 4)) + PREFILL, stol,
                        10 * stol * max(1.0, float(ys[0, 0].numel()) ** 0.5))
    # ---- scale/shift, no activation, no sums
    y2 = B((N, CH, t, h, w), dtype)
    assert _name(struct(y2, ssg.data_ptr(), 0, None, None)) == want
    ops.dw3d_fwd(xg, wg, 1, y=y2, in_ss=ssg, in_act=0, dilation=d)
    torch.cuda.synchronize()
    ref2 = R.fwd_ref(xd, wt, d, ss, 0)
    out["y_none"] = _frac("y_none", y2.cpu(), ref2, rt, at * ref2.abs().max().item())
    # ---- no prologue at all
    y3 = B((N, CH, t, h, w), dtype)
    ops.dw3d_fwd(xg, wg, 1, y=y3, dilation=d)
    torch.cuda.synchronize()
    ref3 = R.fwd_ref(xd, wt, d)
    out["y_raw"] = _frac("y_raw", y3.cpu(), ref3, rt, at * ref3.abs().max().item())
    # ---- the BatchNorm finalize folded into the launch: x3d_bn_finalize's own table, published bit for bit
    xs = xg.double()
    xstats = torch.stack([xs.sum((0, 2, 3, 4)), (xs * xs).sum((0, 2, 3, 4))], 1).contiguous()
    gamma = B.view((1 + 0.3 * torch.randn(CH, generator=g)).to(gpu))
    beta = B.view((0.3 * torch.randn(CH, generator=g)).to(gpu))
    count = N * t * h * w
    mm0, mv0 = torch.full((CH,), 0.25, device=gpu), torch.full((CH,), 1.5, device=gpu)
    ss0, mi0 = torch.zeros((CH, 2), device=gpu), torch.zeros((CH, 2), device=gpu)
    ops.bn_finalize(xstats, count, gamma, beta, mm0, mv0, 1e-5, 0.9, 1, ss0, mi0)
    mm1, mv1 = B((CH,), torch.float32, fill=0.25), B((CH,), torch.float32, fill=1.5)
    ss1, mi1 = B((CH, 2), torch.float32), B((CH, 2), torch.float32)
    fold = ops.bn_fold(xstats, count, gamma, beta, mm1, mv1, 1e-5, 0.9, 1, ss1, mi1)
    y4 = B((N, CH, t, h, w), dtype)
    assert _name(struct(y4, None, 1, None, None, fold)) == want
    ops.dw3d_fwd(xg, wg, 1, y=y4, in_act=1, in_bn=fold, dilation=d)
    torch.cuda.synchronize()
    for name, a_, b_ in (("ss", ss0, ss1), ("mean_invstd", mi0, mi1), ("moving_mean", mm0, mm1), ("moving_var", mv0, mv1)):
        assert torch.equal(a_, b_), f"bn fold: {name} differs from x3d_bn_finalize's"
    assert ss1.abs().sum().item() > 0
    ref4 = R.fwd_ref(xd, wt, d, ss0.cpu(), 1)
    out["y_bn"] = _frac("y_bn", y4.cpu(), ref4, rt, at * ref4.abs().max().item())
    B.check()
    return out


def _bwd_operands(dtype, t, h, w):
    K = _k()
    g_ = K._gen(5)
    araw, ad = rnd((N, CH, t, h, w), dtype, g_)
    dv, dvd = rnd((N, CH, t, h, w), dtype, g_)
    braw, bd = rnd((N, CH, t, h, w), dtype, g_)
    coef = torch.randn((N, CH, 4), generator=g_) * 0.5
    wt = torch.randn((CH, 3, 3, 3), generator=g_) * 0.3
    ss = torch.stack([1 + 0.3 * torch.randn(CH, generator=g_), 0.3 * torch.randn(CH, generator=g_)], 1)
    return (araw, dv, braw, coef, wt, ss), (ad, dvd, bd)


def _bwd_case(gpu, dtype, t, h, w, d, off):
    from x3d_tf_amd import hip, ops
    K = _k()
    (araw, dv, braw, coef, wt, ss), (ad, dvd, bd) = _bwd_operands(dtype, t, h, w)
    ga_ref, dw_ref = R.bwd_ref(dvd, bd, coef, ad, ss, wt, d)
    B = _Bands(gpu, off)
    p = dict(dv=B.view(dv.to(gpu)), braw=B.view(braw.to(gpu)), coef=B.view(coef.to(gpu)), araw=B.view(araw.to(gpu)),
             ss=B.view(ss.to(gpu)), w=B.view(wt.to(gpu).view(CH, 27)), ga=B((N, CH, t, h, w), dtype),
             a_sums=B((CH, 2), torch.float64, fill=PREFILL), dw=B((CH, 27), torch.float32, fill=0.25))
    st = hip.dilated(hip.Dw3dBwdArgs(*(p[k].data_ptr() for k in ("dv", "braw", "coef", "araw", "ss", "w", "ga", "a_sums", "dw")),
                                     N, CH, t, h, w, 1, hip.dtype_code(dtype)), d)
    assert _name(st) == f"dw3d_dil_bwd_kernel<{_tname(dtype)}, {_np(h, w)}, {2 if d == 2 else 0}>"
    ops.dw3d_bwd(p["dv"], p["braw"], p["coef"], p["araw"], p["ss"], p["w"], p["ga"], p["a_sums"], p["dw"], 1, dilation=d)
    torch.cuda.synchronize()
    rt, at = tol_store(dtype)
    out = {"ga": _frac("ga", p["ga"].cpu(), ga_ref, rt, at * ga_ref.abs().max().item())}
    out["dw"] = _frac("dw", p["dw"].cpu(), dw_ref + 0.25, 2e-4, 2e-4 * dw_ref.abs().max().item())
    gs = p["ga"].float().cpu().double()
    sref = torch.stack([gs.sum((0, 2, 3, 4)), (gs * ad).sum((0, 2, 3, 4))], 1) + PREFILL
    stol = K._stol(dtype)
    out["a_sums"] = _frac("a_sums", p["a_sums"].cpu(), sref, 10 * stol, 10 * stol * max(1.0, sref.abs().max().item()))
    B.check()
    return out


@pytest.mark.parametrize("case", CASES, ids=_case_id)
@pytest.mark.parametrize("dtype", DTYPES, ids=_id)
def test_dilated_fwd(gpu, dtype, case):
    print(_case_id(case), _id(dtype), {k: round(v, 3) for k, v in _fwd_forms(gpu, dtype, *case).items()})


@pytest.mark.parametrize("case", CASES, ids=_case_id)
@pytest.mark.parametrize("dtype", DTYPES, ids=_id)
def test_dilated_bwd(gpu, dtype, case):
    print(_case_id(case), _id(dtype), {k: round(v, 3) for k, v in _bwd_case(gpu, dtype, *case).items()})


@pytest.mark.parametrize("dtype", DTYPES, ids=_id)
def test_dilation_one_is_the_dense_entry(gpu, dtype):
    """14 x 14 at d = 1: dilation = 1 (through x3d_dw3d_fwd_dil / x3d_dw3d_bwd_dil, which hand d < 2 to the dense entries) and
    the dense entries themselves run the dense kernel -- the same instantiation, the same bits -- and both
    meet the stencil at d = 1 (the dense 16-bit kernel of this plane multiplies on the matrix cores: operands rounded to the
    storage type, tol_gemm / _wtol, as tests/dw_checks.py holds it)."""
    from x3d_tf_amd import hip, ops
    K = _k()
    t, h, w = 3, 14, 14
    g = K._gen(2)
    x, xd = rnd((N, CH, t, h, w), dtype, g)
    wt = torch.randn((CH, 3, 3, 3), generator=g) * 0.3
    ss = torch.stack([1 + 0.3 * torch.randn(CH, generator=g), 0.3 * torch.randn(CH, generator=g)], 1)
    xg, wg, ssg = x.to(gpu), wt.to(gpu), ss.to(gpu)
    code = hip.dtype_code(dtype)
    ys = {}
    for dil in (0, 1):
        y = torch.full((N, CH, t, h, w), float("nan"), dtype=dtype, device=gpu)
        st = hip.dilated(hip.Dw3dFwdArgs(xg.data_ptr(), wg.data_ptr(), y.data_ptr(), ssg.data_ptr(), 1, None, None, N, CH, t, h, w, 1, code, None), dil)
        if dil:      # the dilated entry itself with d = 1 (ops.dw3d_fwd keeps d < 2 on the dense entry)
            hip.call_struct_dil("x3d_dw3d_fwd_dil", st, 1)
            ys[dil] = (y, _name(st))
        else:
            ys[dil] = (ops.dw3d_fwd(xg, wg, 1, y=y, in_ss=ssg, in_act=1), _name(st))
    torch.cuda.synchronize()
    assert ys[0][1] == ys[1][1] and "_dil_" not in ys[1][1] and torch.equal(ys[0][0], ys[1][0])
    mx = "_mx" in ys[1][1]
    pre = torch.relu(xd * ss[:, 0].double().view(1, -1, 1, 1, 1) + ss[:, 1].double().view(1, -1, 1, 1, 1))
    ref = R.dilated3x3x3(round_to(pre.float(), dtype), round_to(wt, dtype), 1) if mx else R.dilated3x3x3(pre, wt.double(), 1)
    rt, at = tol_gemm(dtype) if mx else tol_store(dtype)
    report("y", ys[1][0], ref, rt, at * ref.abs().max().item())
    # backward
    (araw, dv, braw, coef, wt, ss), (ad, dvd, bd) = _bwd_operands(dtype, t, h, w)
    dev = [v.to(gpu) for v in (dv, braw, coef, araw, ss, wt.view(CH, 27))]
    res = {}
    for dil in (0, 1):
        ga = torch.full((N, CH, t, h, w), float("nan"), dtype=dtype, device=gpu)
        a_sums = torch.zeros((CH, 2), dtype=torch.float64, device=gpu)
        dw = torch.full((CH, 27), 0.25, device=gpu)
        st = hip.dilated(hip.Dw3dBwdArgs(*(v.data_ptr() for v in dev), ga.data_ptr(), a_sums.data_ptr(), dw.data_ptr(), N, CH, t, h, w, 1, code), dil)
        nm = _name(st)
        if dil:
            hip.call_struct_dil("x3d_dw3d_bwd_dil", st, 1)
        else:
            ops.dw3d_bwd(*dev, ga, a_sums, dw, 1)
        res[dil] = (ga, dw, nm)
    torch.cuda.synchronize()
    assert res[0][2] == res[1][2] and "_dil_" not in res[1][2] and torch.equal(res[0][0], res[1][0])
    mx = "_mx" in res[1][2]
    if mx:      # dB, relu(z) and the weights enter the products rounded to the storage type
        import torch.nn.functional as F
        cd = coef.double()
        dB = round_to((cd[:, :, 0, None, None, None] * dvd + cd[:, :, 1, None, None, None] * bd + cd[:, :, 2, None, None, None]).float(), dtype)
        z = ad * ss[:, 0].double().view(1, -1, 1, 1, 1) + ss[:, 1].double().view(1, -1, 1, 1, 1)
        act = round_to(F.relu(z).float(), dtype).requires_grad_(True)
        wref = round_to(wt, dtype).requires_grad_(True)
        dA, dWr = torch.autograd.grad((R.dilated3x3x3(act, wref, 1) * dB).sum(), [act, wref])
        ga_ref, dw_ref = dA * (z > 0), dWr.reshape(CH, 27)
        rt, at, wtol = *tol_gemm(dtype), K._wtol(dtype)
    else:
        ga_ref, dw_ref = R.bwd_ref(dvd, bd, coef, ad, ss, wt, 1)
        rt, at, wtol = *tol_store(dtype), 2e-4
    report("ga", res[1][0], ga_ref, rt, at * ga_ref.abs().max().item())
    report("dw", res[1][1], dw_ref + 0.25, wtol, wtol * dw_ref.abs().max().item())


def test_refused_launches_leave_the_outputs_alone(gpu):
    """dilation = 2 with stride 2, dilation = 5 and a plane over the LDS limit, on real device tensors: the error comes back, y is
    untouched"""
    from x3d_tf_amd import hip, ops
    for (h, w, stride, d), word in (((14, 14, 2, 2), "stride"), ((14, 14, 1, 5), "dilation"), ((61, 61, 1, 2), "LDS")):
        x = torch.zeros((N, CH, 2, h, w), device=gpu)
        wt = torch.zeros((CH, 3, 3, 3), device=gpu)
        y = torch.full((N, CH, 2, h, w), 7.0, device=gpu)
        with pytest.raises(hip.X3DHipError, match=word):
            ops.dw3d_fwd(x, wt, stride, y=y, dilation=d)
        torch.cuda.synchronize()
        assert (y == 7.0).all()


# ---- model level ----------------------------------------------------------------------------------------------------------
DIL = ["NETWORK.RES5_DILATION", 2, "NETWORK.NUM_CLASSES", 5]
XS_STEP = ("XS", 2, 4, 64)


def _dilated_oracle(monkeypatch, overrides):
    """oracle.x3d_oracle.Storage -> DilatedStorage at the dilated sites of the config's architecture, for the oracle calls of the
    runners of tests/test_model_gpu.py (O.forward builds its Storage by that name); returns the architecture"""
    import x3d_tf_amd as x
    from oracle import x3d_oracle as O
    arch = x.build_arch(x.get_config(XS_STEP[0], overrides))
    sites = R.dilated_sites(arch)
    assert len(sites) == len(arch.stages[-1].blocks) and set(sites.values()) == {2}

    class _Storage(R.DilatedStorage):
        def __init__(self, dtype=None, dw_operands=None):
            super().__init__(dtype, dw_operands, sites=sites)

    monkeypatch.setattr(O, "Storage", _Storage)
    return arch


def _check_plan_is_dilated(pl, arch):
    last = [B for B in pl.blocks if B.spec.stage == len(arch.stages) - 1]
    assert len(last) == len(arch.stages[-1].blocks)
    for B in last:
        assert B.sb.dilation == 2 and B.sb.stride == 1 and "dw3d_dil_fwd_kernel" in _name(B.sb)
        assert (B.hh, B.ww) == (B.ho, B.wo) == (4, 4)
    names = [e[0] for e in pl.fwd if e is not None]
    assert names.count("x3d_dw3d_fwd_dil") == len(last) and names.count("x3d_dw3d_fwd") == len(pl.blocks) - len(last)
    assert (pl.h5, pl.w5) == (4, 4)


def test_train_step_fp32_against_the_dilated_oracle(gpu, monkeypatch):
    """X3D-XS, RES5_DILATION = 2, 2 clips of 4 x 64 x 64, 5 classes: test_model_gpu's fp32 training-step comparison -- activations,
    logits, probabilities, moving statistics, the ReLU sign patterns, loss, every gradient and the Nesterov update against
    oracle.forward / oracle.train_step -- at that test's limits, the oracle's channelwise convs of the last stage dilated."""
    from tests import test_model_gpu as M
    arch = _dilated_oracle(monkeypatch, DIL)
    pl = M._train_step_fp32(gpu, *XS_STEP, DIL)
    _check_plan_is_dilated(pl, arch)
    assert all("dw3d_dil_bwd_kernel" in _name(B.db) for B in pl.blocks if B.spec.dilation == 2)


def test_train_step_fp32_needs_the_dilated_oracle(gpu):
    """the same step against the oracle WITHOUT the dilation must fail: the comparison above is not vacuous"""
    from tests import test_model_gpu as M
    with pytest.raises(AssertionError):
        M._train_step_fp32(gpu, *XS_STEP, DIL)


def test_train_step_bf16_against_the_dilated_oracle(gpu, monkeypatch):
    """the same model in bf16 storage: test_model_gpu's teacher-forced block-by-block comparison (its docstring says why 16-bit
    storage cannot be compared end to end) at that test's limits -- activations and input gradients 2 % of each tensor's
    maximum, weight gradients 7.5e-2 relative L2 (8e-2 for the SE biases), median 1.5e-2 -- with oracle.res_block replaying the
    dilated blocks through DilatedStorage (fp32 operands at those sites: the dilated kernels have no matrix-core form)."""
    from tests import test_model_gpu as M
    arch = _dilated_oracle(monkeypatch, DIL)
    pl = M._train_step_half(gpu, *XS_STEP, torch.bfloat16, DIL)
    _check_plan_is_dilated(pl, arch)


def test_inference_against_the_dilated_oracle(gpu):
    import x3d_tf_amd as x
    from oracle import x3d_oracle as O
    from tests import test_model_gpu as M
    over = DIL + ["TEST.NUM_TEMPORAL_VIEWS", 2, "TEST.NUM_SPATIAL_CROPS", 1]
    cfg, arch, params = M._setup("XS", over)
    x_ = torch.randn(4, 4, 64, 64, 3, generator=torch.Generator().manual_seed(0))
    ref, ref_logits = O.forward(params, x_, arch, training=False, return_logits=True,
                                storage=R.DilatedStorage(None, sites=R.dilated_sites(arch)))
    m = M._model(cfg, params, torch.float32, gpu)
    out = m(x_.to(gpu), training=False)
    torch.cuda.synchronize()
    pl = m._plans[(4, 4, 64, 64, False)]
    assert tuple(out.shape) == (2, 5) and (pl.h5, pl.w5) == (4, 4)
    assert all(B.sb.dilation == (2 if B.spec.stage == 3 else 1) for B in pl.blocks)
    M._scaled("logits", pl.logits, ref_logits, 1e-4)
    report("probs", out, ref, 0, 1e-4)
    dense = O.forward(params, x_, arch, training=False)       # the same stride-1 stage without the dilation: told apart
    with pytest.raises(AssertionError):
        report("probs", out, dense, 0, 1e-4)


DET = S.DILATED_DETECTION


def test_detection_step_on_the_stride_16_map(gpu):
    """DETECTION.ENABLE on the dilated model, SPATIAL_SCALE_FACTOR 16, a 64^2 clip (conv5 map 4 x 4), K = 2: the head restated in
    fp64 on the plan's own trunk output, as tests/test_roi_head_gpu.py test_model_step_matches_the_head_restated_in_fp64 does, at
    its limits (loss 1e-5, probabilities 1e-4, dlogits 1e-6 of their maximum, dpooled / gradients / g5 1e-3 relative L2)."""
    from tests import roi_ref
    from tests import test_roi_head_gpu as H
    kb, s, nb = 2, 64, [2, 0]
    cfg, arch, params = H._setup(DET)
    n, t, classes, rows = 2, 4, arch.num_classes, 2 * kb
    g = torch.Generator().manual_seed(1)
    clips = torch.randn(n, t, s, s, 3, generator=g)
    boxes = roi_ref.box_mix(n, kb, s, s, seed=2)
    labels = torch.randint(0, classes, (n, kb), generator=g)
    mask = (torch.rand(rows, arch.fc1_out, generator=g) >= arch.dropout_rate).float()
    m = H._model(cfg, params, gpu)
    _detection_step(m, clips, boxes, nb, labels, mask)


def _detection_step(m, clips, boxes, nb, labels, mask, scale=1.0 / 16):
    """one forward_backward of the live detection model `m` with the head restated in fp64 on the plan's own trunk output and on
    the parameters the device holds at that moment; returns the plan"""
    import numpy as np
    from tests import roi_ref
    from tests import test_roi_head_gpu as H
    arch, gpu = m.arch, m.device
    n, t, kb = clips.shape[0], clips.shape[1], m.det.max_boxes
    classes, rows = arch.num_classes, n * kb
    torch.cuda.synchronize()
    params = {k: m.params[k].detach().cpu().clone() for k in ("fc1/kernel", "fc2/kernel", "fc2/bias")}
    valid = (torch.arange(kb).view(1, kb) < torch.tensor(nb).view(n, 1)).reshape(-1)
    m.set_dropout_mask(mask)
    pl = m.forward_backward(clips.to(gpu), labels, boxes=torch.from_numpy(boxes), num_boxes=nb)
    torch.cuda.synchronize()
    assert (pl.h5, pl.w5) == (4, 4) and tuple(pl.c5_raw.shape) == (n, arch.conv5_out, t, 4, 4) and pl.rows == rows
    c5, ss = pl.c5_raw.cpu().double().numpy(), pl.bn5.ss.cpu().double().numpy()
    am = pl.roi_argmax.cpu().numpy().astype(np.int64)
    _, bins, _, ref_valid = roi_ref.forward(c5, ss, boxes, nb, 7, 0, scale)
    assert not ref_valid[~valid.numpy()].any() and ref_valid.any()
    pooled = torch.from_numpy(np.take_along_axis(bins, am[:, :, None], 2)[:, :, 0]).requires_grad_(True)
    assert (pl.pooled.cpu().double() - pooled.detach()).abs().max().item() <= 1e-4
    w1 = params["fc1/kernel"].double().reshape(arch.fc1_out, arch.conv5_out).requires_grad_(True)
    w2 = params["fc2/kernel"].double().reshape(classes, arch.fc1_out).requires_grad_(True)
    b2 = params["fc2/bias"].double().requires_grad_(True)
    dscale = 1.0 / (1.0 - arch.dropout_rate) if arch.dropout_rate > 0 else 1.0
    z = (torch.relu(pooled @ w1.T) * (mask.double() * dscale if arch.dropout_rate > 0 else 1.0)) @ w2.T + b2
    z.retain_grad()
    per_row = torch.nn.functional.cross_entropy(z, labels.view(rows), reduction="none")
    loss = per_row[valid].sum() / int(valid.sum())
    loss.backward()
    assert abs(pl.loss_rows.double().sum().item() / rows - loss.item()) <= 1e-5
    assert (pl.probs.cpu().double() - torch.softmax(z, 1).detach()).abs().max().item() <= 1e-4
    dl = pl.dlogits.cpu().double()
    assert (dl - z.grad).abs().max().item() <= 1e-6 * z.grad.abs().max().item() + 1e-30
    assert H._rel_l2(pl.backward.dpooled.cpu().double(), pooled.grad) < 1e-3
    for name, ref in (("fc1/kernel", w1.grad), ("fc2/kernel", w2.grad), ("fc2/bias", b2.grad)):
        assert H._rel_l2(m.grads[name].cpu().reshape(ref.shape), ref) < 1e-3, name
    g5_ref, _ = roi_ref.backward(pooled.grad.numpy(), am, boxes, nb, c5, ss, 7, 0, scale)
    g5 = pl.backward.g5.cpu().double()
    assert H._rel_l2(g5, torch.from_numpy(g5_ref)) < 1e-3
    for i in range(n):        # an image without a box sends nothing into the trunk
        assert (g5[i] != 0).any() if nb[i] else (g5[i] == 0).all(), f"g5 of image {i} with {nb[i]} boxes"
    # the trunk's gradients are alive down to the stem
    assert torch.isfinite(m.flat_grads).all() and m.grads["conv1/conv_s/kernel"].abs().sum().item() > 0
    return pl


def test_dilation_one_checkpoint_loads_into_the_dilated_model(gpu, tmp_path):
    """save_weights of a RES5_DILATION = 1 model -> load_weights of a RES5_DILATION = 2 model: every tensor arrives (the weights
    keep their shapes), and the loaded model computes what a dilated model built from the same parameters computes"""
    from tests import test_model_gpu as M
    from x3d_tf_amd.model import X3D
    views = ["TEST.NUM_TEMPORAL_VIEWS", 2, "TEST.NUM_SPATIAL_CROPS", 1, "NETWORK.NUM_CLASSES", 5]
    cfg1, _, params = M._setup("XS", views)
    cfg2, _, _ = M._setup("XS", views + ["NETWORK.RES5_DILATION", 2])
    m1 = M._model(cfg1, params, torch.float32, gpu)
    prefix = str(tmp_path / "ckpt" / "model")
    m1.save_weights(prefix)
    m2 = X3D(cfg2, dtype=torch.float32, device=gpu, seed=123)
    m2.load_weights(str(tmp_path / "ckpt"))
    assert set(m1.params) == set(m2.params)
    for k in m1.params:
        assert m1.params[k].shape == m2.params[k].shape and torch.equal(m1.params[k], m2.params[k]), k
    x_ = torch.randn(2, 4, 64, 64, 3, generator=torch.Generator().manual_seed(0)).to(gpu)
    ref = M._model(cfg2, params, torch.float32, gpu)(x_).clone()
    assert torch.equal(m2(x_), ref) and not torch.equal(m1(x_), ref)


def test_switch_off_keeps_the_bits(gpu):
    """RES5_DILATION = 1 against a config without the key, one training step each on the same inputs.  Bit for bit: logits,
    probabilities, the loss rows and dlogits.  The weight gradients cannot be compared bit for bit on this library: wherever
    several workgroups add into one gradient element they do so with fp32 atomics, in the order the hardware schedules them,
    and two steps of ONE model on the same batch already differ (measured on an MI355X with the model of this test, the config
    without the key run twice: 19 .. 21 of the 308 tensors differ, by at most 3.7e-7 of the tensor's largest element; the set
    changes from run to run).  What the two configs must share is therefore stated where it is exact -- the launch lists are
    identical entry by entry, kernel by kernel (tests/test_dilated_res5.py, test_key_at_one_records_the_list_of_a_config_without_it)
    -- and here every gradient tensor is held to the reordering of an fp32 sum: 2^-20 of its largest element (partial sums of
    at most a few hundred workgroups, each rounded at 2^-24 of the running sum: sqrt(256) * 2^-24 = 2^-20), and at least
    nine tenths of the tensors to the bits."""
    import x3d_tf_amd as x
    from tests import test_model_gpu as M
    over = ["NETWORK.NUM_CLASSES", 5]
    cfg1, arch, params = M._setup("XS", over + ["NETWORK.RES5_DILATION", 1])
    absent = x.get_config("XS", over)
    assert "RES5_DILATION" not in dict(absent.NETWORK) and dict(cfg1.NETWORK)["RES5_DILATION"] == 1
    g = torch.Generator().manual_seed(3)
    clips = torch.randn(2, 4, 64, 64, 3, generator=g).to(gpu)
    labels = torch.randint(0, 5, (2,), generator=g).to(gpu)
    mask = (torch.rand(2, arch.fc1_out, generator=g) >= arch.dropout_rate).float()
    got = []
    for cfg in (cfg1, absent):
        m = M._model(cfg, params, torch.float32, gpu)
        m.set_dropout_mask(mask)
        pl = m.forward_backward(clips, labels)
        torch.cuda.synchronize()
        got.append(((pl.logits.clone(), pl.probs.clone(), pl.loss_rows.clone(), pl.dlogits.clone()),
                    {k: v.clone() for k, v in m.grads.items()}))
    for a, b in zip(got[0][0], got[1][0]):
        assert torch.equal(a, b) and torch.isfinite(a).all()
    same = 0
    for k, a in got[0][1].items():
        b = got[1][1][k]
        assert torch.isfinite(a).all()
        same += int(torch.equal(a, b))
        assert (a - b).abs().max().item() <= 2.0 ** -20 * b.abs().max().item(), k
    print(f"{same} of {len(got[0][1])} gradient tensors bit for bit")
    assert same >= 0.9 * len(got[0][1]) and any(v.abs().sum().item() > 0 for v in got[0][1].values())
