"""Fine-tuning on the device: x3d_seg_grad_sumsq and the x3d_*_pt entry points (frozen tensors, per-tensor learning rates)
against the existing entry points of the same rules -- bit for bit -- and the fp64 references of test_layerwise_gpu.py /
test_solver_gpu.py, and the Trainer paths built on them (SOLVER.FREEZE / LR_MULT / LAYER_DECAY).

Kernel-level layout: solver_cases._fix (segments of 1 ... 2 * SWEEP + 4099 elements, NaN padding).  The tuned table drops
segments 1, 5 and 12 -- a non-l2, an l2 and the all-zero-g segment -- and keeps the largest; the dropped segments' gradient
holds NaN and inf, so a kernel that read a frozen tensor would spread them and one that wrote it would change its bits."""
import json
import os
import sys

import numpy as np
import pytest
import torch
import torch.multiprocessing as mp

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from tests.solver_cases import F32, GS, LAMB, LARS, LENGTHS, SEG_ADAM as ADAM, SGD, U, _bits, _coef, _dirty, _fix, _np  # noqa: E402
from tests.test_layerwise_gpu import (MODES, _adamw_ref, _check_ema, _extras, _free_port, _lamb_ref, _lars_ref,  # noqa: E402
                                      _q_limit)
from tests.test_solver_gpu import OPTS, _batches, _sgd_ref  # noqa: E402

RULES = ["sgd", "adam", "lars", "adamw", "lamb"]
DROPPED = (1, 5, 12)
SCALES = (0.125, 0.31640625, 1.0, 10.0)            # exact in fp32; 0.31640625 = 0.75 ** 4
WD = F32(5e-5)                                     # the coupled L2 term of sgd / adam (solver_cases.SGD["wd"])
DECAY = dict(adamw=F32(0.05), lamb=F32(0.01))      # the decoupled decay, as test_adamw / test_lamb
EMA_DECAY = float(F32(0.9))


def _p(t):
    return None if t is None else t.data_ptr()


class _Tuned:
    pass


_TUNED = {}


def _tuned(f, gpu):
    """the tuned table over _fix's layout (built once): segments, seeded scales, cover arrays, the gradient with NaN / inf in
    the dropped segments"""
    if _TUNED:
        return _TUNED["t"]
    from x3d_tf_amd.segments import SegTable
    t = _Tuned()
    t.keep = [k for k in range(len(LENGTHS)) if k not in DROPPED]
    assert int(np.argmax(LENGTHS)) in t.keep
    t.segs = [f.segs[k] for k in t.keep]
    t.table = SegTable(t.segs).to(gpu)
    rng = np.random.default_rng(11)
    t.scales = np.asarray(SCALES, F32)[rng.integers(0, len(SCALES), len(t.segs))]
    t.scales[int(np.argmax([n for _, n, _ in t.segs]))] = F32(0.31640625)          # the largest: a scale that rounds lr * s
    assert set(t.scales.tolist()) == set(SCALES)
    t.d_scales = torch.from_numpy(t.scales).to(gpu)
    t.cover = np.zeros(f.n, bool)
    for o, n, _ in t.segs:
        t.cover[o:o + n] = True
    t.g = f.g.copy()
    for j, k in enumerate(DROPPED):
        o, n, _ = f.segs[k]
        t.g[o:o + n] = (np.nan, np.inf, -np.inf)[j]
    t.nelem = int(t.cover.sum())
    g64 = f.g.astype(np.float64)
    t.sumsq = float(np.sum(g64[t.cover] ** 2))
    t.norm_total = float(np.sqrt(t.sumsq) * float(GS))
    _TUNED["t"] = t
    return t


def _slots(rule):
    return 1 if rule in ("sgd", "lars") else 2


def _buffers(f, rule, gpu, g=None, off=0):
    """dirty device copies of w, the rule's slots and g: ([tensors], [their host starts], g tensor, its host start)"""
    arrs = [f.w, f.v] + ([f.v2] if _slots(rule) == 2 else [])
    pairs = [_dirty(f, a, gpu, off) for a in arrs]
    gd, g_was = _dirty(f, f.g if g is None else g, gpu, off)
    return [p[0] for p in pairs], [p[1] for p in pairs], gd, g_was


def _run_pt(rule, bufs, gd, table, scale, kw, lr=None, q=None):
    """the _pt entry point of `rule` through its ops wrapper; returns q (lars, lamb) or None"""
    from x3d_tf_amd import ops
    if rule == "sgd":
        h = SGD
        return ops.sgd_pt(bufs[0], bufs[1], gd, table, scale, h["lr"] if lr is None else lr, h["mom"], WD, **kw)
    if rule == "adam":
        h = ADAM
        return ops.adam_pt(bufs[0], bufs[1], bufs[2], gd, table, scale, h["lr"] if lr is None else lr, h["step"], h["b1"], h["b2"],
                           h["eps"], WD, **kw)
    if rule == "lars":
        h = LARS
        return ops.lars_pt(bufs[0], bufs[1], gd, table, scale, h["lr"] if lr is None else lr, h["mom"], h["wd"], h["eta"],
                           h["eps"], True, q=q, **kw)
    if rule == "adamw":
        h = ADAM
        return ops.adamw_pt(bufs[0], bufs[1], bufs[2], gd, table, scale, h["lr"] if lr is None else lr, h["step"], h["b1"], h["b2"],
                            h["eps"], DECAY["adamw"], **kw)
    h = LAMB
    return ops.lamb_pt(bufs[0], bufs[1], bufs[2], gd, table, scale, h["lr"] if lr is None else lr, h["step"], h["b1"], h["b2"],
                       h["eps"], DECAY["lamb"], q=q, **kw)


def _run_existing(rule, bufs, gd, segs, table, kw, lr=None, mask=None):
    """the existing entry point of `rule` on `segs`: x3d_sgd_nesterov_ex / x3d_adam_ex segment by segment (their byte mask
    built from the l2 flags), x3d_lars / x3d_adamw / x3d_lamb on `table`"""
    from x3d_tf_amd import hip, ops
    norm, ema = kw.get("norm"), kw.get("ema")
    tail = (_p(norm), float(kw.get("max_norm", 0.0)))
    ed = float(kw.get("ema_decay", 0.0))
    if rule == "sgd":
        h = SGD
        for o, n, _ in segs:
            hip.call("x3d_sgd_nesterov_ex", bufs[0][o:].data_ptr(), bufs[1][o:].data_ptr(), gd[o:].data_ptr(), mask[o:].data_ptr(),
                     float(h["lr"] if lr is None else lr), float(h["mom"]), float(WD), float(GS), *tail,
                     None if ema is None else ema[o:].data_ptr(), ed, n)
        return None
    if rule == "adam":
        h = ADAM
        for o, n, _ in segs:
            hip.call("x3d_adam_ex", bufs[0][o:].data_ptr(), bufs[1][o:].data_ptr(), bufs[2][o:].data_ptr(), gd[o:].data_ptr(),
                     mask[o:].data_ptr(), float(h["lr"] if lr is None else lr), float(h["b1"]), float(h["b2"]), float(h["eps"]),
                     float(WD), float(GS), h["step"], *tail, None if ema is None else ema[o:].data_ptr(), ed, n)
        return None
    if rule == "lars":
        h = LARS
        return ops.lars(bufs[0], bufs[1], gd, table, h["lr"] if lr is None else lr, h["mom"], h["wd"], h["eta"], h["eps"], True,
                        **kw)
    if rule == "adamw":
        h = ADAM
        return ops.adamw(bufs[0], bufs[1], bufs[2], gd, table, h["lr"] if lr is None else lr, h["step"], h["b1"], h["b2"], h["eps"],
                         DECAY["adamw"], **kw)
    h = LAMB
    return ops.lamb(bufs[0], bufs[1], bufs[2], gd, table, h["lr"] if lr is None else lr, h["step"], h["b1"], h["b2"], h["eps"],
                    DECAY["lamb"], **kw)


def _same_bits(a, b, where=None):
    x, y = _bits(_np(a)), _bits(_np(b) if torch.is_tensor(b) else b)
    return np.array_equal(x, y) if where is None else np.array_equal(x[where], y[where])


# ---- identity: lr_scale NULL / all ones over the full table = the existing entry point, bit for bit -----------------------
@pytest.mark.gpu
@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("rule", RULES)
def test_pt_over_all_segments_is_the_existing_entry_point_bit_for_bit(gpu, rule, mode):
    f = _fix(gpu)
    mask = torch.from_numpy(f.l2e.astype(np.uint8)).to(gpu)
    ones = torch.ones(len(LENGTHS), dtype=torch.float32, device=gpu)
    runs = []
    for which in ("existing", None, ones):
        kw, _, ed, _ = _extras(f, mode, gpu)                                       # a fresh EMA buffer per run
        bufs, was, gd, g_was = _buffers(f, rule, gpu)
        if isinstance(which, str):
            q = _run_existing(rule, bufs, gd, f.segs, f.table, kw, mask=mask)
        else:
            q = _run_pt(rule, bufs, gd, f.table, which, kw)
        assert _same_bits(gd, g_was)
        runs.append(bufs + ([ed] if ed is not None else []) + ([q] if q is not None else []))
    assert len(runs[0]) == _slots(rule) + 1 + (mode == "clip_active_ema") + (rule in ("lars", "lamb"))
    for name, other in (("lr_scale = NULL", runs[1]), ("lr_scale = 1", runs[2])):
        for k, (a, b) in enumerate(zip(runs[0], other)):
            assert _same_bits(a, b), (rule, mode, name, k)
    assert not _same_bits(runs[0][0], was[0], f.covered)                          # (and something was updated)


# ---- scaled and frozen --------------------------------------------------------------------------------------------------
def _reference(rule, f, t, c):
    """per tuned segment, the fp64 reference of the rule at lr' = fl32(lr * s_t): [(offset, n, (w', slots...), limits, q, rel q)]"""
    out = []
    for (o, n, l2), s in zip(t.segs, t.scales):
        sl = slice(o, o + n)
        seg = [(0, n, l2)]
        if rule in ("sgd", "lars"):
            h = SGD if rule == "sgd" else LARS
            lr = F32(F32(h["lr"]) * s)
            if rule == "sgd":
                wn, vn, lim = _sgd_ref(f.w[sl], f.v[sl], f.g[sl], float(l2), c, dict(lr=lr, mom=h["mom"], wd=WD))
                out.append((o, n, (wn, vn), (lim, lim), None, None))
            else:
                wn, vn, lim, q = _lars_ref(f.w[sl], f.v[sl], f.g[sl], seg, c, True, dict(LARS, lr=lr))
                out.append((o, n, (wn, vn), (lim, lim), q[0], _q_limit([n])[0]))
        elif rule in ("adam", "adamw"):
            # adam: the coupled term is off in this reference, so that run passes weight_decay = 0 (with it on, the bits are
            # held to x3d_adam_ex below, which test_solver_gpu.py holds to its own fp64 reference)
            lr = F32(F32(ADAM["lr"]) * s)
            dec = DECAY["adamw"] if rule == "adamw" else F32(0.0)
            want, lims = _adamw_ref(f.w[sl], f.v[sl], f.v2[sl], f.g[sl], np.full(n, float(l2)), c, dec, dict(ADAM, lr=lr))
            out.append((o, n, want, lims, None, None))
        else:
            lr = F32(F32(LAMB["lr"]) * s)
            want, lims, q, rel_q = _lamb_ref(f.w[sl], f.v[sl], f.v2[sl], f.g[sl], seg, c, DECAY["lamb"], dict(LAMB, lr=lr))
            out.append((o, n, want, lims, q[0], rel_q[0]))
    return out


@pytest.mark.gpu
@pytest.mark.parametrize("rule", RULES)
def test_scaled_and_frozen(gpu, rule):
    """clipping active and EMA on; the norm is x3d_seg_grad_sumsq's over the tuned table, on a gradient whose dropped segments
    hold NaN / inf"""
    from x3d_tf_amd import ops
    from x3d_tf_amd.segments import SegTable
    f = _fix(gpu)
    t = _tuned(f, gpu)
    bufs, was, gd, g_was = _buffers(f, rule, gpu, g=t.g)
    ed, e_was = _dirty(f, f.e, gpu)
    norm = ops.seg_grad_sumsq(gd, t.table)
    assert _np(norm)[1] == 0.0
    max_norm = 0.5 * t.norm_total
    c = _coef(_np(norm)[0], GS, max_norm)
    assert c < float(GS)
    kw = dict(grad_scale=float(GS), norm=norm, max_norm=max_norm, ema=ed, ema_decay=EMA_DECAY)
    if rule == "adam":                                                             # the fp64 run: coupled term off (_reference)
        from x3d_tf_amd import ops as _ops
        h = ADAM
        _ops.adam_pt(bufs[0], bufs[1], bufs[2], gd, t.table, t.d_scales, h["lr"], h["step"], h["b1"], h["b2"], h["eps"], 0.0, **kw)
        q = None
    else:
        q = _run_pt(rule, bufs, gd, t.table, t.d_scales, kw)
    got = [_np(b) for b in bufs]
    for j, (o, n, want, lims, q64, rel_q) in enumerate(_reference(rule, f, t, c)):
        for name, g_, ref, lim in zip("w12", got, want, lims):
            err = np.abs(g_[o:o + n] - ref)
            assert np.all(err <= lim), (rule, j, name, np.max(err / np.maximum(lim, 1e-300)))
        if q64 is not None:
            assert abs(float(_np(q)[j]) - q64) <= rel_q * q64, (rule, j)
    assert q is None or tuple(q.shape) == (len(t.segs),)
    _check_ema(f, ed, got[0], covered=t.cover)
    # dropped segments and all padding: the bits they had, in w, the slots and the EMA; the gradient is read-only
    for name, b, w_ in zip(["w", "slot 1", "slot 2"], bufs + [None], was):
        assert _same_bits(b, w_, ~t.cover), (rule, name)
        assert not np.isnan(_np(b)[t.cover]).any(), (rule, name)
    assert _same_bits(ed, e_was, ~t.cover) and _same_bits(gd, g_was)
    for o, n, _ in t.segs:
        if n > 8:
            assert not _same_bits(bufs[0][o:o + n], was[0][o:o + n]), o
    if rule not in ("sgd", "adam", "adamw"):
        return
    # the elementwise rules: every tuned segment = the existing entry point at lr' = fl32(lr * s_t), bit for bit
    mask = torch.from_numpy(f.l2e.astype(np.uint8)).to(gpu)
    b1, _, _, _ = _buffers(f, rule, gpu, g=t.g)
    e1, _ = _dirty(f, f.e, gpu)
    b2, _, _, _ = _buffers(f, rule, gpu, g=t.g)
    e2, _ = _dirty(f, f.e, gpu)
    _run_pt(rule, b1, gd, t.table, t.d_scales, dict(kw, ema=e1))                   # (adam: with the coupled term this time)
    base = F32((SGD if rule == "sgd" else ADAM)["lr"])
    for s in SCALES:
        segs = [sg for sg, sc in zip(t.segs, t.scales) if sc == F32(s)]
        _run_existing(rule, b2, gd, segs, SegTable(segs).to(gpu) if rule == "adamw" else None, dict(kw, ema=e2),
                      lr=F32(base * F32(s)), mask=mask)
    for k, (a, b) in enumerate(zip(b1 + [e1], b2 + [e2])):
        assert _same_bits(a, b), (rule, k)


@pytest.mark.gpu
def test_alignment_paths_agree_bit_for_bit(gpu):
    """base pointers one float behind a 16-byte boundary: the same elements by the same lanes in the same order"""
    from x3d_tf_amd import ops
    f = _fix(gpu)
    t = _tuned(f, gpu)
    for rule in RULES:
        res = []
        for off in (0, 1):
            bufs, was, gd, _ = _buffers(f, rule, gpu, g=t.g, off=off)
            ed, _ = _dirty(f, f.e, gpu, off)
            assert bufs[0].data_ptr() % 16 == 4 * off and gd.data_ptr() % 16 == 4 * off
            norm = ops.seg_grad_sumsq(gd, t.table)
            kw = dict(grad_scale=float(GS), norm=norm, max_norm=0.5 * t.norm_total, ema=ed, ema_decay=EMA_DECAY)
            q = _run_pt(rule, bufs, gd, t.table, t.d_scales, kw)
            res.append(bufs + [ed, norm] + ([q] if q is not None else []))
        for k, (a, b) in enumerate(zip(*res)):
            assert _same_bits(a, b), (rule, k)
        assert _same_bits(res[1][0], was[0], ~t.cover) and not _same_bits(res[1][0], was[0], t.cover)


# ---- x3d_seg_grad_sumsq -------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_seg_grad_sumsq(gpu):
    """out[0] against np.sum(g64 ** 2) over the tuned elements: the squares are exact in fp64 and the N - 1 additions of
    non-negative terms round by at most 2^-53 of the total each, in ANY order: relative N * 2^-53 (test_seg_sumsq's argument,
    the sum part of _q_limit).  out[1]: the non-finite entries inside the chunks, counted exactly."""
    from x3d_tf_amd import ops
    f = _fix(gpu)
    t = _tuned(f, gpu)
    gd, g_was = _dirty(f, t.g, gpu)                                                # NaN / inf in the dropped segments and the padding
    out = _np(ops.seg_grad_sumsq(gd, t.table))
    assert out.shape == (2,) and out[1] == 0.0
    assert abs(out[0] - t.sumsq) <= t.nelem * 2.0 ** -53 * t.sumsq, abs(out[0] - t.sumsq) / t.sumsq
    assert _same_bits(ops.seg_grad_sumsq(gd, t.table), out)                        # the same bits on every run
    g1, _ = _dirty(f, t.g, gpu, off=1)                                             # ... and on the one-by-one load path
    assert g1.data_ptr() % 16 == 4
    assert _same_bits(ops.seg_grad_sumsq(g1, t.table), out)
    assert _same_bits(gd, g_was)                                                   # the input is read-only
    # the full table with a finite gradient = what x3d_grad_sumsq counts on the zero-padded buffer, to the same bound
    full = _np(ops.seg_grad_sumsq(_dirty(f, f.g, gpu)[0], f.table))
    flat = _np(ops.grad_sumsq(torch.from_numpy(f.g).to(gpu)))
    assert full[1] == flat[1] == 0.0 and abs(full[0] - flat[0]) <= 2 * f.covered.sum() * 2.0 ** -53 * flat[0]
    # non-finite entries in tuned segments: the first and the last element of segments, a vector lane, the ragged tail, and the
    # largest segment's second grid sweep and very last element
    g = t.g.copy()
    big_o, big_n, _ = t.segs[int(np.argmax([n for _, n, _ in t.segs]))]
    spots = [t.segs[0][0], t.segs[2][0] + 3, t.segs[3][0] + 4, t.segs[5][0] + 256, t.segs[7][0] + 1024,
             big_o + 5, big_o + big_n // 2 + 1, big_o + big_n - 1]
    assert all(t.cover[i] for i in spots) and len(set(spots)) == len(spots)
    for k, i in enumerate(spots):
        g[i] = (np.nan, np.inf, -np.inf)[k % 3]
    out = _np(ops.seg_grad_sumsq(_dirty(f, g, gpu)[0], t.table))
    g64 = g.astype(np.float64)
    fin = t.cover & np.isfinite(g64)
    want = float(np.sum(g64[fin] ** 2))
    assert out[1] == float(len(spots)) and abs(out[0] - want) <= t.nelem * 2.0 ** -53 * want
    # magnitudes whose squares leave the fp32 range in either direction
    for mag in (1e-30, 1e18):
        g3 = (f.g / 1024.0 * mag).astype(F32)
        out3 = _np(ops.seg_grad_sumsq(_dirty(f, g3, gpu)[0], t.table))
        want3 = float(np.sum(g3.astype(np.float64)[t.cover] ** 2))
        assert out3[1] == 0.0 and np.isfinite(out3[0]) and abs(out3[0] - want3) <= t.nelem * 2.0 ** -53 * want3


@pytest.mark.gpu
def test_non_finite_tuned_gradient_skips_every_launch(gpu):
    """norm[1] != 0: w, the slots, ema and q are what they were, bit for bit -- all five rules"""
    from x3d_tf_amd import ops
    f = _fix(gpu)
    t = _tuned(f, gpu)
    g = t.g.copy()
    g[t.segs[4][0] + 7] = np.inf
    gd, g_was = _dirty(f, g, gpu)
    norm = ops.seg_grad_sumsq(gd, t.table)
    assert _np(norm)[1] == 1.0
    for rule in RULES:
        bufs, was, _, _ = _buffers(f, rule, gpu)
        ed, e_was = _dirty(f, f.e, gpu)
        q = torch.full((len(t.segs),), 7.0, dtype=torch.float32, device=gpu)
        kw = dict(grad_scale=float(GS), norm=norm, max_norm=1.0, ema=ed, ema_decay=EMA_DECAY)
        _run_pt(rule, bufs, gd, t.table, t.d_scales, kw, q=q if rule in ("lars", "lamb") else None)
        for b, w_ in zip(bufs + [ed, gd], was + [e_was, g_was]):
            assert _same_bits(b, w_), rule
        assert np.all(_np(q) == F32(7.0))


@pytest.mark.gpu
def test_ops_refuse_a_bad_lr_scale(gpu):
    from x3d_tf_amd import ops
    f = _fix(gpu)
    t = _tuned(f, gpu)
    bufs, _, gd, _ = _buffers(f, "sgd", gpu)
    for bad in (torch.ones(len(t.segs) + 1, device=gpu), torch.ones(len(t.segs), dtype=torch.float64, device=gpu),
                torch.ones(len(t.segs))):
        with pytest.raises(ValueError, match="lr_scale"):
            ops.sgd_pt(bufs[0], bufs[1], gd, t.table, bad, 0.1, 0.9, 0.0)
    with pytest.raises(ValueError, match="the chunk table covers"):
        ops.seg_grad_sumsq(gd[:100], t.table)


# ---- the Trainer: XS, 10 classes, dropout 0, 2 clips of 4 x 32 x 32, fp32 (the shapes of test_solver_gpu.py) ----------------
FREEZE = ["conv1/", "stages/0/", "stages/1/"]
NEW_CALLS = {"x3d_seg_grad_sumsq", "x3d_sgd_pt", "x3d_adam_pt", "x3d_lars_pt", "x3d_adamw_pt", "x3d_lamb_pt"}
PT_OF = dict(sgd="x3d_sgd_pt", adam="x3d_adam_pt", lars="x3d_lars_pt", adamw="x3d_adamw_pt", lamb="x3d_lamb_pt")


def _cfg(opt, *extra):
    import x3d_tf_amd as x
    return x.get_config("XS", OPTS + ["TRAIN.OPTIMIZER", opt, "OPTIM.LARS_TRUST_COEF", 0.02, "OPTIM.WEIGHT_DECAY", 0.01]
                        + list(extra))


def _trainer(cfg, gpu, seed=1, dtype=torch.float32):
    from x3d_tf_amd.model import X3D
    from x3d_tf_amd.train import Trainer
    m = X3D(cfg, dtype=dtype, device=gpu, seed=seed)
    return m, Trainer(m, cfg)


def _seed_slots(m, seed=1):
    """non-zero optimizer slots on every tensor (zero padding): with them a learning rate of 0 would still move the weights"""
    nt = m.n_trainable_flat
    cv = torch.zeros(nt)
    for s in m.segments:
        cv[s.offset:s.offset + s.length] = 1
    v = 0.01 * torch.randn(nt, generator=torch.Generator().manual_seed(seed))
    v[cv == 0] = 0.0                                                               # (+0: a product with 0 would leave -0 here and there)
    m.flat_velocity.copy_(v)
    if getattr(m, "flat_second", None) is not None:
        m.flat_second.copy_(m.flat_velocity.abs() * 0.01)


def _state(m, ema=None):
    nt = m.n_trainable_flat
    out = [m.flat_params[:nt].clone(), m.flat_velocity.clone()]
    if getattr(m, "flat_second", None) is not None:
        out.append(m.flat_second.clone())
    if ema is not None:
        out.append(ema[:nt].clone())
    return out


def _spy(monkeypatch, hip, calls):
    real = hip.call

    def recorder(name, *args):
        calls.append(name)
        return real(name, *args)

    monkeypatch.setattr(hip, "call", recorder)
    return real


@pytest.mark.gpu
@pytest.mark.parametrize("opt", RULES)
def test_the_default_config_makes_the_launches_it_always_made(gpu, opt, monkeypatch):
    """nothing set: none of the new entry points is called, with clipping on too; FREEZE does reach them"""
    from x3d_tf_amd import hip
    (x1, y1), = _batches(1)
    x1, y1 = x1.to(gpu), y1.to(gpu)
    old = dict(sgd="x3d_sgd_nesterov_ex", adam="x3d_adam_ex", lars="x3d_lars", adamw="x3d_adamw", lamb="x3d_lamb")[opt]
    m, tr = _trainer(_cfg(opt, "SOLVER.CLIP_GRAD_L2NORM", 0.05), gpu)
    assert m._ft is None and tr.finetune == (1.0, (), ())
    calls = []
    real = _spy(monkeypatch, hip, calls)
    tr.step(x1, y1, 0.1)
    monkeypatch.setattr(hip, "call", real)
    assert not NEW_CALLS & set(calls) and "x3d_grad_sumsq" in calls and calls[-1] == old
    m, tr = _trainer(_cfg(opt, "SOLVER.CLIP_GRAD_L2NORM", 0.05, "SOLVER.FREEZE", FREEZE), gpu)
    calls.clear()
    real = _spy(monkeypatch, hip, calls)
    tr.step(x1, y1, 0.1)
    monkeypatch.setattr(hip, "call", real)
    assert [c for c in calls if c in NEW_CALLS] == ["x3d_seg_grad_sumsq", PT_OF[opt]] and calls[-1] == PT_OF[opt]
    assert "x3d_grad_sumsq" not in calls and old not in calls
    m.set_finetune()                                                               # cleared: the old launches again
    calls.clear()
    real = _spy(monkeypatch, hip, calls)
    tr.step(x1, y1, 0.1)
    monkeypatch.setattr(hip, "call", real)
    assert not NEW_CALLS & set(calls) and calls[-1] == old


@pytest.mark.gpu
@pytest.mark.parametrize("opt", RULES)
def test_trainer_freeze_with_clipping_and_ema(gpu, opt):
    """two steps with the stem and two stages frozen: their weights, slots and EMA keep their bits, every other tensor moves,
    and the clip norm is the tuned tensors' -- also when a frozen tensor's gradient holds inf / NaN"""
    batches = [(a.to(gpu), b.to(gpu)) for a, b in _batches(2)]
    lr, max_norm = 0.05, 0.05
    m, tr = _trainer(_cfg(opt, "SOLVER.CLIP_GRAD_L2NORM", max_norm, "SOLVER.EMA_DECAY", 0.5, "SOLVER.FREEZE", FREEZE), gpu)
    if tr.slot_kind == "adam":
        m._adam_slots()
    _seed_slots(m)
    frozen = [s for s in m.segments if s.name.startswith(tuple(FREEZE))]
    assert [s.name for s in frozen] == m.frozen_names and len(frozen) > 20
    assert [s for s in m.segments if s not in frozen] == m.tuned_segments and len(m.tuned_segments) > 20
    before = _state(m, tr.ema)
    for a, b in batches:
        tr.step(a, b, lr)
    assert tr.opt_step == 2

    def check(after, what):
        for k, (x0, x1) in enumerate(zip(before, after)):
            for s in frozen:
                sl = slice(s.offset, s.offset + s.length)
                assert torch.equal(x0[sl].view(torch.int32), x1[sl].view(torch.int32)), (what, k, s.name)
            for s in m.tuned_segments:
                sl = slice(s.offset, s.offset + s.length)
                assert not torch.equal(x0[sl], x1[sl]), (what, k, s.name)
            assert bool(torch.isfinite(x1).all()), (what, k)

    check(_state(m, tr.ema), "two steps")
    g64 = _np(m.flat_grads).astype(np.float64)
    tuned = np.zeros(g64.size, bool)
    for s in m.tuned_segments:
        tuned[s.offset:s.offset + s.length] = True
    norm = np.sqrt(np.sum(g64[tuned] ** 2))
    assert abs(float(tr.last_grad_norm.item()) - norm) <= 1e-6 * norm
    assert norm > max_norm and np.sqrt(np.sum(g64 ** 2)) > norm * (1 + 1e-4)       # clipping is active; the frozen part would show
    if opt in ("lars", "lamb"):
        assert tuple(tr.last_trust_ratios.shape) == (len(m.tuned_segments),)
        l2 = np.array([s.l2 for s in m.tuned_segments])
        qd = _np(tr.last_trust_ratios)
        assert np.all(qd[~l2] == 1.0) and np.any(qd[l2] != 1.0)
    # a third update on the same gradient, the frozen tensors' part now inf and NaN: nothing is skipped, nothing spreads
    for k, s in enumerate(frozen):
        m.flat_grads[s.offset:s.offset + s.length] = (float("inf"), float("nan"))[k % 2]
    mid = _state(m, tr.ema)
    tr._update(None, lr)
    assert tr.opt_step == 3 and abs(float(tr.last_grad_norm.item()) - norm) <= 1e-6 * norm
    after = _state(m, tr.ema)
    check(after, "inf / NaN in the frozen gradient")
    assert not torch.equal(mid[0], after[0])


@pytest.mark.gpu
@pytest.mark.parametrize("opt", ["sgd", "adamw", "lamb"])
def test_trainer_layer_decay_is_the_plain_update_at_the_scaled_rate(gpu, opt):
    """LAYER_DECAY 0.75 and fc2 x 10, nothing frozen, clipping off: the tensors that carry scale s end one update with the bits
    a plain trainer gives them at fl32(lr * s), from the same weights, slots and gradient.  (Two runs of the backward pass
    differ in the last bits -- fp32 atomics in some weight gradients -- so the plain trainer is handed the gradient.)"""
    (x1, y1), = _batches(1)
    lr = 0.05
    m, tr = _trainer(_cfg(opt, "SOLVER.LAYER_DECAY", 0.75, "SOLVER.LR_MULT", [["fc2/", 10.0]]), gpu)
    m2, tr2 = _trainer(_cfg(opt), gpu)
    assert m.frozen_names == [] and m.tuned_segments == m.segments == m2.segments and m2._ft is None
    for mm, t_ in ((m, tr), (m2, tr2)):
        if t_.slot_kind == "adam":
            mm._adam_slots()
        _seed_slots(mm)
    start = [x_.clone() for x_ in (m2.flat_params, m2.flat_velocity)] + ([m2.flat_second.clone()] if tr2.slot_kind == "adam" else [])
    assert torch.equal(m.flat_params, m2.flat_params) and torch.equal(m.flat_velocity, m2.flat_velocity)
    tr.step(x1.to(gpu), y1.to(gpu), lr)
    g = m.flat_grads.clone()
    got = _state(m)
    top = len(m.arch.blocks) + 1
    scales = sorted(set(m.lr_scales.values()))
    assert len(scales) == top + 2 and m.lr_scales["fc2/kernel"] == 10.0 and m.lr_scales["fc1/kernel"] == 1.0
    assert m.lr_scales["conv1/conv_s/kernel"] == float(F32(0.75 ** top))
    for s in scales:
        bufs = [m2.flat_params, m2.flat_velocity] + ([m2.flat_second] if tr2.slot_kind == "adam" else [])
        for b, b0 in zip(bufs, start):
            b.copy_(b0)
        m2.flat_grads.copy_(g)
        tr2.opt_step = 0
        tr2._update(None, float(F32(lr) * F32(s)))
        want = _state(m2)
        for seg in m.segments:
            if m.lr_scales[seg.name] != s:
                continue
            sl = slice(seg.offset, seg.offset + seg.length)
            for k, (a, b) in enumerate(zip(got, want)):
                assert torch.equal(a[sl].view(torch.int32), b[sl].view(torch.int32)), (opt, s, seg.name, k)
                assert k > 0 or not torch.equal(a[sl], start[0][sl]), (opt, seg.name)


FT = ["SOLVER.FREEZE", FREEZE, "SOLVER.LAYER_DECAY", 0.9]


@pytest.mark.gpu
def test_trainer_accumulation_is_one_step_on_the_summed_gradient(gpu):
    """ACCUM_STEPS = 2 with FREEZE + LAYER_DECAY: nothing moves after the first micro-batch; after the second the state is, bit
    for bit, one update of a trainer without accumulation on the total `flat_grads` then holds"""
    (x1, y1), (x2, y2) = [(a.to(gpu), b.to(gpu)) for a, b in _batches(2)]
    lr = 0.05
    m, tr = _trainer(_cfg("sgd", "SOLVER.ACCUM_STEPS", 2, "SOLVER.CLIP_GRAD_L2NORM", 0.05, *FT), gpu)
    m2, tr2 = _trainer(_cfg("sgd", "SOLVER.CLIP_GRAD_L2NORM", 0.05, *FT), gpu)
    _seed_slots(m)                                                                 # (with a velocity every tuned tensor moves, a
    _seed_slots(m2)                                                                # BatchNorm scale whose gradient is 0 too)
    start = _state(m)
    tr.step(x1, y1, lr)
    g1 = m.flat_grads.clone()
    assert all(torch.equal(a, b) for a, b in zip(start, _state(m))) and tr.opt_step == 0
    tr.step(x2, y2, lr)
    assert tr.opt_step == 1 and not torch.equal(m.flat_grads, g1)
    m2.flat_grads.copy_(m.flat_grads)
    tr2._update(None, lr)
    after = _state(m)
    for a, b in zip(after, _state(m2)):
        assert torch.equal(a.view(torch.int32), b.view(torch.int32))
    assert torch.equal(tr.last_grad_norm, tr2.last_grad_norm)
    for s in m.segments:
        sl = slice(s.offset, s.offset + s.length)
        assert torch.equal(start[0][sl], after[0][sl]) == (s.name in m.frozen_names), s.name


@pytest.mark.gpu
def test_trainer_fp16_overflow_skips_the_step(gpu):
    """fp16 storage, FREEZE + LAYER_DECAY: an overflowing loss scale skips the step and halves the scale -- decided by the count
    x3d_seg_grad_sumsq leaves, so an inf in a frozen tensor's gradient alone skips nothing"""
    (x1, y1), = _batches(1)
    m, tr = _trainer(_cfg("adamw", *FT), gpu, dtype=torch.float16)
    assert tr.dynamic_scale and tr.loss_scale == 2.0 ** 15 and m._ft is not None
    # the overflowing step comes first: one AdamW step on two clips fits them so well that p - y no longer overflows at 2^40
    m._adam_slots()
    tr.loss_scale = 2.0 ** 40
    before = _state(m)
    tr.step(x1.to(gpu), y1.to(gpu), 0.01)
    assert tr.skipped_steps == 1 and tr.loss_scale == 2.0 ** 39 and tr.opt_step == 0
    assert all(torch.equal(a.view(torch.int32), b.view(torch.int32)) for a, b in zip(before, _state(m)))
    tr.loss_scale = 2.0 ** 15
    tr.step(x1.to(gpu), y1.to(gpu), 0.01)
    assert tr.skipped_steps == 1 and tr.opt_step == 1 and torch.isfinite(m.flat_params).all()
    assert not torch.equal(before[0], _state(m)[0])
    frozen = next(s for s in m.segments if s.name in m.frozen_names)
    m.flat_grads[frozen.offset] = float("inf")
    assert m.grads_finite()
    tr._update(None, 0.01)
    assert tr.skipped_steps == 1 and tr.opt_step == 2 and torch.isfinite(m.flat_params).all()
    tuned = m.tuned_segments[0]
    m.flat_grads[tuned.offset] = float("nan")
    assert not m.grads_finite()


@pytest.mark.gpu
@pytest.mark.parametrize("opt", ["sgd", "lamb"])
def test_checkpoint_resume_continues_bit_for_bit(gpu, opt, tmp_path):
    """save_checkpoint -> a fresh model and trainer -> resume -> one more update = the uninterrupted run, bit for bit (the
    resumed trainer updates on the gradient the uninterrupted one computed: test_layerwise_gpu.py's reason)"""
    (x1, y1), (x2, y2) = [(a.to(gpu), b.to(gpu)) for a, b in _batches(2)]
    lr = 0.05
    cfg = _cfg(opt, "SOLVER.CLIP_GRAD_L2NORM", 0.05, *FT)
    m, tr = _trainer(cfg, gpu)
    if tr.slot_kind == "adam":
        m._adam_slots()
    _seed_slots(m)                                                                 # (with them every tuned tensor moves)
    start = _state(m)
    tr.step(x1, y1, lr)
    tr.save_checkpoint(str(tmp_path), 1)
    tr.step(x2, y2, lr)
    g2, after = m.flat_grads.clone(), _state(m)
    m2, tr2 = _trainer(cfg, gpu, seed=9)
    assert tr2.resume(str(tmp_path)) == 1 and tr2.opt_step == 1 and m2.frozen_names == m.frozen_names
    m2.flat_grads.copy_(g2)
    tr2._update(None, lr)
    assert tr2.opt_step == 2
    for a, b in zip(after, _state(m2)):
        assert torch.equal(a.view(torch.int32), b.view(torch.int32))
    if opt == "lamb":
        assert torch.equal(tr.last_trust_ratios, tr2.last_trust_ratios)
        assert tuple(tr2.last_trust_ratios.shape) == (len(m.tuned_segments),)
    for s in m.segments:                                                           # the checkpoint holds the frozen tensors as they were
        sl = slice(s.offset, s.offset + s.length)
        assert torch.equal(start[0][sl], after[0][sl]) == (s.name in m.frozen_names), s.name


def _rank_worker(rank, world, port, tmp):
    sys.path.insert(0, ROOT)
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world),
                      LOCAL_RANK=str(rank), X3D_DIST_BACKEND="gloo")
    import torch.distributed as dist
    from x3d_tf_amd import dist as xd
    r, lr_, w = xd.init_process_group()
    dev = torch.device(f"cuda:{xd.local_device(lr_)}")
    torch.cuda.set_device(dev)
    x1, y1 = _batches(1, seed=3 + rank)[0]                                          # every rank its own shard
    m, tr = _trainer(_cfg("adamw", "SOLVER.CLIP_GRAD_L2NORM", 0.05, *FT), dev, seed=1 + rank)
    nt = m.n_trainable_flat
    w0 = m.flat_params[:nt].cpu()                                                   # rank 0's variables, broadcast
    tr.step(x1.to(dev), y1.to(dev), 0.05)
    torch.save(dict(w0=w0, w=m.flat_params[:nt].cpu(), m=m.flat_velocity.cpu(), v=m.flat_second.cpu(),
                    norm=tr.last_grad_norm.cpu()), os.path.join(tmp, f"rank{rank}.pt"))
    with open(os.path.join(tmp, f"rank{rank}.json"), "w") as f:
        json.dump(dict(opt_step=tr.opt_step, world=tr.world, frozen=m.frozen_names,
                       segments=[[s.name, s.offset, s.length] for s in m.segments]), f)
    dist.barrier()
    dist.destroy_process_group()


@pytest.mark.gpu
def test_two_ranks_end_an_adamw_step_identical(gpu, tmp_path):
    """the clip norm comes from the all-reduced gradient of the tuned tensors: both ranks hold the same weights and slots, bit
    for bit, and the frozen tensors are untouched on both"""
    mp.spawn(_rank_worker, args=(2, _free_port(), str(tmp_path)), nprocs=2, join=True)
    r0, r1 = (torch.load(tmp_path / f"rank{r}.pt") for r in (0, 1))
    info = json.load(open(tmp_path / "rank0.json"))
    assert info["opt_step"] == 1 and info["world"] == 2 and len(info["frozen"]) > 20
    for k in ("w0", "w", "m", "v", "norm"):
        assert torch.equal(r0[k], r1[k]), k
    assert bool(torch.isfinite(r0["w"]).all()) and float(r0["norm"]) > 0.05
    for name, o, n in info["segments"]:
        same = torch.equal(r0["w0"][o:o + n], r0["w"][o:o + n])
        assert same == (name in info["frozen"]), name
        if name in info["frozen"]:
            assert float(r0["m"][o:o + n].abs().max()) == 0 and float(r0["v"][o:o + n].abs().max()) == 0
