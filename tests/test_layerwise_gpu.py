"""The layer-wise optimizers on the device: x3d_seg_sumsq, x3d_lars, x3d_adamw, x3d_lamb against fp64 host references of the
rules in include/x3d_hip.h, and the Trainer paths built on them (TRAIN.OPTIMIZER = lars | adamw | lamb, OPTIM.*).

u = 2^-24 is the unit roundoff of fp32: one correctly rounded operation is off by at most u times its result.  Every bound
below is derived from the rounding sequence the header documents; the derivations are in the reference functions' docstrings.

Kernel-level layout: the segments cover the vector / element edges (1, 3, 4, 5, 255, 256, 257), chunk - 1 / chunk / chunk + 1,
several chunks plus a ragged tail, and one segment of more than twice what the grid takes in one sweep (1024 workgroups x 4
waves x one chunk), l2 on and off, an all-zero w and an all-zero g segment.  The padding between segments is NaN in every
device buffer: a kernel that read it would spread it, one that wrote it would change its bits."""
import json
import os
import socket
import sys

import numpy as np
import pytest
import torch
import torch.multiprocessing as mp

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from tests.solver_cases import (CHUNK, F32, GS, L2, LAMB, LARS, LENGTHS, SEG_ADAM as ADAM, SWEEP, U, ZERO_G, ZERO_W,  # noqa: E402,F401
                                _bits, _coef, _dirty, _fix, _norm_of, _np)


def _check_untouched_and_finite(f, named):
    """named: (name, device tensor, the dirty host array it started from).  Padding: the bits it had.  Segments: no NaN."""
    for name, t, was in named:
        got = _np(t)
        assert np.array_equal(_bits(got)[~f.covered], _bits(was)[~f.covered]), f"{name}: padding was written"
        assert not np.isnan(got[f.covered]).any(), f"{name}: NaN inside a segment (padding was read)"


def _seg_sums(f, x64, segs=None):
    return np.array([np.sum(x64[o:o + n] ** 2) for o, n, _ in (segs or f.segs)])


def _expand(q, segs, n):
    e = np.ones(n)
    for (o, k, _), qt in zip(segs, q):
        e[o:o + k] = qt
    return e


MODES = ["plain", "clip_active_ema", "clip_inactive"]


def _extras(f, mode, gpu):
    """(kwargs of the ops call, c in fp64, ema device tensor or None, its dirty host start)"""
    if mode == "plain":
        return dict(grad_scale=float(GS)), float(GS), None, None
    norm = _norm_of(f.g, gpu)
    assert _np(norm)[1] == 0.0
    max_norm = 0.5 * f.norm_total if mode == "clip_active_ema" else 2.0 * f.norm_total + 1.0
    c = _coef(_np(norm)[0], GS, max_norm)
    assert (c < float(GS)) == (mode == "clip_active_ema")
    kw = dict(grad_scale=float(GS), norm=norm, max_norm=max_norm)
    if mode != "clip_active_ema":
        return kw, c, None, None
    ed, e_was = _dirty(f, f.e, gpu)
    kw.update(ema=ed, ema_decay=float(F32(0.9)))
    return kw, c, ed, e_was


def _check_ema(f, ed, w_after, e0=None, decay=F32(0.9), covered=None):
    """ema' = ema + (1 - d)(w' - ema) on the device's own w': the subtraction, 1 - d and the FMA round -- 3 u max(|ema|, |w'|),
    inside 4 u (test_solver_gpu.py::test_ema)"""
    d = float(decay)
    covered = f.covered if covered is None else covered
    e0 = (f.e if e0 is None else e0).astype(np.float64)
    want = d * e0 + (1.0 - d) * w_after.astype(np.float64)
    lim = 4 * U * np.maximum(np.abs(e0), np.abs(w_after))
    assert np.all((np.abs(_np(ed) - want) <= lim)[covered])


def _q_limit(lengths):
    """q_t is two fp64 segment sums (each within len 2^-53 relative, any order: test_grad_sumsq's argument), one fp64 sqrt of
    each (halves that, adds 2^-53), a handful of fp64 products, sums and one division (2^-53 each) and ONE rounding to fp32
    (u).  The reference is the same formula on numpy's fp64 sums (the same bound) with the UNROUNDED clip coefficient c where
    the kernel holds c in fp32 (u more, at most).  Relative: 2 u + 2 (len + 16) 2^-53."""
    return 2 * U + 2.0 * (np.asarray(lengths, np.float64) + 16) * 2.0 ** -53


# ---- x3d_seg_sumsq ----------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_seg_sumsq(gpu):
    """each segment against np.sum(x64 ** 2): the squares are exact in fp64, the len - 1 additions round by at most 2^-53 of a
    partial sum <= the total (non-negative terms), in ANY order: relative len * 2^-53 (test_grad_sumsq's argument)"""
    from x3d_tf_amd import ops
    f = _fix(gpu)
    gd, g_was = _dirty(f, f.g, gpu)
    out = _np(ops.seg_sumsq(gd, f.table))
    want = _seg_sums(f, f.g.astype(np.float64))
    lens = np.array(LENGTHS, np.float64)
    assert out.shape == (len(LENGTHS),) and not np.isnan(out).any()
    assert np.all(np.abs(out - want) <= lens * 2.0 ** -53 * want), np.max(np.abs(out - want) / np.maximum(want, 1e-300))
    assert out[ZERO_G] == 0.0
    assert np.array_equal(_bits(_np(ops.seg_sumsq(gd, f.table))), _bits(out))       # the same bits on every run
    g1, _ = _dirty(f, f.g, gpu, off=1)                                             # ... and on the one-by-one load path
    assert g1.data_ptr() % 16 == 4
    assert np.array_equal(_bits(_np(ops.seg_sumsq(g1, f.table))), _bits(out))
    assert np.array_equal(_bits(_np(gd)), _bits(g_was))                            # the input is read-only
    # magnitudes whose squares leave the fp32 range in either direction
    for mag in (1e-30, 1e18):
        g3 = (f.g / 1024.0 * mag).astype(F32)
        out3 = _np(ops.seg_sumsq(_dirty(f, g3, gpu)[0], f.table))
        want3 = _seg_sums(f, g3.astype(np.float64))
        assert np.all(np.isfinite(out3)) and np.all(np.abs(out3 - want3) <= lens * 2.0 ** -53 * want3)


# ---- LARS -------------------------------------------------------------------------------------------------------------
def _lars_ref(w, v, g, segs, c, clip, hp=LARS):
    """fp64 LARS with the fp32 hyper-parameters the ABI passes; returns w', v', the limit (both) and q.

    With G = q (|c g| + 2 wd |w|) (>= |g'| and every intermediate of it) the kernel rounds, on the way to g': c, q, g c, the
    FMA that adds 2 wd w, the product with q -- 5 u G; an error in g' reaches v' with lr and w' with lr (1 + mom) < 2 lr.
    Then lr g' (u lr G, into v'; into w' times mom), the FMA mom v - lr g' (u (|mom v| + lr G), into w' times mom), the FMA
    w + mom v' (u (|w| + |mom v| + lr G)) and the FMA - lr g' (u (|w| + |mom v| + 2 lr G)).
      |dv| <= u (7 lr G + |mom v|),  |dw| <= u (15 lr G + 3 |mom v| + 2 |w|):  both <= 16 u (|w| + |mom v| + lr G)."""
    lr, mom, wd, eta, eps = (float(F32(hp[k])) for k in ("lr", "mom", "wd", "eta", "eps"))
    w, v, g = (a.astype(np.float64) for a in (w, v, g))
    lam = 2.0 * wd
    sw, sg = _seg_sums(None, w, segs), _seg_sums(None, g, segs)
    q = np.ones(len(segs))
    for t, (_, _, l2) in enumerate(segs):
        if l2 and sw[t] > 0 and sg[t] > 0:
            nw, ng = np.sqrt(sw[t]), np.sqrt(sg[t])
            q[t] = eta * nw / (c * ng + lam * nw + eps)
            if clip:
                q[t] = min(q[t] / lr, 1.0)
    qe = _expand(q, segs, w.size)
    l2e = np.zeros(w.size)
    for o, n, l2 in segs:
        l2e[o:o + n] = l2
    gi = qe * (c * g + lam * w * l2e)
    G = qe * (np.abs(c * g) + lam * np.abs(w) * l2e)
    vn = mom * v - lr * gi
    wn = w + mom * vn - lr * gi
    return wn, vn, 16 * U * (np.abs(w) + np.abs(mom * v) + lr * G), q


def _run_lars(f, gpu, kw, clip, off=0, q0=1.0):
    from x3d_tf_amd import ops
    (wd_, w_was), (vd, v_was), (gd, g_was) = (_dirty(f, a, gpu, off) for a in (f.w, f.v, f.g))
    q = torch.full((len(LENGTHS),), q0, dtype=torch.float32, device=gpu)
    h = LARS
    ops.lars(wd_, vd, gd, f.table, h["lr"], h["mom"], h["wd"], h["eta"], h["eps"], clip, q=q, **kw)
    return (wd_, w_was), (vd, v_was), (gd, g_was), q


@pytest.mark.gpu
@pytest.mark.parametrize("clip", [False, True], ids=["", "lars_clip"])
@pytest.mark.parametrize("mode", MODES)
def test_lars(gpu, mode, clip):
    f = _fix(gpu)
    kw, c, ed, e_was = _extras(f, mode, gpu)
    (wd_, w_was), (vd, v_was), (gd, g_was), q = _run_lars(f, gpu, kw, clip)
    wn, vn, lim, q64 = _lars_ref(f.w, f.v, f.g, f.segs, c, clip)
    qd = _np(q).astype(np.float64)
    assert np.all(np.abs(qd - q64) <= _q_limit(LENGTHS) * q64), np.max(np.abs(qd - q64) / q64)
    for t, l2 in enumerate(L2):
        if not l2 or t in (ZERO_W, ZERO_G):
            assert _np(q)[t] == F32(1.0), t                                         # exactly 1.0f
    if clip:
        assert np.any(q64 == 1.0) and np.any(q64[np.array(L2)] < 1.0)               # LARC clipped some and not others
    cv = f.covered
    assert np.all((np.abs(_np(wd_) - wn) <= lim)[cv]), np.max((np.abs(_np(wd_) - wn) / np.maximum(lim, 1e-300))[cv])
    assert np.all((np.abs(_np(vd) - vn) <= lim)[cv]), np.max((np.abs(_np(vd) - vn) / np.maximum(lim, 1e-300))[cv])
    assert not np.array_equal(_bits(_np(wd_))[cv], _bits(w_was)[cv])
    assert np.array_equal(_bits(_np(gd)), _bits(g_was))                             # flat_grads is read-only
    named = [("w", wd_, w_was), ("v", vd, v_was)]
    if ed is not None:
        _check_ema(f, ed, _np(wd_))
        named.append(("ema", ed, e_was))
    _check_untouched_and_finite(f, named)


@pytest.mark.gpu
def test_lars_without_l2_segments_is_sgd_nesterov_ex_bit_for_bit(gpu):
    """every segment non-l2: q_t = 1 and the step is x3d_sgd_nesterov_ex's without a mask, on each segment"""
    from x3d_tf_amd import hip, ops
    from x3d_tf_amd.segments import SegTable
    f = _fix(gpu)
    table = SegTable([(o, n, False) for o, n, _ in f.segs]).to(gpu)
    norm = _norm_of(f.g, gpu)
    max_norm = 0.5 * f.norm_total
    (wd_, _), (vd, _), (gd, g_was), (ed, _) = (_dirty(f, a, gpu) for a in (f.w, f.v, f.g, f.e))
    (w2, _), (v2, _), (e2, _) = (_dirty(f, a, gpu) for a in (f.w, f.v, f.e))
    h = LARS
    q = ops.lars(wd_, vd, gd, table, h["lr"], h["mom"], h["wd"], h["eta"], h["eps"], True, grad_scale=float(GS), norm=norm,
                 max_norm=max_norm, ema=ed, ema_decay=0.9)
    for o, n, _ in f.segs:
        hip.call("x3d_sgd_nesterov_ex", w2[o:].data_ptr(), v2[o:].data_ptr(), gd[o:].data_ptr(), None, float(h["lr"]),
                 float(h["mom"]), float(h["wd"]), float(GS), norm.data_ptr(), float(max_norm), e2[o:].data_ptr(), 0.9, n)
    assert np.all(_np(q) == F32(1.0))
    for a, b in ((wd_, w2), (vd, v2), (ed, e2)):
        assert np.array_equal(_bits(_np(a)), _bits(_np(b)))
    assert np.array_equal(_bits(_np(gd)), _bits(g_was))


# ---- AdamW ------------------------------------------------------------------------------------------------------------
def _adam_core(w, m, v, g, c, hp):
    """fp64 Adam without the L2 term, with the ABI's fp32 hyper-parameters: (m', v', the bias-corrected factor r, dm, dv).

    With G = |c g| (test_solver_gpu.py::_adam_ref, no L2 term):
      m' = b1 m + (1 - b1) c g: roundings of c, g c, b1 m and the FMA: |dm| <= 8 u (|b1 m| + (1 - b1) G)
      v' = b2 v + (1 - b2) (c g)^2: the square doubles the relative error of c g, then (1 - b2) g', the FMA and b2 v round:
           |dv| <= 16 u (|b2 v| + (1 - b2) G^2)"""
    b1, b2 = float(hp["b1"]), float(hp["b2"])
    gi = c * g
    G = np.abs(gi)
    mn = b1 * m + (1.0 - b1) * gi
    vn = b2 * v + (1.0 - b2) * gi * gi
    dm = 8 * U * (np.abs(b1 * m) + (1.0 - b1) * G)
    dv = 16 * U * (np.abs(b2 * v) + (1.0 - b2) * G * G)
    r = np.sqrt(1.0 - b2 ** hp["step"]) / (1.0 - b1 ** hp["step"])
    return mn, vn, r, dm, dv


def _adamw_ref(w, m, v, g, l2e, c, decay, hp=ADAM):
    """fp64 AdamW; returns (w', m', v') and their limits.

    The Adam step is _adam_ref's: w_a = w - lr_t m' / (sqrt(v') + eps), |dw_a| <= 8 u (|w| + |step|) + (step at the worst
    corner of [m' +- dm] x [v' +- dv] - step).  Then w' = FMA(-(lr decay), w, w_a) where l2: lr decay rounds (u lr decay |w|)
    and the FMA rounds (u |w'| <= u (|w_a| + lr decay |w|)): |dw| <= |dw_a| + 2 u (|w_a| + lr decay |w|)."""
    lr, eps = float(hp["lr"]), float(hp["eps"])
    w, m, v, g = (a.astype(np.float64) for a in (w, m, v, g))
    mn, vn, r, dm, dv = _adam_core(w, m, v, g, c, hp)
    lr_t = float(F32(lr * r))
    step = lr_t * mn / (np.sqrt(vn) + eps)
    worst = lr_t * (np.abs(mn) + dm) / (np.sqrt(np.maximum(vn - dv, 0.0)) + eps)
    wa = w - step
    dwa = 8 * U * (np.abs(w) + np.abs(step)) + (worst - np.abs(step))
    ld = lr * float(F32(decay))
    wn = wa - ld * w * l2e
    return (wn, mn, vn), (dwa + 2 * U * (np.abs(wa) + ld * np.abs(w)), dm, dv)


@pytest.mark.gpu
@pytest.mark.parametrize("mode", MODES)
def test_adamw(gpu, mode):
    from x3d_tf_amd import ops
    f = _fix(gpu)
    kw, c, ed, e_was = _extras(f, mode, gpu)
    decay = F32(0.05)
    (wd_, w_was), (md, m_was), (vd, v_was), (gd, g_was) = (_dirty(f, a, gpu) for a in (f.w, f.v, f.v2, f.g))
    h = ADAM
    ops.adamw(wd_, md, vd, gd, f.table, h["lr"], h["step"], h["b1"], h["b2"], h["eps"], decay, **kw)
    want, lims = _adamw_ref(f.w, f.v, f.v2, f.g, f.l2e, c, decay)
    cv = f.covered
    for got, ref, lim, name in zip((wd_, md, vd), want, lims, "wmv"):
        err = np.abs(_np(got) - ref)
        assert np.all((err <= lim)[cv]), (name, np.max((err / np.maximum(lim, 1e-300))[cv]))
    # the decay is there, and on the l2 segments only: against the same step without it
    (w0, _), (m0, _), (v0, _) = (_dirty(f, a, gpu) for a in (f.w, f.v, f.v2))
    ops.adamw(w0, m0, v0, gd, f.table, h["lr"], h["step"], h["b1"], h["b2"], h["eps"], 0.0,
              **{k: v for k, v in kw.items() if k not in ("ema", "ema_decay")})
    # (where lr decay |w| exceeds one ulp of the undecayed result the FMA cannot round back to it; a weight far smaller than its
    # Adam step decays by less than that and may keep its bits)
    same = _bits(_np(w0)) == _bits(_np(wd_))
    moved = float(h["lr"] * decay) * np.abs(f.w) > np.spacing(np.abs(_np(w0)))
    must = cv & f.l2e & moved
    assert np.all(same[cv & ~f.l2e]) and not np.any(same[must])
    assert must.sum() > 0.99 * (cv & f.l2e & (f.w != 0)).sum()
    assert np.array_equal(_bits(_np(gd)), _bits(g_was))
    named = [("w", wd_, w_was), ("m", md, m_was), ("v", vd, v_was)]
    if ed is not None:
        _check_ema(f, ed, _np(wd_))
        named.append(("ema", ed, e_was))
    _check_untouched_and_finite(f, named)


@pytest.mark.gpu
@pytest.mark.parametrize("mode", MODES)
def test_adamw_without_decay_is_adam_ex_bit_for_bit(gpu, mode):
    """decay = 0: x3d_adam_ex with weight_decay = 0 on every segment (the same l2 mask handed over: the term is off)"""
    from x3d_tf_amd import hip, ops
    f = _fix(gpu)
    kw, _, ed, _ = _extras(f, mode, gpu)
    (wd_, _), (md, _), (vd, _), (gd, g_was) = (_dirty(f, a, gpu) for a in (f.w, f.v, f.v2, f.g))
    (w2, _), (m2, _), (v2, _), (e2, _) = (_dirty(f, a, gpu) for a in (f.w, f.v, f.v2, f.e))
    h = ADAM
    ops.adamw(wd_, md, vd, gd, f.table, h["lr"], h["step"], h["b1"], h["b2"], h["eps"], 0.0, **kw)
    mask = torch.from_numpy(f.l2e.astype(np.uint8)).to(gpu)
    norm = kw.get("norm")
    for o, n, _ in f.segs:
        hip.call("x3d_adam_ex", w2[o:].data_ptr(), m2[o:].data_ptr(), v2[o:].data_ptr(), gd[o:].data_ptr(),
                 mask[o:].data_ptr(), float(h["lr"]), float(h["b1"]), float(h["b2"]), float(h["eps"]), 0.0, float(GS),
                 h["step"], None if norm is None else norm.data_ptr(), float(kw.get("max_norm", 0.0)),
                 None if ed is None else e2[o:].data_ptr(), float(kw.get("ema_decay", 0.0)), n)
    for a, b in ((wd_, w2), (md, m2), (vd, v2)) + (((ed, e2),) if ed is not None else ()):
        assert np.array_equal(_bits(_np(a)), _bits(_np(b)))
    assert np.array_equal(_bits(_np(gd)), _bits(g_was))


# ---- LAMB -------------------------------------------------------------------------------------------------------------
def _lamb_ref(w, m, v, g, segs, c, decay, hp=LAMB):
    """fp64 LAMB; returns (w', m', v'), their limits, q and the relative limit of q.

    m', v', dm, dv: _adam_core.  u0 = r m' / (sqrt(v') + eps): r, r m', the sqrt, + eps and the quotient round (5 u |u0|, 6
    taken) and u0 moves with dm, dv, bounded at the worst corner as _adam_ref does; u = FMA(decay, w, u0) rounds once more:
      |du| <= 8 u (|u0| + decay |w|) + (u0 at the worst corner - |u0|).
    q_t = ||w_t|| / ||u_t|| over the DEVICE's u, which is off by du: ||u|| moves by at most ||du|| (triangle inequality), so
      |dq| / q <= ||du_t|| / ||u_t|| + _q_limit  =: rel_q.
    w' = FMA(-(lr q), u, w): lr q rounds, the FMA rounds:
      |dw| <= lr q (|du| + |u| (rel_q + 2 u)) + 2 u (|w| + lr q |u|)."""
    lr, eps, dec = float(hp["lr"]), float(hp["eps"]), float(F32(decay))
    w, m, v, g = (a.astype(np.float64) for a in (w, m, v, g))
    mn, vn, r, dm, dv = _adam_core(w, m, v, g, c, hp)
    l2e = np.zeros(w.size)
    for o, n, l2 in segs:
        l2e[o:o + n] = l2
    u0 = r * mn / (np.sqrt(vn) + eps)
    worst = r * (np.abs(mn) + dm) / (np.sqrt(np.maximum(vn - dv, 0.0)) + eps)
    u = u0 + dec * w * l2e
    du = 8 * U * (np.abs(u0) + dec * np.abs(w) * l2e) + (worst - np.abs(u0))
    sw, su, sdu = _seg_sums(None, w, segs), _seg_sums(None, u, segs), _seg_sums(None, du, segs)
    q, rel_q = np.ones(len(segs)), np.zeros(len(segs))
    base = _q_limit([n for _, n, _ in segs])
    for t, (_, _, l2) in enumerate(segs):
        if l2 and sw[t] > 0 and su[t] > 0:
            q[t] = np.sqrt(sw[t]) / np.sqrt(su[t])
            rel_q[t] = np.sqrt(sdu[t]) / np.sqrt(su[t]) + base[t]
    qe, rqe = _expand(q, segs, w.size), _expand(rel_q, segs, w.size)
    wn = w - lr * qe * u
    dw = lr * qe * (du + np.abs(u) * (rqe + 2 * U)) + 2 * U * (np.abs(w) + lr * qe * np.abs(u))
    return (wn, mn, vn), (dw, dm, dv), q, rel_q


@pytest.mark.gpu
@pytest.mark.parametrize("decay", [0.0, 0.01], ids=["nodecay", "decay"])
@pytest.mark.parametrize("mode", MODES)
def test_lamb(gpu, mode, decay):
    from x3d_tf_amd import ops
    f = _fix(gpu)
    kw, c, ed, e_was = _extras(f, mode, gpu)
    (wd_, w_was), (md, m_was), (vd, v_was), (gd, g_was) = (_dirty(f, a, gpu) for a in (f.w, f.v, f.v2, f.g))
    h = LAMB
    q = ops.lamb(wd_, md, vd, gd, f.table, h["lr"], h["step"], h["b1"], h["b2"], h["eps"], decay, **kw)
    want, lims, q64, rel_q = _lamb_ref(f.w, f.v, f.v2, f.g, f.segs, c, decay)
    qd = _np(q).astype(np.float64)
    assert np.all(np.abs(qd - q64) <= rel_q * q64), np.max(np.abs(qd - q64) / np.maximum(rel_q * q64, 1e-300))
    assert np.max(rel_q) < 1e-4                                                     # (the limit is a tight one)
    for t, l2 in enumerate(L2):
        if not l2 or t == ZERO_W or (t == ZERO_G and decay == 0.0):                 # ZERO_G: m = v = g = 0, so u = decay w
            assert _np(q)[t] == F32(1.0), t
    cv = f.covered
    for got, ref, lim, name in zip((wd_, md, vd), want, lims, "wmv"):
        err = np.abs(_np(got) - ref)
        assert np.all((err <= lim)[cv]), (name, np.max((err / np.maximum(lim, 1e-300))[cv]))
    assert not np.array_equal(_bits(_np(wd_))[cv], _bits(w_was)[cv])
    assert np.array_equal(_bits(_np(gd)), _bits(g_was))                             # u never lands in the gradient buffer
    named = [("w", wd_, w_was), ("m", md, m_was), ("v", vd, v_was)]
    if ed is not None:
        _check_ema(f, ed, _np(wd_))
        named.append(("ema", ed, e_was))
    _check_untouched_and_finite(f, named)


# ---- both alignment paths, the same bits; a non-finite gradient skips everything -----------------------------------------
@pytest.mark.gpu
def test_alignment_paths_agree_bit_for_bit(gpu):
    """base pointers one float behind a 16-byte boundary take the one-by-one loads: the same elements by the same lanes in
    the same order, so q (the sums) and the updates have the bits of the vector path"""
    from x3d_tf_amd import ops
    f = _fix(gpu)
    kw = dict(grad_scale=float(GS))
    a = _run_lars(f, gpu, kw, False)
    b = _run_lars(f, gpu, kw, False, off=1)
    assert b[0][0].data_ptr() % 16 == 4
    assert np.array_equal(_bits(_np(a[3])), _bits(_np(b[3])))
    for (x, _), (y, _) in zip(a[:2], b[:2]):
        assert np.array_equal(_bits(_np(x)), _bits(_np(y)))
    h = LAMB
    res = []
    for off in (0, 1):
        (wd_, _), (md, _), (vd, _), (gd, _) = (_dirty(f, x, gpu, off) for x in (f.w, f.v, f.v2, f.g))
        q = ops.lamb(wd_, md, vd, gd, f.table, h["lr"], h["step"], h["b1"], h["b2"], h["eps"], 0.01, **kw)
        res.append((wd_, md, vd, q))
    for x, y in zip(*res):
        assert np.array_equal(_bits(_np(x)), _bits(_np(y)))
    _check_untouched_and_finite(f, [("w", res[1][0], _dirty(f, f.w, gpu)[1])])


@pytest.mark.gpu
def test_non_finite_gradient_skips_every_launch(gpu):
    """norm[1] != 0: w, the slots, ema and q are what they were, bit for bit -- all three optimizers"""
    from x3d_tf_amd import ops
    f = _fix(gpu)
    g = f.g.copy()
    g[f.segs[5][0] + 7] = np.inf
    norm = _norm_of(g, gpu)
    assert _np(norm)[1] == 1.0
    (wd_, w_was), (md, m_was), (vd, v_was), (ed, e_was) = (_dirty(f, a, gpu) for a in (f.w, f.v, f.v2, f.e))
    gd, g_was = _dirty(f, g, gpu)
    q = torch.full((len(LENGTHS),), 7.0, dtype=torch.float32, device=gpu)
    kw = dict(grad_scale=float(GS), norm=norm, max_norm=1.0, ema=ed, ema_decay=0.9)
    h = LARS
    ops.lars(wd_, md, gd, f.table, h["lr"], h["mom"], h["wd"], h["eta"], h["eps"], True, q=q, **kw)
    h = ADAM
    ops.adamw(wd_, md, vd, gd, f.table, h["lr"], h["step"], h["b1"], h["b2"], h["eps"], 0.05, **kw)
    h = LAMB
    ops.lamb(wd_, md, vd, gd, f.table, h["lr"], h["step"], h["b1"], h["b2"], h["eps"], 0.01, q=q, **kw)
    for got, was in ((wd_, w_was), (md, m_was), (vd, v_was), (ed, e_was), (gd, g_was)):
        assert np.array_equal(_bits(_np(got)), _bits(was))
    assert np.all(_np(q) == F32(7.0))


# ---- the Trainer, XS config (the shapes of test_model_gpu.py::test_trainer_fp16_loss_scaling_and_adam) --------------------
CLASSES = 11
NEW = ["lars", "adamw", "lamb"]


def _cfg(opt, *extra):
    import x3d_tf_amd as x
    return x.get_config("XS", ["TRAIN.OPTIMIZER", opt, "NETWORK.NUM_CLASSES", CLASSES, "OPTIM.LARS_TRUST_COEF", 0.02,
                               "OPTIM.WEIGHT_DECAY", 0.01] + list(extra))


def _batches(k, seed=3):
    gen = torch.Generator().manual_seed(seed)
    return [(torch.randn(2, 4, 64, 64, 3, generator=gen), torch.randint(0, CLASSES, (2,), generator=gen)) for _ in range(k)]


def _trainer(cfg, gpu, seed=5, dtype=torch.float32):
    import x3d_tf_amd as x
    from x3d_tf_amd.model import X3D
    from x3d_tf_amd.train import Trainer
    m = X3D(cfg, dtype=dtype, device=gpu, seed=seed)
    m.set_dropout_mask(torch.ones(2, x.build_arch(cfg).fc1_out))
    return m, Trainer(m, cfg)


def _host_rule(tr, m, w0, s1, s2, g, lr, c, step):
    """the fp64 rule of the trainer's optimizer on the trainable block: ((w', slots...), limits, q or None, rel limit of q)"""
    segs = [(s.offset, s.length, s.l2) for s in m.segments]
    o = tr.optim
    if tr.optimizer == "lars":
        hp = dict(lr=F32(lr), mom=F32(tr.momentum), wd=F32(m.arch.weight_decay), eta=F32(o.lars_trust_coef), eps=F32(o.lars_eps))
        wn, vn, lim, q = _lars_ref(w0, s1, g, segs, c, o.lars_clip, hp)
        return (wn, vn), (lim, lim), q, _q_limit([n for _, n, _ in segs])
    hp = dict(lr=F32(lr), b1=F32(0.9), b2=F32(0.999), step=step)
    if tr.optimizer == "adamw":
        l2e = _np(m.l2_mask).astype(bool)
        want, lims = _adamw_ref(w0, s1, s2, g, l2e, c, o.weight_decay, dict(hp, eps=F32(1e-7)))
        return want, lims, None, None
    return _lamb_ref(w0, s1, s2, g, segs, c, o.weight_decay, dict(hp, eps=F32(o.lamb_eps)))


def _covered(m):
    cv = np.zeros(m.n_trainable_flat, bool)
    for s in m.segments:
        cv[s.offset:s.offset + s.length] = True
    return cv


def _check_update(tr, m, w0, s1, s2, lr, c, step=1):
    nt = m.n_trainable_flat
    g = _np(m.flat_grads)                                                           # the update leaves the gradient in place
    want, lims, q64, rel_q = _host_rule(tr, m, w0, s1, s2, g, lr, c, step)
    cv = _covered(m)
    got = [m.flat_params[:nt], m.flat_velocity] + ([m.flat_second] if len(want) == 3 else [])
    for t, ref, lim, name in zip(got, want, lims, "w12"):
        err = np.abs(_np(t) - ref)
        assert np.all((err <= lim)[cv]), (tr.optimizer, name, np.max((err / np.maximum(lim, 1e-300))[cv]))
    if q64 is None:
        assert tr.last_trust_ratios is None
    else:
        qd = _np(tr.last_trust_ratios).astype(np.float64)
        assert qd.shape == (len(m.segments),)
        assert np.all(np.abs(qd - q64) <= rel_q * q64), np.max(np.abs(qd - q64) / np.maximum(rel_q * q64, 1e-300))
        l2 = np.array([s.l2 for s in m.segments])
        assert np.all(qd[~l2] == 1.0) and np.any(qd[l2] != 1.0)


@pytest.mark.gpu
@pytest.mark.parametrize("opt", NEW)
def test_trainer_step_with_clipping_and_ema(gpu, opt):
    """one Trainer.step; the weights, slots, EMA and trust ratios against the fp64 rule on the gradient the step left in
    flat_grads, at the kernel-level bounds"""
    (x1, y1), = _batches(1)
    lr, max_norm, decay = 0.05, 0.05, 0.5
    m, tr = _trainer(_cfg(opt, "SOLVER.CLIP_GRAD_L2NORM", max_norm, "SOLVER.EMA_DECAY", decay), gpu)
    nt = m.n_trainable_flat
    m.flat_velocity.copy_(0.01 * torch.randn(nt, generator=torch.Generator().manual_seed(1)) * torch.from_numpy(_covered(m)))
    if opt != "lars":
        m._adam_slots()
        m.flat_second.copy_(m.flat_velocity.abs() * 0.01)
    w0, s1 = _np(m.flat_params[:nt]).copy(), _np(m.flat_velocity).copy()
    s2 = None if opt == "lars" else _np(m.flat_second).copy()
    e0 = _np(tr.ema[:nt]).copy()
    pl = tr.step(x1.to(gpu), y1.to(gpu), lr)
    g64 = _np(m.flat_grads).astype(np.float64)
    norm0 = float(np.sum(g64 * g64))
    assert abs(float(tr.last_grad_norm.item()) - np.sqrt(norm0)) <= 1e-6 * np.sqrt(norm0)
    assert np.sqrt(norm0) > max_norm and tr.opt_step == 1                           # the clip is active
    c = _coef(float(_np(m._norm_out)[0]), 1.0, max_norm)
    _check_update(tr, m, w0, s1, s2, lr, c)
    _check_ema(None, tr.ema[:nt], _np(m.flat_params[:nt]), e0=e0, decay=F32(decay), covered=_covered(m))
    pad = ~_covered(m)
    assert np.all(_np(m.flat_params[:nt])[pad] == 0) and np.all(_np(m.flat_velocity)[pad] == 0)
    # the loss: lars reports what sgd reports (cross-entropy + L2 term), adamw / lamb the cross-entropy alone
    ce = float(pl.loss_rows.sum().item()) / pl.n
    reg = float(m.regularization_loss().item())
    assert reg > 0 and abs(float(tr.loss(pl).item()) - (ce + (reg if opt == "lars" else 0.0))) <= 1e-5 * (ce + reg)


@pytest.mark.gpu
@pytest.mark.parametrize("opt", NEW)
def test_trainer_fp16_overflow_skips_the_step(gpu, opt):
    (x1, y1), = _batches(1)
    m, tr = _trainer(_cfg(opt), gpu, dtype=torch.float16)
    assert tr.dynamic_scale and tr.loss_scale == 2.0 ** 15 and tr.optimizer == opt
    tr.step(x1.to(gpu), y1.to(gpu), 0.01)
    assert tr.skipped_steps == 0 and tr.opt_step == 1 and torch.isfinite(m.flat_params).all()
    tr.loss_scale = 2.0 ** 40
    before, slot = m.flat_params.clone(), m.flat_velocity.clone()
    tr.step(x1.to(gpu), y1.to(gpu), 0.01)
    assert tr.skipped_steps == 1 and tr.loss_scale == 2.0 ** 39 and tr.opt_step == 1
    nt = m.n_trainable_flat
    assert torch.equal(before[:nt], m.flat_params[:nt]) and torch.equal(slot, m.flat_velocity)


@pytest.mark.gpu
@pytest.mark.parametrize("opt", NEW)
def test_trainer_accumulation_is_one_step_on_the_summed_gradient(gpu, opt):
    """ACCUM_STEPS = 2: nothing moves after the first micro-batch; after the second the weights are the rule applied once to
    the total `flat_grads` then holds (that the total is g1 + g2 is test_solver_gpu.py::test_trainer_accumulation's subject)"""
    (x1, y1), (x2, y2) = [(a.to(gpu), b.to(gpu)) for a, b in _batches(2)]
    lr = 0.05
    m, tr = _trainer(_cfg(opt, "SOLVER.ACCUM_STEPS", 2), gpu)
    nt = m.n_trainable_flat
    w0 = _np(m.flat_params[:nt]).copy()
    tr.step(x1, y1, lr)
    g1 = m.flat_grads.clone()
    assert np.array_equal(_bits(_np(m.flat_params[:nt])), _bits(w0)) and tr.opt_step == 0 and tr.last_trust_ratios is None
    tr.step(x2, y2, lr)
    assert tr.opt_step == 1 and not torch.equal(m.flat_grads, g1)
    zeros = np.zeros(nt, F32)
    _check_update(tr, m, w0, zeros, None if opt == "lars" else zeros, lr, 1.0)


def _state(m):
    nt = m.n_trainable_flat
    second = getattr(m, "flat_second", None)
    return [m.flat_params[:nt].clone(), m.flat_velocity.clone()] + ([second.clone()] if second is not None else [])


@pytest.mark.gpu
@pytest.mark.parametrize("opt", ["lars", "lamb"])
def test_checkpoint_resume_continues_bit_for_bit(gpu, opt, tmp_path):
    """save_checkpoint -> a fresh model and trainer -> resume -> one more update = the uninterrupted run, bit for bit: weights,
    slots, trust ratios and the step counter.  The backward pass adds some weight gradients with fp32 atomics, so two runs of
    it differ in the last bits (test_solver_gpu.py: the spread); the resumed trainer therefore updates on the very gradient
    the uninterrupted one computed, handed over in flat_grads."""
    (x1, y1), (x2, y2) = [(a.to(gpu), b.to(gpu)) for a, b in _batches(2)]
    lr = 0.05
    cfg = _cfg(opt, "SOLVER.CLIP_GRAD_L2NORM", 0.05)
    m, tr = _trainer(cfg, gpu)
    tr.step(x1, y1, lr)
    tr.save_checkpoint(str(tmp_path), 1)
    assert tr.opt_step == 1
    tr.step(x2, y2, lr)
    g2, after, q_after = m.flat_grads.clone(), _state(m), tr.last_trust_ratios.clone()
    m2, tr2 = _trainer(cfg, gpu, seed=9)
    assert tr2.resume(str(tmp_path)) == 1 and tr2.opt_step == 1
    assert m2.optimizer_state["kind"] == ("sgd" if opt == "lars" else "adam")
    m2.flat_grads.copy_(g2)
    tr2._update(None, lr)
    assert tr2.opt_step == 2
    for a, b in zip(after, _state(m2)):
        assert torch.equal(a, b)
    assert torch.equal(q_after, tr2.last_trust_ratios)


@pytest.mark.gpu
def test_lamb_checkpoint_in_an_sgd_trainer_zeroes_the_slots(gpu, tmp_path):
    (x1, y1), = _batches(1)
    m, tr = _trainer(_cfg("lamb"), gpu)
    tr.step(x1.to(gpu), y1.to(gpu), 0.05)
    assert float(m.flat_velocity.abs().max()) > 0 and float(m.flat_second.abs().max()) > 0
    tr.save_checkpoint(str(tmp_path), 1)
    for opt, kept in (("sgd", False), ("lars", False), ("adamw", True)):
        m2, tr2 = _trainer(_cfg(opt), gpu, seed=9)
        assert tr2.resume(str(tmp_path)) == 1
        assert torch.equal(m2.flat_params[:m.n_trainable_flat], m.flat_params[:m.n_trainable_flat])
        if kept:                                                                    # the same layout: Adam's m, v and `iter`
            assert torch.equal(m2.flat_velocity, m.flat_velocity) and torch.equal(m2.flat_second, m.flat_second)
            assert tr2.opt_step == 1
        else:
            assert float(m2.flat_velocity.abs().max()) == 0 and tr2.opt_step == 0
            assert getattr(m2, "flat_second", None) is None or float(m2.flat_second.abs().max()) == 0


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


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
    m, tr = _trainer(_cfg("lars", "SOLVER.CLIP_GRAD_L2NORM", 0.05), dev, seed=1 + rank)
    tr.step(x1.to(dev), y1.to(dev), 0.05)
    torch.save(dict(w=m.flat_params[:m.n_trainable_flat].cpu(), v=m.flat_velocity.cpu(), q=tr.last_trust_ratios.cpu()),
               os.path.join(tmp, f"rank{rank}.pt"))
    with open(os.path.join(tmp, f"rank{rank}.json"), "w") as f:
        json.dump(dict(opt_step=tr.opt_step, world=tr.world), f)
    dist.barrier()
    dist.destroy_process_group()


@pytest.mark.gpu
def test_two_ranks_end_a_lars_step_identical(gpu, tmp_path):
    """the trust ratios come from the all-reduced gradient: both ranks hold the same weights, slots and ratios, bit for bit"""
    mp.spawn(_rank_worker, args=(2, _free_port(), str(tmp_path)), nprocs=2, join=True)
    r0, r1 = (torch.load(tmp_path / f"rank{r}.pt") for r in (0, 1))
    info = json.load(open(tmp_path / "rank0.json"))
    assert info == dict(opt_step=1, world=2)
    for k in ("w", "v", "q"):
        assert torch.equal(r0[k], r1[k]), k
    assert float((r0["q"] != 1).sum()) > 0 and bool(torch.isfinite(r0["w"]).all())


@pytest.mark.gpu
def test_sgd_makes_the_launches_it_always_made(gpu, monkeypatch):
    """TRAIN.OPTIMIZER = sgd, with the OPTIM section and without: the same recorded plan and the same library calls per step,
    none of the new entry points; and the switch does reach them"""
    from x3d_tf_amd import hip
    (x1, y1), = _batches(1)
    x1, y1 = x1.to(gpu), y1.to(gpu)
    cfg = _cfg("sgd")
    old = cfg.clone()
    old.defrost()
    del old["OPTIM"]
    calls = []
    real = hip.call

    def recorder(name, *args):
        calls.append(name)
        return real(name, *args)

    new = {"x3d_seg_sumsq", "x3d_lars", "x3d_adamw", "x3d_lamb"}
    seqs, plans = [], []
    for c in (cfg, old):
        m, tr = _trainer(c, gpu)
        pl = tr.step(x1, y1, 0.1)
        plans.append([name for name, *_ in pl.fwd + pl.bwd])
        monkeypatch.setattr(hip, "call", recorder)
        calls.clear()
        tr.step(x1, y1, 0.1)
        monkeypatch.setattr(hip, "call", real)
        seqs.append(list(calls))
        assert tr.last_trust_ratios is None and m._seg_table is None
    assert plans[0] == plans[1] and seqs[0] == seqs[1] and seqs[0][-1] == "x3d_sgd_nesterov"
    assert not new & set(seqs[0]) and not new & set(plans[0])
    for opt, name in (("lars", "x3d_lars"), ("adamw", "x3d_adamw"), ("lamb", "x3d_lamb")):
        m, tr = _trainer(_cfg(opt), gpu)
        monkeypatch.setattr(hip, "call", recorder)
        calls.clear()
        tr.step(x1, y1, 0.1)
        monkeypatch.setattr(hip, "call", real)
        assert [c for c in calls if c in new] == [name] and calls[-1] == name
