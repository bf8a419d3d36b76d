"""fp64 NumPy restatement of the weighted / focal losses (x3d_softmax_xent_w / x3d_sigmoid_bce_w, include/x3d_hip.h): the loss
rows and the closed-form gradients, taking the fp32 logits as given, and the cases the CPU and the GPU tests share.  No autograd
here: test_loss_weights.py holds these formulas to torch.autograd in float64, to torch's BCEWithLogitsLoss(pos_weight) and to a
transcription of Keras' focal losses.  Logits, teacher, labels and targets are distill_ref.inputs'."""
import numpy as np

import distill_ref as R

NS, MS = (1, 3, 7), (1, 2, 157, 256, 257, 400)
HEADS = ("labels", "targets", "multi")
KD = ((0.0, 1.0), (0.0, 4.0), (0.5, 1.0), (0.5, 4.0))          # (alpha, temperature)
# the project's limits (test_mix_gpu.py / test_distill_gpu.py), as (rtol, atol); atol is multiplied by the largest product
# c * w+ * r of the case: the weights scale the error linearly
TOL = dict(probs=(1e-5, 1e-7), loss_rows=(1e-4, 1e-4), kd_rows=(1e-4, 1e-4), dlogits=(1e-3, 1e-6))

# modifier sets: which tables are drawn and the gammas (softmax head: gamma = gp)
SOFTMAX_MODS = dict(none=dict(), cw=dict(cw=1), rw=dict(rw=1), g05=dict(gp=0.5), g2=dict(gp=2.0), all=dict(cw=1, rw=1, gp=2.0))
SIGMOID_MODS = dict(none=dict(), cw=dict(cw=1), rw=dict(rw=1), g05=dict(gp=0.5, gn=0.5), g2=dict(gp=2.0, gn=2.0),
                    pw=dict(pw=1), asym=dict(gp=1.0, gn=4.0), all=dict(cw=1, pw=1, rw=1, gp=2.0, gn=0.5))


def mods_of(head):
    return SIGMOID_MODS if head == "multi" else SOFTMAX_MODS


def weights(n, m, mod):
    """(class_w, pos_w, row_w) as fp32 arrays or None: drawn in [0, 4] with exact zeros (every fifth class but the first;
    row 1 where there is one)"""
    g = np.random.default_rng(77 * n + m)
    cw = g.uniform(0.0, 4.0, m).astype(np.float32)
    pw = g.uniform(0.0, 4.0, m).astype(np.float32)
    rw = g.uniform(0.0, 4.0, n).astype(np.float32)
    cw[5::5] = 0.0
    pw[7::5] = 0.0
    if n > 1:
        rw[1] = 0.0
    return (cw if mod.get("cw") else None, pw if mod.get("pw") else None, rw if mod.get("rw") else None)


def weight_scale(cw, pw, rw):
    """the largest product c * w+ * r of a case (1 for a table that is not given)"""
    return float(np.prod([1.0 if w is None else max(float(np.max(w)), 1.0) for w in (cw, pw, rw)]))


def _ones(w, k):
    return np.ones(k) if w is None else np.asarray(w, dtype=np.float64)


def focal(x, g):
    """f(x) = (1 - x)^g * (-log x) and f'(x); x = 1: both 0 (the kernels' rule for the one-class row)"""
    x = np.asarray(x, dtype=np.float64)
    om = 1.0 - x
    one = om <= 0.0
    oms = np.where(one, 1.0, om)
    L = -np.log(x)
    pw = np.ones_like(x) if g == 0.0 else oms ** g
    f = pw * L
    df = -(0.0 if g == 0.0 else g * pw / oms * L) - pw / x
    return np.where(one, 0.0, f), np.where(one, 0.0, df)


def softmax_w(z, labels=None, targets=None, class_w=None, row_w=None, gamma=0.0):
    """(probs, hard rows, d hard / dz) of hard = r * sum_j c_j y_j f(q_j / sum q), q = clip(softmax(z), 1e-7, 1 - 1e-7)"""
    z = np.asarray(z, dtype=np.float64)
    n, m = z.shape
    e = np.exp(z - z.max(1, keepdims=True))
    p = e / e.sum(1, keepdims=True)
    y = np.eye(m)[np.asarray(labels, dtype=np.int64)] if targets is None else np.asarray(targets, dtype=np.float64)
    q = np.clip(p, 1e-7, 1.0 - 1e-7)
    inr = ((p >= 1e-7) & (p <= 1.0 - 1e-7)).astype(np.float64)
    sumq = q.sum(1, keepdims=True)
    x = q / sumq
    a = _ones(row_w, n)[:, None] * _ones(class_w, m)[None, :] * y
    f, df = focal(x, float(gamma))
    rows = (a * f).sum(1)
    B = (a * df * x).sum(1, keepdims=True)
    dldp = inr * (a * df - B) / sumq
    grad = p * (dldp - (p * dldp).sum(1, keepdims=True))
    return p, rows, grad


def _softplus(x):
    return np.maximum(x, 0.0) + np.log1p(np.exp(-np.abs(x)))


def _sigmoid(z):
    return np.where(z >= 0, 1.0 / (1.0 + np.exp(-np.abs(z))), np.exp(-np.abs(z)) / (1.0 + np.exp(-np.abs(z))))


def _pow(x, g):
    return np.ones_like(x) if g == 0.0 else x ** g


def sigmoid_w(z, y, class_w=None, pos_w=None, row_w=None, gamma_pos=0.0, gamma_neg=0.0):
    """(probs, hard rows, d hard / dz) of hard = r * mean_j c_j [y w+ (1 - s)^g+ softplus(-z) + (1 - y) s^g- softplus(z)]"""
    z, y = np.asarray(z, dtype=np.float64), np.asarray(y, dtype=np.float64)
    n, m = z.shape
    gp, gn = float(gamma_pos), float(gamma_neg)
    s, oms = _sigmoid(z), _sigmoid(-z)
    c, wp, r = _ones(class_w, m)[None, :], _ones(pos_w, m)[None, :], _ones(row_w, n)[:, None]
    sp_pos, sp_neg = _softplus(-z), _softplus(z)
    term = c * (y * wp * _pow(oms, gp) * sp_pos + (1.0 - y) * _pow(s, gn) * sp_neg)
    d = c * ((1.0 - y) * _pow(s, gn) * (gn * oms * sp_neg + s) - y * wp * _pow(oms, gp) * (gp * s * sp_pos + oms))
    return s, r[:, 0] * term.mean(1), r * d / m


def expected(head, z, t, labels, soft, multi, cw, pw, rw, mod, alpha, T, grad_scale):
    """(probs, loss rows, kd rows, dlogits) fp64 of one case: loss = (1 - a) * hard + a * r * kd, kd rows unweighted (0 at
    alpha == 0, where the teacher is not read)"""
    n, m = z.shape
    if head == "multi":
        p, hr, hg = sigmoid_w(z.numpy(), multi.numpy(), cw, pw, rw, mod.get("gp", 0.0), mod.get("gn", 0.0))
    else:
        kw = dict(labels=labels.numpy()) if head == "labels" else dict(targets=soft.numpy())
        p, hr, hg = softmax_w(z.numpy(), class_w=cw, row_w=rw, gamma=mod.get("gp", 0.0), **kw)
    if alpha == 0.0:
        return p, hr, np.zeros(n), grad_scale * hg
    kr, kg = (R.sigmoid_kd if head == "multi" else R.softmax_kd)(z, t, T)
    kr, kg, r = kr.numpy(), kg.numpy(), _ones(rw, n)
    return p, (1.0 - alpha) * hr + alpha * r * kr, kr, grad_scale * ((1.0 - alpha) * hg + alpha * r[:, None] * kg)
