"""fp64 restatement of the distillation losses (x3d_softmax_xent_kd / x3d_sigmoid_bce_kd, include/x3d_hip.h) in closed form,
and the inputs the CPU and the GPU tests share.  No autograd here: test_distill.py holds these formulas to a second,
independent formulation (torch's KLDivLoss and a log-sigmoid Bernoulli KL under fp64 autograd)."""
import numpy as np
import torch

NS, MS = (1, 7, 64), (1, 157, 257, 400)
TEMPS, ALPHAS = (1.0, 2.5, 4.0), (0.3, 1.0)
SAME_ROW = 2              # the row with t = z (shapes with N > 2 and M > 5)


def f32(v):
    """the value a kernel sees for a float argument"""
    return float(np.float32(v))


def has_stress(n, m):
    return m > 5


def has_same_row(n, m):
    return m > 5 and n > SAME_ROW


def inputs(n, m):
    """z = randn * 2, t = randn * 3 (fp32), labels [n] int32, dense soft rows and multi-hot rows [n, m] fp32.  Where m > 5:
    row 0 of z has one logit 40 above the rest (the hard term's clipped regime), row 0 of t one logit 120 above the rest
    (teacher probabilities that underflow to 0 in fp32), and -- where there are more than SAME_ROW rows -- row SAME_ROW has
    t = z.  With a single row the two row-0 cases are all there is."""
    g = torch.Generator().manual_seed(1000 * n + m)
    z = torch.randn(n, m, generator=g) * 2
    t = torch.randn(n, m, generator=g) * 3
    labels = torch.randint(0, m, (n,), generator=g, dtype=torch.int32)
    other = torch.randint(0, m, (n,), generator=g)
    hot = torch.nn.functional.one_hot(labels.long(), m).double()
    soft = 0.9 * hot + 0.1 / m
    lam = f32(0.3)
    soft = (lam * soft + (1.0 - lam) * torch.nn.functional.one_hot(other, m).double()).float()     # a mixed, smoothed row
    multi = (torch.rand(n, m, generator=g) < 0.05).float()
    if has_stress(n, m):
        z[0] = 0.0
        z[0, 3] = 40.0
        t[0] = 0.0
        t[0, 5] = 120.0
    if has_same_row(n, m):
        t[SAME_ROW] = z[SAME_ROW]
    return z, t, labels, soft, multi


# ---- hard terms (the sibling kernels' rules) ----------------------------------------------------------------------------
def softmax_hard(z, labels=None, targets=None):
    """(probs, loss rows, d rows / dz) of Keras' clipped cross-entropy on probabilities; labels [n] or dense rows [n, m]"""
    z = z.double()
    p = torch.softmax(z, -1)
    y = torch.nn.functional.one_hot(labels.long(), z.shape[1]).double() if targets is None else targets.double()
    q = p.clamp(1e-7, 1 - 1e-7)
    inr = ((p >= 1e-7) & (p <= 1 - 1e-7)).double()
    S, sumq = y.sum(1, keepdim=True), q.sum(1, keepdim=True)
    rows = (y * -torch.log(q)).sum(1) + S[:, 0] * torch.log(sumq[:, 0])
    dldp = inr * (S / sumq - y / q)
    grad = p * (dldp - (p * dldp).sum(1, keepdim=True))
    return p, rows, grad


def softplus(x):
    return x.clamp(min=0.0) + torch.log1p(torch.exp(-x.abs()))


def sigmoid_hard(z, y):
    z, y = z.double(), y.double()
    p = torch.sigmoid(z)
    rows = (z.clamp(min=0.0) - z * y + torch.log1p(torch.exp(-z.abs()))).mean(1)
    return p, rows, (p - y) / z.shape[1]


# ---- KD terms -----------------------------------------------------------------------------------------------------------
def softmax_kd(z, t, T):
    """(kd rows, d kd / dz): T^2 * sum_j p_t (log p_t - log p_s) in log space, gradient T * (p_s - p_t)"""
    u, v = z.double() / T, t.double() / T
    lps = u - torch.logsumexp(u, 1, keepdim=True)
    lpt = v - torch.logsumexp(v, 1, keepdim=True)
    pt = torch.exp(lpt)
    return T * T * (pt * (lpt - lps)).sum(1), T * (torch.exp(lps) - pt)


def sigmoid_kd(z, t, T):
    u, v = z.double() / T, t.double() / T
    sv = torch.sigmoid(v)
    kd = T * T * ((softplus(u) - sv * u) - (softplus(v) - sv * v)).mean(1)
    return kd, T * (torch.sigmoid(u) - sv) / z.shape[1]


def combine(hard, kd, alpha, grad_scale):
    """(probs, loss rows, kd rows, dlogits) from a hard-term triple and a KD pair"""
    p, hr, hg = hard
    kr, kg = kd
    return p, (1.0 - alpha) * hr + alpha * kr, kr, grad_scale * ((1.0 - alpha) * hg + alpha * kg)
