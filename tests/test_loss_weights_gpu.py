"""Class-imbalance losses on the GPU: x3d_softmax_xent_w / x3d_sigmoid_bce_w against the fp64 restatement in loss_weights_ref.py
(limits: test_mix_gpu.py's / test_distill_gpu.py's, atol times the largest weight product of the case), with nothing set against
the five existing entry points bit for bit, the unusable and the edge rows, x3d_class_hits against a NumPy count, and the model
and the trainer: set_loss, sample weights, LOSS.* in bf16 and fp16, fit with 3-tuple batches and the per-class metric."""
import itertools
import math
import os
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import x3d_tf_amd as x  # noqa: E402
from x3d_tf_amd import ops  # noqa: E402
import distill_ref as R  # noqa: E402
import loss_weights_ref as W  # noqa: E402

SENTINEL = 7.0
OUTS = ("probs", "loss_rows", "kd_rows", "dlogits")


def _dev(w, gpu):
    return None if w is None else torch.as_tensor(w).to(gpu)


def _run(gpu, head, z, t, labels, soft, multi, cw, pw, rw, mod, gs, alpha, T, give=(True, True, True)):
    """one launch of the head's _w entry point into sentinel-filled buffers: (probs, loss_rows, kd_rows, dlogits), None for an
    output that is not given (`give`: loss_rows, kd_rows, dlogits)"""
    n, m = z.shape
    probs = torch.full((n, m), SENTINEL, device=gpu)
    rows = torch.full((n,), SENTINEL, device=gpu) if give[0] else None
    kd = torch.full((n,), SENTINEL, device=gpu) if give[1] else None
    dl = torch.full((n, m), SENTINEL, device=gpu) if give[2] else None
    kw = dict(class_w=_dev(cw, gpu), row_w=_dev(rw, gpu), teacher_logits=_dev(t, gpu), loss_rows=rows, kd_rows=kd, dlogits=dl,
              grad_scale=gs, alpha=alpha, temperature=T)
    if head == "multi":
        ops.sigmoid_bce_w(z.to(gpu), multi.to(gpu), probs, pos_w=_dev(pw, gpu), gamma_pos=mod.get("gp", 0.0),
                          gamma_neg=mod.get("gn", 0.0), **kw)
    else:
        ops.softmax_xent_w(z.to(gpu), probs, labels=labels.to(gpu) if head == "labels" else None,
                           targets=soft.to(gpu) if head == "targets" else None, gamma=mod.get("gp", 0.0), **kw)
    torch.cuda.synchronize()
    return probs, rows, kd, dl


def _plain(gpu, head, z, t, labels, soft, multi, gs, alpha, T):
    """the matching existing entry point: the plain kernel at alpha == 0, the distillation kernel otherwise"""
    n, m = z.shape
    p, r, d = torch.full((n, m), SENTINEL, device=gpu), torch.full((n,), SENTINEL, device=gpu), torch.full((n, m), SENTINEL, device=gpu)
    k = torch.zeros(n, device=gpu)
    if alpha == 0.0:
        if head == "labels":
            ops.softmax_xent(z.to(gpu), labels.to(gpu), p, r, d, gs)
        elif head == "targets":
            ops.softmax_xent_soft(z.to(gpu), soft.to(gpu), p, r, d, gs)
        else:
            ops.sigmoid_bce(z.to(gpu), multi.to(gpu), p, r, d, gs)
    elif head == "multi":
        ops.sigmoid_bce_kd(z.to(gpu), t.to(gpu), multi.to(gpu), p, r, k, d, gs, alpha, T)
    else:
        ops.softmax_xent_kd(z.to(gpu), t.to(gpu), p, labels=labels.to(gpu) if head == "labels" else None,
                            targets=soft.to(gpu) if head == "targets" else None, loss_rows=r, kd_rows=k, dlogits=d, grad_scale=gs,
                            alpha=alpha, temperature=T)
    torch.cuda.synchronize()
    return p, r, k, d


# ---- the kernels against fp64 ------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("head", W.HEADS)
@pytest.mark.parametrize("n", W.NS)
def test_w_kernels_match_fp64(gpu, head, n):
    worst = dict.fromkeys(OUTS, 0.0)
    cases = 0
    for m in W.MS:
        z, t, labels, soft, multi = R.inputs(n, m)
        gs = R.f32(1.0 / n)
        for name, mod in W.mods_of(head).items():
            cw, pw, rw = W.weights(n, m, mod)
            scale = W.weight_scale(cw, pw, rw)
            for alpha, T in W.KD:
                ref = W.expected(head, z, t, labels, soft, multi, cw, pw, rw, mod, alpha, T, gs)
                for give in itertools.product((True, False), repeat=3):            # every combination of NULL outputs
                    got = _run(gpu, head, z, t, labels, soft, multi, cw, pw, rw, mod, gs, alpha, T, give)
                    cases += 1
                    for what, g, r in zip(OUTS, got, ref):
                        if g is None:
                            continue
                        g = g.cpu().double().numpy()
                        rtol, atol = W.TOL[what]
                        err = np.abs(g - r)
                        worst[what] = max(worst[what], float(err.max()))
                        ok = np.isfinite(g).all() and (err <= atol * scale + rtol * np.abs(r)).all()
                        assert ok, (f"{what} {head} n={n} m={m} {name} alpha={alpha} T={T} outputs={give}: max abs err "
                                    f"{err.max():.3e} (atol {atol * scale:.3e}, rtol {rtol}), max |ref| {np.abs(r).max():.3e}")
    print(f"{head} n={n}: {cases} launches; max abs err " + ", ".join(f"{k} {v:.3e}" for k, v in worst.items()))


# ---- nothing set: the existing entry points, bit for bit ---------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("head", W.HEADS)
@pytest.mark.parametrize("n, m", [(1, 1), (7, 157), (64, 257), (64, 400)])
def test_nothing_set_is_the_existing_entry_point_bit_for_bit(gpu, head, n, m):
    z, t, labels, soft, multi = R.inputs(n, m)
    gs = 0.37
    none = (None, None, None, {})
    want = _plain(gpu, head, z, t, labels, soft, multi, gs, 0.0, 1.0)
    nan_t = torch.full_like(t, float("nan"))
    for teacher in (None, t, nan_t):                                  # a NULL teacher is accepted; a given one is not read
        for T in (1.0, 4.0):
            got = _run(gpu, head, z, teacher, labels, soft, multi, *none, gs, 0.0, T)
            assert all(torch.equal(g, w) for g, w in zip(got, want)), (teacher is None, T)
            assert got[2].abs().sum().item() == 0.0                   # (and with it: no sentinel left anywhere)
    for alpha, T in ((0.5, 1.0), (R.f32(0.3), 2.5), (1.0, 4.0)):
        want_kd = _plain(gpu, head, z, t, labels, soft, multi, gs, alpha, T)
        got = _run(gpu, head, z, t, labels, soft, multi, *none, gs, alpha, T)
        assert all(torch.equal(g, w) for g, w in zip(got, want_kd)), (alpha, T)
    # probs has those bits for every modifier set, distilled or not
    for name, mod in W.mods_of(head).items():
        cw, pw, rw = W.weights(n, m, mod)
        for alpha in (0.0, 0.5):
            got = _run(gpu, head, z, t, labels, soft, multi, cw, pw, rw, mod, gs, alpha, 2.0)
            assert torch.equal(got[0], want[0]), (name, alpha)
            assert not any(bool((g == SENTINEL).any()) for g in got[1:]), (name, alpha)


# ---- edge rows ---------------------------------------------------------------------------------------------------------
ALL = dict(labels=W.SOFTMAX_MODS["all"], targets=W.SOFTMAX_MODS["all"], multi=W.SIGMOID_MODS["all"])


@pytest.mark.gpu
@pytest.mark.parametrize("head", W.HEADS)
@pytest.mark.parametrize("alpha", [0.0, 0.5])
def test_row_weights_zero_and_unusable(gpu, head, alpha):
    n, m = 7, 257
    z, t, labels, soft, multi = R.inputs(n, m)
    mod = ALL[head]
    cw, pw, _ = W.weights(n, m, mod)
    cw = np.maximum(cw, 0.25)                                         # (every row has a loss: the last assertion below)
    rw = np.array([1.5, 0.0, float("nan"), 2.0, -1.0, float("inf"), 0.25], dtype=np.float32)
    clean_rw = np.where(np.isfinite(rw) & (rw >= 0), rw, 1.0).astype(np.float32)
    clean = _run(gpu, head, z, t, labels, soft, multi, cw, pw, clean_rw, mod, 1.0, alpha, 2.0)
    probs, rows, kd, dl = _run(gpu, head, z, t, labels, soft, multi, cw, pw, rw, mod, 1.0, alpha, 2.0)
    assert torch.equal(probs, clean[0]) and torch.equal(kd, clean[2])              # the KD term stays unweighted
    assert rows[1].item() == 0.0 and dl[1].abs().sum().item() == 0.0               # weight 0: a valid row
    for r in (2, 4, 5):                                                            # NaN, negative, inf: that row only
        assert math.isnan(rows[r].item()) and dl[r].abs().sum().item() == 0.0
    good = [0, 1, 3, 6]
    assert torch.equal(rows[good], clean[1][good]) and torch.equal(dl[good], clean[3][good])
    assert bool(torch.isfinite(rows[good]).all()) and bool(torch.isfinite(dl).all())
    # (row 0 is the dominating-logit row: every p is clipped there, so the softmax head's hard gradient is masked to zero)
    assert all(dl[r].abs().sum().item() > 0 and rows[r].item() != 0 for r in (3, 6)) and rows[0].item() != 0


@pytest.mark.gpu
@pytest.mark.parametrize("head", W.HEADS)
def test_bad_labels_targets_and_teachers_void_their_rows_only(gpu, head):
    n, m = 7, 257
    z, t, labels, soft, multi = R.inputs(n, m)
    mod = ALL[head]
    cw, pw, rw = W.weights(n, m, mod)
    rw[1] = 1.0
    clean = _run(gpu, head, z, t, labels, soft, multi, cw, pw, rw, mod, 1.0, 0.5, 2.0)
    others = [0, 1, 2, 4, 5, 6]
    lab, sf, mu = labels.clone(), soft.clone(), multi.clone()
    lab[3] = m
    sf[3, 256] = float("nan")                                         # the ragged last wave's only element
    mu[3, 256] = float("nan")
    for a in (0.0, 0.5):
        base = clean if a == 0.5 else _run(gpu, head, z, t, labels, soft, multi, cw, pw, rw, mod, 1.0, a, 2.0)
        probs, rows, kd, dl = _run(gpu, head, z, t, lab, sf, mu, cw, pw, rw, mod, 1.0, a, 2.0)
        assert math.isnan(rows[3].item()) and dl[3].abs().sum().item() == 0.0
        assert torch.equal(rows[others], base[1][others]) and torch.equal(dl[others], base[3][others])
        assert torch.equal(probs, base[0]) and bool(torch.isfinite(dl).all())
    # a non-finite teacher logit (alpha > 0)
    bad = t.clone()
    bad[3, 256] = float("nan")
    bad[5, 17] = float("-inf")
    probs, rows, kd, dl = _run(gpu, head, z, bad, labels, soft, multi, cw, pw, rw, mod, 1.0, 0.5, 2.0)
    good = [0, 1, 2, 4, 6]
    for r in (3, 5):
        assert math.isnan(rows[r].item()) and math.isnan(kd[r].item()) and dl[r].abs().sum().item() == 0.0
    assert torch.equal(rows[good], clean[1][good]) and torch.equal(dl[good], clean[3][good]) and torch.equal(probs, clean[0])
    assert bool(torch.isfinite(dl).all())


@pytest.mark.gpu
@pytest.mark.parametrize("head", W.HEADS)
def test_one_class_and_a_dominating_logit_give_finite_results(gpu, head):
    # M = 1: the softmax row is p = 1, x = q / q = 1 -- loss 0, gradient 0, for every gamma (0.5: f' has a pole there)
    z, t, labels, soft, multi = R.inputs(3, 1)
    for g in (0.0, 0.5, 2.0, 8.0):
        mod = dict(gp=g, gn=g)
        cw = np.array([3.0], dtype=np.float32)
        probs, rows, kd, dl = _run(gpu, head, z, t, labels, soft, multi, cw, None, None, mod, 1.0, 0.0, 1.0)
        assert all(bool(torch.isfinite(v).all()) for v in (probs, rows, kd, dl))
        if head != "multi":
            assert rows.abs().sum().item() == 0.0 and dl.abs().sum().item() == 0.0 and bool((probs == 1.0).all())
    # a logit 40 (and 200) above the rest: p at the clip edge, sigmoid saturated; the label / the positives on and off it
    n, m = 4, 257
    z = torch.zeros(n, m)
    z[:, 3] = torch.tensor([40.0, 40.0, 200.0, -200.0])
    labels = torch.tensor([3, 5, 3, 3], dtype=torch.int32)
    soft = torch.full((n, m), 0.1 / m)
    soft[torch.arange(n), labels.long()] += 0.9
    multi = torch.zeros(n, m)
    multi[torch.arange(n), labels.long()] = 1.0
    t = torch.zeros(n, m)
    for name, mod in W.mods_of(head).items():
        cw, pw, rw = W.weights(n, m, mod)
        for alpha in (0.0, 0.5):
            got = _run(gpu, head, z, t, labels, soft, multi, cw, pw, rw, mod, 1.0, alpha, 2.0)
            assert all(bool(torch.isfinite(v).all()) for v in got), (name, alpha)
            ref = W.expected(head, z, t, labels, soft, multi, cw, pw, rw, mod, alpha, 2.0, 1.0)
            scale = W.weight_scale(cw, pw, rw)
            for what, g, r in zip(OUTS, got, ref):
                rtol, atol = W.TOL[what]
                err = np.abs(g.cpu().double().numpy() - r)
                assert (err <= atol * scale + rtol * np.abs(r)).all(), (what, name, alpha, float(err.max()))


@pytest.mark.gpu
def test_ops_wrappers_check_their_tensors(gpu):
    from x3d_tf_amd import hip
    n, m = 3, 11
    z, p = torch.zeros(n, m, device=gpu), torch.empty(n, m, device=gpu)
    lab = torch.zeros(n, dtype=torch.int32, device=gpu)
    cw, rw = torch.ones(m, device=gpu), torch.ones(n, device=gpu)
    for bad in (dict(class_w=rw), dict(row_w=cw), dict(class_w=cw.double()), dict(class_w=torch.ones(2 * m, device=gpu)[::2])):
        with pytest.raises((ValueError, hip.X3DHipError)):
            ops.softmax_xent_w(z, p, labels=lab, **bad)
    with pytest.raises(ValueError):
        ops.softmax_xent_w(z, p)
    with pytest.raises(ValueError):
        ops.softmax_xent_w(z, p, labels=lab, targets=z.clone())
    with pytest.raises(ValueError):
        ops.sigmoid_bce_w(z, None, p)
    with pytest.raises(ValueError):
        ops.sigmoid_bce_w(z, z.clone(), p, pos_w=rw)
    with pytest.raises(hip.X3DHipError, match="gamma"):
        ops.softmax_xent_w(z, p, labels=lab, gamma=8.5)
    with pytest.raises(hip.X3DHipError, match="gamma_neg"):
        ops.sigmoid_bce_w(z, z.clone(), p, gamma_neg=-1.0)
    with pytest.raises(hip.X3DHipError, match="teacher_logits"):
        ops.softmax_xent_w(z, p, labels=lab, class_w=cw, alpha=0.5)
    with pytest.raises(ValueError):
        ops.class_hits(p, lab, torch.zeros(m, dtype=torch.int32, device=gpu), torch.zeros(m, dtype=torch.int64, device=gpu))


# ---- x3d_class_hits ----------------------------------------------------------------------------------------------------
def _count(probs, labels, m):
    hits, counts = np.zeros(m, np.int64), np.zeros(m, np.int64)
    for row, y in zip(probs, labels):
        if 0 <= y < m:
            counts[y] += 1
            hits[y] += int(np.isfinite(row).all() and int(np.argmax(row)) == y)       # first-index arg-max
    return hits, counts


@pytest.mark.gpu
@pytest.mark.parametrize("n", [1, 64, 257])
@pytest.mark.parametrize("m", [1, 157, 400])
@pytest.mark.parametrize("ltype", [torch.int32, torch.int64])
def test_class_hits_against_a_numpy_count(gpu, n, m, ltype):
    g = torch.Generator().manual_seed(31 * n + m)
    probs = torch.softmax(torch.randn(n, m, generator=g), 1)
    labels = torch.randint(0, m, (n,), generator=g)
    hit = torch.rand(n, generator=g) < 0.5
    probs[hit, labels[hit]] = 2.0                                     # about half the rows are hits
    if m > 5:
        for r in range(0, n, 5):                                      # ties for the maximum: the first index wins
            j = int(labels[r])
            probs[r, j] = 2.0
            probs[r, (j + 3) % m] = 2.0
    if n > 8:
        labels[3], labels[7] = -1, m                                  # counted nowhere
        probs[8, 0] = float("nan")                                    # a row that holds a NaN is no hit, but it is counted
    want_h, want_c = _count(probs.numpy(), labels.numpy(), m)
    hits, counts = torch.zeros(m, dtype=torch.int64, device=gpu), torch.zeros(m, dtype=torch.int64, device=gpu)
    p, lab = probs.to(gpu), labels.to(ltype).to(gpu)
    ops.class_hits(p, lab, hits, counts)
    torch.cuda.synchronize()
    assert np.array_equal(hits.cpu().numpy(), want_h) and np.array_equal(counts.cpu().numpy(), want_c)
    assert int(counts.sum()) == n - (2 if n > 8 else 0) and (n < 64 or 0 < int(hits.sum()) < n)
    # the counters are added into, and a second run gives the same
    h2, c2 = torch.zeros_like(hits), torch.zeros_like(counts)
    ops.class_hits(p, lab, h2, c2)
    ops.class_hits(p, lab, hits, counts)
    torch.cuda.synchronize()
    assert torch.equal(h2.cpu(), torch.from_numpy(want_h)) and torch.equal(c2.cpu(), torch.from_numpy(want_c))
    assert torch.equal(hits, 2 * h2) and torch.equal(counts, 2 * c2)


@pytest.mark.gpu
def test_device_metrics_per_class_is_opt_in(gpu):
    from x3d_tf_amd.evaluate import DeviceMetrics
    g = torch.Generator().manual_seed(9)
    n, m = 64, 11
    probs = torch.softmax(torch.randn(n, m, generator=g), 1)
    labels = torch.randint(0, m - 2, (n,), generator=g)               # two classes never occur
    plain, per = DeviceMetrics(), DeviceMetrics(per_class=True)
    for dm in (plain, per):
        dm.update(probs[:40].to(gpu), labels[:40])
        dm.update(probs[40:].to(gpu), labels[40:])
    a, b = plain.result(), per.result()
    assert set(a) == {"loss", "acc", "top_5_acc", "videos"} and set(b) == set(a) | {"mean_class_acc"}
    assert all(a[k] == b[k] for k in a) and plain.class_hits is None
    hits, counts = _count(probs.numpy(), labels.numpy(), m)
    have = counts > 0
    assert have.sum() <= m - 2 and abs(b["mean_class_acc"] - float((hits[have] / counts[have]).mean())) < 1e-12
    assert math.isnan(DeviceMetrics(per_class=True).result()["mean_class_acc"])


# ---- the model ---------------------------------------------------------------------------------------------------------
N, T_, S = 4, 4, 64               # the whole-model training step of test_distill_gpu.py's head-slot tests
VIEWS = ["TEST.NUM_TEMPORAL_VIEWS", 1, "TEST.NUM_SPATIAL_CROPS", 3]


def _model(gpu, overrides=(), dtype=torch.float32):
    from x3d_tf_amd.model import X3D
    from x3d_tf_amd.params import init_params, randomize_bn_
    cfg = x.get_config("XS", VIEWS + list(overrides))
    arch = x.build_arch(cfg)
    m = X3D(cfg, dtype=dtype, device=gpu, seed=0)
    m.load_state_dict(randomize_bn_(init_params(arch, seed=3), seed=4))
    return cfg, arch, m


def _batch(arch, n=N, seed=1):
    g = torch.Generator().manual_seed(seed)
    clips = torch.randn(n, T_, S, S, 3, generator=g)
    labels = torch.randint(0, arch.num_classes, (n,), generator=g)
    mask = (torch.rand(n, arch.fc1_out, generator=g) >= arch.dropout_rate).float()
    return clips, labels, mask


@pytest.mark.gpu
def test_forward_backward_with_sample_and_class_weights(gpu):
    cfg, arch, m = _model(gpu)
    clips, labels, mask = _batch(arch)
    clips = clips.to(gpu)
    m.set_dropout_mask(mask)
    classes = arch.num_classes
    pl = m.forward_backward(clips, labels)
    torch.cuda.synchronize()
    assert pl.fwd[pl.grad_scale_slot][0] == "x3d_softmax_xent" and pl.row_w is None and list(pl._heads) == [(False, False)]
    g_plain = m.flat_grads.clone()

    def plain_launch():
        """the plain head on the logits of the step just run (two steps need not give the same logits to the bit)"""
        p, r, d = torch.empty(N, classes, device=gpu), torch.empty(N, device=gpu), torch.empty(N, classes, device=gpu)
        ops.softmax_xent(pl.logits, pl.labels, p, r, d, 1.0 / N)
        torch.cuda.synchronize()
        return d, r, p

    plain = plain_launch()
    assert all(torch.equal(a, b) for a, b in zip(plain, (pl.dlogits, pl.loss_rows, pl.probs)))

    def launch(row_w, class_w, gamma=0.0):
        p, r, d = torch.empty(N, classes, device=gpu), torch.empty(N, device=gpu), torch.empty(N, classes, device=gpu)
        ops.softmax_xent_w(pl.logits, p, labels=pl.labels, class_w=class_w, row_w=row_w, loss_rows=r, dlogits=d, grad_scale=1.0 / N,
                           gamma=gamma)
        torch.cuda.synchronize()
        return p, r, d

    # weights of all ones: the _w kernel runs and gives the ref-checked kernel's bits; the gradients are the plain step's up to
    # the rounding of the head and the step's own run-to-run spread (the weight-gradient kernels add with fp32 atomics)
    ones = torch.ones(N)
    m.set_loss(class_weights=[1.0] * classes)
    pl = m.forward_backward(clips, labels, sample_weight=ones)
    torch.cuda.synchronize()
    assert pl.fwd[pl.grad_scale_slot][0] == "x3d_softmax_xent_w" and torch.equal(pl.row_w.cpu(), ones)
    p, r, d = launch(pl.row_w, m.loss_mods.class_w)
    assert torch.equal(pl.dlogits, d) and torch.equal(pl.loss_rows, r) and torch.equal(pl.probs, p)
    plain = plain_launch()
    assert torch.equal(pl.probs, plain[2])
    err = (pl.dlogits.double() - plain[0].double()).abs().max().item()
    print(f"all-ones weights against the plain head: dlogits max abs diff {err:.3e}, max |dlogits| {plain[0].abs().max().item():.3e}")
    assert err <= 1e-6 + 1e-3 * plain[0].abs().max().item()
    assert (pl.loss_rows.double() - plain[1].double()).abs().max().item() <= 1e-4 * (1 + plain[1].abs().max().item())
    d1 = pl.dlogits.clone()
    assert (m.flat_grads - g_plain).abs().max().item() <= 1e-3 * g_plain.abs().max().item()
    # doubling every sample weight doubles dlogits bit for bit (a power of two), device weights included
    pl = m.forward_backward(clips, labels, sample_weight=(2.0 * ones).to(gpu))
    torch.cuda.synchronize()
    assert torch.equal(pl.dlogits, 2.0 * launch(ones.to(gpu), m.loss_mods.class_w)[2]) and pl.dlogits.abs().max().item() > 0
    # real weights and a focal exponent: the slot gives what the kernel gives on the plan's logits
    cw = torch.linspace(0.0, 4.0, classes)
    m.set_loss(class_weights=cw, focal_gamma=2.0)
    sw = torch.tensor([0.5, 0.0, 3.0, 1.0])
    pl = m.forward_backward(clips, labels, sample_weight=sw)
    torch.cuda.synchronize()
    p, r, d = launch(sw.to(gpu), cw.to(gpu), 2.0)
    assert torch.equal(pl.dlogits, d) and torch.equal(pl.loss_rows, r) and pl.dlogits[1].abs().sum().item() == 0.0
    assert not torch.equal(pl.dlogits, d1) and bool(torch.isfinite(m.flat_grads).all())
    # and off again: the recorded plain entry, the plain gradient
    m.set_loss()
    pl = m.forward_backward(clips, labels)
    torch.cuda.synchronize()
    assert pl.fwd[pl.grad_scale_slot][0] == "x3d_softmax_xent" and torch.equal(pl.dlogits, plain_launch()[0])
    assert (m.flat_grads - g_plain).abs().max().item() <= 1e-3 * g_plain.abs().max().item()
    # arguments
    for bad in (torch.ones(N + 1), torch.tensor([1.0, -1.0, 1.0, 1.0]), torch.tensor([1.0, float("nan"), 1.0, 1.0]),
                torch.ones(N, 1, 1)):
        with pytest.raises(ValueError):
            m.forward_backward(clips, labels, sample_weight=bad)


# ---- Trainer -----------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("mode", ["bf16", "fp16-device-scale", "multi-fp16-device-scale"])
def test_trainer_step_with_loss_settings(gpu, mode):
    from x3d_tf_amd.train import Trainer
    multi = mode.startswith("multi")
    classes = 157 if multi else 400
    cw = [0.5 + 0.5 * (c % 4) for c in range(classes)]
    over = ["LOSS.CLASS_WEIGHTS", cw, "LOSS.FOCAL_GAMMA", 2.0]
    if multi:
        over += ["DATA.MULTI_LABEL", True, "NETWORK.NUM_CLASSES", classes, "LOSS.POS_WEIGHT", [2.0] * classes, "LOSS.FOCAL_GAMMA_NEG", 1.0]
    if "fp16" in mode:
        over += ["SOLVER.DEVICE_LOSS_SCALE", True]
    cfg, arch, m = _model(gpu, over, dtype=torch.bfloat16 if mode == "bf16" else torch.float16)
    tr = Trainer(m, cfg)
    assert m.loss_mods is not None and m.loss_mods.gamma == 2.0 and m.loss_mods.class_w.tolist() == cw
    assert ("fp16" in mode) == (tr._dls is not None)
    clips, labels, mask = _batch(arch)
    m.set_dropout_mask(mask)
    if multi:
        labels = (torch.rand(N, classes, generator=torch.Generator().manual_seed(5)) < 0.05).float()
    before = m.flat_params[:m.n_trainable_flat].clone()
    sw = torch.tensor([1.0, 2.0, 0.0, 0.5])
    for weights in (None, sw):
        pl = tr.step(clips.to(gpu), labels, 0.01, **({} if weights is None else dict(sample_weight=weights)))
        assert pl.fwd[pl.grad_scale_slot][0] == ("x3d_sigmoid_bce_w" if multi else "x3d_softmax_xent_w")
        loss = float(tr.loss(pl))
        assert math.isfinite(loss) and loss > 0, loss
    assert pl.loss_rows[2].item() == 0.0 and pl.dlogits[2].abs().sum().item() == 0.0
    after = m.flat_params[:m.n_trainable_flat]
    print(f"{mode}: loss {loss:.4f}, updates applied {tr.opt_step}, skipped {tr.skipped_steps}")
    assert bool(torch.isfinite(after).all()) and not torch.equal(after, before)


def _batches(gpu, steps, weights=True, seed=7):
    g = torch.Generator().manual_seed(seed)
    for _ in range(steps):
        clips = torch.randn(N, T_, S, S, 3, generator=g).to(gpu)
        labels = torch.randint(0, 5, (N,), generator=g)
        yield (clips, labels, torch.rand(N, generator=g) * 2) if weights else (clips, labels)


@pytest.mark.gpu
def test_fit_takes_weighted_batches_and_fills_mean_class_acc(gpu):
    from x3d_tf_amd.train import Trainer
    over = ["TRAIN.EPOCHS", 2, "LOSS.FOCAL_GAMMA", 1.0]
    cfg, arch, m = _model(gpu, over)
    tr = Trainer(m, cfg)
    val = [(torch.randn(3 * 2, T_, S, S, 3, generator=torch.Generator().manual_seed(2)).to(gpu), torch.tensor([1, 4]))]
    hist = tr.fit(_batches(gpu, 4), steps_per_epoch=2, metrics=("acc", "mean_class_acc"), validation_data=val)
    h = tr.history
    assert len(hist) == 2 and all(np.isfinite(hist))
    assert set(h) == {"loss", "lr", "acc", "mean_class_acc", "val_loss", "val_acc", "val_top_5_acc", "val_mean_class_acc"}
    for k in ("mean_class_acc", "val_mean_class_acc", "acc"):
        assert len(h[k]) == 2 and all(0.0 <= v <= 1.0 for v in h[k]), (k, h[k])
    # 2-tuples still work, the metric stays opt-in, and it is refused for a multi-label model
    tr.epoch = 0
    tr.fit(_batches(gpu, 2, weights=False), steps_per_epoch=1, epochs=1)
    assert set(tr.history) == {"loss", "lr", "acc", "top_5_acc"}
    with pytest.raises(ValueError, match="unknown metrics"):
        tr.fit(_batches(gpu, 2), steps_per_epoch=1, epochs=3, metrics=("mean_acc",))


@pytest.mark.gpu
def test_sample_weight_with_mixup_raises(gpu):
    from x3d_tf_amd.train import Trainer
    cfg, arch, m = _model(gpu, ["MIXUP.ENABLE", True, "LOSS.CLASS_WEIGHTS", [1.0] * 400])
    tr = Trainer(m, cfg)
    clips, labels, mask = _batch(arch)
    before = m.flat_params.clone()
    with pytest.raises(ValueError, match="sample_weight"):
        tr.step(clips.to(gpu), labels, 0.01, sample_weight=torch.ones(N))
    assert torch.equal(m.flat_params, before)
    pl = tr.step(clips.to(gpu), labels, 0.01)                                       # class weights with mixup are fine
    torch.cuda.synchronize()
    assert pl.fwd[pl.grad_scale_slot][0] == "x3d_softmax_xent_w" and bool(torch.isfinite(pl.loss_rows).all())
    # label smoothing alone mixes nothing: sample weights are fine
    cfg, arch, m = _model(gpu, ["TRAIN.LABEL_SMOOTHING", 0.1])
    pl = Trainer(m, cfg).step(clips.to(gpu), labels, 0.01, sample_weight=torch.ones(N))
    torch.cuda.synchronize()
    assert pl.fwd[pl.grad_scale_slot][0] == "x3d_softmax_xent_w" and bool(torch.isfinite(pl.loss_rows).all())
