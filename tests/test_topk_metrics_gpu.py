"""x3d_topk_metrics (ops.topk_metrics, evaluate.DeviceMetrics) against an fp64 numpy restatement of its three row rules:
the Keras cross-entropy on probabilities, tf.math.in_top_k (SparseTopKCategoricalAccuracy) and the first-index argmax
(SparseCategoricalAccuracy)."""
import os
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from x3d_tf_amd import hip, ops  # noqa: E402
from x3d_tf_amd.evaluate import DeviceMetrics, Metrics  # noqa: E402


def _ref(probs, labels, k):
    """[loss sum, top-1 hits, top-k hits, rows] in fp64, row by row."""
    p = np.asarray(probs, dtype=np.float32)
    loss, t1, tk = 0.0, 0, 0
    n, m = p.shape
    for i in range(n):
        y = int(labels[i])
        row = p[i]
        if not 0 <= y < m:
            loss += float("nan")
            continue
        q = np.clip(row.astype(np.float64), 1e-7, 1.0 - 1e-7)
        loss += -np.log(q[y]) + np.log(q.sum())
        if not np.all(np.isfinite(row)):
            continue
        above = int((row > row[y]).sum())
        tk += above < k
        t1 += above == 0 and not np.any(row[:y] == row[y])
    return np.array([loss, t1, tk, n], dtype=np.float64)


def _run(probs, labels, k, gpu, acc=None):
    acc = torch.zeros(4, dtype=torch.float64, device=gpu) if acc is None else acc
    ops.topk_metrics(torch.as_tensor(probs).to(gpu), torch.as_tensor(labels).to(gpu), acc, k)
    torch.cuda.synchronize()
    return acc


def _check(got, want):
    got = got.cpu().numpy()
    assert got[1:].tolist() == want[1:].tolist()
    if np.isnan(want[0]):
        assert np.isnan(got[0])
    else:
        assert abs(got[0] - want[0]) <= 1e-12 * abs(want[0]), (got[0], want[0])


@pytest.mark.gpu
@pytest.mark.parametrize("n", [1, 3, 64, 257, 2000])
@pytest.mark.parametrize("m", [1, 5, 400, 401])
@pytest.mark.parametrize("k", [1, 5])
@pytest.mark.parametrize("ldt", [np.int32, np.int64])
def test_random_rows_match_the_fp64_rules(gpu, n, m, k, ldt):
    rng = np.random.default_rng(n * 1000 + m * 10 + k)
    z = rng.standard_normal((n, m)) * 3
    p = np.exp(z - z.max(1, keepdims=True))
    probs = (p / p.sum(1, keepdims=True)).astype(np.float32)
    labels = rng.integers(0, m, n).astype(ldt)
    if m >= 5:   # make some rows hits: the label at the argmax
        hit = rng.random(n) < 0.3
        labels[hit] = probs[hit].argmax(1)
    _check(_run(probs, labels, k, gpu), _ref(probs, labels, k))


@pytest.mark.gpu
def test_constructed_rows(gpu):
    m = 8
    rows, labels, expect = [], [], []   # expect: (top-1 hit, top-5 hit)

    def add(row, y, t1, t5):
        rows.append(np.asarray(row, np.float32))
        labels.append(y)
        expect.append((t1, t5))

    base = [0.30, 0.20, 0.15, 0.10, 0.08, 0.08, 0.05, 0.04]
    add(base, 4, 0, 1)        # tied with the 5th largest (4 larger values): in_top_k hit
    add(base, 5, 0, 1)        # the other one of the tie: a hit as well
    add(base, 6, 0, 0)        # 6th largest: 6 larger values
    tie_max = [0.1, 0.35, 0.1, 0.35, 0.02, 0.02, 0.03, 0.03]
    add(tie_max, 3, 0, 1)     # tied for the maximum with a smaller index: top-1 miss
    add(tie_max, 1, 1, 1)     # the first index of the tied maximum: top-1 hit
    for bad in (np.inf, -np.inf, np.nan):
        r = list(base)
        r[7] = bad
        add(r, 0, 0, 0)       # a non-finite value anywhere in the row: no hit for either
        r = list(base)
        r[0] = bad
        add(r, 1, 0, 0)
    probs = np.stack(rows)
    lab = np.asarray(labels, np.int64)
    acc = _run(probs, lab, 5, gpu).cpu().numpy()
    want = _ref(probs, lab, 5)
    assert acc[1] == sum(e[0] for e in expect) == want[1]
    assert acc[2] == sum(e[1] for e in expect) == want[2]
    assert acc[3] == len(rows)
    # one row at a time: every row's own verdict
    for row, y, (t1, t5) in zip(rows, labels, expect):
        a = _run(row[None], np.asarray([y], np.int32), 5, gpu).cpu().numpy()
        assert (a[1], a[2]) == (t1, t5), (row, y)


@pytest.mark.gpu
@pytest.mark.parametrize("ldt", [np.int32, np.int64])
def test_out_of_range_label_counts_the_row_without_a_hit(gpu, ldt):
    probs = np.full((4, 5), 0.2, np.float32)
    probs[:, 0] = 0.6
    probs /= probs.sum(1, keepdims=True)
    for bad in (-1, 5, 1000):
        labels = np.asarray([0, bad, 0, 0], ldt)
        acc = _run(probs, labels, 5, gpu).cpu().numpy()
        assert np.isnan(acc[0]) and acc[1] == 3 and acc[2] == 3 and acc[3] == 4
    big = np.asarray([0, 0, 0, 2 ** 32], np.int64)   # an int64 label is not truncated to 32 bits
    acc = _run(probs, big, 5, gpu).cpu().numpy()
    assert np.isnan(acc[0]) and acc[1] == 3 and acc[2] == 3


@pytest.mark.gpu
def test_fewer_classes_than_k_every_valid_row_hits(gpu):
    rng = np.random.default_rng(3)
    probs = rng.random((50, 3)).astype(np.float32)
    labels = rng.integers(0, 3, 50).astype(np.int32)
    labels[7] = 3                                  # out of range: no hit
    probs[9, 2] = np.nan                           # non-finite: no hit
    acc = _run(probs, labels, 5, gpu).cpu().numpy()
    assert acc[2] == 48 and acc[3] == 50
    _check(torch.as_tensor(acc), _ref(probs, labels, 5))


@pytest.mark.gpu
def test_counters_are_deterministic_and_add_up(gpu):
    rng = np.random.default_rng(11)
    probs = torch.from_numpy(rng.dirichlet(np.ones(400) * 0.3, 2000).astype(np.float32)).to(gpu)
    labels = torch.from_numpy(rng.integers(0, 400, 2000)).to(gpu)
    a = torch.zeros(4, dtype=torch.float64, device=gpu)
    b = torch.zeros(4, dtype=torch.float64, device=gpu)
    ops.topk_metrics(probs, labels, a, 5)
    ops.topk_metrics(probs, labels, b, 5)
    torch.cuda.synchronize()
    assert torch.equal(a, b)                       # bit-identical, loss sum included
    one = a.clone()
    ops.topk_metrics(probs, labels, a, 5)
    ops.topk_metrics(probs[:700], labels[:700], a, 5)
    torch.cuda.synchronize()
    part = torch.zeros(4, dtype=torch.float64, device=gpu)
    ops.topk_metrics(probs[:700], labels[:700], part, 5)
    torch.cuda.synchronize()
    assert torch.equal(a[1:], 2 * one[1:] + part[1:])
    assert abs(a[0].item() - (2 * one[0].item() + part[0].item())) <= 1e-12 * a[0].item()


@pytest.mark.gpu
def test_device_metrics_equals_metrics_on_tie_free_batches(gpu):
    rng = np.random.default_rng(5)
    reg = 0.0123
    dm, hm = DeviceMetrics(torch.tensor([reg], dtype=torch.float64, device=gpu)), Metrics(reg)
    for n in (7, 64, 33):
        z = np.stack([rng.permutation(400) / 40.0 for _ in range(n)])   # logits 0.025 apart: no two probabilities tie
        p = np.exp(z - z.max(1, keepdims=True))
        probs = torch.from_numpy((p / p.sum(1, keepdims=True)).astype(np.float32)).to(gpu)
        for r in probs.cpu().numpy():
            assert len(np.unique(r)) == r.size
        labels = torch.from_numpy(rng.integers(0, 400, n))
        labels[: n // 3] = probs[: n // 3].argmax(1).cpu()
        labels[n // 3: n // 2] = probs[n // 3: n // 2].topk(4, dim=1).indices[:, 3].cpu()
        dm.update(probs, labels if n != 64 else labels.to(gpu).int())   # host int64 and device int32 labels
        hm.update(probs, labels)
    got, want = dm.result(), hm.result()
    assert got["videos"] == want["videos"] == 104
    assert got["acc"] == want["acc"] and got["top_5_acc"] == want["top_5_acc"]
    assert abs(got["loss"] - want["loss"]) <= 1e-12 * abs(want["loss"])
    assert want["acc"] > 0.25 and want["top_5_acc"] > want["acc"]


@pytest.mark.gpu
def test_wrapper_refuses_bad_inputs(gpu):
    probs = torch.rand(4, 10, device=gpu)
    labels = torch.zeros(4, dtype=torch.int64, device=gpu)
    acc = torch.zeros(4, dtype=torch.float64, device=gpu)
    with pytest.raises(hip.X3DHipError):
        ops.topk_metrics(probs.cpu(), labels, acc)
    with pytest.raises(hip.X3DHipError):
        ops.topk_metrics(probs, labels.cpu(), acc)
    with pytest.raises(hip.X3DHipError):
        ops.topk_metrics(probs, labels, acc.cpu())
    with pytest.raises(hip.X3DHipError):
        ops.topk_metrics(torch.rand(10, 4, device=gpu).t(), labels, acc)          # non-contiguous
    with pytest.raises(ValueError):
        ops.topk_metrics(probs.double(), labels, acc)
    with pytest.raises(ValueError):
        ops.topk_metrics(probs.half(), labels, acc)
    with pytest.raises(ValueError):
        ops.topk_metrics(probs, labels.short(), acc)
    with pytest.raises(ValueError):
        ops.topk_metrics(probs, labels.float(), acc)
    with pytest.raises(ValueError):
        ops.topk_metrics(probs, labels[:3], acc)
    with pytest.raises(ValueError):
        ops.topk_metrics(probs, labels, acc.float())
    with pytest.raises(ValueError):
        ops.topk_metrics(probs, labels, torch.zeros(3, dtype=torch.float64, device=gpu))
    with pytest.raises(ValueError):
        ops.topk_metrics(probs, labels, acc, k=0)
    torch.cuda.synchronize()
    assert torch.equal(acc, torch.zeros_like(acc))                                # nothing was launched
