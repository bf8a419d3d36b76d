"""Precise BatchNorm on the device: x3d_precise_bn_accum / x3d_precise_bn_final against x3d_bn_finalize (bit for bit, one batch)
and against the fp64 restatement tests/precise_bn_ref.py (several batches and shapes), precise_bn.update_bn_stats on a model,
and the Trainer / fit paths built on it (NETWORK.BN.USE_PRECISE_STATS).

The 1-ulp limit of the comparisons with precise_bn_ref, derived: the device and numpy add the same fp64 terms -- at most 32
copies and 5 batches, about 40 terms -- in different orders, which moves a sum by at most 40 * 2^-53 of the sum of the terms'
magnitudes; the terms of S2 are positive, those of S1 have one sign wherever |mean| exceeds a fraction of the standard
deviation.  mean = S1 / n inherits that; var = S2 / n - mean^2 amplifies it by (mean^2 + var) / var, at most 10 for data drawn
with |mean| <= 3 std.  So the fp64 results agree to about 1e-14 relative, far inside half an fp32 ulp (6e-8): the rounded values
are the same unless the exact value sits on a rounding boundary, where they are neighbours.  Hence 1 ulp, not 0."""
import itertools
import os
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from tests import precise_bn_ref as R  # noqa: E402

SENTINEL = 12345.0


def _bits(t):
    return t.detach().cpu().contiguous().view(torch.int32).numpy()


def _layout(c):
    from x3d_tf_amd import hip
    return hip.stats_layout(c)


def _fill(stats, c, s1, s2):
    """stats: host [replicas][stride] fp64 zeros <- per-replica sums s1, s2 [replicas][c]"""
    stats[:, 0:2 * c:2] = s1
    stats[:, 1:2 * c:2] = s2


def _table(rows, dev):
    return torch.tensor(rows, dtype=torch.int64).to(dev)


def _accum(table, pooled):
    from x3d_tf_amd import hip
    hip.call("x3d_precise_bn_accum", table.data_ptr(), table.shape[0], pooled.data_ptr())


def _final(table, pooled, params):
    from x3d_tf_amd import hip
    hip.call("x3d_precise_bn_final", table.data_ptr(), table.shape[0], pooled.data_ptr(), params.data_ptr())


# ---- kernels: one batch is x3d_bn_finalize(momentum = 0), bit for bit ------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("count", [1, 8])
@pytest.mark.parametrize("c", [1, 3, 24, 54, 432, 2048])
def test_one_batch_equals_bn_finalize_bit_for_bit(gpu, c, count):
    """all 32 copies hold random sums consistent with `count` elements (S2 >= S1^2 / n; every fifth channel has S2 = S1^2 / n
    up to rounding, where the variance clamps at 0).  count = 1: no Bessel factor.  C = 2048: two steps of the channel loop."""
    from x3d_tf_amd import ops
    reps, stride = _layout(c)
    rng = np.random.default_rng(1000 * c + count)
    s1 = rng.normal(0.3, 1.0, size=(reps, c)) * count / reps
    S1 = s1.sum(axis=0)
    spread = rng.uniform(0.0, 4.0, size=c)
    spread[::5] = 0.0
    S2 = S1 * S1 / count * (1.0 + spread)
    wts = rng.uniform(0.5, 1.5, size=(reps, c))
    s2 = S2 * wts / wts.sum(axis=0)
    host = np.zeros((reps, stride))
    _fill(host, c, s1, s2)
    stats = torch.from_numpy(host.ravel()).to(gpu)
    gen = torch.Generator().manual_seed(c)
    mean0, var0 = torch.randn(c, generator=gen).to(gpu), (torch.rand(c, generator=gen) + 0.5).to(gpu)
    gamma, beta = torch.ones(c, device=gpu), torch.zeros(c, device=gpu)
    ss, mi = torch.empty(c, 2, device=gpu), torch.empty(c, 2, device=gpu)
    ops.bn_finalize(stats, count, gamma, beta, mean0, var0, 1e-5, 0.0, 1, ss, mi)
    pooled = torch.zeros(1 + 2 * c, dtype=torch.float64, device=gpu)
    params = torch.full((2 * c + 3,), SENTINEL, device=gpu)
    table = _table([[stats.data_ptr(), c, count, 1, 1 + c, 1]], gpu)        # mean at params[1:], variance behind it
    _accum(table, pooled)
    _final(table, pooled, params)
    torch.cuda.synchronize()
    assert float(pooled[0]) == count
    assert np.array_equal(_bits(params[1:1 + c]), _bits(mean0)), "moving_mean"
    assert np.array_equal(_bits(params[1 + c:1 + 2 * c]), _bits(var0)), "moving_variance"
    assert torch.isfinite(params).all() and float(params[1 + c:1 + 2 * c].min()) >= 0.0
    assert params[0] == SENTINEL and bool((params[1 + 2 * c:] == SENTINEL).all())     # nothing outside the two tensors


# ---- kernels: several batches, two tables, three layers in one launch -----------------------------------------------------------
CS = (3, 54, 432)
PER_REPLICA = (6, 10)          # elements per channel and copy of the two tables: counts 192 and 320
ORDER = (0, 1, 0, 0, 1)        # K = 5 accumulate calls


def _two_tables(gpu):
    """per table and layer: data ~ N(mu, sigma) with |mu| <= 3 sigma, split over the 32 copies; returns the device tables, what
    keeps their buffers alive, and per table the reference (sums [c][2], count) of every layer"""
    rng = np.random.default_rng(7)
    nl = len(CS)
    pooled_off = np.cumsum([nl] + [2 * c for c in CS])
    mean_off = np.cumsum([0] + [2 * c + 4 for c in CS])            # [mean | var | 4 floats of padding] per layer
    tables, keep, refs = [], [], []
    for per in PER_REPLICA:
        rows, ref = [], []
        for l, c in enumerate(CS):
            reps, stride = _layout(c)
            sigma = rng.uniform(0.5, 2.0, size=c)
            mu = rng.uniform(-3.0, 3.0, size=c) * sigma
            data = rng.normal(mu, sigma, size=(reps, per, c))
            host = np.zeros((reps, stride))
            _fill(host, c, data.sum(axis=1), (data * data).sum(axis=1))
            dev = torch.from_numpy(host.ravel()).to(gpu)
            keep.append(dev)
            rows.append([dev.data_ptr(), c, reps * per, int(mean_off[l]), int(mean_off[l]) + c, int(pooled_off[l])])
            ref.append((R.replica_sum(host.ravel(), c, reps, stride), reps * per))
        tables.append(_table(rows, gpu))
        refs.append(ref)
    return tables, keep, refs, int(pooled_off[-1]), int(mean_off[-1]), mean_off


@pytest.mark.gpu
def test_five_batches_from_two_tables_against_the_reference(gpu):
    tables, keep, refs, pooled_size, params_size, mean_off = _two_tables(gpu)
    runs = []
    for _ in range(2):
        pooled = torch.zeros(pooled_size, dtype=torch.float64, device=gpu)
        for k in ORDER:
            _accum(tables[k], pooled)
        runs.append(pooled)
    params = torch.full((params_size,), SENTINEL, device=gpu)
    _final(tables[1], runs[0], params)
    torch.cuda.synchronize()
    a, b = (p.cpu().numpy() for p in runs)
    assert np.array_equal(a.view(np.int64), b.view(np.int64))           # reproducible bit for bit
    got = params.cpu().numpy()
    worst = 0.0
    for l, c in enumerate(CS):
        sums, n = R.pool([refs[k][l] for k in ORDER])
        assert a[l] == n == sum(32 * PER_REPLICA[k] for k in ORDER)
        mean, unb = R.final(sums, n)
        o = int(mean_off[l])
        u = max(R.ulps(got[o:o + c], mean).max(), R.ulps(got[o + c:o + 2 * c], unb).max())
        worst = max(worst, u)
        assert np.all(got[o + 2 * c:o + 2 * c + 4] == SENTINEL)          # the padding between the layers
    print(f"worst distance from the fp64 reference: {worst} ulp")
    assert worst <= 1.0


# ---- the model -------------------------------------------------------------------------------------------------------------
CLASSES = 10
OPTS = ["DATA.TEMP_DURATION", 4, "DATA.TRAIN_CROP_SIZE", 32, "DATA.TEST_CROP_SIZE", 32, "TEST.NUM_TEMPORAL_VIEWS", 1,
        "TEST.NUM_SPATIAL_CROPS", 3, "TEST.BATCH_SIZE", 2, "NETWORK.NUM_CLASSES", CLASSES, "NETWORK.DROPOUT_RATE", 0.0,
        "TRAIN.BATCH_SIZE", 2, "TRAIN.DATASET_SIZE", 4, "TRAIN.EPOCHS", 2]


def _cfg(*extra):
    import x3d_tf_amd as x
    return x.get_config("XS", OPTS + list(extra))


def _batches(k, seed=5, views=1, n=2):
    gen = torch.Generator().manual_seed(seed)
    return [(torch.randn(n * views, 4, 32, 32, 3, generator=gen), torch.randint(0, CLASSES, (n,), generator=gen))
            for _ in range(k)]


def _trainer(cfg, gpu, seed=1):
    from x3d_tf_amd.model import X3D
    from x3d_tf_amd.train import Trainer
    m = X3D(cfg, dtype=torch.float32, device=gpu, seed=seed)
    return m, Trainer(m, cfg)


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["fp32", "bf16"])
def test_update_bn_stats_on_a_model(gpu, dtype):
    """three batches, two plans (N = 2, 2, 3).  The reference pools the raw sums of a second run of the same forward passes, so the
    storage type does not enter the comparison."""
    from x3d_tf_amd.model import X3D
    from x3d_tf_amd.precise_bn import update_bn_stats
    m = X3D(_cfg(), dtype=dtype, device=gpu, seed=1)
    gen = torch.Generator().manual_seed(11)
    clips = [torch.randn(n, 4, 32, 32, 3, generator=gen).to(gpu) for n in (2, 2, 3)]
    m.moving_stats_flat().fill_(SENTINEL)
    trainable = m.flat_params[:m.n_trainable_flat].clone()
    assert update_bn_stats(m, [(c, None) for c in clips[:2]] + [clips[2]], 3) == 3     # (clips, labels) items and bare clips
    got = {k: v.detach().cpu().numpy().copy() for k, v in m.params.items() if k.endswith(("/moving_mean", "/moving_variance"))}
    assert torch.equal(m.flat_params[:m.n_trainable_flat], trainable)
    assert len({(c.shape[0]) for c in clips}) == 2 and len([k for k in m._plans if k[-1]]) == 2
    per_layer = {}
    for c in clips:
        m(c, training=True)
        pl = m._plan(*c.shape[:4], True)
        torch.cuda.synchronize()
        for b in pl.bn_layers:
            reps, stride = _layout(b.c)
            raw = pl._zero_views[b.stats].cpu().numpy()
            per_layer.setdefault(b.prefix, []).append((R.replica_sum(raw, b.c, reps, stride), b.count))
    assert len(per_layer) * 2 == len(got)
    worst = 0.0
    for prefix, parts in per_layer.items():
        sums, n = R.pool(parts)
        mean, unb = R.final(sums, n)
        gm, gv = got[f"{prefix}/moving_mean"], got[f"{prefix}/moving_variance"]
        assert not np.any(gm == SENTINEL) and not np.any(gv == SENTINEL), prefix
        worst = max(worst, R.ulps(gm, mean).max(), R.ulps(gv, unb).max())
    print(f"{dtype}: worst distance from the pooled fp64 reference: {worst} ulp")
    assert worst <= 1.0
    # fewer batches than asked for: allowed, and reported
    assert update_bn_stats(m, iter(clips[:2]), 5) == 2


def _twin_after_the_same_steps(cfg, gpu, steps, m, tr):
    """A twin trainer from the same seed that runs `steps` by hand, as fit did, and then takes fit's weights (and EMA weights).
    It has to take them: the backward pass adds some weight gradients with fp32 atomics (tests/test_solver_gpu.py measures that
    run-to-run spread), so two runs of the same steps do not end on the same bits -- on an MI355X the twin's weights were up to
    3.9e-5 away from fit's after these two steps, and its validation loss 10.0331 against 10.0294.  The statistics blocks are
    NOT copied: the twin's hold its own momentum blend, which precise_bn has to discard."""
    from x3d_tf_amd.train import lr_schedule
    m2, tw = _trainer(cfg, gpu)
    for clips, labels in steps:
        tw.step(clips, labels, lr_schedule(0, cfg))
    nt = m.n_trainable_flat
    print("twin's weights after the same steps, max |difference| from fit's:", float((m2.flat_params[:nt] - m.flat_params[:nt]).abs().max()))
    m2.flat_params[:nt].copy_(m.flat_params[:nt])
    if tr.ema is not None:
        tw.ema[:nt].copy_(tr.ema[:nt])
    return m2, tw


@pytest.mark.gpu
def test_fit_runs_precise_bn_before_validation(gpu):
    """fit with the switch on against a twin from the same seed that runs the same steps by hand, then precise_bn on the batches
    that follow, then validate: the same statistics and the same validation loss, bit for bit"""
    cfg = _cfg("NETWORK.BN.USE_PRECISE_STATS", True, "NETWORK.BN.NUM_BATCHES_PRECISE", 2)
    data = [(a.to(gpu), b.to(gpu)) for a, b in _batches(4, seed=7)]
    val = [(a.to(gpu), b.to(gpu)) for a, b in _batches(2, seed=9, views=3)]
    m, tr = _trainer(cfg, gpu)
    tr.fit(iter(data), epochs=1, validation_data=lambda: val, metrics=())
    m2, tw = _twin_after_the_same_steps(cfg, gpu, data[:2], m, tr)
    momentum_blend = m2.moving_stats_flat().clone()
    assert tw.precise_bn(iter(data[2:])) == 2
    assert not torch.equal(m2.moving_stats_flat(), momentum_blend)
    r = tw.validate(val)
    print("val_loss: fit", repr(tr.history["val_loss"][0]), "twin", repr(r["loss"]))
    assert torch.equal(m2.moving_stats_flat(), m.moving_stats_flat())
    assert tr.history["val_loss"] == [r["loss"]]


@pytest.mark.gpu
def test_fit_with_ema_gives_each_model_its_own_statistics(gpu):
    """SOLVER.EMA_DECAY = 0.5: after fit the statistics block of trainer.ema is what precise_bn inside ema_scope gives (from the
    batches after the raw weights' own), flat_params holds the raw weights' statistics, and the two differ"""
    cfg = _cfg("NETWORK.BN.USE_PRECISE_STATS", True, "NETWORK.BN.NUM_BATCHES_PRECISE", 2, "SOLVER.EMA_DECAY", 0.5)
    data = [(a.to(gpu), b.to(gpu)) for a, b in _batches(6, seed=7)]
    val = [(a.to(gpu), b.to(gpu)) for a, b in _batches(2, seed=9, views=3)]
    m, tr = _trainer(cfg, gpu)
    tr.fit(iter(data), epochs=1, validation_data=lambda: val, metrics=())
    nt = m.n_trainable_flat
    m2, tw = _twin_after_the_same_steps(cfg, gpu, data[:2], m, tr)
    assert tw.precise_bn(iter(data[2:4])) == 2
    with tw.ema_scope():
        assert tw.precise_bn(iter(data[4:6])) == 2
        r = tw.validate(val)
    assert torch.equal(tw.ema[nt:], tr.ema[nt:])                          # the EMA model's own statistics
    assert torch.equal(m2.flat_params[nt:], m.flat_params[nt:])           # the raw weights' statistics
    assert not torch.equal(tr.ema[nt:], m.flat_params[nt:])
    assert tr.history["val_loss"] == [r["loss"]]                          # EMA_EVAL: validation ran on the EMA model


@pytest.mark.gpu
def test_precise_bn_leaves_the_drop_path_stream_alone(gpu):
    cfg = _cfg("NETWORK.DROP_PATH_RATE", 0.2)
    data = [(a.to(gpu), b.to(gpu)) for a, b in _batches(3, seed=7)]
    m, tr = _trainer(cfg, gpu)
    tr.step(*data[0], 0.1)
    before, state = m.drop_path_step(), m._dp_state.clone()
    assert before == 1
    assert tr.precise_bn(iter(data), 3) == 3
    assert m.drop_path_step() == before and torch.equal(m._dp_state, state)


class _Counting:
    """an endless iterator over `data` that counts what was drawn"""

    def __init__(self, data):
        self.it, self.drawn = itertools.cycle(data), 0

    def __iter__(self):
        return self

    def __next__(self):
        self.drawn += 1
        return next(self.it)


@pytest.mark.gpu
def test_fit_draws_what_it_drew_unless_switched_on(gpu, monkeypatch):
    """off (the default): epochs * steps batches, and neither new entry point is called.  On with NUM_BATCHES_PRECISE = 2:
    epochs * (steps + 2); with EMA epochs * (steps + 4); with precise_bn_data the training iterator is left alone."""
    from x3d_tf_amd import hip
    data = [(a.to(gpu), b.to(gpu)) for a, b in _batches(3, seed=7)]
    on = ["NETWORK.BN.USE_PRECISE_STATS", True, "NETWORK.BN.NUM_BATCHES_PRECISE", 2]
    calls = []
    real = hip.call

    def recorder(name, *args):
        calls.append(name)
        return real(name, *args)
    monkeypatch.setattr(hip, "call", recorder)
    new = ["x3d_precise_bn_accum", "x3d_precise_bn_final"]
    for extra, per_epoch, want in (([], 2, [0, 0]), (on, 4, [4, 2]), (on + ["SOLVER.EMA_DECAY", 0.5], 6, [8, 4])):
        src = _Counting(data)
        calls.clear()
        _trainer(_cfg(*extra), gpu)[1].fit(src, metrics=())
        assert src.drawn == 2 * per_epoch, (extra, src.drawn)
        assert [calls.count(k) for k in new] == want, extra
    src, fresh = _Counting(data), []

    def precise_source():
        fresh.append(_Counting(data))
        return fresh[-1]
    _trainer(_cfg(*on), gpu)[1].fit(src, metrics=(), precise_bn_data=precise_source)
    assert src.drawn == 4 and [f.drawn for f in fresh] == [2, 2]
    with pytest.raises(ValueError, match="precise_bn_data"):
        _trainer(_cfg(*on), gpu)[1].fit(src, metrics=(), precise_bn_data=data)


# ---- the all-reduce of the pooled buffer, as far as one rank can show it -------------------------------------------------------
def _free_port():
    import socket
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _rehearsal_worker(rank, port, tmp):
    """one rank with every collective live (X3D_DIST_REHEARSE=1): the pooled buffer goes through a real all-reduce"""
    sys.path.insert(0, ROOT)
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK="0", WORLD_SIZE="1", LOCAL_RANK="0",
                      X3D_DIST_BACKEND="gloo", X3D_DIST_REHEARSE="1")
    import torch.distributed as dist
    from x3d_tf_amd import dist as xd
    xd.init_process_group()
    dev = torch.device("cuda:0")
    torch.cuda.set_device(dev)
    m, tr = _trainer(_cfg(), dev)
    assert tr.collectives
    reduced = []
    real = dist.all_reduce

    def counting(t, *a, **k):
        reduced.append((t.dtype, t.numel()))
        return real(t, *a, **k)
    dist.all_reduce = counting
    used = tr.precise_bn([(a.to(dev), b) for a, b in _batches(2, seed=7)], 2)
    dist.all_reduce = real
    assert used == 2 and reduced == [(torch.float64, m.precise_bn_layout().pooled_size)], reduced
    torch.save(m.moving_stats_flat().cpu(), os.path.join(tmp, "stats.pt"))
    dist.barrier()
    dist.destroy_process_group()


@pytest.mark.gpu
def test_pooled_all_reduce_in_a_one_rank_rehearsal(gpu, tmp_path):
    """one fp64 all-reduce of the whole pooled buffer, and -- the sum over one rank being the identity -- the statistics of a run
    without a process group, bit for bit.  More than one rank is not exercised here."""
    import torch.multiprocessing as mp
    mp.spawn(_rehearsal_worker, args=(_free_port(), str(tmp_path)), nprocs=1, join=True)
    m, tr = _trainer(_cfg(), gpu)
    assert not tr.collectives
    tr.precise_bn([(a.to(gpu), b) for a, b in _batches(2, seed=7)], 2)
    assert torch.equal(torch.load(tmp_path / "stats.pt"), m.moving_stats_flat().cpu())
