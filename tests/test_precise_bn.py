"""Precise BatchNorm (NETWORK.BN.USE_PRECISE_STATS), the parts that need no GPU: the config keys and their validator, the two
entry points in the derived binding, and -- on dry plans of the five shipped configs -- the layer table the kernels walk."""
import os
import re

import numpy as np
import pytest
import torch

import x3d_tf_amd as x
from x3d_tf_amd import hip
from x3d_tf_amd.config import precise_bn_settings

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---- config ------------------------------------------------------------------------------------------------------------------
def test_config_defaults_are_off():
    d = x.get_default_config()
    assert d.NETWORK.BN.USE_PRECISE_STATS is False and d.NETWORK.BN.NUM_BATCHES_PRECISE == 200
    assert precise_bn_settings(d) == (False, 200)
    for name in ("XS", "S", "M", "L", "XL"):
        assert precise_bn_settings(x.get_config(name)).enable is False
    on = x.get_config("M", ["NETWORK.BN.USE_PRECISE_STATS", True, "NETWORK.BN.NUM_BATCHES_PRECISE", 7])
    assert precise_bn_settings(on) == (True, 7)


@pytest.mark.parametrize("bad", [0, -1, 2.5, True])
def test_config_refuses_a_bad_batch_count(bad):
    with pytest.raises(ValueError):
        x.get_config("M", ["NETWORK.BN.NUM_BATCHES_PRECISE", bad])
    cfg = x.get_config("M", freeze=False)
    cfg.NETWORK.BN.NUM_BATCHES_PRECISE = bad          # set behind the merge's type check: the validator itself refuses
    with pytest.raises(ValueError, match="NUM_BATCHES_PRECISE"):
        precise_bn_settings(cfg)


def test_config_tree_without_the_keys_means_off():
    cfg = x.get_config("M", freeze=False)
    del cfg.NETWORK.BN["USE_PRECISE_STATS"]
    del cfg.NETWORK.BN["NUM_BATCHES_PRECISE"]
    assert precise_bn_settings(cfg) == (False, 200)
    del cfg.NETWORK["BN"]
    assert precise_bn_settings(cfg) == (False, 200)


# ---- ABI ---------------------------------------------------------------------------------------------------------------------
def test_abi_additions_only():
    from ctypes import c_int as i, c_void_p as vp
    assert hip.ABI_VERSION == 138
    lib = hip.load()
    assert lib.x3d_version() == 138
    assert {"x3d_precise_bn_accum", "x3d_precise_bn_final"} <= set(hip.exported_symbols())
    assert (list(lib.x3d_precise_bn_accum.argtypes), lib.x3d_precise_bn_accum.restype) == ([vp, i, vp, vp], i)
    assert (list(lib.x3d_precise_bn_final.argtypes), lib.x3d_precise_bn_final.restype) == ([vp, i, vp, vp, vp], i)
    assert (hip.PBN_COLS, hip.PBN_STATS, hip.PBN_C, hip.PBN_COUNT, hip.PBN_MEAN, hip.PBN_VAR, hip.PBN_POOLED) == (6, 0, 1, 2, 3, 4, 5)
    # no new struct: the header's set is the one tests/abi_layout_probe.cpp walks
    header = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "x3d_hip.h")).read(), flags=re.S)
    structs = re.findall(r"typedef struct \{[^{}]*\}\s*(x3d_\w+)\s*;", header)
    probe = open(os.path.join(ROOT, "tests", "abi_layout_probe.cpp")).read()
    assert len(structs) == 16 and all(re.search(rf"\b{s}\b", probe) for s in structs)


def test_argument_checks_refuse_before_any_launch():
    """null pointers, nlayers < 1 and misaligned buffers are refused on the host: no device needed"""
    lib = hip.load()
    ok = 4096
    for args in ((None, 1, ok), (ok, 1, None), (ok, 0, ok), (ok, -3, ok), (ok + 4, 1, ok), (ok, 1, ok + 4)):
        assert lib.x3d_precise_bn_accum(*args, None) == 1, args
        assert b"precise_bn_accum" in lib.x3d_last_error()
    for args in ((None, 1, ok, ok), (ok, 1, None, ok), (ok, 1, ok, None), (ok, 0, ok, ok), (ok, 1, ok + 4, ok), (ok, 1, ok, ok + 2)):
        assert lib.x3d_precise_bn_final(*args, None) == 1, args
        assert b"precise_bn_final" in lib.x3d_last_error()


# ---- the layer table, on dry plans ---------------------------------------------------------------------------------------------
def _dry(name, n, overrides=None):
    from x3d_tf_amd.model import X3D
    cfg = x.get_config(name, overrides)
    m = X3D(cfg, dtype=torch.bfloat16, device="dry")
    t, s = cfg.DATA.TEMP_DURATION, cfg.DATA.TRAIN_CROP_SIZE
    return m, m._plan(n, t, s, s, True), (t, s)


def _expected_counts(arch, n, t, s):
    """prefix -> N * T * H * W of the layer's output, from the block specs and the TF-SAME rule (out = ceil(in / stride)); the
    stem's spatial conv pads (0, 1, 1) and strides 2 without SAME: out = (in - 1) // 2 + 1"""
    h = w = (s - 1) // 2 + 1
    want = {"conv1/bn": n * t * h * w}
    for b in arch.blocks:
        pre = f"stages/{b.stage}/stage/layer_with_weights-{b.index}"
        ho, wo = -(-h // b.stride), -(-w // b.stride)
        want[f"{pre}/bottleneck/bn_a"] = n * t * h * w             # the `a` conv keeps the block's input resolution
        want[f"{pre}/bottleneck/bn_b"] = n * t * ho * wo           # the depthwise conv strides
        want[f"{pre}/bottleneck/bn_c"] = n * t * ho * wo
        if b.has_shortcut_conv:
            want[f"{pre}/bn_r"] = n * t * ho * wo
        h, w = ho, wo
    want["conv5/layer_with_weights-1"] = n * t * h * w
    return want


_DRY = {}


def _dry_cached(name):
    if name not in _DRY:
        _DRY[name] = _dry(name, 2)
    return _DRY[name]


@pytest.mark.parametrize("name", ["XS", "S", "M", "L", "XL"])
def test_table_of_a_dry_training_plan(name):
    m, pl, (t, s) = _dry_cached(name)
    lay = m.precise_bn_layout()
    tb = pl.precise_bn_table()
    assert tb is pl.precise_bn_table()                                  # built once
    assert tb.dtype == torch.int64 and tb.dim() == 2 and tb.shape[1] == hip.PBN_COLS
    tb = tb.numpy()
    means = [k for k in m.param_order if k.endswith("/moving_mean")]
    assert len(tb) == len(means) == len(lay.prefixes) and (name != "M" or len(tb) == 84)
    # counts and channels, derived here from the architecture
    want = _expected_counts(m.arch, 2, t, s)
    assert sorted(want) == sorted(lay.prefixes)
    for row, prefix in zip(tb, lay.prefixes):
        assert row[hip.PBN_COUNT] == want[prefix], prefix
        assert row[hip.PBN_C] == m.params[f"{prefix}/moving_mean"].numel(), prefix
    # the statistics addresses: distinct, 8-byte aligned, each range inside the plan's zeroed accumulator buffer
    lo, hi = pl.zero_buf.data_ptr(), pl.zero_buf.data_ptr() + 8 * pl.zero_buf.numel()
    spans = sorted((int(r[hip.PBN_STATS]), int(r[hip.PBN_STATS]) + 8 * m._stats_r * hip.stats_layout(int(r[hip.PBN_C]))[1]) for r in tb)
    assert all(a % 8 == 0 and lo <= a and b <= hi for a, b in spans)
    assert all(spans[k][1] <= spans[k + 1][0] for k in range(len(spans) - 1))
    # columns MEAN / VAR hit every moving tensor of flat_params exactly once
    base, flat = m.flat_params.data_ptr(), {}
    for k in m.param_order:
        if k.endswith(("/moving_mean", "/moving_variance")):
            flat[(m.params[k].data_ptr() - base) // 4] = k
    hit = [flat.pop(int(r[hip.PBN_MEAN])) for r in tb] + [flat.pop(int(r[hip.PBN_VAR])) for r in tb]
    assert not flat and hit == [f"{q}/moving_mean" for q in lay.prefixes] + [f"{q}/moving_variance" for q in lay.prefixes]
    assert all(int(r[hip.PBN_MEAN]) >= m.n_trainable_flat and int(r[hip.PBN_VAR]) + int(r[hip.PBN_C]) <= m.flat_params.numel() for r in tb)
    # the pooled ranges: behind the count slots, disjoint, and together the whole buffer
    ranges = sorted((int(r[hip.PBN_POOLED]), int(r[hip.PBN_POOLED]) + 2 * int(r[hip.PBN_C])) for r in tb)
    assert ranges[0][0] == len(tb) and ranges[-1][1] == lay.pooled_size
    assert all(ranges[k][1] == ranges[k + 1][0] for k in range(len(ranges) - 1))
    assert tuple(int(r[hip.PBN_POOLED]) for r in tb) == lay.pooled_offsets


def test_plans_of_different_shapes_share_the_pooled_layout():
    m, pl2, (t, s) = _dry_cached("XS")
    pl3 = m._plan(3, t, s, s, True)
    a, b = pl2.precise_bn_table().numpy(), pl3.precise_bn_table().numpy()
    shared = [hip.PBN_C, hip.PBN_MEAN, hip.PBN_VAR, hip.PBN_POOLED]
    assert np.array_equal(a[:, shared], b[:, shared])
    assert np.array_equal(a[:, hip.PBN_COUNT] * 3, b[:, hip.PBN_COUNT] * 2)
    assert not np.any(a[:, hip.PBN_STATS] == b[:, hip.PBN_STATS])


def test_table_refuses_an_incomplete_plan():
    """a registered layer without `count` (no finalize recorded for it) or without `stats`, a layer registered twice or
    missing, and an inference plan"""
    m, _, (t, s) = _dry("XS", 2)

    def fresh():
        pl = m._plan(2, t, s, s, True)
        pl._pbn_table = None
        return pl
    pl = fresh()
    b = pl.bn_layers[5]
    keep = b.count
    b.count = None
    with pytest.raises(ValueError, match="count"):
        pl.precise_bn_table()
    b.count = keep
    stats, b.stats = b.stats, None
    with pytest.raises(ValueError, match="stats"):
        pl.precise_bn_table()
    b.stats = stats
    pl.bn_layers.append(b)
    with pytest.raises(ValueError, match="twice"):
        pl.precise_bn_table()
    pl.bn_layers.pop()
    gone = pl.bn_layers.pop(3)
    with pytest.raises(ValueError, match=re.escape(gone.prefix)):
        pl.precise_bn_table()
    pl.bn_layers.insert(3, gone)
    assert pl.precise_bn_table().shape[0] == len(pl.bn_layers)
    with pytest.raises(ValueError, match="training plan"):
        m._plan(m.arch.num_preds, t, s, s, False).precise_bn_table()


def test_feature_off_records_the_same_launches():
    """the registry and the count are additions to records: a plan of a config tree without the keys records the launches, by name
    and order, of one with them, and building the table adds none"""
    from x3d_tf_amd.model import X3D
    cfg = x.get_config("XS", freeze=False)
    old = cfg.clone()
    del old.NETWORK.BN["USE_PRECISE_STATS"]
    del old.NETWORK.BN["NUM_BATCHES_PRECISE"]
    lists = []
    for c in (cfg, old):
        pl = X3D(c, dtype=torch.bfloat16, device="dry")._plan(2, 4, 64, 64, True)
        before = ([e[0] for e in pl.fwd], [e[0] for e in pl.bwd])
        pl.precise_bn_table()
        assert ([e[0] for e in pl.fwd], [e[0] for e in pl.bwd]) == before
        lists.append(before)
    assert lists[0] == lists[1]


# ---- update_bn_stats: what it refuses before it touches a device ----------------------------------------------------------------
def test_update_bn_stats_refuses_bad_counts():
    from x3d_tf_amd.precise_bn import update_bn_stats
    m, _, _ = _dry_cached("XS")
    for bad in (0, -1, 2.5, True, None):
        with pytest.raises(ValueError, match="num_batches"):
            update_bn_stats(m, [], bad)
    with pytest.raises(ValueError, match="yielded nothing"):
        update_bn_stats(m, iter([]), 3)


# ---- the reference itself --------------------------------------------------------------------------------------------------------
def test_reference_matches_the_definition():
    """precise_bn_ref against numpy's own mean / var on data split over batches of different sizes and over replicas"""
    from tests import precise_bn_ref as R
    rng = np.random.default_rng(0)
    c, reps, stride = 5, 4, 16
    data = [rng.normal(1.5, 2.0, size=(k, c)) for k in (7, 11, 3)]
    batches = []
    for d in data:
        acc = np.zeros((reps, stride))
        for r, part in enumerate(np.array_split(d, reps)):
            acc[r, 0:2 * c:2] = part.sum(axis=0)
            acc[r, 1:2 * c:2] = (part ** 2).sum(axis=0)
        batches.append((R.replica_sum(acc.ravel(), c, reps, stride), len(d)))
    sums, n = R.pool(batches)
    mean, unb = R.final(sums, n)
    every = np.concatenate(data)
    assert n == 21 and np.allclose(mean, every.mean(axis=0), rtol=1e-13) and np.allclose(unb, every.var(axis=0, ddof=1), rtol=1e-12)
    one = R.final(np.array([[3.0, 9.0]]), 1)                           # a single element: no Bessel factor, variance 0
    assert one[0][0] == 3.0 and one[1][0] == 0.0
    assert np.array_equal(R.ulps(np.float32([1.0, np.nextafter(np.float32(1.0), np.float32(2.0))]), np.float64([1.0, 1.0])), [0.0, 1.0])
