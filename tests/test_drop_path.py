"""Stochastic depth (NETWORK.DROP_PATH_RATE), the parts that need no GPU: the host Philox the device draw is checked against,
the config key, the per-block rate schedule, the three entry points in the derived binding, and -- on dry plans -- which launches
a training plan records with the feature off and on."""
import ctypes as C
import math

import pytest
import torch

from tests import drop_path_ref as R


def test_philox_known_answers():
    for counter, key, want in R.KNOWN_ANSWERS:
        assert R.philox4x32_10(counter, key) == want


def test_keep_table_values():
    rates = [0.0, 0.25, 0.5]
    t = R.keep_table(7, 3, rates, 64)
    assert (t[0] == 1.0).all()                                       # rate 0: always kept, scale 1
    for l in (1, 2):
        sc = R.keep_scale(rates)[l]
        assert set(t[l].tolist()) <= {0.0, float(sc)}
        assert 0 < (t[l] == 0).sum() < 64                            # (64 draws at 0.25 / 0.5: both outcomes occur)
    assert not (R.keep_table(7, 4, rates, 64) == t).all()            # another step, another table
    assert not (R.keep_table(8, 3, rates, 64) == t).all()            # another seed, another table


@pytest.mark.parametrize("bad", [-0.1, 1.0, float("nan")])
def test_drop_path_settings_rejects(bad):
    import x3d_tf_amd as x
    from x3d_tf_amd.config import drop_path_settings
    cfg = x.get_config("XS", freeze=False)
    cfg.NETWORK.DROP_PATH_RATE = bad
    with pytest.raises(ValueError):
        drop_path_settings(cfg)
    with pytest.raises(ValueError):
        x.get_config("XS", ["NETWORK.DROP_PATH_RATE", bad])


def test_drop_path_settings_default_and_missing_key():
    import x3d_tf_amd as x
    from x3d_tf_amd.config import drop_path_settings
    assert x.get_default_config().NETWORK.DROP_PATH_RATE == 0.0
    cfg = x.get_config("XS", freeze=False)
    assert drop_path_settings(cfg) == 0.0
    del cfg.NETWORK["DROP_PATH_RATE"]
    assert drop_path_settings(cfg) == 0.0
    assert x.build_arch(cfg).drop_path_rate == 0.0
    assert drop_path_settings(x.get_config("XS", ["NETWORK.DROP_PATH_RATE", 0.3])) == 0.3


@pytest.mark.parametrize("name,blocks", [("XS", 26), ("M", 26), ("XL", 55)])
def test_rate_schedule(name, blocks):
    import x3d_tf_amd as x
    from x3d_tf_amd.arch import drop_path_rates
    arch = x.build_arch(x.get_config(name, ["NETWORK.DROP_PATH_RATE", 0.4]))
    r = drop_path_rates(arch)
    assert len(r) == len(arch.blocks) == blocks
    assert r[0] == 0.0 and r[-1] == 0.4
    assert all(b > a for a, b in zip(r, r[1:]))
    assert all(math.isclose(v, 0.4 * l / (blocks - 1)) for l, v in enumerate(r))
    assert drop_path_rates(x.build_arch(x.get_config(name))) == [0.0] * blocks


def test_entry_points_in_the_derived_binding():
    from x3d_tf_amd import hip
    vp, i, ll = C.c_void_p, C.c_int, C.c_longlong
    want = {
        "x3d_drop_path_draw": [vp, vp, vp, i, i, vp],
        "x3d_tail_fwd_dp": [vp, vp, vp, vp, vp, vp, i, i, ll, i, vp],
        "x3d_tail_bwd_dp": [vp, vp, vp, vp, vp, vp, vp, vp, i, i, ll, i, vp],
    }
    for name, argtypes in want.items():
        assert name in hip.exported_symbols()
        got, ret = hip._SIGS[name]
        assert got == argtypes and ret is i, name
        assert getattr(hip.load(), name).argtypes == argtypes
    assert hip.ABI_VERSION == 138


# ---- launch lists, on dry plans --------------------------------------------------------------------------------------------
def _dry_plan(name, dtype, overrides=None, drop_key=False, n=4, t=4, s=64):
    import x3d_tf_amd as x
    from x3d_tf_amd.model import X3D
    cfg = x.get_config(name, overrides, freeze=False)
    if drop_key:
        del cfg.NETWORK["DROP_PATH_RATE"]
    m = X3D(cfg, dtype=dtype, device="dry")
    return m, m._plan(n, t, s, s, True)


def _names(lst):
    return [item[0] for item in lst if item is not None]


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("name", ["XS", "M"])
def test_rate_zero_records_todays_launches(name, dtype):
    """The switch off -- key 0.0, the default -- records the forward and backward launches, by name and order, of a config tree
    that has no such key, and owns neither a keep table nor a g_branch buffer."""
    _, base = _dry_plan(name, dtype, drop_key=True)
    m, pl = _dry_plan(name, dtype, ["NETWORK.DROP_PATH_RATE", 0.0])
    assert _names(pl.fwd) == _names(base.fwd)
    assert _names(pl.bwd) == _names(base.bwd)
    assert pl.dp_keep is None and pl.backward.gbr is None
    assert not any("_dp" in n for n in _names(pl.fwd) + _names(pl.bwd))
    assert [B.tail_fwd_folded for B in pl.blocks] == [B.tail_fwd_folded for B in base.blocks]
    assert [B.tail_folded for B in pl.blocks] == [B.tail_folded for B in base.blocks]


def _structs_of(pl, lst):
    return [(i, item[0], pl.structs.get((id(lst), i))) for i, item in enumerate(lst) if item is not None]


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("name", ["XS", "M"])
def test_rate_on_unfolds_the_dropped_blocks(name, dtype):
    """Rate > 0: every block with a rate has exactly one x3d_tail_fwd_dp and one x3d_tail_bwd_dp on its tensors, no x3d_tail_fwd /
    x3d_tail_bwd launch and no in_store / tail_c field points at them, its `c` backward reads the g_branch buffer and the `add` of
    its `a` backward (the shortcut's gradient) does not.  Block 0 (rate 0) keeps the launches of the rate-0 plan."""
    from x3d_tf_amd import hip
    _, base = _dry_plan(name, dtype)
    m, pl = _dry_plan(name, dtype, ["NETWORK.DROP_PATH_RATE", 0.2])
    rates = m.drop_path_rates
    assert pl.dp_keep is not None and tuple(pl.dp_keep.shape) == (len(pl.blocks), pl.n)
    gbr = pl.backward.gbr.data_ptr()
    fwd_dp = [it for it in pl.fwd if it is not None and it[0] == "x3d_tail_fwd_dp"]
    bwd_dp = [it for it in pl.bwd if it is not None and it[0] == "x3d_tail_bwd_dp"]
    assert len(fwd_dp) == len(bwd_dp) == sum(r > 0 for r in rates) == len(pl.blocks) - 1
    fwd_structs, bwd_structs = _structs_of(pl, pl.fwd), _structs_of(pl, pl.bwd)
    for l, (B, R0) in enumerate(zip(pl.blocks, pl.backward.blocks)):
        y, c_raw = B.y.data_ptr(), B.c_raw.data_ptr()
        mine_f = [it for it in fwd_dp if it[2][5] == y]
        mine_b = [it for it in bwd_dp if it[2][2] == y]
        if rates[l] == 0.0:
            assert not mine_f and not mine_b and B.dp_keep is None and R0.g_branch is None
            continue
        assert len(mine_f) == 1 and len(mine_b) == 1
        row = pl.dp_keep.data_ptr() + 4 * pl.n * l
        assert mine_f[0][2][0] == c_raw and mine_f[0][2][4] == row and B.dp_keep == row
        assert mine_b[0][2][1] == gbr and mine_b[0][2][3] == c_raw and mine_b[0][2][5] == row
        assert not B.tail_fwd_folded and not B.tail_folded
        # no plain tail launch on this block's tensors
        assert not [it for it in pl.fwd if it is not None and it[0] == "x3d_tail_fwd" and it[2][4] == y]
        assert not [it for it in pl.bwd if it is not None and it[0] == "x3d_tail_bwd" and it[2][1] == y]
        # no folded form builds or differentiates this block's tail
        for _, nm, st in fwd_structs:
            if isinstance(st, hip.PwFwdArgs):
                assert st.in_store is None or st.in_store != y
                assert st.x is None or st.x != c_raw or nm != "x3d_pw_fwd" or st.in_store is None
        for _, nm, st in bwd_structs:
            if isinstance(st, hip.PwBwdArgs):
                assert st.tail_c is None or st.tail_c != c_raw
        # the `c` backward of this block reads g_branch; the `a` backward adds the shortcut path's gradient, which is not g_branch
        mine = bwd_structs[B.bwd_start:B.bwd_stop]
        c_bwd = [st for _, nm, st in mine if isinstance(st, (hip.PwBwdArgs, hip.PwWgradArgs, hip.PwDgradArgs)) and st.yraw == c_raw]
        assert c_bwd and all(st.g == gbr for st in c_bwd)
        a_bwd = [st for _, nm, st in mine if isinstance(st, (hip.PwBwdArgs, hip.PwDgradArgs)) and st.dx == B.dx_view.data_ptr()]
        assert a_bwd and all(st.add is not None and st.add != gbr for st in a_bwd)
        others = [st for _, nm, st in mine if isinstance(st, (hip.PwBwdArgs, hip.PwWgradArgs, hip.PwDgradArgs)) and st not in c_bwd]
        assert all(st.g != gbr for st in others)
    # block 0 is never dropped: its tail stays folded where the rate-0 plan folds it, and its own backward launches are the same
    b0, base0 = pl.blocks[0], base.blocks[0]
    assert b0.tail_fwd_folded == base0.tail_fwd_folded and b0.tail_folded == base0.tail_folded
    assert _names(pl.bwd[b0.bwd_start:b0.bwd_stop]) == _names(base.bwd[base0.bwd_start:base0.bwd_stop])
    from x3d_tf_amd.dispatch import scratch_hazards
    assert scratch_hazards(pl) == []
