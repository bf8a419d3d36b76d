"""NETWORK.RES5_DILATION without a GPU: the config key, the architecture it builds, the dry plans of the five shipped configs,
the dry-run dispatch of x3d_dw3d_fwd_dil / x3d_dw3d_bwd_dil and the launches the library refuses."""
import ctypes as C
import re

import pytest
import torch

import x3d_tf_amd as x
from x3d_tf_amd import hip
from x3d_tf_amd.config import res5_dilation_settings

NAMES = ["XS", "S", "M", "L", "XL"]
ONE_VIEW = ["TEST.NUM_SPATIAL_CROPS", 1, "TEST.NUM_TEMPORAL_VIEWS", 1]
KEY = "NETWORK.RES5_DILATION"


# ---- config ---------------------------------------------------------------------------------------------------------------
def test_config_default_and_a_tree_without_the_key():
    cfg = x.get_config("M")
    assert res5_dilation_settings(cfg) == 1 and cfg.NETWORK.RES5_DILATION == 1
    assert "RES5_DILATION" not in dict(cfg.NETWORK)           # known, not held: a saved config is what it was
    on = x.get_config("M", [KEY, 2])
    assert res5_dilation_settings(on) == 2 and dict(on.NETWORK)["RES5_DILATION"] == 2
    assert set(dict(on.NETWORK)) == set(dict(cfg.NETWORK)) | {"RES5_DILATION"}


@pytest.mark.parametrize("value", [0, 3, True, -2, 4])
def test_config_refuses_other_values(value):
    with pytest.raises(ValueError, match="RES5_DILATION"):
        x.get_config("XS", [KEY, value])
    cfg = x.get_config("XS", freeze=False)
    cfg.NETWORK["RES5_DILATION"] = value
    with pytest.raises(ValueError, match=re.escape(KEY)):
        res5_dilation_settings(cfg)
    with pytest.raises(ValueError, match=re.escape(KEY)):
        x.build_arch(cfg)


def test_config_detection_scale_factor_must_be_the_stride():
    det = ONE_VIEW + ["DETECTION.ENABLE", True]
    with pytest.raises(ValueError, match=r"DETECTION\.SPATIAL_SCALE_FACTOR.*NETWORK\.RES5_DILATION"):
        x.get_config("XS", det + [KEY, 2])                    # the section's default, 32
    with pytest.raises(ValueError, match=r"DETECTION\.SPATIAL_SCALE_FACTOR.*NETWORK\.RES5_DILATION"):
        x.get_config("XS", det + [KEY, 2, "DETECTION.SPATIAL_SCALE_FACTOR", 8])
    x.get_config("XS", det + [KEY, 2, "DETECTION.SPATIAL_SCALE_FACTOR", 16])
    x.get_config("XS", [KEY, 2])                              # detection off: a dilated classification model is legal
    x.get_config("XS", [KEY, 2, "DETECTION.SPATIAL_SCALE_FACTOR", 32])
    x.get_config("XS", det + [KEY, 1, "DETECTION.SPATIAL_SCALE_FACTOR", 16])     # the check runs only when the key is not 1


# ---- architecture ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", NAMES)
def test_build_arch_out_shape_and_spatial_stride(name):
    a1, a2 = x.build_arch(x.get_config(name, [KEY, 1])), x.build_arch(x.get_config(name, [KEY, 2]))
    a0 = x.build_arch(x.get_config(name))
    assert a0 == a1 and a1.res5_dilation == 1 and a1.spatial_stride == 32 and a2.spatial_stride == 16
    assert all(b.dilation == 1 for b in a1.blocks)
    assert [st.blocks[0].stride for st in a1.stages] == [2, 2, 2, 2]
    assert [st.blocks[0].stride for st in a2.stages] == [2, 2, 2, 1]
    for s1, s2 in zip(a1.stages[:-1], a2.stages[:-1]):
        assert s1 == s2
    last1, last2 = a1.stages[-1].blocks, a2.stages[-1].blocks
    assert len(last1) == len(last2)
    for b1, b2 in zip(last1, last2):
        assert b2.dilation == 2 and b2.stride == 1
        assert b2.has_shortcut_conv == b1.has_shortcut_conv == (b2.index == 0)
        assert (b2.cin != b2.cout) == (b2.index == 0)         # the stride-1 projection shortcut exists because the widths differ
        assert (b1.cin, b1.inner, b1.cout, b1.has_se, b1.se_width, b1.global_index) == \
               (b2.cin, b2.inner, b2.cout, b2.has_se, b2.se_width, b2.global_index)
    # the weights keep their shapes: a Kinetics checkpoint loads into the dilated network
    from x3d_tf_amd.arch import param_specs
    assert [(s.name, s.shape) for s in param_specs(a1)] == [(s.name, s.shape) for s in param_specs(a2)]
    for t, s in ((16, 224), (4, 64), (13, 160), (16, 312), (16, 256)):
        assert a1.out_shape(t, s, s) == (t, -(-s // 32), -(-s // 32))
        assert a2.out_shape(t, s, s) == (t, -(-s // 16), -(-s // 16))
    from x3d_tf_amd.arch import summary_rows
    rows = dict((r[0], r[1]) for r in summary_rows(a2, 16, 224, 224))
    assert rows["res_stage_5"][1:3] == (14, 14) and rows["conv_5"][1:3] == (14, 14) and rows["res_stage_4"][1:3] == (14, 14)


# ---- dry plans ------------------------------------------------------------------------------------------------------------
def _dry(cfg, n, t, s, training, dtype=torch.bfloat16):
    from x3d_tf_amd.model import X3D
    return X3D(cfg, dtype=dtype, device="dry")._plan(n, t, s, s, training)


def _dw_structs(pl):
    return [st for st in pl.structs.values() if isinstance(st, (hip.Dw3dFwdArgs, hip.Dw3dBwdArgs))]


SIZES = {"XS": (4, 160), "S": (13, 160), "M": (16, 224), "L": (16, 312), "XL": (16, 312)}


@pytest.mark.parametrize("training", [True, False], ids=["train", "infer"])
@pytest.mark.parametrize("name", NAMES)
def test_dry_plans_record_and_carry_the_dilation(name, training):
    t, s = SIZES[name]
    cfg = x.get_config(name, ONE_VIEW + [KEY, 2])
    arch = x.build_arch(cfg)
    pl = _dry(cfg, 2, t, s, training)
    c_last = arch.stages[-1].inner
    h5 = arch.out_shape(t, s, s)[1]
    res5 = [st for st in _dw_structs(pl) if st.C == c_last and st.H == h5]
    other = [st for st in _dw_structs(pl) if not (st.C == c_last and st.H == h5)]
    per = 2 if training else 1
    assert len(res5) == per * len(arch.stages[-1].blocks) and len(other) == per * (len(arch.blocks) - len(arch.stages[-1].blocks))
    for st in res5:
        assert st.dilation == 2 and st.stride == 1
        assert hip.dw3d_kernel_name(st).startswith("dw3d_dil_fwd_kernel<bf16" if isinstance(st, hip.Dw3dFwdArgs) else "dw3d_dil_bwd_kernel<bf16")
    for st in other:
        assert st.dilation in (0, 1) and "_dil_" not in hip.dw3d_kernel_name(st)
    # the dilated launches are recorded on the dilated entry points, the dilation behind the struct; every other one as always
    for lst in (pl.fwd, pl.bwd):
        for i, e in enumerate(lst):
            st = pl.structs.get((id(lst), i))
            if isinstance(st, (hip.Dw3dFwdArgs, hip.Dw3dBwdArgs)):
                base = "x3d_dw3d_fwd" if isinstance(st, hip.Dw3dFwdArgs) else "x3d_dw3d_bwd"
                assert (e[0], len(e[2])) == ((base + "_dil", 2) if st.dilation == 2 else (base, 1))
                assert st.dilation != 2 or e[2][1] == 2
    assert (pl.h5, pl.w5) == (h5, h5) and tuple(pl.c5_raw.shape) == (2, arch.conv5_out, t, h5, h5)
    # the first block of the stage: a projection shortcut at stride 1, read from the block input itself
    B = next(B for B in pl.blocks if B.spec.stage == 3 and B.spec.index == 0)
    assert (B.hh, B.ww) == (B.ho, B.wo) == (h5, h5) and B.xs is None
    assert B.sr.stride == 1 and (B.sr.H, B.sr.W) == (h5, h5) and tuple(B.r_raw.shape) == (2, B.spec.cout, t, h5, h5)
    if training:
        from x3d_tf_amd import dispatch
        assert dispatch.scratch_hazards(pl) == []
        names = [e[0] for e in pl.bwd]
        assert "x3d_dw3d_bwd" in names
        # no launch of the last stage takes the strided-add epilogue or a strided x
        for st in pl.structs.values():
            if isinstance(st, hip.PwDgradArgs) and st.H == h5 and st.Cout == c_last:
                assert st.epi != hip.EPI_ADD_STRIDED
        tbl = pl.precise_bn_table()
        counts = {int(r[hip.PBN_C]): int(r[hip.PBN_COUNT]) for r in tbl.tolist()}
        assert counts[arch.conv5_out] == 2 * t * h5 * h5


@pytest.mark.parametrize("training", [True, False], ids=["train", "infer"])
def test_key_at_one_records_the_list_of_a_config_without_it(training):
    def launches(cfg):
        pl = _dry(cfg, 2, 16, 224, training)
        out = []
        for lst in (pl.fwd, pl.bwd):
            for i, e in enumerate(lst):
                st = pl.structs.get((id(lst), i))
                out.append((e[0], None if st is None else (type(st).__name__, hip.kernel_name(st) if hasattr(st, "dtype") and
                                                            type(st).__name__.startswith(("Pw", "Dw3d")) else None,
                                                            getattr(st, "dilation", None))))
        return out
    absent, at1 = launches(x.get_config("M", ONE_VIEW)), launches(x.get_config("M", ONE_VIEW + [KEY, 1]))
    assert absent == at1 and len(absent) > 100
    at2 = launches(x.get_config("M", ONE_VIEW + [KEY, 2]))
    assert at2 != absent


def test_detection_plan_on_the_stride_16_map():
    cfg = x.get_config("XS", ONE_VIEW + ["DATA.TEMP_DURATION", 4, KEY, 2, "DETECTION.ENABLE", True, "DETECTION.MAX_BOXES", 2,
                                         "DETECTION.SPATIAL_SCALE_FACTOR", 16])
    pl = _dry(cfg, 2, 4, 64, True, torch.float32)
    i = [e[0] for e in pl.fwd].index("x3d_roi_pool_fwd")
    args = pl.fwd[i][2]
    assert (pl.h5, pl.w5) == (4, 4) and args[9:11] == (4, 4) and abs(args[14] - 1.0 / 16) < 1e-12
    # the ROI head's H * W <= 1024 limit is met at the map's real size: 33 x 33 conv5 pixels are refused, 32 x 32 are not
    from x3d_tf_amd.model import X3D
    m = X3D(cfg, dtype=torch.float32, device="dry")
    m._plan(1, 4, 512, 512, False)
    with pytest.raises(ValueError):
        m._plan(1, 4, 528, 528, False)


def test_keras_surface_shows_the_dilation_rate():
    from x3d_tf_amd.model import X3D
    m = X3D(x.get_config("XS", [KEY, 2]), dtype=torch.float32, device="dry")
    convs = [rb.bottleneck.b for stage in m.stages for rb in stage.stage]
    rates = [(c.strides, c.dilation_rate) for c in convs]
    n5 = len(m.arch.stages[-1].blocks)
    assert len(rates) == len(m.arch.blocks)
    assert all(r == ((1, 1, 1), (1, 2, 2)) for r in rates[-n5:])
    assert all(r[1] == (1, 1, 1) for r in rates[:-n5])
    first = m.stages[-1].stage[0]
    assert first.residual.strides == (1, 1, 1) and tuple(first.residual.kernel.shape) == (first.out_channels, first.in_channels)


# ---- dispatch and refusals ------------------------------------------------------------------------------------------------
def _fwd(h=14, w=14, stride=1, dilation=2, dtype=None, t=4):
    return hip.dilated(hip.Dw3dFwdArgs(4096, 4096, 4096, None, hip.ACT_NONE, None, None, 2, 3, t, h, w, stride,
                                       hip.BF16 if dtype is None else dtype, None), dilation)


def _bwd(h=14, w=14, stride=1, dilation=2, dtype=None, t=4):
    return hip.dilated(hip.Dw3dBwdArgs(4096, 4096, 4096, 4096, 4096, 4096, 4096, 4096, 4096, 2, 3, t, h, w, stride,
                                       hip.BF16 if dtype is None else dtype), dilation)


def test_the_structs_are_untouched_and_small_dilations_are_the_dense_entry():
    """the dilation is an argument of x3d_dw3d_fwd_dil / x3d_dw3d_bwd_dil, not a field: the argument structs and the library's ABI
    number are what they were, and d = 0 / 1 through the dilated entries name the kernel the dense entries name"""
    assert [n for n, _ in hip.Dw3dFwdArgs._fields_][-2:] == ["dtype", "in_bn"] and len(hip.Dw3dFwdArgs._fields_) == 15
    assert [n for n, _ in hip.Dw3dBwdArgs._fields_][-2:] == ["stride", "dtype"] and len(hip.Dw3dBwdArgs._fields_) == 16
    lib = hip.load()
    for name, nargs in (("x3d_dw3d_fwd_dil", 3), ("x3d_dw3d_bwd_dil", 3), ("x3d_dw3d_kernel_name_dil", 5)):
        assert name in hip.exported_symbols() and len(getattr(lib, name).argtypes) == nargs
    buf = C.create_string_buffer(128)
    for make in (_fwd, _bwd):
        for stride in (1, 2):
            plain = make(stride=stride, dilation=1)
            del plain.dilation                                   # an untagged struct, as every caller before built it
            dense = hip.dw3d_kernel_name(plain)
            assert "_dil_" not in dense
            for d in (0, 1):
                slots = (C.byref(plain), None) if make is _fwd else (None, C.byref(plain))
                assert lib.x3d_dw3d_kernel_name_dil(*slots, d, buf, 128) == 0 and buf.value.decode() == dense
                assert hip.dw3d_kernel_name(make(stride=stride, dilation=d)) == dense


@pytest.mark.parametrize("code, tname", [("F32", "float"), ("BF16", "bf16"), ("F16", "f16")])
def test_dry_run_names_the_new_kernels(code, tname):
    dt = getattr(hip, code)
    for hw, np_ in (((1, 1), 1), ((14, 14), 1), ((16, 16), 1), ((17, 19), 2), ((20, 20), 2), ((23, 24), 0)):
        for d in (2, 3, 4):
            dd = 2 if d == 2 else 0        # the model's dilation is a template argument, the others are taken at run time
            assert hip.dw3d_kernel_name(_fwd(*hw, dilation=d, dtype=dt)) == f"dw3d_dil_fwd_kernel<{tname}, {np_}, {dd}>"
            assert hip.dw3d_kernel_name(_bwd(*hw, dilation=d, dtype=dt)) == f"dw3d_dil_bwd_kernel<{tname}, {np_}, {dd}>"


@pytest.mark.parametrize("make", [_fwd, _bwd], ids=["fwd", "bwd"])
@pytest.mark.parametrize("kw, word", [
    (dict(stride=2), "stride"), (dict(dilation=5), "dilation"), (dict(dilation=-1), "dilation"),
    (dict(h=61, w=61), "LDS"), (dict(h=60, w=61, dilation=2), "LDS"), (dict(h=56, w=57, dilation=4), "LDS")])
def test_refused_launches_name_the_argument_and_launch_nothing(make, kw, word):
    """the entry points themselves, on a host without a GPU: the refusal comes back as X3D_ERR_INVALID with its message before any
    HIP call (the pointers are not even addresses of memory), and the dry run reports the same"""
    lib = hip.load()
    st = make(**kw)
    entry = lib.x3d_dw3d_fwd_dil if make is _fwd else lib.x3d_dw3d_bwd_dil
    assert entry(C.byref(st), st.dilation, None) != 0
    assert word in lib.x3d_last_error().decode() and "dw3d_" in lib.x3d_last_error().decode()
    with pytest.raises(hip.X3DHipError, match=word):
        hip.dw3d_kernel_name(st)


def test_the_plane_limit_is_4096_haloed_elements():
    assert "_dil_" in hip.dw3d_kernel_name(_fwd(60, 60, dilation=2))          # 64 x 64
    assert "_dil_" in hip.dw3d_kernel_name(_bwd(60, 60, dilation=2))
    assert "_dil_" in hip.dw3d_kernel_name(_fwd(56, 56, dilation=4))          # 64 x 64 again
    with pytest.raises(hip.X3DHipError, match="4096"):
        hip.dw3d_kernel_name(_fwd(60, 61, dilation=2))


def test_ops_wrappers_take_the_keyword():
    import inspect
    from x3d_tf_amd import ops
    assert inspect.signature(ops.dw3d_fwd).parameters["dilation"].default == 1
    assert inspect.signature(ops.dw3d_bwd).parameters["dilation"].default == 1


# ---- the reference itself -------------------------------------------------------------------------------------------------
def test_reference_at_dilation_one_is_the_oracles_dense_conv():
    from oracle import x3d_oracle as O
    from tests import dilated_ref as R
    g = torch.Generator().manual_seed(0)
    xx = torch.randn(2, 3, 4, 5, 7, generator=g, dtype=torch.float64)
    w = torch.randn(3, 3, 3, 3, generator=g, dtype=torch.float64)
    assert torch.equal(R.dilated3x3x3(xx, w, 1), O.depthwise3x3x3(xx, w, 1))
    # d = 2 by hand at one pixel: taps two apart, zeros outside
    y = R.dilated3x3x3(xx, w, 2)
    n, c, t, h, ww = 1, 2, 0, 1, 6
    acc = 0.0
    for kt in range(3):
        for kh in range(3):
            for kw in range(3):
                tt, hh, w2 = t + kt - 1, h + 2 * (kh - 1), ww + 2 * (kw - 1)
                if 0 <= tt < 4 and 0 <= hh < 5 and 0 <= w2 < 7:
                    acc += float(w[c, kt, kh, kw]) * float(xx[n, c, tt, hh, w2])
    assert abs(float(y[n, c, t, h, ww]) - acc) < 1e-12
    st = R.DilatedStorage(None, sites={"p": 2})
    assert torch.equal(st.depthwise(xx, w, 1, "p"), y) and torch.equal(st.depthwise(xx, w, 2, "q"), O.depthwise3x3x3(xx, w, 2))


def test_cut_plans_with_the_seam_around_the_dilated_stage():
    """SOLVER.FREEZE_EVAL's cut plans (plan.record_training frozen_prefix) with the seam in front of, inside and behind the
    dilated stage: they record, the seam tensor has the stage's stride-16 extents, and a frozen block of the stage is recorded
    with the inference form of the dilated conv"""
    from x3d_tf_amd import plan
    from x3d_tf_amd.model import X3D
    m = X3D(x.get_config("XS", ONE_VIEW + [KEY, 2]), dtype=torch.bfloat16, device="dry")
    blocks, n5 = len(m.arch.blocks), len(m.arch.stages[-1].blocks)
    c4, c5 = m.arch.stages[-2].cout, m.arch.stages[-1].cout
    for k, want in ((blocks - n5 + 1, c4), (blocks - n5 + 2, c5), (blocks, c5), (blocks + 1, c5)):
        pl = plan.record_training(m, 2, 4, 64, 64, frozen_prefix=k)
        assert tuple(pl.seam.shape) == (2, want, 4, 4, 4) and (pl.h5, pl.w5) == (4, 4), k
        frozen5 = [B for B in pl.blocks[:k - 1] if B.spec.dilation == 2]
        assert len(frozen5) == max(0, k - 1 - (blocks - n5))
        for B in pl.blocks:
            assert B.sb.dilation == B.spec.dilation and B.sb.stride == B.spec.stride
