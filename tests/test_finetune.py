"""Fine-tuning on the host: the SOLVER.LAYER_DECAY / LR_MULT / FREEZE switches (config.finetune_settings), the name-level
logic (finetune.lr_scales: depth groups, scales, frozen names) and the chunk table of the tuned segments.  The kernels and the
trainer are held to their references in test_finetune_gpu.py."""
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import x3d_tf_amd as x  # noqa: E402
from x3d_tf_amd import hip  # noqa: E402
from x3d_tf_amd.arch import block_prefix, build_arch, param_specs  # noqa: E402
from x3d_tf_amd.config import FinetuneSettings, finetune_settings, solver_settings  # noqa: E402
from x3d_tf_amd.finetune import depth_groups, flat_segments, lr_scales  # noqa: E402
from x3d_tf_amd.segments import SegTable  # noqa: E402

F32 = np.float32
OFF = FinetuneSettings(1.0, (), ())
NEW_SYMBOLS = ("x3d_seg_grad_sumsq", "x3d_sgd_pt", "x3d_adam_pt", "x3d_lars_pt", "x3d_adamw_pt", "x3d_lamb_pt")


# ---- config -----------------------------------------------------------------------------------------------------------
def test_config_defaults_and_overrides():
    d = x.get_default_config()
    assert (d.SOLVER.LAYER_DECAY, d.SOLVER.LR_MULT, d.SOLVER.FREEZE) == (1.0, [], [])
    assert finetune_settings(d) == finetune_settings(x.get_config("M")) == OFF == (1.0, (), ())
    s = finetune_settings(x.get_config("M"))
    assert (s.layer_decay, s.lr_mult, s.freeze) == (1.0, (), ())
    c = x.get_config("M", ["SOLVER.LAYER_DECAY", 0.75, "SOLVER.LR_MULT", [["fc2/", 10], ["fc1/", 2.5]],
                           "SOLVER.FREEZE", ["conv1/", "stages/0/"]])
    assert finetune_settings(c) == (0.75, (("fc2/", 10.0), ("fc1/", 2.5)), ("conv1/", "stages/0/"))
    assert c.SOLVER.FREEZE == ["conv1/", "stages/0/"] and "FREEZE" in c.SOLVER and "FREEZE" in c.clone().SOLVER
    # the written forms a command line hands over: literal strings
    c = x.get_config("M", ["SOLVER.LAYER_DECAY", "0.5", "SOLVER.LR_MULT", "[['fc2/', 10.0]]", "SOLVER.FREEZE", "['conv1/']"])
    assert finetune_settings(c) == (0.5, (("fc2/", 10.0),), ("conv1/",))
    assert finetune_settings(x.get_config("M", ["SOLVER.LAYER_DECAY", 1])) == OFF
    # the other solver switches are what they were, and an unknown key is still refused
    assert solver_settings(c) == (0.0, 1, 0.0, True)
    with pytest.raises(KeyError, match="LAYER_DECAI"):
        x.get_config("M", ["SOLVER.LAYER_DECAI", 0.5])
    with pytest.raises(ValueError, match="Type mismatch"):
        x.get_config("M", ["SOLVER.FREEZE", "conv1/"])


def test_config_without_the_keys_means_off():
    m = x.get_config("M")
    assert finetune_settings(m) == OFF
    old = m.clone()
    old.defrost()
    del old["SOLVER"]
    assert finetune_settings(old) == OFF
    bare = x.config.CfgNode(dict(SOLVER=dict(CLIP_GRAD_L2NORM=0.0)))            # a tree from before the keys existed
    assert finetune_settings(bare) == OFF
    # defaults that are off leave the section's items alone: a saved default config reads as it always did
    assert set(m.SOLVER) == {"CLIP_GRAD_L2NORM", "ACCUM_STEPS", "EMA_DECAY", "EMA_EVAL"}
    c = m.clone()
    c.defrost()
    c.SOLVER.FREEZE = ["conv1/"]
    assert finetune_settings(c).freeze == ("conv1/",) and finetune_settings(m) == OFF


@pytest.mark.parametrize("key,value", [
    ("LAYER_DECAY", 0.0), ("LAYER_DECAY", -0.5), ("LAYER_DECAY", 1.5), ("LAYER_DECAY", float("nan")),
    ("LAYER_DECAY", float("inf")), ("LAYER_DECAY", "0.5x"), ("LAYER_DECAY", True),
    ("LR_MULT", [["fc2/", 0.0]]), ("LR_MULT", [["fc2/", -1.0]]), ("LR_MULT", [["fc2/", float("nan")]]),
    ("LR_MULT", [["fc2/", float("inf")]]), ("LR_MULT", [[3, 2.0]]), ("LR_MULT", [["fc2/", "2"]]), ("LR_MULT", [["fc2/"]]),
    ("LR_MULT", ["fc2/", 10.0]), ("LR_MULT", [["fc2/", 2.0, 3.0]]), ("LR_MULT", [["fc2/", True]]), ("LR_MULT", "fc2/"),
    ("FREEZE", [1]), ("FREEZE", ["conv1/", None]), ("FREEZE", [["conv1/"]]), ("FREEZE", "conv1/"),
])
def test_config_rejects(key, value):
    c = x.get_config("M", freeze=False)
    setattr(c.SOLVER, key, value)             # (merge_from_list would refuse some of the types before finetune_settings sees them)
    with pytest.raises(ValueError, match="SOLVER." + key):
        finetune_settings(c)


def test_get_config_validates_the_keys():
    for over in (["SOLVER.LAYER_DECAY", 0.0], ["SOLVER.LR_MULT", [["fc2/", 0.0]]], ["SOLVER.FREEZE", [7]]):
        with pytest.raises(ValueError, match=over[0]):
            x.get_config("M", over)


# ---- ABI --------------------------------------------------------------------------------------------------------------
def test_abi_is_additive_and_the_new_symbols_are_declared_exported_and_typed():
    assert hip.ABI_VERSION == 138
    lib = hip.load()
    assert lib.x3d_version() == 138
    from ctypes import c_float as f, c_int as i, c_longlong as ll, c_void_p as vp
    table = [vp, i, vp, i]
    sigs = {
        "x3d_seg_grad_sumsq": ([vp] + table + [vp, vp, vp], i),
        "x3d_sgd_pt": ([vp, vp, vp] + table + [vp, f, f, f, f, vp, f, vp, f, vp], i),
        "x3d_adam_pt": ([vp, vp, vp, vp] + table + [vp, f, f, f, f, f, f, ll, vp, f, vp, f, vp], i),
        "x3d_lars_pt": ([vp, vp, vp] + table + [vp, f, f, f, f, f, f, i, vp, f, vp, f, vp, vp, vp], i),
        "x3d_adamw_pt": ([vp, vp, vp, vp] + table + [vp, f, f, f, f, f, f, ll, vp, f, vp, f, vp], i),
        "x3d_lamb_pt": ([vp, vp, vp, vp] + table + [vp, f, f, f, f, f, f, ll, vp, f, vp, f, vp, vp, vp], i),
    }
    assert set(sigs) == set(NEW_SYMBOLS)
    for name, (argtypes, restype) in sigs.items():
        assert name in hip.exported_symbols(), name
        fn = getattr(lib, name)
        assert (list(fn.argtypes), fn.restype) == (argtypes, restype), name
    # the existing entry points of the same rules: the _pt signature without lr_scale
    for name, buffers in (("lars", 3), ("adamw", 4), ("lamb", 4)):
        pt = list(getattr(lib, f"x3d_{name}_pt").argtypes)
        k = buffers + len(table)                                               # lr_scale sits behind the chunk table
        assert pt[:k] + pt[k + 1:] == list(getattr(lib, f"x3d_{name}").argtypes), name


def test_argument_checks_need_no_gpu():
    """bad arguments are refused with X3D_ERR_INVALID before any launch (so also without a device)"""
    lib = hip.load()
    a = 4096                                   # any aligned non-null address: nothing is dereferenced on the refused paths

    def refused(rc, what):
        assert rc != 0 and what in lib.x3d_last_error().decode(), (rc, lib.x3d_last_error())

    refused(lib.x3d_seg_grad_sumsq(None, a, 1, a, 1, a, a, None), "seg_grad_sumsq: bad args")
    refused(lib.x3d_seg_grad_sumsq(a, a, 0, a, 1, a, a, None), "seg_grad_sumsq: bad chunk table")
    refused(lib.x3d_seg_grad_sumsq(a, a, 1, a, 1, a + 4, a, None), "seg_grad_sumsq: misaligned pointer")
    refused(lib.x3d_sgd_pt(a, None, a, a, 1, a, 1, None, 0.1, 0.9, 0.0, 1.0, None, 0.0, None, 0.0, None), "sgd_pt: bad args")
    refused(lib.x3d_sgd_pt(a, a, a, a, 1, a, 1, a + 2, 0.1, 0.9, 0.0, 1.0, None, 0.0, None, 0.0, None), "sgd_pt: misaligned lr_scale")
    refused(lib.x3d_sgd_pt(a, a, a, a, 1, a, 1, a, 0.1, 0.9, 0.0, 1.0, a, 0.0, None, 0.0, None), "sgd_pt: max_norm")
    refused(lib.x3d_sgd_pt(a, a, a, a, 1, a, 1, a, 0.1, 0.9, 0.0, 1.0, None, 0.0, a, 1.0, None), "sgd_pt: ema_decay")
    refused(lib.x3d_adam_pt(a, a, a, a, a, 1, a, 1, a, 1e-3, 0.9, 0.999, 1e-7, 0.0, 1.0, 0, None, 0.0, None, 0.0, None),
            "adam_pt: bad args")
    refused(lib.x3d_adam_pt(a, a, a, a, a, 1, a, 0, a, 1e-3, 0.9, 0.999, 1e-7, 0.0, 1.0, 1, None, 0.0, None, 0.0, None),
            "adam_pt: bad chunk table")
    refused(lib.x3d_lars_pt(a, a, a, a, 1, a, 1, a, 0.1, 0.9, 0.0, 1.0, 0.0, 0.0, 0, None, 0.0, None, 0.0, a, a, None),
            "lars_pt: trust_coef")
    refused(lib.x3d_lars_pt(a, a, a, a, 1, a, 1, a, 0.0, 0.9, 0.0, 1.0, 0.02, 0.0, 1, None, 0.0, None, 0.0, a, a, None),
            "lars_pt: clip needs lr > 0")
    refused(lib.x3d_adamw_pt(a, a, a, a, a, 1, a, 1, a, 1e-3, 0.9, 0.999, 1e-7, -0.1, 1.0, 1, None, 0.0, None, 0.0, None),
            "adamw_pt: decay")
    refused(lib.x3d_lamb_pt(a, a, a, a, a, 1, a, 1, a, 1e-3, 0.9, 0.999, 0.0, 0.0, 1.0, 1, None, 0.0, None, 0.0, a, a, None),
            "lamb_pt: eps")
    refused(lib.x3d_lamb_pt(a, a, a, a, a, 1, a, 1, a + 1, 1e-3, 0.9, 0.999, 1e-6, 0.0, 1.0, 1, None, 0.0, None, 0.0, a, a, None),
            "lamb_pt: misaligned lr_scale")


# ---- names -> depth groups, scales, frozen names ------------------------------------------------------------------------
def _arch(name):
    arch = build_arch(x.get_config(name))
    return arch, param_specs(arch)


@pytest.mark.parametrize("name", ["XS", "M"])
def test_depth_groups(name):
    arch, specs = _arch(name)
    group, top = depth_groups(arch)
    blocks = arch.blocks
    assert top == len(blocks) + 1 and len(blocks) == sum(s.depth for s in arch.stages)
    trainable = [s.name for s in specs if s.trainable]
    for n in trainable:
        if n.startswith("conv1/"):
            assert group(n) == 0
        elif n.startswith(("conv5/", "fc1/", "fc2/")):
            assert group(n) == top
    # every block: all of its tensors in its own group, the shortcut conv and its BatchNorm of a stage's first block too
    seen = set()
    for i, b in enumerate(blocks):
        mine = [n for n in trainable if n.startswith(block_prefix(b) + "/")]
        assert mine and all(group(n) == i + 1 for n in mine)
        seen |= set(mine)
        if b.index == 0:
            assert b.has_shortcut_conv
            assert group(block_prefix(b) + "/residual/kernel") == group(block_prefix(b) + "/bn_r/gamma") == i + 1
            assert block_prefix(b) + "/residual/kernel" in mine
    groups = [group(n) for n in trainable]
    assert groups == sorted(groups) and set(groups) == set(range(top + 1))      # network order, no group empty
    assert len(seen) + sum(g in (0, top) for g in groups) == len(trainable)
    first_of_stage_2 = next(b for b in blocks if b.stage == 2 and b.index == 0)
    assert group(block_prefix(first_of_stage_2) + "/residual/kernel") == 1 + arch.stages[0].depth + arch.stages[1].depth
    with pytest.raises(ValueError, match="not a tensor"):
        group("stages/9/stage/layer_with_weights-0/bottleneck/a/kernel")


@pytest.mark.parametrize("name", ["XS", "M"])
def test_lr_scales(name):
    arch, specs = _arch(name)
    group, top = depth_groups(arch)
    segs = flat_segments(specs)
    decay = 0.75
    mult = (("fc2/", 10.0), ("stages/3/", 2.0), ("fc2/bias", 3.0), ("stages/3/stage/layer_with_weights-1/", 0.5))
    freeze = ("conv1/", "stages/0/", "stages/1/stage/layer_with_weights-0/bn_r/")
    tuned, scales, frozen = lr_scales(arch, specs, FinetuneSettings(decay, mult, freeze))
    assert frozen == [s.name for s in segs if s.name.startswith(freeze)] and len(frozen) > 6
    assert tuned == [s for s in segs if not s.name.startswith(freeze)] and len(tuned) == len(scales)
    assert len(tuned) + len(frozen) == len(segs)
    got = {s.name: c for s, c in zip(tuned, scales)}
    assert not set(got) & set(frozen)                                           # frozen names absent
    for n, c in got.items():
        hits = [(len(p), f) for p, f in mult if n.startswith(p)]
        m = max(hits)[1] if hits else 1.0                                       # the longest prefix wins
        assert c == float(F32(decay ** (top - group(n)) * m)), n
    assert got["fc2/kernel"] == 10.0 and got["fc2/bias"] == 3.0 and got["fc1/kernel"] == 1.0
    assert got["stages/3/stage/layer_with_weights-1/bottleneck/a/kernel"] == float(F32(decay ** (top - group(
        "stages/3/stage/layer_with_weights-1/bottleneck/a/kernel")) * 0.5))
    assert got["stages/3/stage/layer_with_weights-0/residual/kernel"] == float(F32(decay ** len(arch.stages[3].blocks) * 2.0))
    # everything off: every tensor, scale 1
    tuned, scales, frozen = lr_scales(arch, specs, OFF)
    assert tuned == segs and scales == [1.0] * len(segs) and frozen == []
    # the layout is the model's: offsets padded to 4 floats, trainable tensors in creation order
    assert all(s.offset % 4 == 0 for s in segs) and segs[0].offset == 0
    assert all(b.offset == a.offset + (a.length + 3) // 4 * 4 for a, b in zip(segs, segs[1:]))


def test_lr_scales_rejects():
    arch, specs = _arch("XS")
    with pytest.raises(ValueError, match="SOLVER.FREEZE.*'stages/7/' matches no trainable tensor"):
        lr_scales(arch, specs, FinetuneSettings(1.0, (), ("conv1/", "stages/7/")))
    with pytest.raises(ValueError, match="SOLVER.LR_MULT.*'fc3/' matches no trainable tensor"):
        lr_scales(arch, specs, FinetuneSettings(1.0, (("fc3/", 2.0),), ()))
    with pytest.raises(ValueError, match="matches no trainable tensor"):        # a moving statistic is not trainable
        lr_scales(arch, specs, FinetuneSettings(1.0, (), ("conv1/bn/moving_mean",)))
    with pytest.raises(ValueError, match="fc2/bias: matched by SOLVER.FREEZE .* and by SOLVER.LR_MULT"):
        lr_scales(arch, specs, FinetuneSettings(1.0, (("fc2/", 10.0),), ("fc2/bias",)))
    with pytest.raises(ValueError, match="leaves nothing to train"):
        lr_scales(arch, specs, FinetuneSettings(1.0, (), ("conv1/", "stages/", "conv5/", "fc")))
    with pytest.raises(ValueError, match="not positive and finite in fp32"):
        lr_scales(arch, specs, FinetuneSettings(1e-9, (), ()))


@pytest.mark.parametrize("name", ["XS", "M"])
def test_the_tuned_chunk_table_covers_exactly_the_unfrozen_tensors(name):
    arch, specs = _arch(name)
    segs = flat_segments(specs)
    freeze = ("conv1/", "stages/0/", "stages/1/", "fc2/bias")
    tuned, scales, frozen = lr_scales(arch, specs, FinetuneSettings(0.9, (), freeze))
    n = segs[-1].offset + segs[-1].length + 3
    want = np.zeros(n, bool)
    for s in segs:
        if s.name not in frozen:
            want[s.offset:s.offset + s.length] = True
    table = SegTable(tuned)
    hits = np.zeros(n, np.int32)
    for t, first, cnt in table.chunks:
        assert 0 < cnt <= hip.SEG_CHUNK and first % 4 == 0
        s = tuned[t]
        assert s.offset <= first and first + cnt <= s.offset + s.length         # inside its own segment
        hits[first:first + cnt] += 1
    assert np.array_equal(hits == 1, want) and hits.max() == 1                 # every tuned element once, nothing else
    assert table.nseg == len(tuned) == len(scales)
    assert [bool(f) for f in table.segs[:, 2]] == [s.l2 for s in tuned]
    frozen_elems = sum(s.length for s in segs if s.name in frozen)
    assert frozen_elems > 0 and hits.sum() == sum(s.length for s in segs) - frozen_elems


def test_the_model_keeps_what_set_finetune_built():
    """on a dry model (no device): the tuned table, the name -> scale dict and the frozen names; clearing restores the defaults;
    the layout finetune.flat_segments assumes is the model's"""
    from x3d_tf_amd.model import X3D
    cfg = x.get_config("XS", ["NETWORK.NUM_CLASSES", 10])
    m = X3D(cfg, device="dry")
    assert m.segments == flat_segments(param_specs(m.arch))
    assert m._ft is None and m.tuned_segments == m.segments and m.frozen_names == []
    assert m.lr_scales == {s.name: 1.0 for s in m.segments}
    m.set_finetune(freeze=["conv1/", "stages/0/"], lr_mult=[["fc2/", 10.0]], layer_decay=0.5)
    assert m._ft is not None and m._ft.table.nseg == len(m.tuned_segments) < len(m.segments)
    assert m.frozen_names and all(n.startswith(("conv1/", "stages/0/")) for n in m.frozen_names)
    assert not set(m.lr_scales) & set(m.frozen_names) and set(m.lr_scales) | set(m.frozen_names) == {s.name for s in m.segments}
    assert m.lr_scales["fc2/kernel"] == 10.0 and m.lr_scales["fc1/kernel"] == 1.0
    assert [s.name for s in m.tuned_segments] == list(m.lr_scales)
    with pytest.raises(ValueError, match="layer_decay"):
        m.set_finetune(layer_decay=0.0)
    with pytest.raises(ValueError, match="matches no trainable tensor"):
        m.set_finetune(freeze=["nothing/"])
    m.set_finetune()
    assert m._ft is None and m.tuned_segments == m.segments and m.frozen_names == []
