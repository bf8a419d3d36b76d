"""Soft-target training on the host: the MIXUP.* / TRAIN.LABEL_SMOOTHING config switches, the mix-parameter draws and
the launch lists of dry plans (the kernels and the trainer are held to fp64 references in test_mix_gpu.py)."""
import math
import os
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import x3d_tf_amd as x  # noqa: E402
from x3d_tf_amd.config import mix_settings  # noqa: E402
from x3d_tf_amd.mix import MixParams, draw_mix_params  # noqa: E402


def _strip(cfg):
    """the config tree as it was before the soft-target keys existed"""
    c = cfg.clone()
    c.defrost()
    del c["MIXUP"]
    del c["TRAIN"]["LABEL_SMOOTHING"]
    return c


# ---- config -----------------------------------------------------------------------------------------------------------
def test_config_defaults_and_overrides():
    d = x.get_default_config()
    assert dict(d.MIXUP) == dict(ENABLE=False, ALPHA=0.8, CUTMIX_ALPHA=1.0, PROB=1.0, SWITCH_PROB=0.5)
    assert d.TRAIN.LABEL_SMOOTHING == 0.0
    m = x.get_config("M")
    s = mix_settings(m)
    assert not s.enable and s.label_smoothing == 0.0 and (s.alpha, s.cutmix_alpha, s.prob, s.switch_prob) == (0.8, 1.0, 1.0, 0.5)
    c = x.get_config("M", ["MIXUP.ENABLE", True, "MIXUP.ALPHA", 0.2, "MIXUP.CUTMIX_ALPHA", 0, "MIXUP.PROB", 0.5,
                           "MIXUP.SWITCH_PROB", 1, "TRAIN.LABEL_SMOOTHING", 0.1])
    assert mix_settings(c) == (True, 0.2, 0.0, 0.5, 1.0, 0.1)
    # mixup / CutMix go with both heads
    assert mix_settings(x.get_config("M", ["MIXUP.ENABLE", True, "DATA.MULTI_LABEL", True])).enable


def test_config_without_the_new_keys_means_off_and_is_the_old_tree():
    m = x.get_config("M")
    old = _strip(m)
    assert "MIXUP" not in old and "LABEL_SMOOTHING" not in old.TRAIN
    s = mix_settings(old)
    assert not s.enable and s.label_smoothing == 0.0
    assert draw_mix_params(old, 224, 224, np.random.default_rng(0)).mode == "none"
    # apart from the new keys the tree is what it was: the defaults of the other sections, key for key
    assert set(m) == set(old) | {"MIXUP"}
    assert set(m.TRAIN) == set(old.TRAIN) | {"LABEL_SMOOTHING"}
    assert set(old.TRAIN) == {"DATASET_SIZE", "BATCH_SIZE", "EPOCHS", "OPTIMIZER", "MOMENTUM", "BASE_LR", "WARMUP_EPOCHS",
                              "WARMUP_LR"}
    assert all(m.TRAIN[k] == v for k, v in old.TRAIN.items())
    for k in ("NETWORK", "DATA", "TEST", "WANDB"):
        assert m[k] == old[k]


@pytest.mark.parametrize("over", [
    ["MIXUP.ALPHA", -0.1], ["MIXUP.CUTMIX_ALPHA", -1.0],
    ["MIXUP.ENABLE", True, "MIXUP.ALPHA", 0.0, "MIXUP.CUTMIX_ALPHA", 0.0],
    ["MIXUP.PROB", 1.5], ["MIXUP.PROB", -0.5], ["MIXUP.SWITCH_PROB", 1.01], ["MIXUP.SWITCH_PROB", -0.01],
    ["TRAIN.LABEL_SMOOTHING", 1.0], ["TRAIN.LABEL_SMOOTHING", -0.1],
    ["TRAIN.LABEL_SMOOTHING", 0.1, "DATA.MULTI_LABEL", True],
])
def test_config_refusals(over):
    with pytest.raises(ValueError):
        x.get_config("M", over)
    cfg = x.get_config("M", freeze=False)
    cfg.merge_from_list(over)
    with pytest.raises(ValueError):
        mix_settings(cfg)


def test_both_alphas_zero_is_fine_while_disabled():
    assert not mix_settings(x.get_config("M", ["MIXUP.ALPHA", 0.0, "MIXUP.CUTMIX_ALPHA", 0.0])).enable


# ---- draw_mix_params --------------------------------------------------------------------------------------------------
def _cfg(*over):
    return x.get_config("M", ["MIXUP.ENABLE", True] + list(over))


def test_draws_repeat_with_the_seed():
    cfg = _cfg()
    a = [draw_mix_params(cfg, 224, 224, r) for r in [np.random.default_rng(5)] for _ in range(50)]
    b = [draw_mix_params(cfg, 224, 224, r) for r in [np.random.default_rng(5)] for _ in range(50)]
    c = [draw_mix_params(cfg, 224, 224, r) for r in [np.random.default_rng(6)] for _ in range(50)]
    assert a == b and a != c
    assert all(isinstance(p, MixParams) for p in a)


def _within_5_sigma(k, n, p):
    """a binomial(n, p) count k within 5 standard deviations of its mean (a false alarm once in ~2e6 runs; the draws are seeded
    anyway)"""
    return abs(k - n * p) <= 5.0 * math.sqrt(n * p * (1.0 - p))


def test_draw_statistics_boxes_and_corrected_lambda():
    n, h, w = 2000, 224, 224
    prob, switch = 0.7, 0.4
    cfg = _cfg("MIXUP.PROB", prob, "MIXUP.SWITCH_PROB", switch)
    rng = np.random.default_rng(11)
    draws = [draw_mix_params(cfg, h, w, rng) for _ in range(n)]
    modes = [p.mode for p in draws]
    assert set(modes) == {"none", "mixup", "cutmix"}
    mixed = n - modes.count("none")
    assert _within_5_sigma(mixed, n, prob), (mixed, n, prob)
    assert _within_5_sigma(modes.count("cutmix"), mixed, switch), (modes.count("cutmix"), mixed, switch)
    for p in draws:
        assert 0.0 <= p.lam <= 1.0
        if p.mode == "none":
            assert p == ("none", 1.0, 0, 0, 0, 0)
        elif p.mode == "mixup":
            assert (p.y0, p.y1, p.x0, p.x1) == (0, 0, 0, 0)
        else:
            assert 0 <= p.y0 <= p.y1 <= h and 0 <= p.x0 <= p.x1 <= w
            assert p.lam == 1 - (p.y1 - p.y0) * (p.x1 - p.x0) / (h * w)
    # Beta(0.8, 0.8) has mean 1/2: the mixup lambdas' mean lies within 5 standard errors (variance 1 / (4 (2 alpha + 1)))
    lams = [p.lam for p in draws if p.mode == "mixup"]
    assert abs(np.mean(lams) - 0.5) <= 5.0 * math.sqrt(1.0 / (4 * 2.6) / len(lams))
    # a non-square frame: boxes stay inside it
    for _ in range(500):
        p = draw_mix_params(cfg, 18, 22, rng)
        assert 0 <= p.y0 <= p.y1 <= 18 and 0 <= p.x0 <= p.x1 <= 22


def test_prob_zero_never_mixes_and_a_zero_alpha_never_picks_its_mode():
    rng = np.random.default_rng(3)
    assert all(draw_mix_params(_cfg("MIXUP.PROB", 0.0), 224, 224, rng).mode == "none" for _ in range(500))
    assert all(draw_mix_params(_cfg("MIXUP.ALPHA", 0.0), 224, 224, rng).mode == "cutmix" for _ in range(500))
    assert all(draw_mix_params(_cfg("MIXUP.CUTMIX_ALPHA", 0.0), 224, 224, rng).mode == "mixup" for _ in range(500))
    # disabled: nothing is drawn at all (the generator's state does not move)
    off = x.get_config("M")
    r1, r2 = np.random.default_rng(9), np.random.default_rng(9)
    assert draw_mix_params(off, 224, 224, r1).mode == "none"
    assert r1.random() == r2.random()


# ---- dry plans --------------------------------------------------------------------------------------------------------
def test_default_dry_plans_are_unchanged_and_a_soft_target_call_swaps_only_the_loss():
    from x3d_tf_amd.model import X3D
    base = ["DATA.TEMP_DURATION", 4]

    def plan(cfg):
        m = X3D(cfg, dtype=torch.float32, device="dry")
        return m._plan(2, 4, 64, 64, True)

    def names(pl):
        return [e[0] for e in pl.fwd], [e[0] for e in pl.bwd]

    cfg = x.get_config("XS", base)
    f_old, b_old = names(plan(_strip(cfg)))          # a config tree that lacks the new keys altogether
    pl = plan(cfg)
    f0, b0 = names(pl)
    assert (f0, b0) == (f_old, b_old)
    assert f0.count("x3d_softmax_xent") == 1 and "x3d_softmax_xent_soft" not in f0
    assert pl.targets is None                         # nothing allocated for soft targets until some arrive
    # switched on in the config, the plan is still the same list: mixing happens in Trainer.step, in front of the plan
    f1, b1 = names(plan(x.get_config("XS", base + ["MIXUP.ENABLE", True, "TRAIN.LABEL_SMOOTHING", 0.1])))
    assert (f1, b1) == (f0, b0)
    # a soft-target call
    pl.use_soft_targets(True)
    f2, b2 = names(pl)
    assert f2 == [("x3d_softmax_xent_soft" if n == "x3d_softmax_xent" else n) for n in f0] and b2 == b0
    assert tuple(pl.targets.shape) == (2, 400) and pl.targets.dtype == torch.float32
    assert pl.fwd[pl.grad_scale_slot][2][1] == pl.targets.data_ptr()
    # and back: an [N] integer tensor takes the recorded path, launch for launch
    pl.use_soft_targets(False)
    assert names(pl) == (f0, b0) and pl.fwd[pl.grad_scale_slot][2][1] == pl.labels.data_ptr()


def test_binding_declares_the_new_entry_points():
    from x3d_tf_amd import hip
    assert {"x3d_mix_clips", "x3d_mix_targets", "x3d_softmax_xent_soft"} <= set(hip.exported_symbols())
    assert hip.ABI_VERSION >= 137 and hip.load().x3d_version() == hip.ABI_VERSION
    # refusals need no GPU: they come before any launch
    lib = hip.load()
    assert lib.x3d_mix_clips(None, None, hip.MIX_MIXUP, 0.5, 0, 0, 0, 0, 2, 1, 4, 4, 3, hip.F32, None) != 0
    assert b"null" in lib.x3d_last_error()
    assert lib.x3d_mix_clips(256, 256, hip.MIX_MIXUP, float("nan"), 0, 0, 0, 0, 2, 1, 4, 4, 3, hip.F32, None) != 0
    assert b"lam" in lib.x3d_last_error()
    assert lib.x3d_mix_clips(256, 256, hip.MIX_CUTMIX, 0.5, 0, 5, 0, 4, 2, 1, 4, 4, 3, hip.F32, None) != 0
    assert b"box" in lib.x3d_last_error()
    assert lib.x3d_mix_clips(256, 256 + 64, hip.MIX_MIXUP, 0.5, 0, 0, 0, 0, 2, 1, 4, 4, 3, hip.F32, None) != 0
    assert b"overlaps" in lib.x3d_last_error()
