"""Host side of the batched training augmentation (AUG.* of the config, x3d_tf_amd/aug.py): settings and their validation,
the random draws of a clip, and the fold of the colour chain into one affine map against its sequential fp64 definition."""
import itertools
import math

import numpy as np
import pytest

import x3d_tf_amd as x
from x3d_tf_amd import aug, hip
from x3d_tf_amd.config import aug_settings

from tests.aug_ref import color_chain_sequential


def _cfg(*over):
    return x.get_config("M", list(over))


def test_defaults_and_overrides():
    s = aug_settings(x.get_config("M"))
    assert s == (False, "jitter", (0.08, 1.0), (0.75, 1.3333), 0.5, 0.4, 0.4, 0.4, 1.0, 0.0, 0.25, "pixel", (0.02, 0.3333),
                 (0.3, 3.3333))
    s = aug_settings(_cfg("AUG.ENABLE", True, "AUG.CROP", "rrc", "AUG.RRC_SCALE", [0.25, 0.5], "AUG.FLIP_PROB", 1.0,
                          "AUG.CONTRAST", 0.0, "AUG.GRAYSCALE_PROB", 0.2, "AUG.RE_MODE", "const", "AUG.RE_PROB", 1))
    assert s.enable and s.crop == "rrc" and s.rrc_scale == (0.25, 0.5) and s.flip_prob == 1.0 and s.contrast == 0.0
    assert s.grayscale_prob == 0.2 and s.re_mode == "const" and s.re_prob == 1.0 and s.brightness == 0.4


def test_a_tree_without_the_section_means_off():
    cfg = x.get_config("M", freeze=False)
    del cfg["AUG"]
    s = aug_settings(cfg)
    assert not s.enable and s.crop == "jitter"


@pytest.mark.parametrize("over", [
    ("AUG.RRC_SCALE", [0.0, 1.0]), ("AUG.RRC_SCALE", [0.5, 0.25]), ("AUG.RRC_SCALE", [0.5, 1.5]), ("AUG.RRC_RATIO", [-1.0, 2.0]),
    ("AUG.RE_AREA", [0.3, 0.1]), ("AUG.RE_RATIO", [0.0, 3.0]), ("AUG.RE_RATIO", [float("nan"), 3.0]),
    ("AUG.FLIP_PROB", 1.5), ("AUG.FLIP_PROB", -0.1), ("AUG.COLOR_PROB", 2.0), ("AUG.GRAYSCALE_PROB", -1.0), ("AUG.RE_PROB", 1.01),
    ("AUG.BRIGHTNESS", 1.0), ("AUG.CONTRAST", -0.1), ("AUG.SATURATION", 1.5),
    ("AUG.CROP", "center"), ("AUG.RE_MODE", "rand"),
])
def test_invalid_settings_raise(over):
    with pytest.raises(ValueError, match=over[0]):
        _cfg(*over)


def test_get_config_leaves_the_other_sections_alone():
    on = _cfg("AUG.ENABLE", True, "AUG.CROP", "rrc")
    off = x.get_config("M")
    assert set(on) == set(off) and "AUG" in on
    for k in off:
        if k != "AUG":
            assert on[k] == off[k], k
    assert "ENABLE" in on.AUG and on.is_frozen()


def test_binding_exposes_the_constants_and_version():
    assert hip.load().x3d_version() == 138 == hip.ABI_VERSION
    assert (hip.AUG_CROP_JITTER, hip.AUG_CROP_RRC, hip.AUG_ERASE_CONST, hip.AUG_ERASE_PIXEL) == (0, 1, 0, 1)
    assert hip.AUG_GEOM_COLS == 18 and hip.AUG_COLOR_COLS == 10 and hip.AUG_C_K == 9
    assert sorted(hip.AUG_G.values()) == list(range(hip.AUG_GEOM_COLS))
    assert {"F", "H", "W", "START", "MODE", "NH", "NW", "Y0", "X0", "BH", "BW", "FLIP", "EY0", "EY1", "EX0", "EX1",
            "SEED_LO", "SEED_HI"} == set(hip.AUG_G)
    assert "x3d_train_clips_aug" in hip.exported_symbols() and "x3d_train_clips_aug_scratch" in hip.exported_symbols()
    assert hip.load().x3d_train_clips_aug_scratch(64, 16, 224) == 64 * hip.AUG_MEAN_PARTS * 8


# ---- draws ---------------------------------------------------------------------------------------------------------
OPTS = ["DATA.TEMP_DURATION", 4, "DATA.TRAIN_CROP_SIZE", 160, "DATA.TRAIN_JITTER_SCALES", [182, 228]]
FRAMES = [(37, 240, 320), (21, 340, 256)]


def test_draws_are_deterministic_per_seed():
    for crop in ("jitter", "rrc"):
        cfg = _cfg("AUG.ENABLE", True, "AUG.CROP", crop, "AUG.GRAYSCALE_PROB", 0.3, *OPTS)
        a = [aug.draw_aug_params(cfg, *FRAMES[i % 2], np.random.default_rng(5)) for i in range(4)]
        b = [aug.draw_aug_params(cfg, *FRAMES[i % 2], np.random.default_rng(5)) for i in range(4)]
        c = [aug.draw_aug_params(cfg, *FRAMES[i % 2], np.random.default_rng(6)) for i in range(4)]
        assert a == b and a != c
        rng = np.random.default_rng(5)
        seq = [aug.draw_aug_params(cfg, *FRAMES[0], rng) for _ in range(4)]
        assert seq[0] == a[0] and len(set(seq)) == 4


def _sigma4(p, n):
    """4 standard deviations of the rate of n Bernoulli(p) draws: a fair generator leaves it with probability 6e-5"""
    return 4.0 * math.sqrt(p * (1.0 - p) / n)


@pytest.mark.parametrize("crop", ["jitter", "rrc"])
def test_boxes_lie_inside_and_rates_match(crop):
    n = 3000
    flip_p, gray_p, re_p = 0.3, 0.2, 0.6
    cfg = _cfg("AUG.ENABLE", True, "AUG.CROP", crop, "AUG.FLIP_PROB", flip_p, "AUG.GRAYSCALE_PROB", gray_p, "AUG.RE_PROB", re_p,
               *OPTS)
    s = aug_settings(cfg)
    size = 160
    rng = np.random.default_rng(2024)
    flips = grays = erases = 0
    for i in range(n):
        f, h, w = FRAMES[i % 2]
        p = aug.draw_aug_params(cfg, f, h, w, rng)
        assert p.crop == crop and 0 <= p.start < f
        if crop == "rrc":
            ry0, rx0, rh, rw = p.box
            assert rh >= 1 and rw >= 1 and 0 <= ry0 and ry0 + rh <= h and 0 <= rx0 and rx0 + rw <= w
        else:
            from x3d_tf_amd.views import train_resized_hw
            assert 182 <= p.jitter <= 228
            nh, nw = train_resized_hw(h, w, p.jitter)
            assert 0 <= p.y0 <= nh - size and 0 <= p.x0 <= nw - size
        ey0, ey1, ex0, ex1 = p.erase
        assert 0 <= ey0 <= ey1 <= size and 0 <= ex0 <= ex1 <= size
        if p.erase != aug.NO_ERASE:
            assert ey1 > ey0 and ex1 > ex0
            eh, ew = ey1 - ey0, ex1 - ex0
            # h = round(sqrt(A r)), w = round(sqrt(A / r)): each side is within 0.5 of its real value
            lo_a, hi_a = s.re_area[0] * size * size, s.re_area[1] * size * size
            assert (eh - 0.5) * (ew - 0.5) <= hi_a and (eh + 0.5) * (ew + 0.5) >= lo_a
            assert (eh - 0.5) / (ew + 0.5) <= s.re_ratio[1] and (eh + 0.5) / (ew - 0.5) >= s.re_ratio[0]
        for fac, v in ((p.brightness, s.brightness), (p.contrast, s.contrast), (p.saturation, s.saturation)):
            assert 1 - v <= fac <= 1 + v
        assert sorted(p.order) == sorted(aug.COLOR_OPS)
        flips += p.flip
        grays += p.gray
        erases += p.erase != aug.NO_ERASE
    assert abs(flips / n - flip_p) <= _sigma4(flip_p, n)
    assert abs(grays / n - gray_p) <= _sigma4(gray_p, n)
    # a drawn erase fails only when all 10 tries miss; a try misses with probability < 0.1 for these ranges (the side
    # sqrt(area * aspect) reaches the crop size only for area * aspect >= 1, i.e. in a corner of the (area, log aspect)
    # rectangle), so the miss rate is below 1e-10 and the erase rate is RE_PROB
    assert abs(erases / n - re_p) <= _sigma4(re_p, n)


def test_rrc_tries_respect_area_and_aspect_and_the_fallback_is_reachable():
    rng = np.random.default_rng(9)
    scale, ratio = (0.08, 1.0), (0.75, 1.3333)
    accepted = 0
    for i in range(4000):
        _, h, w = FRAMES[i % 2]
        (ry0, rx0, rh, rw), ok = aug.rrc_box(h, w, scale, ratio, rng)
        assert 0 <= ry0 and ry0 + rh <= h and 0 <= rx0 and rx0 + rw <= w and rh >= 1 and rw >= 1
        if ok:
            accepted += 1
            # both sides are rounded to the nearest integer: within 0.5 of sqrt(A r) and sqrt(A / r)
            assert (rh - 0.5) * (rw - 0.5) <= scale[1] * h * w and (rh + 0.5) * (rw + 0.5) >= scale[0] * h * w
            assert (rw - 0.5) / (rh + 0.5) <= ratio[1] and (rw + 0.5) / (rh - 0.5) >= ratio[0]
    assert accepted > 3900
    # no box of aspect 100-200 fits either frame: the centre crop with the aspect clamped to the range
    box, ok = aug.rrc_box(240, 320, scale, (100.0, 200.0), rng)
    assert not ok and box == ((240 - 3) // 2, 0, 3, 320)
    box, ok = aug.rrc_box(340, 256, scale, (0.001, 0.002), rng)
    assert not ok and box == (0, (256 - 1) // 2, 340, 1)
    cfg = _cfg("AUG.ENABLE", True, "AUG.CROP", "rrc", "AUG.RRC_RATIO", [100.0, 200.0], *OPTS)
    assert aug.draw_aug_params(cfg, 9, 240, 320, rng).box == (118, 0, 3, 320)


def test_switched_off_ops_draw_neutral_values():
    cfg = _cfg("AUG.ENABLE", True, "AUG.BRIGHTNESS", 0.0, "AUG.CONTRAST", 0.0, "AUG.SATURATION", 0.0, "AUG.RE_PROB", 0.0,
               "AUG.FLIP_PROB", 1.0, *OPTS)
    rng = np.random.default_rng(1)
    for _ in range(50):
        p = aug.draw_aug_params(cfg, 10, 240, 320, rng)
        assert (p.brightness, p.contrast, p.saturation, p.gray, p.erase, p.flip) == (1.0, 1.0, 1.0, False, aug.NO_ERASE, True)
        m, k = aug.fold_color(p)
        assert np.array_equal(m, np.eye(3)) and k == 0.0
    cfg = _cfg("AUG.ENABLE", True, "AUG.COLOR_PROB", 0.0, *OPTS)
    p = aug.draw_aug_params(cfg, 10, 240, 320, rng)
    assert (p.brightness, p.contrast, p.saturation) == (1.0, 1.0, 1.0)


# ---- the fold ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("gray", [False, True])
@pytest.mark.parametrize("order", list(itertools.permutations(aug.COLOR_OPS)))
def test_fold_equals_the_sequential_chain(order, gray):
    rng = np.random.default_rng(2 * list(itertools.permutations(aug.COLOR_OPS)).index(order) + gray)
    clip = rng.uniform(0.0, 255.0, (3, 6, 5, 3))
    p = aug.neutral_params()._replace(brightness=1.31, contrast=0.64, saturation=1.22, order=order, gray=gray)
    want = color_chain_sequential(clip, p)
    m, k = aug.fold_color(p)
    m0 = (clip @ np.asarray(aug.GRAY)).mean()
    got = clip @ m.T + k * m0
    assert np.abs(got - want).max() <= 1e-12 * np.abs(want).max()
    # a factor of 1 is the identity of its op
    p1 = p._replace(contrast=1.0)
    m1, k1 = aug.fold_color(p1)
    assert k1 == 0.0
    assert np.abs(clip @ m1.T - color_chain_sequential(clip, p1)).max() <= 1e-12 * 255 * 2
