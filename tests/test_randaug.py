"""RandAugment without a GPU: the AUG.AA_TYPE grammar, the level mappings, the order of the draws, and the NumPy restatement
(tests/randaug_ref.py) of x3d_randaug_clips' arithmetic against Pillow -- exactly for the point and ImageEnhance ops, within one
level for Sharpness (float smooth there, integer here) and the affine ops (double positions there, fixed point here)."""
import math

import numpy as np
import pytest
from PIL import Image, ImageEnhance, ImageOps

import x3d_tf_amd as x
from x3d_tf_amd import aug
from x3d_tf_amd.config import RandAugSpec, parse_aa_type, randaug_settings

from tests import randaug_ref as R

Op = aug.RandAugOp


# ---- config ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("text, want", [
    ("rand", RandAugSpec(10, 2, 0.0, False, 0.5)),
    ("rand-m7-n4-mstd0.5-inc1", RandAugSpec(7, 4, 0.5, True, 0.5)),
    ("rand-inc0-p0.25-mstd1-n1-m0", RandAugSpec(0, 1, 1.0, False, 0.25)),       # any order
    ("rand-p1-m10", RandAugSpec(10, 2, 0.0, False, 1.0)),
    ("rand-p0", RandAugSpec(10, 2, 0.0, False, 0.0)),
])
def test_grammar_accepts(text, want):
    assert parse_aa_type(text) == want
    cfg = x.get_config("XS", ["AUG.ENABLE", True, "AUG.AA_TYPE", text])
    assert randaug_settings(cfg) == want


@pytest.mark.parametrize("text", [
    "augmix-m5", "randaugment", "rand-", "rand-m", "rand--m7",        # another policy / an empty field
    "rand-q3", "rand-w0",                                            # an unknown field
    "rand-m7-m8",                                                    # a repeated field
    "rand-m11", "rand-m-1", "rand-m7.5",                             # magnitude outside 0..10 / not an integer
    "rand-n0", "rand-n2.0",                                          # layers
    "rand-mstd-0.5", "rand-mstdinf", "rand-mstdnan",                 # noise
    "rand-inc2", "rand-incyes",                                      # increasing
    "rand-p1.5", "rand-p-0.1",                                       # probability
    "Rand-m7", " rand-m7",
])
def test_grammar_refuses(text):
    with pytest.raises(ValueError, match="AA_TYPE"):
        parse_aa_type(text)
    with pytest.raises(ValueError, match="AA_TYPE"):
        x.get_config("XS", ["AUG.ENABLE", True, "AUG.AA_TYPE", text])


def test_aa_type_needs_aug_enable_and_defaults_are_off():
    with pytest.raises(ValueError, match="AUG.ENABLE"):
        x.get_config("XS", ["AUG.AA_TYPE", "rand-m7"])
    cfg = x.get_config("M")
    assert cfg.AUG.AA_TYPE == "" and randaug_settings(cfg) is None
    assert randaug_settings(x.get_config("M", ["AUG.ENABLE", True])) is None
    bare = x.get_config("M", freeze=False)
    del bare["AUG"]["AA_TYPE"]                      # a config tree from before the key
    assert randaug_settings(bare) is None
    del bare["AUG"]
    assert randaug_settings(bare) is None


# ---- level mappings --------------------------------------------------------------------------------------------------
def test_level_mappings():
    H, W = 40, 56
    arg = lambda name, m, inc, neg=False: aug.randaug_arg(name, m, inc, neg, H, W)     # noqa: E731
    for inc in (False, True):
        for m, lv in ((0, 0.0), (5, 0.5), (10, 1.0)):
            assert arg("Rotate", m, inc) == 30.0 * lv and arg("Rotate", m, inc, True) == -30.0 * lv
            for name in ("ShearX", "ShearY"):
                assert arg(name, m, inc) == 0.3 * lv and arg(name, m, inc, True) == -(0.3 * lv)
            assert arg("TranslateXRel", m, inc) == 0.45 * lv * W and arg("TranslateYRel", m, inc, True) == -(0.45 * lv) * H
            assert arg("SolarizeAdd", m, inc) == int(110 * lv)
            for name in ("AutoContrast", "Equalize", "Invert"):
                assert arg(name, m, inc) is None
    for name in aug.RANDAUG_ENHANCE:
        ap = lambda v: pytest.approx(v, rel=1e-15, abs=0)                                     # noqa: E731  (one ulp)
        assert [arg(name, m, False) for m in (0, 5, 10)] == ap([0.1, 1.0, 1.9])
        assert [arg(name, m, False, True) for m in (0, 5, 10)] == ap([0.1, 1.0, 1.9])        # no sign without inc
        assert [arg(name, m, True) for m in (0, 5, 10)] == ap([1.0, 1.45, 1.9])
        assert [arg(name, m, True, True) for m in (0, 5, 10)] == ap([1.0, 0.55, 0.1])
        assert arg(name, 10, True, True) >= 0.1                                              # max(0.1, 1 - 0.9)
    assert [arg("Posterize", m, False) for m in (0, 5, 10)] == [0, 2, 4]
    assert [arg("Posterize", m, True) for m in (0, 5, 10)] == [4, 2, 0]
    assert [arg("Solarize", m, False) for m in (0, 5, 10)] == [0, 128, 256]
    assert [arg("Solarize", m, True) for m in (0, 5, 10)] == [256, 128, 0]
    assert [arg("SolarizeAdd", m, True) for m in (0, 5, 10)] == [0, 55, 110]
    with pytest.raises(ValueError):
        arg("Cutout", 5, False)
    assert len(aug.RANDAUG_OPS) == 15 and len(set(aug.RANDAUG_OPS)) == 15


# ---- the draw --------------------------------------------------------------------------------------------------------
def _replay(spec, h, w, rng):
    """the documented order, written out once more"""
    out = []
    for _ in range(spec.layers):
        name = aug.RANDAUG_OPS[int(rng.integers(0, 15))]
        if not rng.random() < spec.prob:
            out.append(Op("none", None))
            continue
        mag = spec.magnitude
        if spec.mstd > 0:
            mag = min(max(float(rng.normal(spec.magnitude, spec.mstd)), 0.0), 10.0)
        neg = False
        if name in aug.RANDAUG_SIGNED or (spec.inc and name in aug.RANDAUG_ENHANCE):
            neg = bool(rng.random() < 0.5)
        out.append(Op(name, aug.randaug_arg(name, mag, spec.inc, neg, h, w)))
    return tuple(out)


def test_seeded_draw_is_pinned():
    spec = parse_aa_type("rand-m7-n6-mstd0.5-inc1-p0.7")
    got = aug.draw_randaug(spec, 40, 56, np.random.default_rng(2024))
    assert got == PINNED, got
    for seed in range(20):
        for text in ("rand-m7-n4-mstd0.5-inc1", "rand-n3", "rand-m3-n5-p0.9"):
            s = parse_aa_type(text)
            a, b = np.random.default_rng(seed), np.random.default_rng(seed)
            assert aug.draw_randaug(s, 33, 18, a) == _replay(s, 33, 18, b)
            assert a.integers(0, 2 ** 32) == b.integers(0, 2 ** 32)           # and the same number of draws
    none = aug.draw_randaug(parse_aa_type("rand-n5-p0"), 8, 8, np.random.default_rng(1))
    assert none == (aug.RANDAUG_NONE,) * 5
    names = {o.name for sd in range(40) for o in aug.draw_randaug(parse_aa_type("rand-n4-p1"), 8, 8, np.random.default_rng(sd))}
    assert names == set(aug.RANDAUG_OPS)


# rng.integers / random / normal / random of default_rng(2024) in the documented order (layer 2 misses its probability)
PINNED = (Op("Rotate", 22.72007929439492), Op("none", None), Op("Equalize", None), Op("Invert", None), Op("SolarizeAdd", 70),
          Op("Contrast", 0.3677989418618709))


# ---- the restatement against Pillow ------------------------------------------------------------------------------------
def _noise(h, w, seed, const_channel=None):
    f = np.random.default_rng(seed).integers(0, 256, (h, w, 3), dtype=np.uint8)
    if const_channel is not None:
        f[..., const_channel] = 77
    return f


FRAMES = [_noise(17, 23, 1), _noise(40, 56, 2), _noise(17, 23, 3, const_channel=1),
          (_noise(40, 56, 4) // 4 + 90).astype(np.uint8),                      # a narrow range: autocontrast stretches it
          np.repeat(np.repeat(_noise(10, 14, 5), 4, axis=0), 4, axis=1)]       # 4 x 4 blocks: equalize step > 1 bins


def _pil(f):
    return Image.fromarray(f, "RGB")


def _solarize_add(img, add, thresh=128):          # timm's solarize_add
    lut = [min(255, i + add) if i < thresh else i for i in range(256)]
    return img.point(lut + lut + lut)


@pytest.mark.parametrize("k", range(len(FRAMES)))
def test_point_ops_equal_pillow(k):
    f = FRAMES[k]
    img = _pil(f)
    eq = lambda op, want: np.testing.assert_array_equal(R.apply_op(f, op), np.asarray(want), err_msg=str(op))   # noqa: E731
    eq(Op("Invert", None), ImageOps.invert(img))
    for t in (0, 1, 77, 128, 255, 256):
        eq(Op("Solarize", t), ImageOps.solarize(img, t))
    for bits in (0, 1, 2, 4, 7, 8):
        eq(Op("Posterize", bits), ImageOps.posterize(img, bits) if bits else Image.fromarray(np.zeros_like(f)))
    for add in (0, 55, 110):
        eq(Op("SolarizeAdd", add), _solarize_add(img, add))
    eq(Op("AutoContrast", None), ImageOps.autocontrast(img))
    eq(Op("Equalize", None), ImageOps.equalize(img))


@pytest.mark.parametrize("k", range(len(FRAMES)))
def test_enhance_ops_equal_pillow(k):
    f = FRAMES[k]
    img = _pil(f)
    for factor in (0.1, 0.55, 1.0, 1.45, 1.9, 0.1 + 1.8 * 0.7):
        for name, enh in (("Color", ImageEnhance.Color), ("Contrast", ImageEnhance.Contrast), ("Brightness", ImageEnhance.Brightness)):
            np.testing.assert_array_equal(R.apply_op(f, Op(name, factor)), np.asarray(enh(img).enhance(factor)),
                                          err_msg=f"{name} {factor}")


@pytest.mark.parametrize("k", range(len(FRAMES)))
def test_sharpness_within_one_level_of_pillow(k):
    """the smooth's division may round differently (Pillow: float, +0.5, truncate; here (s + 6) // 13): at most one level in
    d, scaled by |1 - f| <= 0.9, plus less than one from the truncation -> at most 1 after truncation"""
    f = FRAMES[k]
    for factor in (0.1, 0.55, 1.0, 1.45, 1.9):
        got = R.apply_op(f, Op("Sharpness", factor)).astype(int)
        want = np.asarray(ImageEnhance.Sharpness(_pil(f)).enhance(factor)).astype(int)
        assert np.abs(got - want).max() <= 1, factor
        np.testing.assert_array_equal(got[0], f[0])              # the border is copied
        np.testing.assert_array_equal(got[:, -1], f[:, -1])


def _smooth_frame(h, w):
    """horizontally and vertically neighbouring pixels differ by at most 4 levels"""
    yy, xx = np.mgrid[0:h, 0:w].astype(np.float64)
    f = np.stack([128 + 1.9 * xx - 1.7 * yy, 40 + 1.5 * yy + 1.2 * xx, 200 - 1.8 * xx + 30 * np.sin(yy / 9.0)], axis=-1)
    f = np.clip(np.rint(f), 0, 255).astype(np.uint8)
    d = f.astype(int)
    assert max(np.abs(np.diff(d, axis=0)).max(), np.abs(np.diff(d, axis=1)).max()) <= 4
    return f


GEOM = [Op("Rotate", 21.0), Op("Rotate", -30.0), Op("Rotate", 7.3), Op("ShearX", 0.21), Op("ShearX", -0.3), Op("ShearY", 0.3),
        Op("ShearY", -0.13), Op("TranslateXRel", 0.45 * 0.7), Op("TranslateXRel", -0.2), Op("TranslateYRel", 0.315),
        Op("TranslateYRel", -0.45)]


@pytest.mark.parametrize("hw", [(40, 56), (61, 37)])
@pytest.mark.parametrize("op", GEOM, ids=lambda o: f"{o.name}{o.arg}")
def test_geometric_ops_within_one_level_of_pillow(op, hw):
    """Pillow maps in doubles, the kernel in fixed point with 32 fractional bits and 8-bit weights: the position differs by less
    than 2^-8 pixel (the weight's truncation), times the 4 levels between neighbours far below one level; each side's rounding
    brings the total to one.  Pixels whose source position lies within 1/64 pixel of the frame's edge are left out (the
    inside / outside decision may flip there): under 2 % of the frame."""
    h, w = hw
    if op.name.startswith("Translate"):           # the op carries pixels: the stated fraction of this frame
        op = Op(op.name, op.arg * (w if op.name == "TranslateXRel" else h))
    f = _smooth_frame(h, w)
    fill = (115, 110, 128)
    a, b, c, d, e, ff = aug.randaug_matrix(op, h, w)
    want = np.asarray(_pil(f).transform((w, h), Image.AFFINE, (a, b, c, d, e, ff), resample=Image.BILINEAR, fillcolor=fill)).astype(int)
    if op.name == "Rotate":                       # and the matrix is PIL.Image.rotate's
        np.testing.assert_array_equal(want, np.asarray(_pil(f).rotate(op.arg, resample=Image.BILINEAR, fillcolor=fill)))
    got = R.apply_op(f, op, fill).astype(int)
    yy, xx = np.mgrid[0:h, 0:w].astype(np.float64)
    sx, sy = a * (xx + 0.5) + b * (yy + 0.5) + c, d * (xx + 0.5) + e * (yy + 0.5) + ff
    eps = 1.0 / 64
    near = (np.abs(sx) < eps) | (np.abs(sx - w) < eps) | (np.abs(sy) < eps) | (np.abs(sy - h) < eps)
    assert near.mean() < 0.02
    assert np.abs(got - want)[~near].max() <= 1
    inside = (sx >= eps) & (sx < w - eps) & (sy >= eps) & (sy < h - eps)
    assert 0.3 < inside.mean() < 1.0               # the op moved something, and not everything out


def test_identity_maps_are_exact():
    f = FRAMES[1]
    for op in (Op("Rotate", 0.0), Op("TranslateXRel", 0.0), Op("TranslateYRel", 0.0), Op("ShearX", 0.0), Op("ShearY", 0.0)):
        np.testing.assert_array_equal(R.apply_op(f, op, (1, 2, 3)), f)
    one = 1 << 32
    assert aug.randaug_fixed_matrix(Op("Rotate", 0.0), 40, 56) == (one, 0, one // 2, 0, one, one // 2)
    m = aug.randaug_matrix(Op("Rotate", 90.0), 40, 40)
    assert m[:2] == (0.0, -1.0) and m[3:5] == (1.0, 0.0) and math.isclose(m[2], 40.0) and math.isclose(m[5], 0.0)


def test_apply_clip_samples_and_chains():
    v = np.stack([_noise(9, 11, 10 + i) for i in range(5)])
    got = R.apply_clip(v, (Op("Invert", None), Op("none", None), Op("Solarize", 100)), 4, rate=2, start=3)
    for j, fr in enumerate([3, 0, 2, 4]):
        inv = 255 - v[fr].astype(int)
        np.testing.assert_array_equal(got[j], np.where(inv < 100, inv, 255 - inv))
