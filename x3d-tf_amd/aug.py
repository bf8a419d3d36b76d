"""Training augmentation parameters of one clip (AUG.* of the config; the kernels are x3d_train_clips_aug, the batch call
`views.make_train_batch_aug`).

The draws happen on the host, in the manner of `mix.draw_mix_params`, from a seeded `numpy.random.Generator`; ONE parameter
set applies to every frame of a clip.  The algorithms, in the order their draws are made:

geometry   "jitter": `views.draw_train_params` (start, short-side target, crop offsets; reference transforms.py:33, 124,
           199-203), from a torch generator seeded with one draw of `rng`.
           "rrc": start ~ U{0..F-1}, then torchvision's `RandomResizedCrop.get_params` [TV-3p]: up to 10 tries of
           area = U(RRC_SCALE) * H * W, aspect = exp(U(log RRC_RATIO)), w = round(sqrt(area * aspect)),
           h = round(sqrt(area / aspect)), accepted when 0 < w <= W and 0 < h <= H, the corner uniform over the valid
           positions; if all fail, the centre crop of the whole frame with its aspect clamped to RRC_RATIO.
flip       with probability FLIP_PROB.
colour     PySlowFast's `color_jitter` [PSF-3p]: with probability COLOR_PROB the clip gets brightness, contrast and
           saturation factors 1 + U(-v, v) (strength 0: factor 1, no draw) applied in a uniformly random order, nothing
           clamped in between; with probability GRAYSCALE_PROB the clip is turned grey afterwards.
erase      timm's `RandomErasing` [TIMM-3p], one box per clip: with probability RE_PROB up to 10 tries of
           area = U(RE_AREA) * S * S, aspect = exp(U(log RE_RATIO)), h = round(sqrt(area * aspect)),
           w = round(sqrt(area / aspect)), accepted when 0 < h < S and 0 < w < S, top ~ U{0..S-h}, left ~ U{0..S-w}; no box if
           all fail.  The box is in OUTPUT-crop coordinates (after the mirror).
seed       63 bits for the noise of RE_MODE "pixel".

RandAugment (AUG.AA_TYPE) is drawn separately, by `draw_randaug` below (its own record type and its own generator: AugParams
and the draws above do not move), and runs on the uint8 frames before all of the above (x3d_randaug_clips)."""
import collections
import math

import numpy as np

from .config import aug_settings

GRAY = (0.299, 0.587, 0.114)      # ITU-R BT.601 luma, as PySlowFast's `grayscale`
COLOR_OPS = ("brightness", "contrast", "saturation")

# crop: "jitter" (start, jitter, y0, x0 as views.draw_train_params; box unused) or "rrc" (start and box = (ry0, rx0, rh, rw) in
# the source frame; jitter, y0, x0 unused).  order: the three COLOR_OPS in application order; a factor of 1.0 is the identity.
# erase: (ey0, ey1, ex0, ex1), rows [ey0, ey1) x columns [ex0, ex1) of the output crop; all 0: no box.
# seed: keys the N(0, 1) noise of RE_MODE "pixel" of THIS clip (the noise of an element depends on the clip's seed, the clip's
# index in the batch and the element's index in the clip; not on the other clips).
AugParams = collections.namedtuple("AugParams", "crop start jitter y0 x0 box flip brightness contrast saturation order gray erase "
                                   "seed")
NO_ERASE = (0, 0, 0, 0)


def rrc_box(height: int, width: int, scale, ratio, rng: np.random.Generator):
    """torchvision RandomResizedCrop.get_params -> ((ry0, rx0, rh, rw), accepted); accepted False: the centre-crop fallback."""
    h_, w_ = int(height), int(width)
    area = h_ * w_
    lo, hi = math.log(ratio[0]), math.log(ratio[1])
    for _ in range(10):
        target = area * rng.uniform(scale[0], scale[1])
        aspect = math.exp(rng.uniform(lo, hi))
        w = int(round(math.sqrt(target * aspect)))
        h = int(round(math.sqrt(target / aspect)))
        if 0 < w <= w_ and 0 < h <= h_:
            return (int(rng.integers(0, h_ - h + 1)), int(rng.integers(0, w_ - w + 1)), h, w), True
    in_ratio = w_ / h_
    if in_ratio < ratio[0]:
        w = w_
        h = min(max(int(round(w / ratio[0])), 1), h_)
    elif in_ratio > ratio[1]:
        h = h_
        w = min(max(int(round(h * ratio[1])), 1), w_)
    else:
        w, h = w_, h_
    return ((h_ - h) // 2, (w_ - w) // 2, h, w), False


def erase_box(size: int, area, ratio, rng: np.random.Generator):
    """timm RandomErasing's box search on a size x size crop -> (ey0, ey1, ex0, ex1), NO_ERASE when all 10 tries fail."""
    s = int(size)
    lo, hi = math.log(ratio[0]), math.log(ratio[1])
    for _ in range(10):
        target = rng.uniform(area[0], area[1]) * s * s
        aspect = math.exp(rng.uniform(lo, hi))
        h = int(round(math.sqrt(target * aspect)))
        w = int(round(math.sqrt(target / aspect)))
        if 0 < h < s and 0 < w < s:
            top, left = int(rng.integers(0, s - h + 1)), int(rng.integers(0, s - w + 1))
            return (top, top + h, left, left + w)
    return NO_ERASE


def draw_aug_params(cfg, num_video_frames: int, height: int, width: int, rng: np.random.Generator) -> AugParams:
    """The random draws of one training clip from a video of F frames of height x width (module docstring).  The settings are
    AUG.* whatever AUG.ENABLE says (the switch decides who calls this, not what it draws)."""
    s = aug_settings(cfg)
    f, h, w = int(num_video_frames), int(height), int(width)
    if f <= 0 or h <= 0 or w <= 0:
        raise ValueError(f"draw_aug_params: video {f} x {h} x {w}")
    size = int(cfg.DATA.TRAIN_CROP_SIZE)
    if s.crop == "jitter":
        import torch
        from .views import draw_train_params
        g = torch.Generator()
        g.manual_seed(int(rng.integers(0, 2 ** 63)))
        p = draw_train_params(f, h, w, cfg, g)
        start, jitter, y0, x0, box = p["start"], p["jitter"], p["y0"], p["x0"], (0, 0, 0, 0)
    else:
        start = int(rng.integers(0, f))
        box, _ = rrc_box(h, w, s.rrc_scale, s.rrc_ratio, rng)
        jitter, y0, x0 = 0.0, 0, 0
    flip = bool(rng.random() < s.flip_prob)
    factors = dict(brightness=1.0, contrast=1.0, saturation=1.0)
    order = COLOR_OPS
    if rng.random() < s.color_prob:
        order = tuple(COLOR_OPS[i] for i in rng.permutation(3))
        for op in COLOR_OPS:
            v = getattr(s, op)
            if v > 0.0:
                factors[op] = 1.0 + float(rng.uniform(-v, v))
    gray = bool(rng.random() < s.grayscale_prob)
    erase = NO_ERASE
    if rng.random() < s.re_prob:
        erase = erase_box(size, s.re_area, s.re_ratio, rng)
    seed = int(rng.integers(0, 2 ** 63))
    return AugParams(s.crop, start, jitter, y0, x0, box, flip, factors["brightness"], factors["contrast"],
                     factors["saturation"], order, gray, erase, seed)


def neutral_params(crop="jitter", start=0, jitter=0.0, y0=0, x0=0, box=(0, 0, 0, 0), flip=False, seed=0) -> AugParams:
    """AugParams with the given geometry, no colour change and no erase box."""
    return AugParams(crop, int(start), float(jitter), int(y0), int(x0), tuple(int(b) for b in box), bool(flip), 1.0, 1.0, 1.0,
                     COLOR_OPS, False, NO_ERASE, int(seed))


def fold_color(params: AugParams):
    """The colour chain of `params` followed by its grayscale as ONE affine map per pixel: returns (M, k), M a 3 x 3 float64
    array and k a float, such that the chain takes a pixel x = (R, G, B) (0-255 scale) to  M @ x + k * m0 * (1, 1, 1),  m0 the
    mean gray of the whole clip BEFORE the chain.

    Why it folds: no op clamps, so each is affine in (x, m): brightness a: x -> a x; saturation a: x -> a x + (1 - a) gray(x);
    contrast a: x -> a x + (1 - a) m with m the clip's mean gray at that moment.  The gray weights w sum to 1, so saturation
    leaves every pixel's gray -- and m -- unchanged, contrast leaves m unchanged, brightness scales it: m = mu * m0 with mu the
    product of the brightness factors applied so far.  A constant added to all three channels passes saturation and grayscale
    unchanged and is scaled by brightness and contrast, so the offset stays one scalar k * m0."""
    w = np.asarray(GRAY, dtype=np.float64)
    m, k, mu = np.eye(3), 0.0, 1.0
    fac = dict(brightness=float(params.brightness), contrast=float(params.contrast), saturation=float(params.saturation))
    if sorted(params.order) != sorted(COLOR_OPS):
        raise ValueError(f"order must be a permutation of {COLOR_OPS}, not {params.order!r}")
    for op in params.order:
        a = fac[op]
        if op == "brightness":
            m, k, mu = a * m, a * k, a * mu
        elif op == "contrast":
            m, k = a * m, a * k + (1.0 - a) * mu
        else:
            m = (a * np.eye(3) + (1.0 - a) * np.outer(np.ones(3), w)) @ m
    if params.gray:
        m = np.outer(np.ones(3), w) @ m
    return m, float(k)


# ---- RandAugment (AUG.AA_TYPE; config.RandAugSpec) -----------------------------------------------------------------------
# timm's `rand_augment_transform` [TIMM-3p] as PySlowFast's rand_augment.py applies it to clips: ONE op and argument per layer
# and clip, applied to every sampled frame, on the uint8 frames at their decoded size (x3d_randaug_clips, before
# x3d_train_clips_aug).  The two op sets hold the same 15 ops in timm's order; "increasing" changes the level mappings of
# Posterize, Solarize and the four ImageEnhance ops so that every op grows stronger with the magnitude.
RANDAUG_OPS = ("AutoContrast", "Equalize", "Invert", "Rotate", "Posterize", "Solarize", "SolarizeAdd", "Color", "Contrast",
               "Brightness", "Sharpness", "ShearX", "ShearY", "TranslateXRel", "TranslateYRel")
RANDAUG_SIGNED = ("Rotate", "ShearX", "ShearY", "TranslateXRel", "TranslateYRel")
RANDAUG_ENHANCE = ("Color", "Contrast", "Brightness", "Sharpness")
RANDAUG_GEOMETRIC = RANDAUG_SIGNED
# name: one of RANDAUG_OPS or "none" (the layer's draw missed its probability).  arg: Rotate degrees (counter-clockwise, as
# PIL.Image.rotate), ShearX / ShearY the shear factor, TranslateXRel / TranslateYRel the offset in PIXELS (fraction * W / H
# of the video it was drawn for), Color / Contrast / Brightness / Sharpness the ImageEnhance factor, Posterize bits kept,
# Solarize threshold, SolarizeAdd addend (threshold 128); None for AutoContrast, Equalize, Invert and "none".
RandAugOp = collections.namedtuple("RandAugOp", "name arg")
RANDAUG_NONE = RandAugOp("none", None)


def randaug_arg(name: str, magnitude: float, inc: bool, negate: bool, height: int, width: int):
    """The argument of op `name` at `magnitude` (0..10), L = magnitude / 10; `negate` is the coin of the "±" ops:
    Rotate ±30 L degrees; ShearX / ShearY ±0.3 L; TranslateXRel / TranslateYRel ±0.45 L of W / H (returned in pixels);
    Color / Contrast / Brightness / Sharpness 0.1 + 1.8 L, increasing: max(0.1, 1 ± 0.9 L); Posterize int(4 L) bits,
    increasing: 4 - int(4 L); Solarize int(256 L), increasing: 256 - int(256 L); SolarizeAdd int(110 L); else None."""
    lv = float(magnitude) / 10.0
    sign = -1.0 if negate else 1.0
    if name == "Rotate":
        return sign * 30.0 * lv
    if name in ("ShearX", "ShearY"):
        return sign * 0.3 * lv
    if name == "TranslateXRel":
        return sign * 0.45 * lv * int(width)
    if name == "TranslateYRel":
        return sign * 0.45 * lv * int(height)
    if name in RANDAUG_ENHANCE:
        return max(0.1, 1.0 + sign * 0.9 * lv) if inc else 0.1 + 1.8 * lv
    if name == "Posterize":
        return 4 - int(4 * lv) if inc else int(4 * lv)
    if name == "Solarize":
        return 256 - int(256 * lv) if inc else int(256 * lv)
    if name == "SolarizeAdd":
        return int(110 * lv)
    if name in ("AutoContrast", "Equalize", "Invert"):
        return None
    raise ValueError(f"unknown RandAugment op {name!r}")


def draw_randaug(spec, height: int, width: int, rng: np.random.Generator):
    """The RandAugment draws of one clip from a video of height x width: a tuple of spec.layers RandAugOp.

    ORDER OF THE DRAWS, per layer, layers in ascending order (pinned by tests/test_randaug.py):
      1. the op:         rng.integers(0, 15), an index into RANDAUG_OPS (uniform, with replacement)
      2. the apply coin: rng.random() < spec.prob; a miss ends the layer with RANDAUG_NONE -- draws 3 and 4 are not made
      3. the magnitude:  only when spec.mstd > 0: clip(rng.normal(spec.magnitude, spec.mstd), 0, 10)
      4. the sign coin:  only for the "±" ops (Rotate, ShearX/Y, TranslateX/YRel) and, with spec.inc, the four ImageEnhance
                         ops: negated when rng.random() < 0.5
    The magnitude is drawn for every applied op, also for those that take no argument."""
    h, w = int(height), int(width)
    if h <= 0 or w <= 0:
        raise ValueError(f"draw_randaug: frame {h} x {w}")
    out = []
    for _ in range(int(spec.layers)):
        name = RANDAUG_OPS[int(rng.integers(0, len(RANDAUG_OPS)))]
        if not rng.random() < spec.prob:
            out.append(RANDAUG_NONE)
            continue
        mag = float(spec.magnitude)
        if spec.mstd > 0.0:
            mag = min(max(float(rng.normal(spec.magnitude, spec.mstd)), 0.0), 10.0)
        negate = False
        if name in RANDAUG_SIGNED or (spec.inc and name in RANDAUG_ENHANCE):
            negate = bool(rng.random() < 0.5)
        out.append(RandAugOp(name, randaug_arg(name, mag, spec.inc, negate, h, w)))
    return tuple(out)


def randaug_matrix(op: RandAugOp, height: int, width: int):
    """The inverse affine map (a, b, c, d, e, f) of a geometric op in fp64, in PIL's convention: output pixel (x, y) reads the
    source position (a (x + 0.5) + b (y + 0.5) + c, d (x + 0.5) + e (y + 0.5) + f).  Rotate as PIL.Image.rotate builds it
    (expand=False, centre (W / 2, H / 2), sine and cosine rounded to 15 decimals); ShearX (1, s, 0; 0, 1, 0); ShearY
    (1, 0, 0; s, 1, 0); TranslateXRel / TranslateYRel an offset of `arg` pixels."""
    h, w = int(height), int(width)
    v = float(op.arg)
    if op.name == "Rotate":
        ang = -math.radians(v % 360.0)
        m = [round(math.cos(ang), 15), round(math.sin(ang), 15), 0.0, round(-math.sin(ang), 15), round(math.cos(ang), 15), 0.0]
        cx, cy = w / 2.0, h / 2.0
        m[2] = m[0] * -cx + m[1] * -cy + m[2] + cx
        m[5] = m[3] * -cx + m[4] * -cy + m[5] + cy
        return tuple(m)
    if op.name == "ShearX":
        return (1.0, v, 0.0, 0.0, 1.0, 0.0)
    if op.name == "ShearY":
        return (1.0, 0.0, 0.0, v, 1.0, 0.0)
    if op.name == "TranslateXRel":
        return (1.0, 0.0, v, 0.0, 1.0, 0.0)
    if op.name == "TranslateYRel":
        return (1.0, 0.0, 0.0, 0.0, 1.0, v)
    raise ValueError(f"{op.name!r} is not a geometric op")


def randaug_fixed_matrix(op: RandAugOp, height: int, width: int, frac_bits: int = 32):
    """randaug_matrix with the half-pixel centres folded into c and f (sx = a x + b y + (c + a / 2 + b / 2), likewise sy) and
    every coefficient rounded to nearest as signed fixed point with `frac_bits` fractional bits: six Python ints."""
    a, b, c, d, e, f = randaug_matrix(op, height, width)
    c, f = c + 0.5 * a + 0.5 * b, f + 0.5 * d + 0.5 * e
    one = float(1 << frac_bits)
    return tuple(int(round(k * one)) for k in (a, b, c, d, e, f))
