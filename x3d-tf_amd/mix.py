"""Mixup / CutMix parameters of one training batch (MIXUP.* of the config; the kernels are x3d_mix_clips / x3d_mix_targets).

The batch is mixed with its own reverse, clip i with clip N-1-i, with ONE set of parameters per batch (timm's `Mixup` in
"batch" mode, PySlowFast's `MixUp`): the draws happen on the host, in the manner of `views.draw_train_params`, from a seeded
`numpy.random.Generator` -- it has `beta`, and a torch CPU generator has no Beta draw that takes a generator."""
import collections
import math

import numpy as np

from .config import mix_settings

MixParams = collections.namedtuple("MixParams", "mode lam y0 y1 x0 x1")
NO_MIX = MixParams("none", 1.0, 0, 0, 0, 0)


def draw_mix_params(cfg, height: int, width: int, rng: np.random.Generator) -> MixParams:
    """The random draws of one batch of height x width frames.  With probability MIXUP.PROB the batch is mixed at all; the
    mode is CutMix with probability MIXUP.SWITCH_PROB when both alphas are positive, else the one whose alpha is positive;
    lam ~ Beta(alpha, alpha) of that mode.  CutMix: timm's box -- r = sqrt(1 - lam), cut_h = int(H r), cut_w = int(W r),
    centre uniform over the frame, edges clipped to it -- and lam corrected to 1 - box_area / (H W).
    Returns MixParams(mode, lam, y0, y1, x0, x1), mode in {"none", "mixup", "cutmix"}; "none" has lam = 1 and an empty box, and
    so has a configuration with MIXUP.ENABLE off, which draws nothing."""
    s = mix_settings(cfg)
    h, w = int(height), int(width)
    if h <= 0 or w <= 0:
        raise ValueError(f"draw_mix_params: frame {h} x {w}")
    if not s.enable:
        return NO_MIX
    if not rng.random() < s.prob:
        return NO_MIX
    if s.alpha > 0.0 and s.cutmix_alpha > 0.0:
        cutmix = bool(rng.random() < s.switch_prob)
    else:
        cutmix = s.cutmix_alpha > 0.0
    if not cutmix:
        return MixParams("mixup", float(rng.beta(s.alpha, s.alpha)), 0, 0, 0, 0)
    lam = float(rng.beta(s.cutmix_alpha, s.cutmix_alpha))
    r = math.sqrt(1.0 - lam)
    cut_h, cut_w = int(h * r), int(w * r)
    cy, cx = int(rng.integers(0, h)), int(rng.integers(0, w))
    y0, y1 = min(max(cy - cut_h // 2, 0), h), min(max(cy + cut_h // 2, 0), h)
    x0, x1 = min(max(cx - cut_w // 2, 0), w), min(max(cx + cut_w // 2, 0), w)
    return MixParams("cutmix", 1.0 - (y1 - y0) * (x1 - x0) / (h * w), y0, y1, x0, x1)
