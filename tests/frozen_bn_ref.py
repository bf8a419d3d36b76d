"""What the SOLVER.FREEZE_BN tests share.  The numerical reference is the one of the SOLVER.FREEZE_EVAL tests
(tests/freeze_eval_ref.py): oracle/x3d_oracle.py with `eval_prefix(layers)` around it, so that the frozen layers -- any set, not
only a prefix -- run with training=False (moving statistics, no update, no entry in BNState) and autograd does the rest; a
layer whose statistics are constants then has exactly the backward rule the kernels implement, dYraw = gamma * invstd * g.

Inputs (measured on the CPU when the tests were written): parameters from `randomize_all_bn_` -- moving variances >= 0.5 --
keep the fp32 oracle within 3.3e-5 (relative L2) / 5.3e-5 (of the largest value) of its fp64 evaluation over the cases of
tests/test_frozen_bn_gpu.py.  Moving variances taken from a batch WITHOUT a floor do not: dead channels with a variance near 0
give invstd ~ 316 and the reference is 2e-2 .. 9e-2 away from its fp64 evaluation -- unusable at the 1e-3 / 2e-3 the device is
held to.  `calibrated_moving_stats_` therefore floors the variance.
"""
import torch

from oracle import x3d_oracle as O
from tests.freeze_eval_ref import (eval_prefix, mask_mismatch, prefix_bn_layers, randomize_all_bn_, reference_is_fit,  # noqa: F401
                                   split_names, trained_relu_masks, unit_of)


def bn_layers(params):
    """Every BatchNorm layer (the part of its name in front of /gamma), in layout order."""
    return [n[:-len("/gamma")] for n in params if n.endswith("/gamma")]


def frozen_layers(params, prefixes):
    """The layers SOLVER.FREEZE_BN = `prefixes` names ("" matches every layer)."""
    return [q for q in bn_layers(params) if any(q.startswith(p) for p in prefixes)]


def stat_names(layers):
    return {f"{q}/{w}" for q in layers for w in ("moving_mean", "moving_variance")}


def calibrated_moving_stats_(params, arch, clips, floor=0.5):
    """Moving statistics that belong to the activations: one training-mode oracle pass over `clips` (a batch of its own),
    momentum 0 -- mean and unbiased variance of that batch -- with the variance floored at `floor` (see the module docstring).
    In place; returns params."""
    st = O.BNState()
    O.forward({a: v.clone() for a, v in params.items()}, clips, arch, training=True, state=st,
              dropout_mask=torch.ones(clips.shape[0], arch.fc1_out))
    m = arch.bn_momentum
    for name, new in st.new_moving.items():
        batch = (new - m * params[name]) / (1.0 - m)          # undo the blend: moving * m + batch * (1 - m)
        params[name].copy_(batch.clamp_min(floor) if name.endswith("/moving_variance") else batch)
    return params


def bn_bwd_closed_form(sums, mi, gamma, count=None):
    """fp64 (A, B, C, dgamma, dbeta) per channel from the backward sums (sum g, sum g * yraw), mean / invstd and gamma.
    count = None: the frozen rule (mean and invstd are constants); a number: the batch-statistics rule over that many
    elements per channel."""
    sums, mi, gamma = sums.double().cpu(), mi.double().cpu(), gamma.double().cpu()
    mean, invstd = mi[:, 0], mi[:, 1]
    dbe = sums[:, 0]
    dga = (sums[:, 1] - mean * dbe) * invstd
    k1 = gamma * invstd
    if count is None:
        return k1, torch.zeros_like(k1), torch.zeros_like(k1), dga, dbe
    b = -k1 * invstd * dga / count
    return k1, b, -k1 * dbe / count - b * mean, dga, dbe
