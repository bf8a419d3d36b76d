"""The reference of the SOLVER.FREEZE_EVAL tests: oracle/x3d_oracle.py with the BatchNorm layers of a frozen prefix in inference
mode.  The oracle file is not edited: `eval_prefix` wraps its module-level `batch_norm` for the length of a `with` block
(unittest.mock.patch.object), so that the layers named get training=False -- the moving statistics, no update, no entry in
BNState -- while every other layer keeps what the caller asked for.  Plus what the tests share: which layers and tensors
belong to a prefix of k units, and the device's ReLU signs of the TRAINED region of a cut plan (tests/util.hip_relu_masks
walks blocks a cut plan does not keep in training form).
"""
import contextlib
from unittest import mock

import torch

from oracle import x3d_oracle as O


def unit_of(arch):
    """name -> unit: 0 the stem, 1..L the residual blocks in network order, L + 1 conv5 and the dense head."""
    from x3d_tf_amd.finetune import depth_groups
    return depth_groups(arch)[0]


def prefix_bn_layers(arch, params, k):
    """BatchNorm layer prefixes (the part in front of /gamma) of units 0..k-1."""
    unit = unit_of(arch)
    return [n[:-len("/gamma")] for n in params if n.endswith("/gamma") and unit(n) < k]


def split_names(arch, params, k):
    """(prefix tensor names, trained tensor names) over the TRAINABLE tensors, for a prefix of k units."""
    unit = unit_of(arch)
    names = O.trainable_names(params)
    return [n for n in names if unit(n) < k], [n for n in names if unit(n) >= k]


def seam_tap(arch, k):
    """The oracle's tap of the seam tensor: the output of unit k - 1."""
    return "conv1/out" if k == 1 else O.block_prefix(arch.blocks[k - 2]) + "/out"


@contextlib.contextmanager
def eval_prefix(layers):
    """Within the block, oracle.batch_norm runs the layers in `layers` (prefixes) with training=False."""
    frozen, real = set(layers), O.batch_norm

    def batch_norm(x, p, prefix, training, *args, **kw):
        return real(x, p, prefix, training and prefix not in frozen, *args, **kw)

    with mock.patch.object(O, "batch_norm", batch_norm):
        yield


def randomize_all_bn_(params, seed):
    """Every BatchNorm layer gets random gamma (0.5 + U(0, 1)), beta and moving mean (OFFSET * N(0, 1)) and moving variance
    (0.5 + U(0, 1)): batch statistics and moving statistics then give visibly different activations (the moving variances
    alone see to that: the tests assert it).  In place; returns params.

    OFFSET is small for the sake of the REFERENCE, not of the code under test.  A Glorot-initialised trunk run on moving
    statistics that do not belong to its activations is not re-normalised from layer to layer: the signal shrinks while every
    layer adds its beta - gamma * mean / std again, so deep activations become nearly constant per channel (|mean| / std above
    100 at conv5's input with all blocks frozen), and the batch-statistics BatchNorm above the seam then divides fp32 rounding
    noise by a tiny deviation.  With offsets of 0.3 the fp32 oracle's own conv5 weight gradient is 9e-4 of its largest value
    away from the same oracle evaluated in fp64 -- half of the 2e-3 the device is to be held to; with 0.1, 3.4e-4; with 0.03,
    6e-5, and at most 1.1e-4 over the five cases of test_cut_step_fp32_against_the_eval_prefix_oracle.  The tests require the
    reference to agree with its fp64 evaluation within a tenth of each limit (reference_is_fit) before they judge the device."""
    OFFSET = 0.03
    g = torch.Generator().manual_seed(seed)
    for k, v in params.items():
        if k.endswith("/gamma"):
            v.copy_(0.5 + torch.rand(v.shape, generator=g))
        elif k.endswith("/beta"):
            v.copy_(OFFSET * torch.randn(v.shape, generator=g))
        elif k.endswith("/moving_mean"):
            v.copy_(OFFSET * torch.randn(v.shape, generator=g))
        elif k.endswith("/moving_variance"):
            v.copy_(0.5 + torch.rand(v.shape, generator=g))
    return params


def trained_relu_masks(pl, k):
    """Sign patterns of every ReLU of the trained region of a (cut) training plan -- blocks k - 1 .. L - 1, conv5, fc1 -- keyed
    like the oracle's ReLU sites, computed as tests/util.hip_relu_masks computes them.  Sites of the prefix are absent: the
    oracle runs them free."""
    def affine_mask(raw, ss):
        ss = ss.detach().double().cpu()
        z = raw.detach().double().cpu() * ss[:, 0].view(1, -1, 1, 1, 1) + ss[:, 1].view(1, -1, 1, 1, 1)
        return z > 0

    masks = {"conv5": affine_mask(pl.c5_raw, pl.bn5.ss), "fc1": pl.h1.detach().cpu() > 0}
    for B in pl.blocks[max(k - 1, 0):]:
        pre = O.block_prefix(B.spec)
        masks[pre + "/a"] = affine_mask(B.a_raw, B.bn_a.ss)
        masks[pre + "/out"] = B.y.detach().float().cpu() > 0
        if B.spec.has_se:
            masks[pre + "/se"] = B.hidden.detach().cpu() > 0
    return masks


def mask_mismatch(dev_masks, free_masks):
    """(fraction, differing, sites) over the sites of dev_masks: device signs against a free-running oracle's RecordMasks."""
    bad = tot = 0
    for site, d in dev_masks.items():
        bad += int((d != free_masks[site]).sum())
        tot += d.numel()
    return bad / max(tot, 1), bad, tot


def reference_is_fit(grads32, grads64, names, rel_l2_limit, max_limit):
    """The fp32 oracle's gradients against the same oracle evaluated in fp64 (same inputs, same ReLU signs): a reference can
    judge at (rel_l2_limit, max_limit of a tensor's largest value) only if its own error is well inside them.  Returns the
    worst (relative L2, max error / largest value) over `names`; AssertionError beyond a TENTH of either limit."""
    worst_l2 = worst_max = 0.0
    for name in names:
        a, b = grads32[name].detach().double(), grads64[name].detach().double()
        worst_l2 = max(worst_l2, ((a - b).norm() / (b.norm() + 1e-30)).item())
        worst_max = max(worst_max, ((a - b).abs().max() / (b.abs().max() + 1e-30)).item())
    assert worst_l2 <= 0.1 * rel_l2_limit and worst_max <= 0.1 * max_limit, (
        f"the fp32 oracle is {worst_l2:.2e} (relative L2) / {worst_max:.2e} (of the largest value) away from its fp64 evaluation: "
        f"these inputs are too ill-conditioned to judge at {rel_l2_limit} / {max_limit}")
    return worst_l2, worst_max


def head_sign_margin(params, arch, seam):
    """For a plan cut at conv5 (all blocks frozen): how far the ReLU pre-activations of the trained region -- bn5's output and
    fc1's -- stay from zero on this input, in units of a worst-case fp32 rounding bound on each value, from an fp64 evaluation
    of the head on the oracle's seam tensor.  Below 1 the sign of some site is not determined in fp32 arithmetic: whether
    two correct implementations agree on it is a coin toss, and with the 35 840 sites of that region the 1e-5 of
    test_train_step_fp32 allows not one.  (bn5 normalises a nearly constant tensor there, see randomize_all_bn_: a rounding
    of its input is worth eps * |x| / std of its output, and fc1 sums 432 such values.)"""
    p = {a: v.double() for a, v in params.items()}
    eps, q = 2.0 ** -24, "conv5/layer_with_weights-1"
    raw = O.pointwise(seam.double(), p["conv5/layer_with_weights-0/kernel"])
    z = O.batch_norm(raw, p, q, True, arch.bn_eps, arch.bn_momentum)
    shape = (1, -1, 1, 1, 1)
    noise = eps * raw.abs() / raw.std((0, 2, 3, 4)).view(shape) * p[q + "/gamma"].view(shape)
    pooled, w = torch.relu(z).mean((2, 3, 4)), p["fc1/kernel"]
    h_noise = eps * (pooled.abs() @ w.abs().t()) + noise.mean((2, 3, 4)) @ w.abs().t()
    return min((z.abs() / noise).min().item(), ((pooled @ w.t()).abs() / h_noise).min().item())
