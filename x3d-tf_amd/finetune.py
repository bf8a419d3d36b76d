"""Fine-tuning at the level of tensor names: which trainable tensors the solver step leaves alone (SOLVER.FREEZE) and the
learning-rate scale of every other one (SOLVER.LAYER_DECAY, SOLVER.LR_MULT).  Plain Python: no device needed.

Depth groups (timm's layer decay): d = 0 is the stem (`conv1/`), d = 1..L are the residual blocks in network order
(`arch.blocks`; a block's shortcut conv `residual/` and its BatchNorm `bn_r/` belong to that block), d = D = L + 1 is the
head (`conv5/`, `fc1/`, `fc2/`).  A tuned tensor of group d gets

    scale = LAYER_DECAY ** (D - d) * factor of the LONGEST LR_MULT prefix its name starts with (1 without one)

rounded to fp32 -- the value the kernels multiply the learning rate with (x3d_*_pt, include/x3d_hip.h).

Frozen is not "scale 0".  Nesterov SGD with a velocity left over still moves a weight at lr = 0, and 0 * inf is NaN; so a
frozen tensor is simply in no chunk of the table the solver step walks (segments.SegTable over the tuned segments): its
weights, optimizer slots and EMA copy are never read or written, whatever its gradient holds, and its gradient is in neither
the clip norm nor the finite check.  What freezing alone does NOT do: the backward pass still computes (and data parallelism
still all-reduces) the frozen tensors' gradients, BatchNorm inside frozen layers still normalises with batch statistics and
still updates its moving statistics, and the reported regularisation loss still sums over all regularised kernels.

SOLVER.FREEZE_EVAL cuts the passes for the frozen PREFIX (`frozen_prefix`): units are numbered in network order, u0 the stem,
u1..uL the residual blocks; the prefix is the longest run u0..u(k-1) whose every trainable tensor is frozen.  A training step
then runs those units as `training=False` runs them -- BatchNorm on the moving statistics, which are not updated; no block
dropped by NETWORK.DROP_PATH_RATE; nothing kept for a backward pass -- and the backward list ends at the seam, the first unit
above the prefix, with that unit's weight gradients: no gradient of a prefix tensor is computed, its slice of `flat_grads`
stays at the zero the step starts from (data parallelism reduces those zeros: the buckets and their order do not change).
conv5, bn5 and the dense head are never part of the prefix.  Frozen tensors OUTSIDE the prefix keep the behaviour above
(gradient computed, batch statistics), and the regularisation loss is unchanged either way.

SOLVER.FREEZE_BN (`frozen_bn_layers`) is about BatchNorm layers, trained or not, anywhere in the network: a named layer normalises
with its moving statistics in a training step, does not update them, and its backward pass treats them as the constants they then
are (dYraw = gamma * invstd * g).  gamma and beta still receive gradients; whether they move is FREEZE's."""
import math

import numpy as np

from .arch import block_prefix
from .segments import Segment


def depth_groups(arch):
    """(group(name) -> d, D): the depth group of a parameter name and the head's group D = len(arch.blocks) + 1."""
    blocks = [(block_prefix(b) + "/", i + 1) for i, b in enumerate(arch.blocks)]
    top = len(blocks) + 1

    def group(name):
        if name.startswith("conv1/"):
            return 0
        for p, d in blocks:
            if name.startswith(p):
                return d
        if name.startswith(("conv5/", "fc1/", "fc2/")):
            return top
        raise ValueError(f"{name}: not a tensor of the stem, a residual block or the head")

    return group, top


def _prefix_break(arch, param_specs, frozen_names):
    """(k, name): the frozen prefix length and the first trainable tensor, in network order, that is not frozen -- the one
    that ends the prefix (None when the stem and every block are frozen)."""
    group, top = depth_groups(arch)
    frozen = set(frozen_names)
    first = {}                                # unit -> its first trainable tensor that is not frozen
    for s in param_specs:
        if s.trainable and s.name not in frozen:
            first.setdefault(group(s.name), s.name)
    for d in range(top):
        if d in first:
            return d, first[d]
    return top, None


def frozen_prefix(arch, param_specs, frozen_names) -> int:
    """k: the length of the longest run of units u0..u(k-1) -- u0 the stem (`conv1/`), u1..uL the residual blocks of
    `arch.blocks` -- in which every trainable tensor of every unit is in `frozen_names`.  0: the stem is not fully frozen;
    1: the stem only; L + 1: the stem and all blocks.  conv5, bn5 and the dense head are never part of it."""
    return _prefix_break(arch, param_specs, frozen_names)[0]


def frozen_bn_layers(param_specs, prefixes):
    """The BatchNorm layers SOLVER.FREEZE_BN names, in layout order: a layer is the part of its `gamma`'s name in front of
    `/gamma` (`conv1/bn`, `stages/2/blocks/0/bottleneck/bn_a`, ...), matched when it starts with one of `prefixes`; "" matches
    every layer.  ValueError for a prefix that matches no BatchNorm layer."""
    layers = [s.name[:-len("/gamma")] for s in param_specs if s.name.endswith("/gamma")]
    for p in prefixes:
        if not any(q.startswith(p) for q in layers):
            raise ValueError(f"SOLVER.FREEZE_BN: prefix {p!r} matches no BatchNorm layer")
    return tuple(q for q in layers if any(q.startswith(p) for p in prefixes))


def flat_segments(param_specs):
    """The trainable tensors as segments of the flat buffers, in the order and at the offsets model.X3D lays them out:
    trainable tensors first, in creation order, each padded to a multiple of 4 floats."""
    out, off = [], 0
    for s in param_specs:
        if not s.trainable:
            continue
        n = int(np.prod(s.shape, dtype=np.int64))
        out.append(Segment(s.name, off, n, bool(s.l2)))
        off += (n + 3) // 4 * 4
    return out


def lr_scales(arch, param_specs, settings):
    """(tuned segments, scales, frozen names) of `settings` = config.FinetuneSettings (layer_decay, lr_mult, freeze).

    tuned segments: the segments.Segment of every trainable tensor no FREEZE prefix matches, in layout order; scales: their
    learning-rate scales, fp32 values as Python floats, in the same order; frozen names: the rest, in layout order.
    ValueError for a prefix (of either list) that matches no trainable tensor, a tensor that FREEZE and LR_MULT both match, a
    FREEZE that leaves nothing to train, and a scale that is not positive and finite in fp32."""
    segs = flat_segments(param_specs)
    group, top = depth_groups(arch)
    decay, mults, freeze = float(settings.layer_decay), list(settings.lr_mult), list(settings.freeze)
    for what, prefixes in (("SOLVER.FREEZE", freeze), ("SOLVER.LR_MULT", [p for p, _ in mults])):
        for p in prefixes:
            if not any(s.name.startswith(p) for s in segs):
                raise ValueError(f"{what}: prefix {p!r} matches no trainable tensor")
    tuned, scales, frozen = [], [], []
    for s in segs:
        hits = [(len(p), f, p) for p, f in mults if s.name.startswith(p)]
        cold = [p for p in freeze if s.name.startswith(p)]
        if cold and hits:
            raise ValueError(f"{s.name}: matched by SOLVER.FREEZE ({cold[0]!r}) and by SOLVER.LR_MULT ({hits[0][2]!r})")
        if cold:
            frozen.append(s.name)
            continue
        factor = max(hits)[1] if hits else 1.0
        scale = float(np.float32(decay ** (top - group(s.name)) * factor))
        if not (scale > 0.0 and math.isfinite(scale)):
            raise ValueError(f"{s.name}: learning-rate scale {decay} ** {top - group(s.name)} * {factor} is not positive and "
                             "finite in fp32")
        tuned.append(s)
        scales.append(scale)
    if not tuned:
        raise ValueError("SOLVER.FREEZE leaves nothing to train")
    return tuned, scales, frozen
