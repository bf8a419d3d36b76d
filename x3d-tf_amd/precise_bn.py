"""Precise BatchNorm statistics (PySlowFast BN.USE_PRECISE_STATS / NUM_BATCHES_PRECISE, fvcore's update_bn_stats): every
BatchNorm layer's moving mean and variance recomputed exactly from a few hundred training batches, for the weights the model
holds NOW, instead of trusted to the exponential moving average of statistics that belonged to earlier weights.

fvcore averages per-batch means and variances; here the population itself is pooled.  Every training plan keeps each layer's raw
fp64 (sum, sum of squares) on the device, intact after a forward-only `model(clips, training=True)`, so a batch costs that forward
pass plus one small launch (x3d_precise_bn_accum adds the sums into one pooled fp64 buffer) and the end one more
(x3d_precise_bn_final: mean, unbiased variance -> `flat_params`).  Batches of different shapes and data-parallel ranks pool into
the same buffer; nothing returns to the host inside the loop.
"""
import itertools

import torch

from . import dist as xdist
from . import hip


def recomputed_layers(model):
    """The BatchNorm layers update_bn_stats recomputes: the model's, in layout order, less those of a frozen prefix in inference
    form and the frozen layers (X3D.set_finetune freeze_eval / freeze_bn) -- the rows of every training plan's table."""
    from .finetune import depth_groups
    group, _ = depth_groups(model.arch)
    held = set(getattr(model, "frozen_bn", ()))
    k = getattr(model, "frozen_prefix", 0)
    return [q for q in model.precise_bn_layout().prefixes if q not in held and group(q + "/gamma") >= k]


def update_bn_stats(model, batches, num_batches, group=None) -> int:
    """Overwrites the moving statistics of every BatchNorm layer of `model` with the exact statistics of the first `num_batches`
    items of `batches`; returns how many were used (an iterable that ends early is allowed, an empty one is not).

    batches: an iterable of (clips, labels) or bare clips [N, T, H, W, C]; labels are ignored.  Each batch runs
        `model(clips, training=True)` -- forward only, on the cached training plan of its shape, dropout and stochastic depth
        as in training (fvcore / PySlowFast run the model in train mode) -- followed by one x3d_precise_bn_accum on that plan's
        table.  Shapes may differ from batch to batch.
    group: with an active process group the pooled sums and counts of all ranks are added once, in fp64 (one all-reduce),
        so every rank ends with the statistics of the whole population.

    The momentum blend the forward passes write into the moving statistics is discarded by construction: the last launch
    overwrites every element.  The stochastic-depth state (seed, step) is copied on the device before the passes and copied
    back after them, so the training random stream does not depend on whether this ran.  Launches and device copies only: no
    host synchronisation.  `batches` is not closed: it may be the training iterator.  ValueError for num_batches < 1 and for
    no batch at all.

    A model with a frozen prefix in inference form (X3D.set_finetune freeze_eval): its training plans keep no statistics for
    the prefix layers, and their tables have rows for the layers of the trained region only -- the same rows on every plan and
    every rank, since the prefix is the model's, so the two launches and the all-reduce see one subset.  The prefix's moving
    statistics are neither read nor written.  The same holds for frozen BatchNorm layers (set_finetune freeze_bn): no rows, their
    moving statistics untouched.  With no layer left to recompute -- every layer frozen, or frozen or in the prefix -- nothing
    runs, `batches` is not drawn from, and the result is 0."""
    if isinstance(num_batches, bool) or not isinstance(num_batches, int) or num_batches < 1:
        raise ValueError(f"num_batches must be an integer >= 1, not {num_batches!r}")
    lay = model.precise_bn_layout()
    if len(recomputed_layers(model)) == 0:
        return 0
    nlayers = None                            # rows of the plans' tables: the model's layers, less a frozen prefix in inference form
    pooled = torch.zeros(lay.pooled_size, dtype=torch.float64, device=model.device)
    dp_state = model._dp_state.clone() if getattr(model, "_dp_state", None) is not None else None
    used = 0
    it = iter(batches)
    try:
        for item in itertools.islice(it, num_batches):
            clips = item[0] if isinstance(item, (tuple, list)) else item
            n, t, h, w, _ = clips.shape
            if getattr(model, "det", None) is not None:
                # DETECTION.ENABLE: trunk statistics do not depend on the head -- every box slot empty, the ROI launch reads no plane
                model(clips, training=True, boxes=torch.zeros(n, model.det.max_boxes, 4), num_boxes=[0] * n)
            else:
                model(clips, training=True)
            table = model._plan(n, t, h, w, True).precise_bn_table()
            if nlayers is not None and table.shape[0] != nlayers:
                raise ValueError("update_bn_stats: the model's frozen prefix changed between batches")
            nlayers = int(table.shape[0])
            hip.call("x3d_precise_bn_accum", table.data_ptr(), nlayers, pooled.data_ptr())
            used += 1
    finally:
        if dp_state is not None:
            model._dp_state.copy_(dp_state)
    if used == 0:
        raise ValueError("update_bn_stats: `batches` yielded nothing")
    if xdist._active(group):
        torch.distributed.all_reduce(pooled, op=torch.distributed.ReduceOp.SUM, group=group)
    hip.call("x3d_precise_bn_final", table.data_ptr(), nlayers, pooled.data_ptr(), model.flat_params.data_ptr())
    return used
