"""The train step the reference compiles with Keras (reference train.py:85-125): SGD with Nesterov
momentum, SparseCategoricalCrossentropy on the model's probabilities + L2 regularisation, per-epoch
warm-up/cosine learning-rate schedule -- as an explicit step loop over the HIP model, data-parallel
over RCCL when launched with torchrun.
"""
import contextlib
import math
import os
from typing import Optional

import torch

from . import dist as xdist
from . import ops
from .config import (OPTIMIZERS, device_loss_scale_settings, distill_settings, finetune_settings, freeze_bn_settings, freeze_eval_settings,
                     loss_settings,
                     mix_settings, optim_settings, precise_bn_settings, solver_settings)
from .mix import NO_MIX, draw_mix_params
from .solver import RULES


def lr_schedule(epoch, cfg):
    """reference train.py:114-125: linear warm-up while epoch <= WARMUP_EPOCHS, then half-cosine."""
    tr = cfg.TRAIN
    if epoch > tr.WARMUP_EPOCHS:
        return tr.BASE_LR * (0.5 * (math.cos(math.pi * (epoch / tr.EPOCHS)) + 1))
    return tr.WARMUP_LR + epoch * (tr.BASE_LR - tr.WARMUP_LR) / tr.WARMUP_EPOCHS


class SaveSchedule:
    """When Keras' `ModelCheckpoint(save_freq=...)` writes (reference utils.py:128-132, train.py:110-112).

    save_freq="epoch": `ckpt-{epoch + 1}` after every epoch.  save_freq=n (a positive int): a batch counter runs from the
    start of the `fit` call across epoch boundaries; when it reaches n the checkpoint of the RUNNING epoch is written --
    `ckpt-{epoch index + 1}`, so a save in the middle of epoch index e is named as if e had finished and `resume` continues
    at epoch e + 1, as the reference's does -- the counter resets, and nothing is written at epoch end."""

    def __init__(self, save_freq="epoch"):
        if save_freq != "epoch" and not (isinstance(save_freq, int) and not isinstance(save_freq, bool) and save_freq > 0):
            raise ValueError(f"save_freq must be 'epoch' or a positive int, got {save_freq!r}")
        self.save_freq = save_freq
        self.batches = 0

    def after_batch(self, epoch: int) -> Optional[int]:
        """Called after every batch of epoch index `epoch`; the checkpoint number to write now, or None."""
        if self.save_freq == "epoch":
            return None
        self.batches += 1
        if self.batches < self.save_freq:
            return None
        self.batches = 0
        return epoch + 1

    def after_epoch(self, epoch: int) -> Optional[int]:
        """Called when epoch index `epoch` has finished; the checkpoint number to write now, or None."""
        return epoch + 1 if self.save_freq == "epoch" else None


def check_accum_schedule(steps_per_epoch: int, save_freq, accum_steps: int):
    """`fit` counts batches as steps; with SOLVER.ACCUM_STEPS = A > 1 an epoch and a step-based checkpoint must both end on an
    optimizer update (a checkpoint inside an accumulation would drop the micro-batches gathered so far).  ValueError else."""
    if accum_steps <= 1:
        return
    if steps_per_epoch % accum_steps:
        raise ValueError(f"steps_per_epoch ({steps_per_epoch}) must be a multiple of SOLVER.ACCUM_STEPS ({accum_steps})")
    if isinstance(save_freq, int) and not isinstance(save_freq, bool) and save_freq % accum_steps:
        raise ValueError(f"save_freq ({save_freq}) must be a multiple of SOLVER.ACCUM_STEPS ({accum_steps}): a checkpoint "
                         "must not fall inside an accumulation")


TRAIN_METRICS = ("acc", "top_5_acc")
MULTI_LABEL_METRICS = ("mAP",)
OPT_IN_METRICS = ("mean_class_acc",)   # single-label models, only when asked for: per-class counters (x3d_class_hits)
_DEFAULT_METRICS = object()      # fit(metrics=...) default: TRAIN_METRICS, or MULTI_LABEL_METRICS for a multi-label model


def _validation_source(validation_data, epochs_to_run: int):
    """validation_data -> a zero-argument callable returning a fresh iterable of (clips, labels) batches."""
    if validation_data is None:
        return None
    if callable(validation_data) and not hasattr(validation_data, "__iter__"):
        return validation_data
    if iter(validation_data) is validation_data and epochs_to_run > 1:
        raise ValueError("validation_data is a one-shot iterator and would be exhausted after the first epoch: pass a "
                         "callable that returns a fresh one, e.g. validation_data=lambda: InputReader(cfg, False, True)"
                         "(pattern, cfg.TEST.BATCH_SIZE)")
    return lambda: validation_data


NO_CLIP = 3.0e38      # a max_norm that cannot clip: the largest the update launches accept (they refuse what is not finite)


class DeviceLossScale:
    """The dynamic loss scaler of SOLVER.DEVICE_LOSS_SCALE: `state`, the [8] fp64 device tensor the launches read and
    x3d_loss_scale_update writes (ops.loss_scale_state: scale, 1 / scale, finite steps in a row, skipped, applied, last-skipped),
    and what the host knows of it -- ONE STEP LATE.  `publish` (behind a step's update) copies the state into one of two pinned
    host slots and records an event; `previous` (in the next step) waits for that event, which belongs to a step whose launches
    have long run, never for the step in flight.  `read` is the explicit, synchronising read behind the trainer's properties."""

    def __init__(self, device, scale):
        self.state = ops.loss_scale_state(scale, device)
        self.host = torch.zeros(2, ops.LOSS_SCALE_STATE, dtype=torch.float64).pin_memory()
        self.events = [torch.cuda.Event(), torch.cuda.Event()]
        self.turn, self.pending = 0, None         # the slot the next copy goes to; the slot whose copy nobody has waited for
        self.known = [float(scale), 1.0 / float(scale), 0.0, 0.0, 0.0, 0.0, 0.0, 0.0]
        self.dirty = False                        # launches have written the state since `known` was read

    def publish(self):
        self.host[self.turn].copy_(self.state, non_blocking=True)
        self.events[self.turn].record()
        self.pending, self.turn, self.dirty = self.turn, self.turn ^ 1, True

    def previous(self):
        """the state as the last published step left it (the initial one before any)"""
        if self.pending is not None:
            self.events[self.pending].synchronize()
            self.known = self.host[self.pending].tolist()
            self.pending = None
        return self.known

    def read(self):
        """the state now: drains the stream when a step has run since the last read"""
        if self.dirty:
            self.known = self.state.tolist()
            self.dirty, self.pending = False, None
        return self.known

    def write(self, values: dict, sync: bool):
        """state[slot] = value for slot, value in `values`, in stream order.  sync (the counters: the host derives Adam's step
        from them): read first, so that `known` stays what the device holds.  Without it `known` is as current as it was"""
        if sync:
            self.read()
        for slot, value in values.items():
            self.state[slot:slot + 1].fill_(float(value))
            self.known[slot] = float(value)


class Trainer:
    """fwd + bwd + gradient all-reduce + optimizer for one replica.

    model: x3d_tf_amd.model.X3D.  The process group (if any) must already be initialised; every
    replica is given rank 0's initial variables, as variables created under MirroredStrategy are.
    """

    def __init__(self, model, cfg, momentum: Optional[float] = None, sync_moving_stats: bool = True, group=None,
                 loss_scale="auto", mix_seed: int = 0, drop_path_seed: int = 0, teacher=None):
        self.optimizer = cfg.TRAIN.OPTIMIZER.lower()
        if self.optimizer not in OPTIMIZERS:   # reference train.py:88-97: SGD(nesterov) / Adam / NotImplementedError; + lars, adamw, lamb
            raise NotImplementedError(f"{cfg.TRAIN.OPTIMIZER} not supported")
        self.model, self.cfg, self.group = model, cfg, group
        # lars keeps SGD's slot (momentum) and checkpoint layout, adamw and lamb keep Adam's (m, v, `iter`)
        self.rule = RULES[self.optimizer]
        self.slot_kind = self.rule.slot_kind
        self.optim = optim_settings(cfg)      # OPTIM.*: read by the lars / adamw / lamb branches only
        self.last_trust_ratios = None         # lars / lamb: device [nseg] fp32 trust ratios of the last update (model.segments order; fine-tuning: model.tuned_segments)
        self._dls = None                      # DeviceLossScale with SOLVER.DEVICE_LOSS_SCALE and dynamic scaling (below)
        self.opt_step = 0                     # optimizer steps applied (Adam's bias correction counts them)
        # Loss scaling = tf.keras.mixed_precision.LossScaleOptimizer(opt) with its defaults (train.py:99-100): dynamic,
        # initial scale 2^15, doubled after 2000 consecutive finite steps, halved (and the step skipped) when a gradient
        # is inf / nan.  "auto": on for float16 storage (the reference's mixed_float16), off for float32 / bfloat16;
        # a number = fixed scale; None = off.
        if loss_scale == "auto":
            loss_scale = "dynamic" if model.dtype == torch.float16 else None
        self.dynamic_scale = loss_scale == "dynamic"
        self.loss_scale = 2.0 ** 15 if self.dynamic_scale else (float(loss_scale) if loss_scale else 1.0)
        self.growth_steps, self._good_steps, self.skipped_steps = 2000, 0, 0
        # SOLVER.DEVICE_LOSS_SCALE: the dynamic scaler's state lives in device memory, the step decides, skips and rescales
        # there and reads nothing back (`_update`); `loss_scale`, `skipped_steps` and `opt_step` are then synchronising reads
        # of it.  Inert with a fixed scale or none.  Not written to checkpoints (nor is the host's): a resumed run starts at 2^15.
        if device_loss_scale_settings(cfg) and self.dynamic_scale:
            self._dls = DeviceLossScale(model.device, self._loss_scale)
        self.momentum = cfg.TRAIN.MOMENTUM if momentum is None else momentum
        self.world = torch.distributed.get_world_size(group) if torch.distributed.is_initialized() else 1
        self.collectives = xdist._active(group)      # world > 1, or the one-rank rehearsal (X3D_DIST_REHEARSE=1)
        self.sync_moving_stats = sync_moving_stats and self.collectives
        n_st = len(model.arch.stages)
        # bucket order = order in which the backward pass finishes them: head, stage 3..0, stem.  (Merging them into two
        # all-reduces -- {head + last stage}, {rest} -- was measured with X3D_DIST_REHEARSE=1: 26.19 -> 26.16 ms per
        # step, i.e. the per-call cost is not what the 0.45 ms of collective overhead on one rank is made of.)
        per_stage = [n_st] + list(range(n_st - 1, -1, -1)) + [-1]
        self.stage_order = per_stage
        buckets = [model.grad_bucket(s) for s in per_stage]
        self._launch_at = {s: i for i, s in enumerate(per_stage)}
        self.reducer = xdist.BucketReducer(buckets, group)
        self._slot = dict(self._launch_at)
        self._stats_work = None
        xdist.broadcast_([model.flat_params, model.flat_velocity], 0, group)
        # soft-target training (MIXUP.*, TRAIN.LABEL_SMOOTHING; both off by default: `step` is then what it was).  The draws
        # come from a host generator seeded with mix_seed + rank: ranks mix differently, a rerun repeats.
        self.mix = mix_settings(cfg)
        if self.mix.label_smoothing > 0.0 and getattr(model, "multi_label", False):
            raise ValueError("TRAIN.LABEL_SMOOTHING is defined for the softmax head only, not for a multi-label model")
        self._mix_active = self.mix.enable or self.mix.label_smoothing > 0.0
        if self._mix_active:
            import numpy as np
            rank = torch.distributed.get_rank(group) if torch.distributed.is_initialized() else xdist.env_world()[0]
            self._mix_rng = np.random.default_rng(int(mix_seed) + rank)
        self._mix_buf = self._mix_labels = None
        self.last_mix = NO_MIX                # MixParams of the last step
        self.epoch = 0
        self.skipped_keys = []                # variables of the pretrained checkpoint resume(skip_mismatch=True) did not load
        # the solver step around the optimizer (SOLVER.*; all off by default: `step` is then what it was, launch for launch)
        self.solver = solver_settings(cfg)
        self._clip = self.solver.clip_grad_l2norm > 0.0
        self._accum = self.solver.accum_steps
        self._micro = 0                       # micro-batches gathered of the running accumulation
        self._grad_acc = None                 # their summed local gradients (allocated by the first accumulation)
        self.last_grad_norm = None            # device scalar: global L2 norm of the unscaled gradient of the last update
        # fine-tuning (SOLVER.FREEZE / LR_MULT / LAYER_DECAY; off by default: the model is then not told anything).  The update,
        # the clip norm and the finite check then cover the tuned tensors only, at lr * scale per tensor (X3D.set_finetune)
        # SOLVER.FREEZE_EVAL: the frozen prefix also runs in inference form and the backward pass ends above it.  The buckets
        # and the hooks are what they were -- the prefix's buckets carry the zeros the step starts from
        self.finetune = finetune_settings(cfg)
        # SOLVER.FREEZE_BN: the named BatchNorm layers normalise with their moving statistics, which no step then writes
        self.freeze_eval = freeze_eval_settings(cfg)
        self.freeze_bn = freeze_bn_settings(cfg)
        if self.finetune != (1.0, (), ()) or self.freeze_eval or self.freeze_bn:
            model.set_finetune(freeze=self.finetune.freeze, lr_mult=self.finetune.lr_mult, layer_decay=self.finetune.layer_decay,
                               **(dict(freeze_eval=True) if self.freeze_eval else {}),
                               **(dict(freeze_bn=self.freeze_bn) if self.freeze_bn else {}))
        # weight EMA: trainable block + moving statistics, laid out as flat_params; starts from the (broadcast) weights
        self.ema = model.flat_params.clone() if self.solver.ema_decay > 0.0 else None
        # stochastic depth (NETWORK.DROP_PATH_RATE): the tables are drawn on the device from (seed, step); rank r seeds with
        # drop_path_seed + r, so data-parallel ranks drop different samples.  A no-op for a model without the rate.
        rank = torch.distributed.get_rank(group) if torch.distributed.is_initialized() else xdist.env_world()[0]
        self._drop_path_seed = int(drop_path_seed) + rank
        if hasattr(model, "set_drop_path_state"):
            model.set_drop_path_state(self._drop_path_seed, 0)
        # precise BatchNorm (NETWORK.BN.USE_PRECISE_STATS; off by default: `fit` then draws the batches it always drew)
        self.precise = precise_bn_settings(cfg)
        # knowledge distillation (DISTILL.*; off by default: `step` is then what it was, launch for launch).  `teacher`: an X3D
        # model of the student's class layout, or built here from DISTILL.TEACHER / TEACHER_CKPT.  It only ever runs `logits`:
        # never trained, in no bucket, no checkpoint and no EMA, not part of `validate` or `precise_bn`.
        self.distill = distill_settings(cfg, have_teacher=teacher is not None)
        self.teacher = None
        if teacher is not None:
            self._check_teacher(teacher)
        if self.distill.enable:
            self.teacher = teacher if teacher is not None else self._build_teacher()
        self._kd = (self.distill.alpha, self.distill.temperature)
        # class-imbalance losses (LOSS.*; off by default: the model is then not told anything and `step` is what it was).  The
        # tables go to the device once; sample weights come with the batches (`step`, `fit`)
        self.loss_mods = loss_settings(cfg)
        if self.loss_mods != ((), (), 0.0, 0.0):
            model.set_loss(class_weights=self.loss_mods.class_weights or None, pos_weight=self.loss_mods.pos_weight or None,
                           focal_gamma=self.loss_mods.focal_gamma, focal_gamma_neg=self.loss_mods.focal_gamma_neg)

    def _check_teacher(self, teacher):
        m = self.model
        if teacher.num_classes != m.num_classes:
            raise ValueError(f"the teacher has {teacher.num_classes} classes, the student {m.num_classes}: distillation "
                             "compares their logits class by class")
        if bool(getattr(teacher, "multi_label", False)) != bool(getattr(m, "multi_label", False)):
            raise ValueError("teacher and student must both be multi-label (DATA.MULTI_LABEL) or both single-label")

    def _build_teacher(self):
        """The teacher of DISTILL.TEACHER -- a shipped config name (XS .. XL) or a yaml path -- on the student's device and
        storage type, NETWORK.NUM_CLASSES and DATA.MULTI_LABEL forced to the student's, with the weights of
        DISTILL.TEACHER_CKPT.  Every rank loads its own copy: no collective."""
        from .config import get_config, get_default_config
        from .model import X3D
        m, d = self.model, self.distill
        if not d.teacher_ckpt:
            raise ValueError("DISTILL.TEACHER_CKPT is empty: a teacher built from DISTILL.TEACHER needs its checkpoint (a "
                             "randomly initialised teacher teaches nothing)")
        over = ["NETWORK.NUM_CLASSES", int(m.num_classes), "DATA.MULTI_LABEL", bool(getattr(m, "multi_label", False))]
        if d.teacher.endswith((".yaml", ".yml")) or os.sep in d.teacher:
            cfg = get_default_config()
            cfg.merge_from_file(d.teacher)
            cfg.merge_from_list(over)
            cfg.freeze()
        else:
            cfg = get_config(d.teacher, over)
        teacher = X3D(cfg, dtype=m.dtype, device=m.device)
        teacher.load_weights(d.teacher_ckpt)
        self._check_teacher(teacher)
        return teacher

    def _teacher_kw(self, clips):
        """forward_backward's distillation arguments: the teacher's logits of the clips the student sees (after mixing, as
        DeiT / timm feed the teacher); {} with DISTILL off.  Launches only."""
        if self.teacher is None:
            return {}
        return dict(teacher_logits=self.teacher.logits(clips), distill=self._kd)

    def step(self, clips, labels, lr: Optional[float] = None, sample_weight=None, boxes=None, num_boxes=None):
        """clips: this replica's shard [B, T, H, W, 3]; labels [B] (multi-label models: targets [B, classes]).  Returns the
        plan (loss_rows, probs).  With MIXUP.ENABLE or TRAIN.LABEL_SMOOTHING the batch is mixed and the targets are built
        first (`_mix_batch`; `last_mix` holds the parameters drawn).  With DISTILL.ENABLE the teacher's logits of the (mixed)
        clips join the loss (`_teacher_kw`; `plan.kd_rows` holds the KD term per row).  sample_weight: [B] weights of this
        shard's samples (host or device), Keras' `(x, y, sample_weight)`; the weighted rows are still divided by the global batch
        (SUM_OVER_BATCH_SIZE), so `loss` and the data-parallel reduction are what they were.  ValueError together with
        MIXUP.ENABLE: mixing the weights of two samples is not defined here (class weights are fine, the loss is linear in y).
        boxes [B, K, 4], num_boxes [B] (host): DETECTION.ENABLE -- labels are then [B, K] (targets [B, K, classes]) and the loss is
        the mean over this shard's valid boxes (`forward_backward`); missing with the switch on, or given with it off: ValueError."""
        m = self.model
        n = clips.shape[0]
        if lr is None:
            lr = lr_schedule(self.epoch, self.cfg)
        sw = {}
        if boxes is not None or num_boxes is not None or getattr(m, "det", None) is not None:
            sw = dict(boxes=boxes, num_boxes=num_boxes)      # (checked by forward_backward, before any launch)
        if sample_weight is not None:
            if self.mix.enable:
                raise ValueError("sample_weight with MIXUP.ENABLE: the weight of a mixed sample is not defined")
            sw = dict(sw, sample_weight=sample_weight)
        if self._mix_active:
            clips, labels = self._mix_batch(clips, labels)
        if self._accum > 1:
            return self._accum_step(clips, labels, lr, n, sw)
        pl = m.forward_backward(clips, labels, global_batch=n * self.world,
                                on_stage_done=self._on_stage_done if self.collectives else None,
                                loss_scale=self._fb_scale(), **self._teacher_kw(clips), **sw)
        self.reducer.mark_backward_done()     # (an event on the compute stream: finish() measures the exposed exchange from it)
        self.reducer.finish()
        self._finish_stats()
        return self._update(pl, lr)

    # loss_scale / skipped_steps / opt_step: plain host numbers -- except in device mode, where reading one reads the device
    # state (DeviceLossScale.read: an explicit synchronisation of the caller's) and setting one writes it in stream order
    def _ls_get(slot, name, as_type):
        def get(self):
            return getattr(self, name) if self._dls is None else as_type(self._dls.read()[slot])

        def put(self, value):
            if self._dls is None:
                setattr(self, name, value)
            elif slot == ops.LS_SCALE:
                value = ops.loss_scale_value(value)
                self._dls.write({ops.LS_SCALE: value, ops.LS_INV: 1.0 / value}, sync=False)
            else:
                self._dls.write({slot: int(value)}, sync=True)
        return property(get, put)

    loss_scale = _ls_get(ops.LS_SCALE, "_loss_scale", float)
    skipped_steps = _ls_get(ops.LS_SKIPPED, "_skipped_steps", int)
    opt_step = _ls_get(ops.LS_APPLIED, "_opt_step", int)
    del _ls_get

    def _fb_scale(self):
        """forward_backward's loss_scale: the host number, or the device state"""
        return self._loss_scale if self._dls is None else self._dls.state

    def _finish_stats(self):
        if self._stats_work is not None:      # mirrored-variable MEAN aggregation of the BN moving statistics [TF-3p]
            self._stats_work.wait()
            self._stats_work = None
            self.model.trained_moving_stats_flat().div_(self.world)

    def _update(self, pl, lr):
        """Finite check (fp16 loss scaling), clip, optimizer, EMA on the all-reduced gradient in `flat_grads`."""
        m = self.model
        if self._dls is not None:
            return self._update_on_device(pl, lr)
        if self.dynamic_scale:                # after the all-reduce: every replica sees the same sums, takes the same branch
            if not m.grads_finite():
                self.loss_scale = max(self.loss_scale / 2.0, 1.0)
                self._good_steps = 0
                self.skipped_steps += 1
                return pl                     # LossScaleOptimizer skips the update
            self._good_steps += 1
        self.opt_step += 1
        grad_scale = 1.0 / self.loss_scale
        extras = {}
        if self._clip:
            # the norm stays on the device: the _ex launch derives the clip coefficient from it, and skips itself (weights,
            # slots and EMA untouched) when the gradient holds an inf / nan.  `opt_step` has counted such a step all the
            # same -- the host never learns of it -- so after one Adam's bias correction runs one step ahead.
            norm = m.grad_norm_sq()
            self.last_grad_norm = norm[0].sqrt() * grad_scale
            extras.update(norm=norm, max_norm=self.solver.clip_grad_l2norm)
        self._apply_rule(lr, grad_scale, self.opt_step, extras)
        if self.dynamic_scale and self._good_steps >= self.growth_steps:
            self.loss_scale *= 2.0
            self._good_steps = 0
        return pl

    def _apply_rule(self, lr, grad_scale, step, extras):
        """The optimizer launch and the EMA of the moving statistics behind it.  extras: norm + max_norm of the clip / skip
        channel, if any; `step`: the bias-correction step of the rules that have one."""
        m = self.model
        if self.ema is not None:
            extras.update(ema=self.ema, ema_decay=self.solver.ema_decay)
        # the rule's scalars (solver.RULES): the trainer's own state for those it has, OPTIM.* for those the record maps there
        mine = dict(momentum=self.momentum, step=step)
        kw = {k: mine[k] for k in self.rule.scalars if k in mine}
        kw.update({k: getattr(self.optim, field) for k, field in self.rule.settings.items()})
        q = getattr(m, "apply_" + self.optimizer)(lr, grad_scale=grad_scale, **kw, **extras)
        if self.rule.trust:                   # of the all-reduced, accumulated gradient: the same on every rank
            self.last_trust_ratios = q
        if self.ema is not None:              # the moving statistics behind the trainable block: skipped together with the step
            ops.ema_update(self.ema[m.n_trainable_flat:], m.moving_stats_flat(), self.solver.ema_decay, extras.get("norm"))

    def _update_on_device(self, pl, lr):
        """`_update` with SOLVER.DEVICE_LOSS_SCALE: launches only, in stream order --
          1. x3d_unscale_sumsq (set_finetune: x3d_seg_unscale_sumsq) divides the scale out of `flat_grads`, which from here on
             holds the UNSCALED gradient, and leaves its norm block: squared norm, number of non-finite entries;
          2. the rule's launch with grad_scale = 1 and norm = that block -- the skip channel of the clipping launches decides on
             the device; without CLIP_GRAD_L2NORM max_norm is NO_CLIP, which no gradient reaches;
          3. the EMA of the moving statistics, skipped through the same block;
          4. x3d_loss_scale_update halves or grows the scale and counts the step, and the state is published to the host.
        The host waits, at most, for the copy the PREVIOUS step published: the rules with a bias correction take their step
        from it, applied steps so far + 1, so a skipped step does not advance the correction."""
        ds = self._dls
        norm = self.model.unscale_norm_sq(ds.state)
        self.last_grad_norm = norm[0].sqrt()
        step = int(ds.previous()[ops.LS_APPLIED]) + 1 if "step" in self.rule.scalars else 0
        self._apply_rule(lr, 1.0, step, dict(norm=norm, max_norm=self.solver.clip_grad_l2norm if self._clip else NO_CLIP))
        ops.loss_scale_update(ds.state, norm, self.growth_steps)
        ds.publish()
        return pl

    def _accum_step(self, clips, labels, lr, n, sw):
        """One micro-batch of SOLVER.ACCUM_STEPS = A > 1.  Micro-batches 1..A-1 add their local gradient to the accumulator
        (no gradient all-reduce; weights, slots, EMA and `opt_step` untouched; the moving statistics are averaged as always).
        Micro-batch A adds the accumulator back -- under data parallelism bucket by bucket in the backward hook, in front of
        that bucket's all-reduce, so the exchange still hides behind the backward pass -- and updates on the total, which
        `flat_grads` then holds.  The loss scale changes with an update only, so it is one value within an accumulation."""
        m = self.model
        self._micro += 1
        last = self._micro == self._accum
        if self._grad_acc is None:
            self._grad_acc = torch.zeros_like(m.flat_grads)
        hook = (self._on_stage_done if last else self._on_stage_done_no_grads) if self.collectives else None
        pl = m.forward_backward(clips, labels, global_batch=n * self.world * self._accum, on_stage_done=hook,
                                loss_scale=self._fb_scale(), **self._teacher_kw(clips), **sw)
        if not last:
            ops.grad_accum(self._grad_acc, m.flat_grads, first=self._micro == 1)
            self._finish_stats()
            return pl
        self._micro = 0
        if not self.collectives:
            ops.grad_accum(m.flat_grads, self._grad_acc)
        self.reducer.mark_backward_done()
        self.reducer.finish()
        self._finish_stats()
        return self._update(pl, lr)

    def _mix_batch(self, clips, labels):
        """Soft-target training: draws this batch's MixParams, mixes the clips with the reversed batch (x3d_mix_clips) and
        builds the soft targets in the plan's `targets` (x3d_mix_targets).  Returns what `forward_backward` gets.  The
        caller's tensors are never written: the clips are mixed in place only where bringing them to the device and the
        storage type -- which binding them would do anyway -- made a copy, else into a buffer the trainer keeps.  With
        smoothing only (mode "none") the clips are passed through and lam = 1.  Single-label models: `plan.labels` receives
        the hard labels the training metrics count against.  Launches only, no host synchronisation."""
        m = self.model
        n, t, h, w, _ = clips.shape
        p = draw_mix_params(self.cfg, h, w, self._mix_rng)
        self.last_mix = p
        pl = m._plan(n, t, h, w, True)
        if p.mode != "none":
            x = clips
            if not x.is_cuda:
                x = x.to(m.device, non_blocking=True)
            if not x.is_contiguous():
                x = x.contiguous()
            if x.dtype != m.dtype:
                x = x.to(m.dtype)
            if x is clips or x.data_ptr() == clips.data_ptr():
                if self._mix_buf is None or self._mix_buf.shape != x.shape or self._mix_buf.dtype != x.dtype:
                    self._mix_buf = torch.empty_like(x)
                out = self._mix_buf
            else:
                out = x
            clips = ops.mix_clips(x, p.mode, p.lam, (p.y0, p.y1, p.x0, p.x1), out=out)
        if m.multi_label:
            m._bind_targets(pl, labels, n)
            if p.mode != "none":
                ops.mix_targets(pl.targets, m.num_classes, p.lam, out=pl.targets)
        else:
            if not torch.is_tensor(labels):
                labels = torch.as_tensor(labels)
            if labels.dim() != 1:
                raise ValueError(f"labels must be {n} class indices when MIXUP / LABEL_SMOOTHING build the targets, got "
                                 f"{tuple(labels.shape)}")
            if not labels.is_cuda:   # as forward_backward: host labels are validated for free, device labels by the kernel
                if labels.numel() != n or int(labels.min()) < 0 or int(labels.max()) >= m.num_classes:
                    raise ValueError(f"labels must be {n} class indices in [0, {m.num_classes})")
            if self._mix_labels is None or self._mix_labels.numel() != n:
                self._mix_labels = torch.zeros(n, dtype=torch.int32, device=m.device)
            self._mix_labels.copy_(labels.to(m.device, non_blocking=True).to(torch.int32))
            pl.use_soft_targets(True)
            ops.mix_targets(self._mix_labels, m.num_classes, p.lam, self.mix.label_smoothing, out=pl.targets, hard=pl.labels)
        return clips, pl.targets

    def fit(self, dataset, epochs: Optional[int] = None, steps_per_epoch: Optional[int] = None, model_dir: Optional[str] = None,
            initial_epoch: Optional[int] = None, on_step=None, validation_data=None, validation_steps: Optional[int] = None,
            metrics=_DEFAULT_METRICS, save_freq="epoch", precise_bn_data=None):
        """The loop `model.fit(dataset, epochs, steps_per_epoch, initial_epoch, validation_data, callbacks)` runs in reference
        train.py:145-152, with the metrics it was compiled with (train.py:102-108), its LearningRateScheduler (per-epoch
        `lr_schedule`, train.py:114-125) and ModelCheckpoint (utils.py:128-132) callbacks -- nothing else of the Keras harness
        (TensorBoard / wandb callbacks are out of scope).  `dataset`: an iterator of (clips, labels) batches, e.g.
        `dataloader.InputReader(cfg, True, True)(pattern, cfg.TRAIN.BATCH_SIZE)`, or of (clips, labels, sample_weight)
        batches as Keras' `model.fit` takes them (`step`; infinite in training mode, like
        `dataset.repeat()`; under torchrun the reader shards the records by rank and yields BATCH_SIZE // world clips per
        step, so `steps_per_epoch` = DATASET_SIZE // BATCH_SIZE is one pass over the data on every world size, as with
        MirroredStrategy).  Returns the per-epoch mean losses.

        validation_data: None, a zero-argument callable returning a fresh iterable of (clips [B * views * crops, T, S, S, 3],
            labels [B]) -- e.g. `lambda: InputReader(cfg, False, True)(val_pattern, cfg.TEST.BATCH_SIZE)` -- or an iterable
            `iter()` can walk again every epoch.  After every epoch `model(clips, training=False)` runs over the whole stream
            (or its first `validation_steps` batches) into `evaluate.DeviceMetrics`; under data parallelism every rank
            validates its shard and the counters are summed once.  The training plan stays cached across it.
        metrics: any of "acc", "top_5_acc": the hits of the training batches' probabilities, one x3d_topk_metrics launch
            after every step (skipped fp16 steps too, as Keras updates compiled metrics), read once per epoch.
            "mean_class_acc" (single-label models, never a default): the mean over the classes that occurred of the per-class
            top-1 accuracy -- one x3d_class_hits launch more per step, and `val_mean_class_acc` when validating.  Validation
            metrics and `val_loss` are unweighted, as in Keras.
        save_freq: "epoch" or a positive int (`SaveSchedule`); rank 0 writes the checkpoints into `model_dir`.

        Multi-label models (DATA.MULTI_LABEL): batches are (clips, targets [B, classes]); `metrics` defaults to ("mAP",) --
            the mean average precision of the epoch's training probabilities (evaluate.DeviceMAP), "acc" / "top_5_acc" are
            refused -- and validation fills `val_loss` / `val_mAP`.

        self.history: per-epoch lists like keras.callbacks.History.history -- `loss` (= the returned list), `lr`, the
        requested `metrics`, and `val_loss` / `val_acc` / `val_top_5_acc` when validating; `val_frame_mAP` when the validation
        batches of a detection model have seven items (`validate`), created at the first validation that returns it.

        DISTILL.ENABLE: `history["kd_loss"]` is the epoch mean of the unweighted KD term (`kd_loss`); `loss` stays the combined
        loss (+ L2).

        SOLVER.DEVICE_LOSS_SCALE (dynamic fp16 loss scaling on the device): no step reads the scaler; `history["loss_scale"]` is the
        scale at the end of the epoch and `history["skipped_steps"]` the epoch's skipped updates, from one read of the device
        state per epoch; `grad_norm` is summed on the device over the applied updates only.

        SOLVER.* (INTEGRATION.md): with CLIP_GRAD_L2NORM `history["grad_norm"]` is the epoch's mean gradient norm before
        clipping; with ACCUM_STEPS = A every batch is a micro-batch, steps_per_epoch and an integer save_freq must be multiples
        of A (ValueError); with EMA_DECAY and EMA_EVAL validation runs on the EMA weights (`ema_scope`).

        NETWORK.BN.USE_PRECISE_STATS: after an epoch's training steps, before its validation and its end-of-epoch checkpoint,
        `precise_bn` recomputes the moving statistics of the raw weights from NUM_BATCHES_PRECISE batches and, with
        EMA_DECAY, those of the EMA weights (inside `ema_scope`) from the NEXT NUM_BATCHES_PRECISE batches of the same source.
        precise_bn_data: None -- the batches are drawn from `dataset`, which then has to yield steps + NUM_BATCHES_PRECISE
            (with EMA: + 2 * NUM_BATCHES_PRECISE) batches per epoch -- or a zero-argument callable returning a fresh iterable,
            called once per epoch.  Mixup / CutMix are not applied to these batches (PySlowFast's precise-BN loop does not
            either).  A checkpoint an integer save_freq writes in the middle of an epoch carries whatever statistics exist
            at that moment: the momentum blend of the steps since the last recomputation."""
        from .evaluate import DeviceMAP, DeviceMetrics
        tr = self.cfg.TRAIN
        epochs = int(tr.EPOCHS if epochs is None else epochs)
        steps = int(steps_per_epoch if steps_per_epoch is not None else tr.DATASET_SIZE // tr.BATCH_SIZE)
        if steps <= 0:
            raise ValueError("steps_per_epoch must be positive (cfg.TRAIN.DATASET_SIZE // cfg.TRAIN.BATCH_SIZE)")
        check_accum_schedule(steps, save_freq, self.solver.accum_steps)
        multi = bool(getattr(self.model, "multi_label", False))
        det = getattr(self.model, "det", None) is not None
        known = MULTI_LABEL_METRICS if multi else TRAIN_METRICS
        if metrics is _DEFAULT_METRICS:
            metrics = known
        metrics = tuple(metrics or ())
        unknown = [k for k in metrics if k not in known + (() if multi else OPT_IN_METRICS)]
        if unknown:
            kind = "a multi-label model" if multi else "fit"
            raise ValueError(f"unknown metrics {unknown}: {kind} computes {known}")
        per_class = "mean_class_acc" in metrics
        val_keys = ("loss",) + known + (("mean_class_acc",) if per_class else ())
        schedule = SaveSchedule(save_freq)
        if initial_epoch is not None:
            self.epoch = int(initial_epoch)
        val_source = _validation_source(validation_data, epochs - self.epoch)
        if precise_bn_data is not None and not callable(precise_bn_data):
            raise ValueError("precise_bn_data must be None or a zero-argument callable returning a fresh iterable of batches")
        it = iter(dataset)
        history = []
        self.history = {"loss": [], "lr": []}
        self.history.update({k: [] for k in metrics})
        if self._clip:
            self.history["grad_norm"] = []
        ds = self._dls
        if ds is not None:                    # device loss scaling: the scale at epoch end and the epoch's skipped steps
            self.history.update(loss_scale=[], skipped_steps=[])
            seen = list(ds.read())            # (no synchronisation unless a step has run since the last read)
        if self.teacher is not None:
            self.history["kd_loss"] = []
        if val_source is not None:
            self.history.update({"val_" + k: [] for k in val_keys})
        writer = model_dir is not None and xdist.env_world()[0] == 0
        while self.epoch < epochs:
            lr = lr_schedule(self.epoch, self.cfg)
            tot = torch.zeros((), dtype=torch.float64, device=self.model.device)
            train_m = (DeviceMAP() if multi else DeviceMetrics(**(dict(per_class=True) if per_class else {}))) if metrics else None
            gn_tot, updates = (torch.zeros((), dtype=torch.float64, device=self.model.device) if self._clip else None), 0
            kd_tot = torch.zeros((), dtype=torch.float64, device=self.model.device) if self.teacher is not None else None
            for _ in range(steps):
                clips, labels, *weights = next(it)
                before = self.opt_step if ds is None else None
                if det:                       # (clips, labels, boxes, num_boxes)
                    pl = self.step(clips, labels, lr, **dict(zip(("boxes", "num_boxes"), weights)))
                else:
                    pl = self.step(clips, labels, lr, *weights)
                tot += self.loss(pl).double()
                if kd_tot is not None:
                    kd_tot += self.kd_loss(pl).double()
                if gn_tot is not None and ds is not None:
                    if self._micro == 0:      # an update was launched: it adds its norm unless the device skipped it
                        gn_tot += self.last_grad_norm * (1.0 - ds.state[ops.LS_LAST_SKIPPED])
                elif gn_tot is not None and self.opt_step != before:   # an update ran (not inside an accumulation / fp16 skip)
                    gn_tot += self.last_grad_norm
                    updates += 1
                if train_m is not None:
                    train_m.update(*self._valid_rows(pl, pl.probs, pl.targets if multi else pl.labels))
                if on_step is not None:
                    on_step(self, pl)
                ckpt = schedule.after_batch(self.epoch)
                if ckpt is not None and writer:
                    self.save_checkpoint(model_dir, ckpt)
            ckpt = schedule.after_epoch(self.epoch)
            self.epoch += 1
            history.append(float(tot.item()) / steps)
            self.history["loss"].append(history[-1])
            self.history["lr"].append(lr)
            if kd_tot is not None:            # the epoch mean of the unweighted KD term; read once per epoch, like the loss
                self.history["kd_loss"].append(float(kd_tot.item()) / steps)
            if ds is not None:                # the one read of the scaler state per epoch
                now = ds.read()
                updates = int(now[ops.LS_APPLIED] - seen[ops.LS_APPLIED])
                self.history["loss_scale"].append(now[ops.LS_SCALE])
                self.history["skipped_steps"].append(int(now[ops.LS_SKIPPED] - seen[ops.LS_SKIPPED]))
                seen = list(now)
            if gn_tot is not None:            # mean over the epoch's updates; read once per epoch, like the loss
                self.history["grad_norm"].append(float(gn_tot.item()) / max(updates, 1))
            if train_m is not None:
                r = train_m.all_reduce_(self.group).result()
                for k in metrics:
                    self.history[k].append(r[k])
            if self.precise.enable:
                if precise_bn_data is None:
                    self._fit_precise_bn(it, close=False)          # the training iterator goes on into the next epoch
                else:
                    self._fit_precise_bn(iter(precise_bn_data()), close=True)
            if val_source is not None:
                with (self.ema_scope() if self.ema is not None and self.solver.ema_eval else contextlib.nullcontext()):
                    r = self.validate(val_source(), validation_steps, **(dict(per_class=True) if per_class else {}))
                for k in val_keys:
                    self.history["val_" + k].append(r[k])
                if "frame_mAP" in r:          # seven-item detection batches (validate): created at the first validation that has it
                    self.history.setdefault("val_frame_mAP", []).append(r["frame_mAP"])
            if ckpt is not None and writer:
                self.save_checkpoint(model_dir, ckpt)
        return history

    def precise_bn(self, batches, num_batches: Optional[int] = None) -> int:
        """precise_bn.update_bn_stats on this replica's model and process group: the moving statistics of the weights in
        `flat_params` recomputed exactly from the first `num_batches` (default NETWORK.BN.NUM_BATCHES_PRECISE) items of
        `batches`, pooled over the ranks; returns the batches used.  Inside `ema_scope()` the model is the EMA model, so this
        computes the EMA weights' statistics, and the swap on exit carries them into `self.ema`."""
        from .precise_bn import update_bn_stats
        return update_bn_stats(self.model, batches, self.precise.num_batches if num_batches is None else num_batches,
                               group=self.group)

    def _fit_precise_bn(self, src, close: bool):
        """`fit`, end of an epoch: the raw weights' statistics, then the EMA weights' from the batches that follow in the
        iterator `src`; close: `src` is a fresh reader of this epoch's own (precise_bn_data)"""
        try:
            self.precise_bn(src)
            if self.ema is not None:
                with self.ema_scope():
                    self.precise_bn(src)
        finally:
            if close and getattr(src, "close", None) is not None:
                src.close()   # a reader's generator: stops its prefetch thread

    def validate(self, batches, steps: Optional[int] = None, per_class: bool = False, iou_threshold: float = 0.5):
        """`model.evaluate` inside `fit` (reference train.py:148-151): `model(clips, training=False)` over `batches` (the
        first `steps` of them when given) into a DeviceMetrics, counters summed over the ranks once.  Unlike
        `evaluate_dataset` this releases no plan, so the training plan is still cached in the next epoch.  Returns
        {"loss", "acc", "top_5_acc", "videos"}; for a multi-label model the DeviceMAP result {"loss", "mAP", "videos",
        "classes"} (batches of (clips, targets)).  DETECTION.ENABLE: batches of (clips, labels [B, K] | targets [B, K, classes],
        boxes, num_boxes); loss and metrics are taken over the filled box slots only, "videos" counts them.  per_class (single-label models): + "mean_class_acc".  The loss is
        unweighted: LOSS.* and sample weights act on the training loss only.

        Frame-mAP (DETECTION.ENABLE): batches of seven items (clips, labels, boxes, num_boxes, gt_boxes [B, G, 4], gt_labels
        [B, G, classes], num_gt [B]) -- `boxes` are then the proposals the ROI head pools, e.g. a person detector's -- also feed an
        `evaluate.DeviceFrameMAP(iou_threshold)` (one x3d_frame_match launch per batch behind the forward pass), and the result
        gains "frame_mAP", "frame_classes", "detections" and "gt_boxes".  `labels` may be None in such a batch (proposals have
        no labels of their own): "loss" and the row-wise metric are then NaN.  Every batch of the set has seven items or every
        one four, and `labels` is None in every batch or in none: a mixture of either kind is a ValueError.  Four-item sets
        return exactly the keys above.  Under data parallelism the ranks' sets are of one form (all labelled or all unlabelled:
        an unlabelled rank skips the exchange of the row-wise metric) and of equal size (`DeviceFrameMAP.all_reduce_`), as the
        reader's shards are."""
        import itertools
        from .evaluate import DeviceFrameMAP, DeviceMAP, DeviceMetrics
        m = self.model
        if getattr(m, "multi_label", False):
            dm = DeviceMAP(m.regularization_loss())
        else:
            dm = DeviceMetrics(m.regularization_loss(), **(dict(per_class=True) if per_class else {}))
        fm = None                     # the frame-mAP of seven-item batches, next to dm
        forms, labelled = set(), set()          # the batch lengths seen; whether labels were given (True) or None (False)
        it = iter(batches)
        try:
            for clips, labels, *box_args in itertools.islice(it, None if steps is None else int(steps)):
                if getattr(m, "det", None) is not None or box_args:      # (clips, labels, boxes, num_boxes): the valid rows only
                    forms.add(2 + len(box_args))
                    if len(forms) > 1 or (len(box_args) > 2 and len(box_args) != 5):
                        raise ValueError("validate: every detection batch must have four items (clips, labels, boxes, num_boxes) "
                                         "or every one seven (+ gt_boxes, gt_labels, num_gt); got batches of "
                                         f"{sorted(forms)} items")
                    labelled.add(labels is not None)
                    if len(labelled) > 1:
                        raise ValueError("validate: labels must be None in every batch of the set or in none")
                    if labels is None and len(box_args) != 5:
                        raise ValueError("validate: labels may be None only in a seven-item batch")
                    probs = m(clips, training=False, **dict(zip(("boxes", "num_boxes"), box_args)))
                    pl = m._plan(*clips.shape[:4], False)
                    probs = probs.reshape(pl.rows, -1)
                    if len(box_args) == 5:
                        if fm is None:
                            fm = DeviceFrameMAP(iou_threshold)
                        fm.update(probs, *box_args)
                    if labels is None:                # detector proposals carry no labels of their own: the frame keys only
                        continue
                    labels = torch.as_tensor(labels)
                    dm.update(*self._valid_rows(pl, probs, labels.reshape((pl.rows,) + tuple(labels.shape[2:]))))
                else:
                    dm.update(m(clips, training=False), labels)
        finally:
            close = getattr(it, "close", None)
            if close is not None:
                close()       # a reader's generator: stops its prefetch thread
        if False in labelled:         # no row-wise metric without labels: the keys stay, NaN and zero rows (no exchange: every
            r = {k: (0 if k in ("videos", "classes") else float("nan")) for k in dm.result()}    # rank's set is unlabelled, below)
        else:
            r = dm.all_reduce_(self.group).result()
        if fm is not None:
            f = fm.all_reduce_(self.group).result()
            r.update(frame_mAP=f["frame_mAP"], frame_classes=f["classes"], detections=f["detections"], gt_boxes=f["gt_boxes"])
        return r

    @staticmethod
    def _valid_rows(pl, probs, labels):
        """(probs, labels) of a plan's filled box slots (DETECTION.ENABLE; the index comes from the host-side num_boxes: a device
        gather, no read) -- both as they are for a clip-level plan"""
        if getattr(pl, "det", None) is None:
            return probs, labels
        idx = pl._box_keepalive.nonzero().flatten()
        return (probs.index_select(0, idx.to(probs.device, non_blocking=True)),
                labels.index_select(0, idx.to(labels.device, non_blocking=True)))

    def collective_stats(self):
        """What the exchange step of this replica did so far (bench.py's `collectives` block)."""
        r = self.reducer
        return {"backend": (torch.distributed.get_backend(self.group) if torch.distributed.is_initialized() else None),
                "world": self.world, "buckets_per_step": len(r.buckets),
                "bytes_per_step": sum(b.numel() * b.element_size() for b in r.buckets),
                "allreduces_launched": r.launched, "allreduce_bytes": r.launched_bytes,
                "launched_from_backward_hooks": bool(self.collectives and r.launched > 0),
                "moving_stats_mean": bool(self.sync_moving_stats),
                # time between the end of the backward pass and the last bucket landing, averaged over the steps since the
                # last call (0 = fully hidden; None = single rank); "device" = HIP events on the compute stream (RCCL)
                "exposed_ms": r.exposed_ms(),
                "exposed_clock": ("device" if (r.active and r._device_events()) else ("host" if r.active else None))}

    def _on_stage_done(self, stage):
        """backward hook (model.forward_backward): 'fwd' = forward finished (the moving statistics are final: their
        all-reduce overlaps the whole backward pass), else a stage whose gradients are final."""
        if stage == "fwd":
            if self.sync_moving_stats:
                # (with SOLVER.FREEZE_EVAL: not the frozen prefix's, which no step writes)
                self._stats_work = torch.distributed.all_reduce(self.model.trained_moving_stats_flat(), group=self.group,
                                                                async_op=True)
            return
        i = self._launch_at.get(stage)
        if i is not None:
            if self._accum > 1:               # the last micro-batch of an accumulation: the earlier ones join their bucket first
                b = self.reducer.buckets[i]
                lo = b.storage_offset() - self.model.flat_grads.storage_offset()
                ops.grad_accum(b, self._grad_acc[lo:lo + b.numel()])
            self.reducer.launch(i)

    def _on_stage_done_no_grads(self, stage):
        """backward hook of the micro-batches inside an accumulation: the moving statistics only, no gradient all-reduce"""
        if stage == "fwd":
            self._on_stage_done(stage)

    @contextlib.contextmanager
    def ema_scope(self):
        """Within the scope the model IS the EMA model: the contents of `flat_params` and `self.ema` are swapped (every
        plan holds addresses into `flat_params`, so the values move, not the buffers) and swapped back on exit, bit for bit.
        Nothing the inference path derives from the weights outlives a call -- the bf16 / fp16 weight panels are repacked
        and the BatchNorm coefficients recomputed at the head of every forward -- so the swap has nothing to invalidate."""
        if self.ema is None:
            raise ValueError("ema_scope needs SOLVER.EMA_DECAY > 0")
        p = self.model.flat_params

        if getattr(self, "_ema_swap", None) is None:
            self._ema_swap = torch.empty_like(p)      # kept: a scope is entered for every validation and every checkpoint

        def swap():
            self._ema_swap.copy_(p)
            p.copy_(self.ema)
            self.ema.copy_(self._ema_swap)
        swap()
        try:
            yield self
        finally:
            swap()

    # -- checkpoints in the reference's layout (utils.py:128-132 ModelCheckpoint 'ckpt-{epoch:d}', train.py:131-136) --
    def save_checkpoint(self, model_dir: str, epoch: int) -> str:
        """Writes `<model_dir>/ckpt-<epoch>` as a TF tensor bundle -- weights, the optimizer's slot variables (SGD:
        `momentum`; Adam: `m` and `v`), its hyper-parameter variables (`iter`, `learning_rate`, `decay` + `momentum` |
        `beta_1`, `beta_2`) and the `_CHECKPOINTABLE_OBJECT_GRAPH` Keras' `load_weights` restores by -- and the
        `checkpoint` state file, so that the reference's `tf.train.latest_checkpoint(model_dir)` finds it (ModelCheckpoint
        saves the whole optimizer, utils.py:128-132)."""
        import os
        os.makedirs(model_dir, exist_ok=True)
        prefix = os.path.join(model_dir, f"ckpt-{int(epoch)}")
        hyper = dict(iter=self.opt_step, learning_rate=lr_schedule(self.epoch, self.cfg), decay=0.0)
        if self.slot_kind == "adam":
            hyper.update(beta_1=0.9, beta_2=0.999)
        else:
            hyper.update(momentum=self.momentum)
        self.model.save_weights(prefix, optimizer_hyper=hyper, optimizer=self.slot_kind)
        if self.ema is not None:
            # the EMA model as a bundle of its own, in its own directory: `<model_dir>/checkpoint` still names ckpt-<epoch>,
            # and model.load_weights("<model_dir>/ema") loads the EMA weights for evaluation
            os.makedirs(os.path.join(model_dir, "ema"), exist_ok=True)
            with self.ema_scope():
                self.model.save_weights(os.path.join(model_dir, "ema", f"ckpt-{int(epoch)}"), optimizer_hyper=hyper,
                                        optimizer=self.slot_kind)
        return prefix

    def resume(self, model_dir: str, pretrained_ckpt: Optional[str] = None, skip_mismatch: bool = False) -> int:
        """train.py:131-143: load the latest `ckpt-<epoch>` of `model_dir` if there is one; returns the epoch to
        continue from (0 without a checkpoint) and sets `self.epoch`.  Without one, `pretrained_ckpt` (the reference's
        --pretrained_ckpt) is loaded when given -- a directory through its latest checkpoint (FileNotFoundError when it
        holds none), anything else as a checkpoint prefix -- with the same optimizer-slot and `iter` rules, and training
        starts at epoch 0.  skip_mismatch applies to `pretrained_ckpt` only: its variables whose shapes differ from the
        model's (a Kinetics-400 fc2 in a 157-class model) are not loaded (model.load_weights(skip_mismatch=True)); the
        names skipped are in `self.skipped_keys`."""
        import os
        from .checkpoint import latest_checkpoint
        path = latest_checkpoint(model_dir)
        if not path and pretrained_ckpt is not None:
            pre = str(pretrained_ckpt)
            if os.path.isdir(pre):
                found = latest_checkpoint(pre)
                if not found:
                    raise FileNotFoundError(f"pretrained_ckpt {pre}: the directory holds no checkpoint")
                pre = found
            self._load(pre, skip_mismatch=skip_mismatch)
            self.epoch = 0
            return 0
        if not path:
            return 0
        self._load(path)
        self.epoch = int(os.path.basename(path).split("-")[1])
        if hasattr(self.model, "set_drop_path_state"):
            # the stochastic-depth step counts forward_backward calls: ACCUM_STEPS per optimizer update (`iter`), so a resumed
            # run goes on with new tables instead of replaying those of step 0
            self.model.set_drop_path_state(self._drop_path_seed, self.opt_step * self._accum)
        if self.ema is not None:              # the EMA of that epoch (save_checkpoint: <model_dir>/ema/ckpt-<epoch>), if there
            ema_prefix = os.path.join(model_dir, "ema", os.path.basename(path))
            if os.path.exists(ema_prefix + ".index"):
                from .checkpoint import read_checkpoint
                sd = read_checkpoint(ema_prefix, self.model.specs)
                with self.ema_scope():
                    self.model.load_state_dict(sd)
        return self.epoch

    def _load(self, path: str, skip_mismatch: bool = False):
        """Weights + this optimizer branch's slots from the checkpoint prefix `path`; sets `opt_step` from its `iter`."""
        m = self.model
        if skip_mismatch:
            self.skipped_keys = m.load_weights(path, optimizer=self.slot_kind, skip_mismatch=True)
        else:
            m.load_weights(path, optimizer=self.slot_kind)   # weights + this branch's optimizer slots; unknown keys tolerated as Keras does
        st = getattr(m, "optimizer_state", None) or {}
        kind = st.get("kind")
        if kind is not None and kind != self.slot_kind:
            # a checkpoint written by the other optimizer branch: Keras restores the variables and leaves the new
            # optimizer's slots at their initial value -- never reuse SGD momentum as Adam's first moment or vice versa
            m.zero_slots()
            self.opt_step = 0
        else:
            # optimizer/iter: Adam's bias correction continues from the saved step count
            self.opt_step = int(st.get("hyper", {}).get("iter", 0))
            if self.slot_kind == "adam" and kind is None:
                m.zero_slots()
                self.opt_step = 0
        if self.ema is not None:              # restart the EMA from the loaded weights (resume replaces it by a saved one)
            self.ema.copy_(m.flat_params)

    def loss(self, pl):
        """global-batch mean cross-entropy + L2 term (what Keras reports as `loss`).  adamw / lamb decay the weights outside
        the loss (OPTIM.WEIGHT_DECAY) and ignore NETWORK.WEIGHT_DECAY: for them this is the cross-entropy alone."""
        ce = pl.loss_rows.sum() / (pl.rows * self.world)      # (DETECTION.ENABLE: rows = n * K, weighted to the mean over valid boxes)
        if self.collectives:
            torch.distributed.all_reduce(ce, group=self.group)
        if not self.rule.l2_in_loss:
            return ce
        return ce + self.model.regularization_loss().float().squeeze()

    def kd_loss(self, pl):
        """global-batch mean of the unweighted distillation term T^2 * KL(teacher || student) of the last distilled step
        (`plan.kd_rows`), reduced as `loss` is"""
        kd = pl.kd_rows.sum() / (pl.n * self.world)
        if self.collectives:
            torch.distributed.all_reduce(kd, group=self.group)
        return kd
