"""Configuration tree for ``X3D(cfg)``.

The reference drives the model with a yacs ``CfgNode`` (reference configs/default.py:1-141,
merged with configs/kinetics/X3D_*.yaml at train.py:39-41).  yacs is not available here, so this
is a small attribute-access node with the same surface the hot path uses:
``get_default_config()``, ``.merge_from_file(path)``, ``.freeze()``, ``.clone()``, attribute and
item access, ``dict(cfg)``.
"""
import ast
import collections
import copy
import os
import re

import yaml

from .solver import RULES

_CONFIG_DIR = os.path.join(os.path.dirname(os.path.abspath(__file__)), "configs")


class CfgNode(dict):
    """Attribute-access dict with freeze, in the shape of yacs.config.CfgNode.

    optional: {key: default} of keys the section KNOWS but does not hold until a config file or an override sets them.  Reading
    one as an attribute gives its default, merging one is allowed (and type-checked against the default), and the section's
    items -- what `dict(node)`, iteration and a saved config show -- are what they were without them."""

    _FROZEN = "__frozen__"
    _OPTIONAL = "__optional__"

    def __init__(self, init=None, optional=None):
        super().__init__()
        object.__setattr__(self, CfgNode._FROZEN, False)
        object.__setattr__(self, CfgNode._OPTIONAL, copy.deepcopy(dict(optional or {})))
        for k, v in (init or {}).items():
            self[k] = CfgNode(v) if isinstance(v, dict) and not isinstance(v, CfgNode) else v

    def optional_keys(self):
        return object.__getattribute__(self, CfgNode._OPTIONAL)

    def __getattr__(self, name):
        try:
            return self[name]
        except KeyError:
            pass
        try:
            return copy.deepcopy(self.optional_keys()[name])
        except KeyError:
            raise AttributeError(name)

    def __setattr__(self, name, value):
        if self.is_frozen():
            raise AttributeError(f"attempted to set {name} on a frozen CfgNode")
        self[name] = value

    def __setitem__(self, key, value):
        if getattr(self, CfgNode._FROZEN, False):
            raise AttributeError(f"attempted to set {key} on a frozen CfgNode")
        super().__setitem__(key, value)

    def is_frozen(self):
        return object.__getattribute__(self, CfgNode._FROZEN)

    def _set_frozen(self, flag):
        object.__setattr__(self, CfgNode._FROZEN, flag)
        for v in self.values():
            if isinstance(v, CfgNode):
                v._set_frozen(flag)

    def freeze(self):
        self._set_frozen(True)

    def defrost(self):
        self._set_frozen(False)

    def clone(self):
        return copy.deepcopy(self)

    def __deepcopy__(self, memo):
        out = CfgNode(optional=self.optional_keys())
        for k, v in self.items():
            dict.__setitem__(out, k, copy.deepcopy(v, memo))
        return out

    @staticmethod
    def _decode(value):
        # yacs decodes string leaves with literal_eval, which is how "5e-5" / "1e-5"
        # (strings to a YAML-1.1 parser) become floats.
        if isinstance(value, str):
            try:
                return ast.literal_eval(value)
            except (ValueError, SyntaxError):
                return value
        return value

    def merge_from_dict(self, other, _path=""):
        for k, v in other.items():
            full = f"{_path}.{k}" if _path else k
            if k not in self and k not in self.optional_keys():
                raise KeyError(f"Non-existent config key: {full}")
            if isinstance(v, dict):
                if not isinstance(self[k], CfgNode):
                    raise ValueError(f"{full} is a leaf in the defaults but a section in the override")
                self[k].merge_from_dict(v, full)
            else:
                v = CfgNode._decode(v)
                old = self[k] if k in self else self.optional_keys()[k]
                if isinstance(old, float) and isinstance(v, int) and not isinstance(v, bool):
                    v = float(v)
                if isinstance(old, tuple) and isinstance(v, list):
                    v = tuple(v)
                if isinstance(old, list) and isinstance(v, tuple):
                    v = list(v)
                if old is not None and type(old) is not type(v):
                    raise ValueError(
                        f"Type mismatch ({type(old)} vs. {type(v)}) for config key: {full}")
                self[k] = v

    def merge_from_file(self, path):
        with open(path, "r") as f:
            self.merge_from_dict(yaml.safe_load(f) or {})

    def merge_from_list(self, kv):
        assert len(kv) % 2 == 0
        for key, val in zip(kv[0::2], kv[1::2]):
            node = self
            parts = key.split(".")
            for p in parts[:-1]:
                node = node[p]
            node.merge_from_dict({parts[-1]: val})


def get_default_config():
    """Defaults with the keys and values of reference configs/default.py:3-140, plus DATA.MULTI_LABEL and
    TEST.ENSEMBLE_METHOD (multi-label training), MIXUP.* and TRAIN.LABEL_SMOOTHING (soft-target training),
    AUG.* (batched training augmentation, AUG.AA_TYPE: RandAugment), SOLVER.* (gradient clipping, accumulation, weight EMA;
    LAYER_DECAY / LR_MULT / FREEZE / FREEZE_EVAL / FREEZE_BN: fine-tuning),
    NETWORK.DROP_PATH_RATE (stochastic depth), NETWORK.RES5_DILATION (dilated stride-1 res5 for detection), OPTIM.* (LARS / AdamW / LAMB: TRAIN.OPTIMIZER = lars | adamw | lamb),
    NETWORK.BN.USE_PRECISE_STATS / NUM_BATCHES_PRECISE (precise BatchNorm statistics before validation and save),
    DISTILL.* (knowledge distillation against a teacher's logits), LOSS.* (class / positive weights and focal terms),
    DETECTION.* (the ROI head for action detection), AVA.* (the frame-list dataset of ava.AvaReader)."""
    c = CfgNode()
    c.NETWORK = CfgNode(dict(
        C1_TEMP_FILTER=5, C1_CHANNELS=12, SCALE_RES2=False, WIDTH_FACTOR=1.0, DEPTH_FACTOR=1.0,
        BOTTLENECK_WIDTH_FACTOR=1.0, NUM_CLASSES=400, DROPOUT_RATE=0.0, WEIGHT_DECAY=0.00005,
        # stochastic depth (PySlowFast's DROPCONNECT_RATE): the chance that the bottleneck branch of the LAST residual block is
        # dropped for a sample of a training step; linear in depth from 0 at the first block (0 = off)
        DROP_PATH_RATE=0.0,
        # USE_PRECISE_STATS (PySlowFast's BN section): Trainer.fit recomputes every layer's moving statistics exactly, from
        # NUM_BATCHES_PRECISE training batches, after each epoch's steps -- before its validation and its checkpoint
        BN=dict(MOMENTUM=0.9, EPS=1e-5, USE_PRECISE_STATS=False, NUM_BATCHES_PRECISE=200)),
        # RES5_DILATION (res5_dilation_settings; 1 = off): 2 runs the last stage at stride 1 with its 3x3x3 convs dilated by 2 in
        # space -- PySlowFast's RESNET.SPATIAL_STRIDES [[1],[2],[2],[1]] / SPATIAL_DILATIONS [[1],[1],[1],[2]], the X3D detection
        # setup: conv5 at stride 16.  The weights keep their shapes.  Known without being held, as the SOLVER keys below
        optional=dict(RES5_DILATION=1))
    c.DATA = CfgNode(dict(
        FRAME_RATE=1, TEMP_DURATION=1, NUM_INPUT_CHANNELS=3, TRAIN_JITTER_SCALES=[182, 228],
        TRAIN_CROP_SIZE=112, TEST_CROP_SIZE=160, MEAN=[0.45, 0.45, 0.45],
        STD=[0.225, 0.225, 0.225],
        # multi-label (Charades-style) datasets: sigmoid / binary cross-entropy head, multi-hot targets, mAP
        MULTI_LABEL=False))
    c.TRAIN = CfgNode(dict(
        DATASET_SIZE=0, BATCH_SIZE=1, EPOCHS=1, OPTIMIZER="SGD", MOMENTUM=0.9, BASE_LR=0.1,
        WARMUP_EPOCHS=1, WARMUP_LR=0.01,
        # label smoothing of the softmax head: targets (1 - eps) * one_hot + eps / classes (0 = off)
        LABEL_SMOOTHING=0.0))
    # mixup / CutMix of a training batch with its own reverse (names as PySlowFast's MIXUP section): ALPHA / CUTMIX_ALPHA are the
    # Beta parameters of the two modes (0 = that mode off), PROB the chance a batch is mixed at all, SWITCH_PROB the chance of
    # CutMix when both modes are on
    c.MIXUP = CfgNode(dict(ENABLE=False, ALPHA=0.8, CUTMIX_ALPHA=1.0, PROB=1.0, SWITCH_PROB=0.5))
    # training augmentation built on the device in one batched call (aug.py, x3d_train_clips_aug; names after PySlowFast's AUG /
    # DATA sections); inert unless ENABLE.  CROP "jitter": the reference's short-side resize + random crop; "rrc": a
    # random-resized crop of RRC_SCALE area fraction and RRC_RATIO aspect.  FLIP_PROB 1.0 is the reference's mirror of every
    # clip.  BRIGHTNESS / CONTRAST / SATURATION: strengths v, factor 1 + U(-v, v), 0 = that op off; COLOR_PROB the chance a
    # clip gets the colour chain, GRAYSCALE_PROB that it is turned grey after it.  RE_*: random erasing.
    c.AUG = CfgNode(dict(ENABLE=False, CROP="jitter", RRC_SCALE=[0.08, 1.0], RRC_RATIO=[0.75, 1.3333], FLIP_PROB=0.5,
                         BRIGHTNESS=0.4, CONTRAST=0.4, SATURATION=0.4, COLOR_PROB=1.0, GRAYSCALE_PROB=0.0, RE_PROB=0.25,
                         RE_MODE="pixel", RE_AREA=[0.02, 0.3333], RE_RATIO=[0.3, 3.3333],
                         # RandAugment on the uint8 frames before everything above (x3d_randaug_clips), written as PySlowFast /
                         # timm write it: "rand-m7-n4-mstd0.5-inc1" (randaug_settings); "" = off
                         AA_TYPE=""))
    # the solver step around the optimizer (all off by default; CLIP_GRAD_L2NORM as PySlowFast's SOLVER section): the max global
    # L2 norm of the unscaled, all-reduced gradient (0 = off), micro-batches per optimizer update, the decay of the weight EMA
    # (0 = off) and whether fit's validation runs on the EMA weights
    # Fine-tuning (finetune_settings; all off by default).  LAYER_DECAY: tensor of depth group d gets the learning-rate scale
    # LAYER_DECAY ** (D - d) (timm's layer decay: stem 0, the residual blocks 1..L, head D = L + 1); LR_MULT: [[name prefix,
    # factor], ...] on top of it, the longest matching prefix wins; FREEZE: name prefixes of the tensors the solver step leaves
    # alone; FREEZE_EVAL (freeze_eval_settings): the frozen PREFIX of the network -- the stem and the residual blocks behind it,
    # as far as every trainable tensor is frozen -- runs in inference form during training (moving statistics, nothing kept)
    # and the backward pass ends above it.  FREEZE_BN (freeze_bn_settings): name prefixes of BatchNorm layers that normalise with
    # their moving statistics while training, and leave them alone, though their layers still train.  DEVICE_LOSS_SCALE (device_loss_scale_settings): the dynamic fp16 loss scaler lives
    # in device memory and the training step reads nothing back (inert with a fixed scale or none).  The section knows the
    # six keys without holding them: its items stay the four above until one is set.
    c.SOLVER = CfgNode(dict(CLIP_GRAD_L2NORM=0.0, ACCUM_STEPS=1, EMA_DECAY=0.0, EMA_EVAL=True),
                       optional=dict(LAYER_DECAY=1.0, LR_MULT=[], FREEZE=[], FREEZE_EVAL=False, FREEZE_BN=[], DEVICE_LOSS_SCALE=False))
    # the layer-wise optimizers (TRAIN.OPTIMIZER = lars | adamw | lamb; inert for sgd / adam).  LARS (PySlowFast's SOLVER.LARS_ON):
    # trust coefficient eta, the eps of its denominator, LARC clipping q <- min(q / lr, 1).  WEIGHT_DECAY: the DECOUPLED decay
    # of adamw / lamb (they ignore NETWORK.WEIGHT_DECAY); LAMB_EPS: the eps of LAMB's denominator
    c.OPTIM = CfgNode(dict(LARS_TRUST_COEF=0.001, LARS_EPS=1e-8, LARS_CLIP=False, WEIGHT_DECAY=0.0, LAMB_EPS=1e-6))
    # knowledge distillation (distill_settings; off by default): the training loss becomes (1 - ALPHA) * hard + ALPHA * T^2 *
    # KL(teacher || student) on logits softened by TEMPERATURE.  TEACHER: a shipped config name (XS .. XL) or a yaml path,
    # TEACHER_CKPT its checkpoint prefix; both unused when the trainer is handed a teacher model
    c.DISTILL = CfgNode(dict(ENABLE=False, TEACHER="", TEACHER_CKPT="", ALPHA=0.5, TEMPERATURE=1.0))
    # class-imbalance losses (loss_settings; all off by default).  CLASS_WEIGHTS: one weight per class on the hard term of either
    # head (Keras class_weight; losses.class_weights_from_counts builds them); POS_WEIGHT: one weight per class on the positive
    # term of the sigmoid head (torch BCEWithLogitsLoss(pos_weight)); FOCAL_GAMMA: the focusing exponent (Keras
    # Categorical / BinaryFocalCrossentropy), on the sigmoid head that of the positive term; FOCAL_GAMMA_NEG: that of the
    # sigmoid head's negative term (the symmetric focal loss sets both to one value, asymmetric focusing to two).  [] = all ones
    c.LOSS = CfgNode(dict(CLASS_WEIGHTS=[], POS_WEIGHT=[], FOCAL_GAMMA=0.0, FOCAL_GAMMA_NEG=0.0))
    # the ROI head for action detection (detection_settings; off by default; names as PySlowFast's DETECTION section): per person
    # box, the temporal mean of relu(bn5(conv5)), ROIAlign at ROI_XFORM_RESOLUTION^2 bins, a spatial max, fc1 / fc2 and the head's
    # loss over the valid boxes (x3d_roi_pool_fwd / x3d_roi_pool_bwd).  MAX_BOXES: the fixed number of box slots K per clip;
    # SPATIAL_SCALE_FACTOR: clip pixels per conv5 pixel (the network's stride, 32); ROI_SAMPLING_RATIO: samples per bin and axis,
    # 0 = ceil(bin size)
    c.DETECTION = CfgNode(dict(ENABLE=False, MAX_BOXES=8, ROI_XFORM_RESOLUTION=7, SPATIAL_SCALE_FACTOR=32, ROI_SAMPLING_RATIO=0))
    # the AVA frame-list dataset (ava_settings, ava.AvaReader; names as PySlowFast's AVA section; inert unless that reader is
    # constructed).  FRAME_DIR: root of the extracted frames; FRAME_LIST_DIR: where TRAIN_LISTS / TEST_LISTS (frame lists) live;
    # ANNOTATION_DIR: where the box lists, GROUNDTRUTH_FILE and EXCLUSION_FILE live.  Training boxes are TRAIN_GT_BOX_LISTS plus
    # the rows of TRAIN_PREDICT_BOX_LISTS scored at least DETECTION_SCORE_THRESH; evaluation proposals the thresholded
    # TEST_PREDICT_BOX_LISTS.  Second `sec` of a video is frame (sec - START_SEC) * FPS of its list; only seconds inside
    # VALID_SECS = [first, last] are keyframes
    c.AVA = CfgNode(dict(FRAME_DIR="", FRAME_LIST_DIR="", ANNOTATION_DIR="", TRAIN_LISTS=["train.csv"], TEST_LISTS=["val.csv"],
                         TRAIN_GT_BOX_LISTS=["ava_train_v2.2.csv"], TRAIN_PREDICT_BOX_LISTS=[],
                         TEST_PREDICT_BOX_LISTS=["ava_val_predicted_boxes.csv"], DETECTION_SCORE_THRESH=0.9,
                         GROUNDTRUTH_FILE="ava_val_v2.2.csv", EXCLUSION_FILE="ava_val_excluded_timestamps_v2.2.csv",
                         FPS=30, START_SEC=900, VALID_SECS=[902, 1798]))
    # ENSEMBLE_METHOD: how the views x crops of a video are combined at inference, "mean" (the reference's) or "max"
    c.TEST = CfgNode(dict(NUM_SPATIAL_CROPS=3, NUM_TEMPORAL_VIEWS=1, BATCH_SIZE=1, ENSEMBLE_METHOD="mean"))
    c.WANDB = CfgNode(dict(
        ENABLE=False, PROJECT_NAME="X3D-tf", GROUP_NAME=" ", MODE="online", TENSORBOARD=True))
    return c


def config_path(name):
    """Path of a shipped model config: name in {XS, S, M, L, XL} or 'X3D_M'."""
    name = name.upper().replace("X3D-", "").replace("X3D_", "")
    return os.path.join(_CONFIG_DIR, "kinetics", f"X3D_{name}.yaml")


def get_config(name, overrides=None, freeze=True):
    """Defaults + configs/kinetics/X3D_<name>.yaml (+ optional [key, value, ...] overrides)."""
    cfg = get_default_config()
    cfg.merge_from_file(config_path(name))
    if overrides:
        cfg.merge_from_list(list(overrides))
    ensemble_method(cfg)
    mix_settings(cfg)
    aug_settings(cfg)
    randaug_settings(cfg)
    solver_settings(cfg)
    finetune_settings(cfg)
    freeze_eval_settings(cfg)
    freeze_bn_settings(cfg)
    device_loss_scale_settings(cfg)
    optim_settings(cfg)
    drop_path_settings(cfg)
    res5_dilation_settings(cfg)
    precise_bn_settings(cfg)
    distill_settings(cfg, have_teacher=True)   # (whether a teacher exists is the trainer's to check)
    loss_settings(cfg)
    detection_settings(cfg)
    ava_settings(cfg)
    if freeze:
        cfg.freeze()
    return cfg


ENSEMBLE_METHODS = ("mean", "max")


def multi_label(cfg) -> bool:
    """cfg.DATA.MULTI_LABEL (False for a config tree without the key)."""
    return bool(getattr(cfg.DATA, "MULTI_LABEL", False))


def ensemble_method(cfg) -> str:
    """cfg.TEST.ENSEMBLE_METHOD ("mean" for a config tree without the key); anything else raises ValueError."""
    m = getattr(cfg.TEST, "ENSEMBLE_METHOD", "mean")
    if m not in ENSEMBLE_METHODS:
        raise ValueError(f"TEST.ENSEMBLE_METHOD must be one of {ENSEMBLE_METHODS}, not {m!r}")
    return m


MixSettings = collections.namedtuple("MixSettings", "enable alpha cutmix_alpha prob switch_prob label_smoothing")


def mix_settings(cfg) -> MixSettings:
    """cfg.MIXUP.* and cfg.TRAIN.LABEL_SMOOTHING as one tuple (a config tree without the keys: everything off).  ValueError
    for a negative alpha, ENABLE with both alphas 0, PROB / SWITCH_PROB outside [0, 1], LABEL_SMOOTHING outside [0, 1), and
    LABEL_SMOOTHING > 0 with DATA.MULTI_LABEL (smoothing is defined for the softmax head; mixup / CutMix work with both)."""
    mx = getattr(cfg, "MIXUP", None)
    s = MixSettings(bool(getattr(mx, "ENABLE", False)), float(getattr(mx, "ALPHA", 0.0)),
                    float(getattr(mx, "CUTMIX_ALPHA", 0.0)), float(getattr(mx, "PROB", 1.0)),
                    float(getattr(mx, "SWITCH_PROB", 0.5)), float(getattr(cfg.TRAIN, "LABEL_SMOOTHING", 0.0)))
    if not (s.alpha >= 0.0 and s.cutmix_alpha >= 0.0):      # (NaN fails too)
        raise ValueError(f"MIXUP.ALPHA / MIXUP.CUTMIX_ALPHA must be >= 0, not {s.alpha} / {s.cutmix_alpha}")
    if s.enable and s.alpha == 0.0 and s.cutmix_alpha == 0.0:
        raise ValueError("MIXUP.ENABLE needs MIXUP.ALPHA > 0 or MIXUP.CUTMIX_ALPHA > 0")
    if not 0.0 <= s.prob <= 1.0:
        raise ValueError(f"MIXUP.PROB must lie in [0, 1], not {s.prob}")
    if not 0.0 <= s.switch_prob <= 1.0:
        raise ValueError(f"MIXUP.SWITCH_PROB must lie in [0, 1], not {s.switch_prob}")
    if not 0.0 <= s.label_smoothing < 1.0:
        raise ValueError(f"TRAIN.LABEL_SMOOTHING must lie in [0, 1), not {s.label_smoothing}")
    if s.label_smoothing > 0.0 and multi_label(cfg):
        raise ValueError("TRAIN.LABEL_SMOOTHING is defined for the softmax head only, not with DATA.MULTI_LABEL")
    return s


AUG_CROPS = ("jitter", "rrc")
AUG_RE_MODES = ("pixel", "const")
AugSettings = collections.namedtuple("AugSettings", "enable crop rrc_scale rrc_ratio flip_prob brightness contrast saturation "
                                     "color_prob grayscale_prob re_prob re_mode re_area re_ratio")
_AUG_OFF = AugSettings(False, "jitter", (0.08, 1.0), (0.75, 1.3333), 0.5, 0.4, 0.4, 0.4, 1.0, 0.0, 0.25, "pixel",
                       (0.02, 0.3333), (0.3, 3.3333))


def aug_settings(cfg) -> AugSettings:
    """cfg.AUG.* as one tuple (a config tree without the section: off, the defaults otherwise).  ValueError for a range that is
    not 0 < lo <= hi (RRC_SCALE, RRC_RATIO, RE_AREA, RE_RATIO), a probability outside [0, 1] (FLIP_PROB, COLOR_PROB,
    GRAYSCALE_PROB, RE_PROB), a strength outside [0, 1) (BRIGHTNESS, CONTRAST, SATURATION: the factor 1 + U(-v, v) stays
    positive), an unknown CROP or RE_MODE."""
    a = getattr(cfg, "AUG", None)
    if a is None:
        return _AUG_OFF

    def rng(key, dflt):
        v = getattr(a, key, dflt)
        try:
            lo, hi = (float(x) for x in v)
        except (TypeError, ValueError):
            raise ValueError(f"AUG.{key} must be a pair [lo, hi], not {v!r}")
        if not 0.0 < lo <= hi or hi == float("inf"):          # (NaN fails too)
            raise ValueError(f"AUG.{key} must satisfy 0 < lo <= hi, not {v!r}")
        return lo, hi

    def prob(key, dflt):
        v = float(getattr(a, key, dflt))
        if not 0.0 <= v <= 1.0:
            raise ValueError(f"AUG.{key} must lie in [0, 1], not {v}")
        return v

    def strength(key, dflt):
        v = float(getattr(a, key, dflt))
        if not 0.0 <= v < 1.0:
            raise ValueError(f"AUG.{key} must lie in [0, 1), not {v}")
        return v
    d = _AUG_OFF
    s = AugSettings(bool(getattr(a, "ENABLE", False)), getattr(a, "CROP", d.crop), rng("RRC_SCALE", d.rrc_scale),
                    rng("RRC_RATIO", d.rrc_ratio), prob("FLIP_PROB", d.flip_prob), strength("BRIGHTNESS", d.brightness),
                    strength("CONTRAST", d.contrast), strength("SATURATION", d.saturation), prob("COLOR_PROB", d.color_prob),
                    prob("GRAYSCALE_PROB", d.grayscale_prob), prob("RE_PROB", d.re_prob), getattr(a, "RE_MODE", d.re_mode),
                    rng("RE_AREA", d.re_area), rng("RE_RATIO", d.re_ratio))
    if s.crop not in AUG_CROPS:
        raise ValueError(f"AUG.CROP must be one of {AUG_CROPS}, not {s.crop!r}")
    if s.re_mode not in AUG_RE_MODES:
        raise ValueError(f"AUG.RE_MODE must be one of {AUG_RE_MODES}, not {s.re_mode!r}")
    if s.rrc_scale[1] > 1.0 or s.re_area[1] > 1.0:
        raise ValueError(f"AUG.RRC_SCALE / AUG.RE_AREA are area fractions (<= 1), not {s.rrc_scale} / {s.re_area}")
    return s


# RandAugment (AUG.AA_TYPE): magnitude 0..10, layers (ops drawn per clip), mstd (sigma of the magnitude noise), inc (the
# "increasing" op set: every op grows stronger with the magnitude), prob (chance a drawn op is applied)
RandAugSpec = collections.namedtuple("RandAugSpec", "magnitude layers mstd inc prob")
_AA_FIELD = re.compile(r"(mstd|inc|m|n|p)(.+)")


def parse_aa_type(text: str) -> RandAugSpec:
    """"rand" followed by "-"-separated fields in any order: m<int 0..10> magnitude (default 10), n<int >= 1> layers (2),
    mstd<float >= 0> magnitude noise (0), inc<0|1> the increasing op set (0), p<float in [0, 1]> per-op probability (0.5).
    ValueError for anything else: another policy name, an unknown or repeated field, a value outside its range."""
    def bad(why):
        return ValueError(f"AUG.AA_TYPE {text!r}: {why} (grammar: rand[-m<0..10>][-n<int>=1>][-mstd<float>=0>][-inc<0|1>][-p<0..1>])")
    if not isinstance(text, str):
        raise bad("not a string")
    parts = text.split("-")
    if parts[0] != "rand":
        raise bad("only the 'rand' policy is implemented")
    vals = dict(m=10, n=2, mstd=0.0, inc=0, p=0.5)
    seen = set()
    for part in parts[1:]:
        f = _AA_FIELD.fullmatch(part)
        if not f:
            raise bad(f"cannot read field {part!r}")
        key, val = f.groups()
        if key in seen:
            raise bad(f"field {key!r} given twice")
        seen.add(key)
        if key in ("m", "n", "inc"):
            if not re.fullmatch(r"\d+", val):
                raise bad(f"{key} takes a non-negative integer, not {val!r}")
            v = int(val)
            if (key == "m" and v > 10) or (key == "n" and v < 1) or (key == "inc" and v > 1):
                raise bad(f"{key} = {v} out of range")
        else:
            if not re.fullmatch(r"\d+(\.\d*)?|\.\d+", val):
                raise bad(f"{key} takes a non-negative decimal number, not {val!r}")
            v = float(val)
            if key == "p" and v > 1.0:
                raise bad(f"p = {v} outside [0, 1]")
        vals[key] = v
    return RandAugSpec(vals["m"], vals["n"], vals["mstd"], bool(vals["inc"]), vals["p"])


def randaug_settings(cfg):
    """cfg.AUG.AA_TYPE as a RandAugSpec; None for "" and for a config tree without the key (or without AUG).  ValueError for a
    string outside the grammar (parse_aa_type) and for AA_TYPE set while AUG.ENABLE is off (the batched call is the only path
    that runs it: a silently ignored policy would be a wrong recipe)."""
    a = getattr(cfg, "AUG", None)
    text = getattr(a, "AA_TYPE", "") if a is not None else ""
    if text == "":
        return None
    spec = parse_aa_type(text)
    if not bool(getattr(a, "ENABLE", False)):
        raise ValueError(f"AUG.AA_TYPE = {text!r} needs AUG.ENABLE")
    return spec


SolverSettings = collections.namedtuple("SolverSettings", "clip_grad_l2norm accum_steps ema_decay ema_eval")
_SOLVER_OFF = SolverSettings(0.0, 1, 0.0, True)


def solver_settings(cfg) -> SolverSettings:
    """cfg.SOLVER.* as one tuple (a config tree without the section: everything off).  ValueError for a negative or
    non-finite CLIP_GRAD_L2NORM, an ACCUM_STEPS that is not an integer >= 1, an EMA_DECAY outside [0, 1)."""
    import math
    sv = getattr(cfg, "SOLVER", None)
    if sv is None:
        return _SOLVER_OFF
    d = _SOLVER_OFF
    clip = float(getattr(sv, "CLIP_GRAD_L2NORM", d.clip_grad_l2norm))
    if not (clip >= 0.0 and math.isfinite(clip)):           # (NaN fails too)
        raise ValueError(f"SOLVER.CLIP_GRAD_L2NORM must be finite and >= 0 (0 = off), not {clip}")
    accum = getattr(sv, "ACCUM_STEPS", d.accum_steps)
    if isinstance(accum, bool) or not isinstance(accum, int) or accum < 1:
        raise ValueError(f"SOLVER.ACCUM_STEPS must be an integer >= 1, not {accum!r}")
    decay = float(getattr(sv, "EMA_DECAY", d.ema_decay))
    if not 0.0 <= decay < 1.0:
        raise ValueError(f"SOLVER.EMA_DECAY must lie in [0, 1), not {decay}")
    return SolverSettings(clip, accum, decay, bool(getattr(sv, "EMA_EVAL", d.ema_eval)))


FinetuneSettings = collections.namedtuple("FinetuneSettings", "layer_decay lr_mult freeze")
_FINETUNE_OFF = FinetuneSettings(1.0, (), ())


def finetune_settings(cfg) -> FinetuneSettings:
    """cfg.SOLVER.LAYER_DECAY / LR_MULT / FREEZE as one tuple: (layer_decay, ((prefix, factor), ...), (prefix, ...)).  A config
    tree without the keys (or without the section): everything off = (1.0, (), ()).  ValueError for a LAYER_DECAY outside
    (0, 1], an LR_MULT entry that is not [str, finite float > 0] and a FREEZE entry that is not a string (NaN fails too).
    Freezing is FREEZE's alone: a factor of 0 is refused, it would not freeze anything (finetune.py).  Whether the prefixes
    match a tensor is finetune.lr_scales' to check: it needs the architecture."""
    import math
    sv = getattr(cfg, "SOLVER", None)
    if sv is None:
        return _FINETUNE_OFF
    d = _FINETUNE_OFF
    decay = getattr(sv, "LAYER_DECAY", d.layer_decay)
    if isinstance(decay, bool) or not isinstance(decay, (int, float)) or not 0.0 < float(decay) <= 1.0:
        raise ValueError(f"SOLVER.LAYER_DECAY must lie in (0, 1], not {decay!r}")
    mult = getattr(sv, "LR_MULT", d.lr_mult)
    if not isinstance(mult, (list, tuple)):
        raise ValueError(f"SOLVER.LR_MULT must be a list of [name prefix, factor], not {mult!r}")
    pairs = []
    for e in mult:
        ok = isinstance(e, (list, tuple)) and len(e) == 2 and isinstance(e[0], str) and not isinstance(e[1], bool) \
            and isinstance(e[1], (int, float)) and math.isfinite(e[1]) and e[1] > 0
        if not ok:
            raise ValueError(f"SOLVER.LR_MULT entries must be [name prefix (str), finite factor > 0], not {e!r}")
        pairs.append((e[0], float(e[1])))
    freeze = getattr(sv, "FREEZE", d.freeze)
    if not isinstance(freeze, (list, tuple)) or not all(isinstance(f, str) for f in freeze):
        raise ValueError(f"SOLVER.FREEZE must be a list of name prefixes (str), not {freeze!r}")
    return FinetuneSettings(float(decay), tuple(pairs), tuple(freeze))


def freeze_eval_settings(cfg) -> bool:
    """cfg.SOLVER.FREEZE_EVAL (False for a config tree without the key or the section): the frozen prefix of SOLVER.FREEZE runs
    in inference form and the backward pass is cut above it (finetune.frozen_prefix, X3D.set_finetune).  Kept apart from
    FinetuneSettings, which stays the 3-tuple of the solver step.  ValueError for a value that is not a bool; whether FREEZE
    freezes a prefix at all is the model's to check: it needs the architecture."""
    sv = getattr(cfg, "SOLVER", None)
    on = False if sv is None else getattr(sv, "FREEZE_EVAL", False)
    if not isinstance(on, bool):
        raise ValueError(f"SOLVER.FREEZE_EVAL must be a bool, not {on!r}")
    return on


def freeze_bn_settings(cfg) -> tuple:
    """cfg.SOLVER.FREEZE_BN as a tuple of name prefixes (() for a config tree without the key or the section): the BatchNorm
    layers whose name -- the part in front of `/gamma` -- starts with one of them normalise with their moving statistics in a
    training step and do not update them (PySlowFast's MODEL.FROZEN_BN, detectron2's FrozenBatchNorm); [""] is every layer.
    Whether gamma and beta are updated stays SOLVER.FREEZE's business.  ValueError for anything that is not a list of strings;
    whether a prefix matches a layer is the model's to check (finetune.frozen_bn_layers): it needs the architecture."""
    sv = getattr(cfg, "SOLVER", None)
    names = [] if sv is None else getattr(sv, "FREEZE_BN", [])
    if not isinstance(names, (list, tuple)) or not all(isinstance(f, str) for f in names):
        raise ValueError(f"SOLVER.FREEZE_BN must be a list of BatchNorm name prefixes (str), not {names!r}")
    return tuple(names)


def device_loss_scale_settings(cfg) -> bool:
    """cfg.SOLVER.DEVICE_LOSS_SCALE (False for a config tree without the key or the section): the trainer's DYNAMIC loss scaling
    -- float16 storage with loss_scale="auto", or loss_scale="dynamic" -- keeps its state in device memory and decides, skips
    and rescales there (train.Trainer, x3d_loss_scale_update).  Inert with a fixed scale or none.  ValueError for a value that
    is not a bool."""
    sv = getattr(cfg, "SOLVER", None)
    on = False if sv is None else getattr(sv, "DEVICE_LOSS_SCALE", False)
    if not isinstance(on, bool):
        raise ValueError(f"SOLVER.DEVICE_LOSS_SCALE must be a bool, not {on!r}")
    return on


OptimSettings = collections.namedtuple("OptimSettings", "lars_trust_coef lars_eps lars_clip weight_decay lamb_eps")
_OPTIM_DEFAULTS = OptimSettings(0.001, 1e-8, False, 0.0, 1e-6)
OPTIMIZERS = tuple(RULES)                                   # TRAIN.OPTIMIZER, case-insensitive
SLOT_KIND = {name: rule.slot_kind for name, rule in RULES.items()}   # whose slot / checkpoint layout a branch uses


def optim_settings(cfg) -> OptimSettings:
    """cfg.OPTIM.* as one tuple (a config tree without the section: the defaults).  ValueError for a LARS_TRUST_COEF that is
    not positive and finite, a negative LARS_EPS, a WEIGHT_DECAY that is negative or not finite, a LAMB_EPS that is not
    positive (NaN fails all of them)."""
    import math
    ov = getattr(cfg, "OPTIM", None)
    d = _OPTIM_DEFAULTS
    if ov is None:
        return d
    eta = float(getattr(ov, "LARS_TRUST_COEF", d.lars_trust_coef))
    if not (eta > 0.0 and math.isfinite(eta)):
        raise ValueError(f"OPTIM.LARS_TRUST_COEF must be positive and finite, not {eta}")
    eps = float(getattr(ov, "LARS_EPS", d.lars_eps))
    if not (eps >= 0.0 and math.isfinite(eps)):
        raise ValueError(f"OPTIM.LARS_EPS must be finite and >= 0, not {eps}")
    decay = float(getattr(ov, "WEIGHT_DECAY", d.weight_decay))
    if not (decay >= 0.0 and math.isfinite(decay)):
        raise ValueError(f"OPTIM.WEIGHT_DECAY must be finite and >= 0, not {decay}")
    lamb_eps = float(getattr(ov, "LAMB_EPS", d.lamb_eps))
    if not (lamb_eps > 0.0 and math.isfinite(lamb_eps)):
        raise ValueError(f"OPTIM.LAMB_EPS must be positive and finite, not {lamb_eps}")
    return OptimSettings(eta, eps, bool(getattr(ov, "LARS_CLIP", d.lars_clip)), decay, lamb_eps)


def drop_path_settings(cfg) -> float:
    """cfg.NETWORK.DROP_PATH_RATE (0.0 for a config tree without the key).  ValueError outside [0, 1) and for NaN."""
    rate = float(getattr(cfg.NETWORK, "DROP_PATH_RATE", 0.0))
    if not 0.0 <= rate < 1.0:           # (NaN fails too)
        raise ValueError(f"NETWORK.DROP_PATH_RATE must lie in [0, 1), not {rate}")
    return rate


RES5_DILATIONS = (1, 2)


def res5_dilation_settings(cfg) -> int:
    """cfg.NETWORK.RES5_DILATION (1 for a config tree without the key).  ValueError for anything but the integers 1 and 2, and --
    only when the key is not 1 -- for DETECTION.ENABLE with a DETECTION.SPATIAL_SCALE_FACTOR that is not the network's stride,
    32 // RES5_DILATION."""
    d = getattr(cfg.NETWORK, "RES5_DILATION", 1)
    if isinstance(d, bool) or not isinstance(d, int) or d not in RES5_DILATIONS:
        raise ValueError(f"NETWORK.RES5_DILATION must be one of {RES5_DILATIONS}, not {d!r}")
    dv = getattr(cfg, "DETECTION", None)
    if d != 1 and dv is not None and bool(getattr(dv, "ENABLE", False)):
        f = getattr(dv, "SPATIAL_SCALE_FACTOR", 32)
        if f != 32 // d:
            raise ValueError(f"DETECTION.SPATIAL_SCALE_FACTOR = {f} with NETWORK.RES5_DILATION = {d}: conv5 is at stride "
                             f"{32 // d}, set DETECTION.SPATIAL_SCALE_FACTOR to {32 // d}")
    return d


PreciseBNSettings = collections.namedtuple("PreciseBNSettings", "enable num_batches")


def precise_bn_settings(cfg) -> PreciseBNSettings:
    """cfg.NETWORK.BN.USE_PRECISE_STATS / NUM_BATCHES_PRECISE as one tuple (a config tree without the keys: off, 200 batches).
    ValueError for a NUM_BATCHES_PRECISE that is not an integer >= 1 -- checked whether the switch is on or not."""
    bn = getattr(cfg.NETWORK, "BN", None)
    num = getattr(bn, "NUM_BATCHES_PRECISE", 200)
    if isinstance(num, bool) or not isinstance(num, int) or num < 1:
        raise ValueError(f"NETWORK.BN.NUM_BATCHES_PRECISE must be an integer >= 1, not {num!r}")
    return PreciseBNSettings(bool(getattr(bn, "USE_PRECISE_STATS", False)), num)


DistillSettings = collections.namedtuple("DistillSettings", "enable teacher teacher_ckpt alpha temperature")
_DISTILL_OFF = DistillSettings(False, "", "", 0.5, 1.0)


def distill_settings(cfg, have_teacher: bool = False) -> DistillSettings:
    """cfg.DISTILL.* as one tuple (a config tree without the section: off).  ValueError for an ALPHA outside [0, 1], a
    TEMPERATURE that is not finite and > 0 (NaN fails both) -- checked whether the switch is on or not -- and for ENABLE
    with an empty TEACHER unless `have_teacher`: the trainer was handed a teacher model (get_config cannot know, it passes
    True and leaves that check to the trainer)."""
    import math
    dv = getattr(cfg, "DISTILL", None)
    if dv is None:
        return _DISTILL_OFF
    d = _DISTILL_OFF
    alpha = float(getattr(dv, "ALPHA", d.alpha))
    if not 0.0 <= alpha <= 1.0:
        raise ValueError(f"DISTILL.ALPHA must lie in [0, 1], not {alpha}")
    temp = float(getattr(dv, "TEMPERATURE", d.temperature))
    if not (temp > 0.0 and math.isfinite(temp)):
        raise ValueError(f"DISTILL.TEMPERATURE must be finite and > 0, not {temp}")
    s = DistillSettings(bool(getattr(dv, "ENABLE", False)), str(getattr(dv, "TEACHER", d.teacher)),
                        str(getattr(dv, "TEACHER_CKPT", d.teacher_ckpt)), alpha, temp)
    if s.enable and not s.teacher and not have_teacher:
        raise ValueError("DISTILL.ENABLE needs DISTILL.TEACHER (a shipped config name or a yaml path) or a teacher model "
                         "handed to the trainer")
    return s


LossSettings = collections.namedtuple("LossSettings", "class_weights pos_weight focal_gamma focal_gamma_neg")
_LOSS_OFF = LossSettings((), (), 0.0, 0.0)
FOCAL_GAMMA_MAX = 8.0          # the bound x3d_softmax_xent_w / x3d_sigmoid_bce_w refuse above


def loss_settings(cfg) -> LossSettings:
    """cfg.LOSS.* as one tuple (a config tree without the section: off; an empty list: no table).  The weight lists come back
    as tuples of floats.  ValueError for a weight that is not finite and >= 0 or a list of all zeros, a gamma outside
    [0, 8] (NaN fails), POS_WEIGHT or FOCAL_GAMMA_NEG without DATA.MULTI_LABEL, and a list whose length is not
    NETWORK.NUM_CLASSES."""
    import math
    lv = getattr(cfg, "LOSS", None)
    if lv is None:
        return _LOSS_OFF
    multi, classes = multi_label(cfg), int(cfg.NETWORK.NUM_CLASSES)

    def table(key):
        w = tuple(float(v) for v in (getattr(lv, key, None) or ()))
        if not w:
            return ()
        if len(w) != classes:
            raise ValueError(f"LOSS.{key} has {len(w)} entries, NETWORK.NUM_CLASSES is {classes}")
        if not all(math.isfinite(v) and v >= 0.0 for v in w):
            raise ValueError(f"LOSS.{key} must be finite and >= 0")
        if not any(v > 0.0 for v in w):
            raise ValueError(f"LOSS.{key} is all zeros: nothing would be trained")
        return w

    def gamma(key):
        g = float(getattr(lv, key, 0.0))
        if not 0.0 <= g <= FOCAL_GAMMA_MAX:
            raise ValueError(f"LOSS.{key} must lie in [0, {FOCAL_GAMMA_MAX:g}], not {g}")
        return g

    s = LossSettings(table("CLASS_WEIGHTS"), table("POS_WEIGHT"), gamma("FOCAL_GAMMA"), gamma("FOCAL_GAMMA_NEG"))
    if not multi and s.pos_weight:
        raise ValueError("LOSS.POS_WEIGHT weighs the positive term of the sigmoid head: it needs DATA.MULTI_LABEL")
    if not multi and s.focal_gamma_neg != 0.0:
        raise ValueError("LOSS.FOCAL_GAMMA_NEG focuses the negative term of the sigmoid head: it needs DATA.MULTI_LABEL")
    return s


DetectionSettings = collections.namedtuple("DetectionSettings", "enable max_boxes resolution spatial_scale_factor sampling_ratio")
_DETECTION_OFF = DetectionSettings(False, 8, 7, 32, 0)
# the limits of x3d_roi_pool_fwd / x3d_roi_pool_bwd (include/x3d_hip.h)
ROI_MAX_BOXES, ROI_MAX_RESOLUTION = 64, 15


def detection_settings(cfg) -> DetectionSettings:
    """cfg.DETECTION.* as one tuple (a config tree without the section: off).  ValueError -- whether the switch is on or not -- for
    MAX_BOXES outside [1, 64], ROI_XFORM_RESOLUTION outside [1, 15], a SPATIAL_SCALE_FACTOR < 1 and a
    negative ROI_SAMPLING_RATIO (the kernels' own limits); with ENABLE also for MIXUP.ENABLE (a mixed clip has no boxes),
    DISTILL.ENABLE, and TEST.NUM_SPATIAL_CROPS * TEST.NUM_TEMPORAL_VIEWS > 1 (box rows are not views of one video)."""
    dv = getattr(cfg, "DETECTION", None)
    if dv is None:
        return _DETECTION_OFF
    d = _DETECTION_OFF

    def whole(key, dflt):
        v = getattr(dv, key, dflt)
        if isinstance(v, bool) or not isinstance(v, int):
            raise ValueError(f"DETECTION.{key} must be an integer, not {v!r}")
        return v

    k = whole("MAX_BOXES", d.max_boxes)
    if not 1 <= k <= ROI_MAX_BOXES:
        raise ValueError(f"DETECTION.MAX_BOXES must lie in [1, {ROI_MAX_BOXES}], not {k}")
    r = whole("ROI_XFORM_RESOLUTION", d.resolution)
    if not 1 <= r <= ROI_MAX_RESOLUTION:
        raise ValueError(f"DETECTION.ROI_XFORM_RESOLUTION must lie in [1, {ROI_MAX_RESOLUTION}], not {r}")
    f = whole("SPATIAL_SCALE_FACTOR", d.spatial_scale_factor)
    if f < 1:
        raise ValueError(f"DETECTION.SPATIAL_SCALE_FACTOR must be >= 1, not {f}")
    sr = whole("ROI_SAMPLING_RATIO", d.sampling_ratio)
    if sr < 0:
        raise ValueError(f"DETECTION.ROI_SAMPLING_RATIO must be >= 0, not {sr}")
    s = DetectionSettings(bool(getattr(dv, "ENABLE", False)), k, r, f, sr)
    if s.enable:
        if bool(getattr(getattr(cfg, "MIXUP", None), "ENABLE", False)):
            raise ValueError("DETECTION.ENABLE with MIXUP.ENABLE: a mixed clip has no boxes")
        if bool(getattr(getattr(cfg, "DISTILL", None), "ENABLE", False)):
            raise ValueError("DETECTION.ENABLE with DISTILL.ENABLE: a clip-level teacher has no logits per box")
        views = int(getattr(cfg.TEST, "NUM_SPATIAL_CROPS", 1)) * int(getattr(cfg.TEST, "NUM_TEMPORAL_VIEWS", 1))
        if views > 1:
            raise ValueError(f"DETECTION.ENABLE with TEST.NUM_SPATIAL_CROPS * TEST.NUM_TEMPORAL_VIEWS = {views}: box rows are "
                             "not views of one video, set both to 1")
    return s


AvaSettings = collections.namedtuple("AvaSettings", "frame_dir frame_list_dir annotation_dir train_lists test_lists "
                                     "train_gt_box_lists train_predict_box_lists test_predict_box_lists detection_score_thresh "
                                     "groundtruth_file exclusion_file fps start_sec valid_secs")
_AVA_DEFAULTS = AvaSettings("", "", "", ("train.csv",), ("val.csv",), ("ava_train_v2.2.csv",), (), ("ava_val_predicted_boxes.csv",),
                            0.9, "ava_val_v2.2.csv", "ava_val_excluded_timestamps_v2.2.csv", 30, 900, (902, 1798))


def ava_settings(cfg) -> AvaSettings:
    """cfg.AVA.* as one tuple (a config tree without the section: the defaults; the lists come back as tuples).  ValueError for a
    list key that is not a list of strings, a DETECTION_SCORE_THRESH outside [0, 1] (NaN fails), an FPS that is not an integer
    >= 1, a START_SEC that is not an integer >= 0 and VALID_SECS that is not a pair of integers first <= last with first >=
    START_SEC.  What only the reader needs of the other sections is `ava_reader_check`'s."""
    av = getattr(cfg, "AVA", None)
    d = _AVA_DEFAULTS
    if av is None:
        return d

    def text(key, dflt):
        v = getattr(av, key, dflt)
        if not isinstance(v, str):
            raise ValueError(f"AVA.{key} must be a string, not {v!r}")
        return v

    def names(key, dflt):
        v = getattr(av, key, list(dflt))
        if not isinstance(v, (list, tuple)) or not all(isinstance(f, str) for f in v):
            raise ValueError(f"AVA.{key} must be a list of file names (str), not {v!r}")
        return tuple(v)

    def whole(key, dflt, lo):
        v = getattr(av, key, dflt)
        if isinstance(v, bool) or not isinstance(v, int) or v < lo:
            raise ValueError(f"AVA.{key} must be an integer >= {lo}, not {v!r}")
        return v

    thresh = float(getattr(av, "DETECTION_SCORE_THRESH", d.detection_score_thresh))
    if not 0.0 <= thresh <= 1.0:
        raise ValueError(f"AVA.DETECTION_SCORE_THRESH must lie in [0, 1], not {thresh}")
    start = whole("START_SEC", d.start_sec, 0)
    secs = getattr(av, "VALID_SECS", list(d.valid_secs))
    if not isinstance(secs, (list, tuple)) or len(secs) != 2 or any(isinstance(s, bool) or not isinstance(s, int) for s in secs) \
            or not start <= secs[0] <= secs[1]:
        raise ValueError(f"AVA.VALID_SECS must be [first, last] with AVA.START_SEC <= first <= last, not {secs!r}")
    return AvaSettings(text("FRAME_DIR", d.frame_dir), text("FRAME_LIST_DIR", d.frame_list_dir),
                       text("ANNOTATION_DIR", d.annotation_dir), names("TRAIN_LISTS", d.train_lists),
                       names("TEST_LISTS", d.test_lists), names("TRAIN_GT_BOX_LISTS", d.train_gt_box_lists),
                       names("TRAIN_PREDICT_BOX_LISTS", d.train_predict_box_lists),
                       names("TEST_PREDICT_BOX_LISTS", d.test_predict_box_lists), thresh,
                       text("GROUNDTRUTH_FILE", d.groundtruth_file), text("EXCLUSION_FILE", d.exclusion_file),
                       whole("FPS", d.fps, 1), start, (int(secs[0]), int(secs[1])))


def ava_reader_check(cfg) -> AvaSettings:
    """What ava.AvaReader needs of the other sections, checked at its construction; returns ava_settings(cfg).  ValueError naming
    the key for DETECTION.ENABLE off (the reader yields boxes), DATA.MULTI_LABEL off (an AVA box carries several actions: the
    sigmoid head is the one that fits), AUG.AA_TYPE set (RandAugment draws Rotate / Shear / Translate, and a rotated box is not a
    box) and TEST.NUM_SPATIAL_CROPS * TEST.NUM_TEMPORAL_VIEWS > 1 (one clip per keyframe; detection_settings refuses it too)."""
    s = ava_settings(cfg)
    views = int(getattr(cfg.TEST, "NUM_SPATIAL_CROPS", 1)) * int(getattr(cfg.TEST, "NUM_TEMPORAL_VIEWS", 1))
    if views > 1:
        raise ValueError(f"the AVA reader builds one clip per keyframe: TEST.NUM_SPATIAL_CROPS * TEST.NUM_TEMPORAL_VIEWS = {views}, "
                         "set both to 1")
    if not detection_settings(cfg).enable:
        raise ValueError("the AVA reader yields boxes: it needs DETECTION.ENABLE")
    if not multi_label(cfg):
        raise ValueError("the AVA reader yields multi-hot targets per box: it needs DATA.MULTI_LABEL")
    aa = getattr(getattr(cfg, "AUG", None), "AA_TYPE", "")
    if aa != "":
        raise ValueError(f"AUG.AA_TYPE = {aa!r} with the AVA reader: RandAugment rotates, shears and translates the frames, and "
                         "boxes are not mapped through it")
    return s
