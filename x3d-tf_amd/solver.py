"""The optimizer rules, stated once: RULES holds one record per value of TRAIN.OPTIMIZER.  config.OPTIMIZERS and config.SLOT_KIND
are read off it, ops.solver_launch makes a rule's launch from its record, X3D._apply chooses the form and Trainer._update the
arguments.  A new rule is a record here, an `apply_*` signature on the model and an `ops` signature.  Data only: no torch, no
library (config.py imports this).

Rule fields
  slot_kind   "sgd": one slot buffer (momentum), SGD's checkpoint layout; "adam": two (m, v) and `iter`, Adam's
  scalars     the rule's scalar arguments in the order of the C ABI (include/x3d_hip.h), name -> Python default; a type instead
              of a default marks an argument the caller has to give.  float, int and bool (an int flag) arguments are told
              apart by the default's type
  flat        (plain, _ex) entry points over the whole flat block under the byte mask, or None
  table       (plain, _pt) entry points over a segments.SegTable; plain None: the rule has the _pt form only
  trust       the rule computes per-segment trust ratios: it takes the scratch `partials` and `q` and returns q
  l2_in_loss  NETWORK.WEIGHT_DECAY is part of the rule (the coupled L2 term) and so of the loss Trainer.loss reports
  bounds      scalar name -> "> 0" | ">= 0" | ">= 1": what the chunk-table forms refuse to go below
  settings    scalar name -> field of config.OptimSettings (OPTIM.*) the trainer takes it from"""
import collections

Rule = collections.namedtuple("Rule", "slot_kind scalars flat table trust l2_in_loss bounds settings")
SLOT_NAMES = dict(sgd=("v",), adam=("m", "v"))     # slot kind -> what the entry points call its buffers

_SGD = dict(lr=float, momentum=0.9, weight_decay=float, grad_scale=1.0)
_ADAM = dict(lr=float, beta1=0.9, beta2=0.999, eps=1e-7, weight_decay=float, grad_scale=1.0, step=int)
_ADAMW = dict(lr=float, beta1=0.9, beta2=0.999, eps=1e-7, decay=0.0, grad_scale=1.0, step=int)

RULES = dict(          # in the order config.OPTIMIZERS has always listed them
    sgd=Rule("sgd", _SGD, ("x3d_sgd_nesterov", "x3d_sgd_nesterov_ex"), (None, "x3d_sgd_pt"), False, True, {}, {}),
    adam=Rule("adam", _ADAM, ("x3d_adam", "x3d_adam_ex"), (None, "x3d_adam_pt"), False, True, dict(step=">= 1"), {}),
    lars=Rule("sgd", dict(_SGD, trust_coef=0.001, eps=1e-8, clip=False), None, ("x3d_lars", "x3d_lars_pt"), True, True,
              dict(trust_coef="> 0", eps=">= 0"), dict(trust_coef="lars_trust_coef", eps="lars_eps", clip="lars_clip")),
    adamw=Rule("adam", _ADAMW, None, ("x3d_adamw", "x3d_adamw_pt"), False, False,
               dict(decay=">= 0", step=">= 1"), dict(decay="weight_decay")),
    lamb=Rule("adam", dict(_ADAMW, eps=1e-6), None, ("x3d_lamb", "x3d_lamb_pt"), True, False,
              dict(decay=">= 0", eps="> 0", step=">= 1"), dict(eps="lamb_eps", decay="weight_decay")),
)
