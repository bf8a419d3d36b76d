"""Launch plans: the buffers and the recorded kernel launches of one (batch, clip shape, mode) of an ``X3D`` model.

``record_training`` / ``record_inference(model, n, t, h, w)`` allocate every buffer once and record the forward list -- and, for training,
the backward list (``record_backward``) -- as pre-bound C calls; ``_Plan.run`` replays a list on the current HIP stream.  The
network has one block shape, so the recorders are straight-line code: stem, one block (repeated), head.  The inference
recorder and the training recorder share what is the same launch in both (stem, shortcut conv, SE, dense head) and keep
apart what is not (the `a` conv with the deferred residual tail against the `c` conv with the tail in its epilogue).
A CUT training plan (``record_training(..., frozen_prefix=k)``, SOLVER.FREEZE_EVAL) holds both forms: the frozen prefix -- the
stem and the first k - 1 blocks -- as the inference recorder records it, everything above as the training recorder does, and
a backward list that ends at the seam between the two (``record_backward(..., first_unit=k)``).
A FROZEN BatchNorm layer of the trained region (SOLVER.FREEZE_BN, ``model.frozen_bn``) keeps the training
recorder's launches around it but takes its coefficients from the moving statistics -- the same batched launch at slot 0 --
has no finalize launch and no statistics accumulator, and its backward finalize is a launch in the frozen form (a negative
count), never derived by its consumers.

fp64 accumulators are zeroed once per step in ONE flat buffer that exists only after recording, so a launch that takes the
address of one records a deferred address instead (``_Plan.acc`` for a positional argument, ``_Plan.defer`` for struct
fields) and ``_Plan.resolve`` patches them all in, for forward, backward and alternate backward lists alike.
"""
import collections
import ctypes as C
import math
import os
from dataclasses import dataclass, field
from typing import Any, Dict, List, Optional

import torch

from . import hip
from .arch import BlockSpec, block_prefix, same_pad
from .hip import (ACT_NONE, ACT_RELU, ACT_SWISH, EPI_ADD, EPI_ADD_STRIDED, EPI_STORE, EPI_SWISH_BWD)

# ------------------------------------------------------------------------------------------------
# Plan options: which of several launch lists -- each covered by the GPU tests -- a plan records.  The defaults are the product;
# the others document what was measured against them and serve the differential tests (X3D(cfg, options=...)).
# They are constructor arguments, not environment switches: the product path reads no X3D_* variable.  Only with
# X3D_EXPERIMENTS=1 (the A/B tools under tools/) are the historical variable names mapped onto them.
PLAN_DEFAULTS = {
    "fused_pw_bwd": True,      # x3d_pw_bwd (data + weight gradient in one launch) where it applies; False: x3d_pw_dgrad + x3d_pw_wgrad
    "pw_bwd_rc": True,         # ... in the form that recomputes the conv output algebraically instead of reading a_raw / r_raw
    "pw_bwd_rc_merge": True,   # its prepare / finish jobs ride on the BatchNorm-backward finalize launches
    "pw_bwd_rc_wide": True,    # ... also for the 48 -> 216 layer
    "stem_nthwc": True,        # the stem reads the caller's channels-last batch in place (16-bit storage)
    "stem_fused": True,        # ... and runs conv_s -> conv_t as ONE launch each way (x3d_stem_fwd / x3d_stem_bwd): no s_raw, no ds
    "shortcut_compact": True,  # strided shortcut convs whose output rows are odd (7, 39, 5 wide: one output per 4-byte load in the
                               #   gather) read an even-pixel copy of the block input instead (x3d_subsample2): dense launches
    "tail_fwd_fold": True,     # residual tail built on load by the next block's `a` conv
    "tail_fold_wst": True,     # ... also where that conv runs the weights-stationary kernel (stages 4 / 5)
    "tail_bwd_fold": True,     # Add + ReLU backward in the epilogue of the kernel that produces dy
    "stem_bwd_fold": True,     # the stem BatchNorm's backward sums in the first block's `a` backward
    "coef_fold": True,         # the BatchNorm-backward finalize derived by its consumers where their kernels take it (no launch)
    "dw_slab": True,           # persistent fused backward kernels store per-workgroup partial weight gradients (plain stores) that
                               #   the next x3d_se_bnb_bwd launch adds up, instead of flushing them with fp32 atomics
}
_ENV_OPTIONS = {   # historical switch -> (option, value the variable's non-default setting selects)
    "X3D_NO_FUSED_PW_BWD": ("fused_pw_bwd", "1", False), "X3D_PW_BWD_RC": ("pw_bwd_rc", "0", False),
    "X3D_PW_BWD_RC_MERGE": ("pw_bwd_rc_merge", "0", False), "X3D_PW_BWD_RC_WIDE": ("pw_bwd_rc_wide", "0", False),
    "X3D_NO_STEM_NTHWC": ("stem_nthwc", "1", False), "X3D_NO_STEM_FUSED": ("stem_fused", "1", False), "X3D_NO_SHORTCUT_COMPACT": ("shortcut_compact", "1", False),
    "X3D_NO_TAIL_FWD_FOLD": ("tail_fwd_fold", "1", False),
    "X3D_NO_TAIL_FOLD_WST": ("tail_fold_wst", "1", False), "X3D_NO_TAIL_FOLD": ("tail_bwd_fold", "1", False),
    "X3D_NO_STEM_BWD_FOLD": ("stem_bwd_fold", "1", False),
    "X3D_NO_DW_SLAB": ("dw_slab", "1", False), "X3D_NO_COEF_FOLD": ("coef_fold", "1", False),
}


def _experiment_options():
    if os.environ.get("X3D_EXPERIMENTS") != "1":
        return {}
    return {opt: val for var, (opt, trigger, val) in _ENV_OPTIONS.items() if os.environ.get(var) == trigger}


# X3D.loss_mods: the modifiers of the head's loss (X3D.set_loss) -- device tables [classes] fp32 or None, the focal exponents
LossMods = collections.namedtuple("LossMods", "class_w pos_w gamma gamma_neg")
NO_LOSS_MODS = LossMods(None, None, 0.0, 0.0)


class _FakeBuf:
    """Stand-in for a device buffer in a DRY plan (X3D(..., device="dry")): an address range that is never touched.
    Dry plans exist so that the launch list of a full-size configuration -- and, through x3d_pw_kernel_name /
    x3d_dw3d_kernel_name, the kernel instantiation behind every launch -- can be enumerated without a GPU
    (x3d_tf_amd/dispatch.py, tests/test_dispatch_coverage.py).  Addresses are 4 KB aligned like real allocations."""
    _next = 0x7000_0000_0000

    def __init__(self, shape, dtype, ptr=None):
        self.shape, self.dtype = tuple(shape), dtype
        self._numel = n = math.prod(self.shape)
        if ptr is None:
            ptr = _FakeBuf._next
            _FakeBuf._next += (n * torch.empty(0, dtype=dtype).element_size() + 4095) // 4096 * 4096 + 4096
        self._ptr = ptr

    def data_ptr(self):
        return self._ptr

    def numel(self):
        return self._numel

    def view(self, *shape):
        if len(shape) == 1 and isinstance(shape[0], (tuple, list, torch.Size)):
            shape = tuple(shape[0])
        return _FakeBuf(shape, self.dtype, self._ptr)

    def __getitem__(self, idx):   # only the `buf[:k]` the plan uses on flat scratch buffers
        assert isinstance(idx, slice) and idx.start is None and idx.step is None and len(self.shape) == 1
        return _FakeBuf((min(idx.stop, self._numel),), self.dtype, self._ptr)


def _p(t):
    return None if t is None else t.data_ptr()


def _view(buf, *shape):
    return buf[:math.prod(shape)].view(*shape)


# records: every field a recorder may set is declared here, so readers never probe for one ----------------------------------------
@dataclass
class BNBuf:
    """The buffers of one BatchNorm layer.  ss / mi: scale-shift and mean-invstd tables [C][2]; training plans add the fp64
    statistics (`stats`: forward sums, the library's replicated layout; `bsums`: backward sums) as accumulator handles, the
    backward coefficient table `coef` [C][4] and `count`, the elements per channel behind `stats` (set where the layer's
    finalize is recorded; read by precise_bn_table).  frozen: a layer of the trained region that normalises with its moving
    statistics (SOLVER.FREEZE_BN) -- ss / mi come from the batched eval-coefficient launch, `stats` stays None (its producer
    accumulates nothing), and the backward sums and table are kept as for any trained layer."""
    prefix: str
    c: int
    ss: Any = None
    mi: Any = None
    stats: Optional[int] = None
    bsums: Optional[int] = None
    coef: Any = None
    count: Optional[int] = None
    frozen: bool = False


@dataclass(kw_only=True)
class BlockBackward:
    """What recording a backward list decided and allocated for one block (Backward.blocks[i]).  A Block has the same fields:
    those of the plan's own backward pass (_Plan.install_backward)."""
    bwd_start: int = 0            # the block's launches are launches[bwd_start:bwd_stop]
    bwd_stop: int = 0
    dy_view: Any = None           # gradient of the block output / input, as views of the ping-pong gradient buffers
    dx_view: Any = None
    tail_folded: bool = False     # the Add + ReLU backward of THIS block ran in the `a` backward of the block above
    a_bwd_rc: bool = False        # the `a` conv / the shortcut conv run the recomputed-output backward
    r_bwd_rc: bool = False
    db: Any = None                # Dw3dBwdArgs of the depthwise backward
    nc_sums: Optional[int] = None
    g_branch: Any = None          # stochastic depth: keep * g, what the `c` backward reads (a view of Backward.gbr); None: g itself


@dataclass
class Block(BlockBackward):
    """Forward state of one residual block.  Inference plans share a_raw / b_raw / r_raw / y between blocks and have no c_raw."""
    spec: BlockSpec
    x: Any
    hh: int
    ww: int
    ho: int
    wo: int
    a_raw: Any = None
    b_raw: Any = None
    c_raw: Any = None
    r_raw: Any = None
    y: Any = None
    xs: Any = None                # even-pixel copy of x for the strided shortcut conv (option shortcut_compact)
    bn_a: Optional[BNBuf] = None
    bn_b: Optional[BNBuf] = None
    bn_c: Optional[BNBuf] = None
    bn_r: Optional[BNBuf] = None
    pool: Optional[int] = None    # SE squeeze sums (accumulator handle), gate and hidden layer
    gate: Any = None
    hidden: Any = None
    sa: Any = None                # argument structs of the a / b / c / shortcut forward launches
    sb: Any = None
    sc: Any = None
    sr: Any = None
    tail_fwd_folded: bool = False     # the residual tail was built on load by the consumer of y
    dp_keep: Optional[int] = None     # stochastic depth: address of this block's row [N] of the plan's keep table; None: never dropped


@dataclass
class Backward:
    """One recorded backward pass over a plan's forward state (record_backward): the launch list, where each stage's gradients
    are final, the scratch it owns and what it decided per block.  _Plan.install_backward makes one the plan's own; the
    differential tests record a second one with other options beside it."""
    launches: List = field(default_factory=list)
    stage_marks: Dict[int, int] = field(default_factory=dict)
    input_slots: List = field(default_factory=list)      # its launches that read the input batch (as _Plan.input_slots)
    blocks: List[BlockBackward] = field(default_factory=list)
    stem_bwd_folded: bool = False
    gbuf: Any = None              # scratch shared by all blocks (sized for the largest user)
    dv: Any = None
    ga: Any = None
    rtmp: Any = None
    gbr: Any = None               # stochastic depth: the branch gradient keep * g of the block at hand (absent with the feature off)
    coef_nc: Any = None
    se_scratch: Any = None
    g5: Any = None
    dh1: Any = None
    dpooled: Any = None
    ds: Any = None


# As a positional argument: the address of fp64 accumulator `handle`, known once the flat buffer exists (_Plan.resolve)
_Acc = collections.namedtuple("_Acc", "handle")


class _Plan:
    """Buffers + recorded launches for one (N, T, H, W, training) configuration."""

    def __init__(self, model, n, t, h, w, training, frozen_prefix=0):
        self.model = model
        self.n, self.t, self.h, self.w, self.training = n, t, h, w, bool(training)
        # a cut training plan (SOLVER.FREEZE_EVAL): units u0..u(frozen_prefix - 1) -- the stem, then blocks -- are recorded in
        # inference form, and the backward list ends at the seam, the first unit above them.  bn_eval: the form `bn` gives
        # the NEXT layer it registers (the recorder flips it at the seam); prefix_bn: the layers registered in inference form
        self.frozen_prefix = int(frozen_prefix) if training else 0
        self.bn_eval = (not self.training) or self.frozen_prefix > 0
        # SOLVER.FREEZE_BN: layers registered in TRAINING form that take their coefficients from the moving statistics all the same
        self.frozen_bn = frozenset(model.frozen_bn) if self.training else frozenset()
        self.prefix_bn: List[str] = []     # (... and those: every layer of a training plan that keeps no batch statistics)
        self.seam = None               # the output of the last prefix unit: a buffer of its own, read again by the backward pass
        self.prefix_bufs: List = []    # the ping-pong / scratch buffers the prefix units share (nothing of them outlives the prefix)
        self.fwd: List = []
        self.bwd: List = []
        self.keep: List = []           # ctypes structs / tensors that must outlive the recording
        self.lib = hip.load()
        self._zero_chunks: List = []   # (numel) fp64 accumulators carved from one flat buffer
        self._zero_views: List = []
        self._deferred: List = []      # (setter, accumulator handle): addresses to patch in once the handle has a view
        self.bwd_stage_marks: Dict[int, int] = {}
        self.backward: Optional[Backward] = None
        self.structs: Dict = {}
        self.side_entries = set()      # always empty: launches on a side stream were removed; bench.py reads it
        self.input_slots = []          # (list, index[, argument position = 0]) of the launches that read the input batch
        self.x_cl = False              # those launches read the caller's channels-last batch in place (no planar copy)
        self.blocks: List[Block] = []
        self.bn_eval_items: List = []
        self.stem_tail_folded = False  # the stem's BatchNorm + ReLU is built on load by the first block's `a` conv
        self._heads: Dict = {}         # the loss launches of a training plan recorded so far: (soft, distill) -> entry (use_soft_targets)
        self.teacher = self.kd_rows = None   # distillation: the teacher's logits [N][classes] and the KD term per row (first distilled call)
        self.row_w = None              # sample weights [N] of the step (first call that brings some)
        self.dp_keep = None            # stochastic depth: the keep table [blocks][N] of the step (training plans with a rate > 0)
        self.bn_layers: List[BNBuf] = []   # every BatchNorm layer of a training plan, as recorded (precise_bn_table)
        self._pbn_table = None
        # DETECTION.ENABLE: the head runs per box slot, K = MAX_BOXES slots per clip -- `rows` = n * K rows of
        # pooled / h1 / logits / probs / dlogits, the boxes of clip i in rows i*K .. i*K+K-1.  boxes / num_boxes are plan-owned and
        # copied into by every call; box_mask [rows] is 1 for a filled slot; roi_argmax belongs to training plans
        self.det = model.det
        self.rows = n * self.det.max_boxes if self.det else n
        self.boxes = self.num_boxes = self.box_mask = self.roi_argmax = None

    # -- allocation ------------------------------------------------------------------------------
    def act(self, *shape):
        if self.model.dry:
            return _FakeBuf(shape, self.model.dtype)
        return torch.empty(shape, dtype=self.model.dtype, device=self.model.device)

    def f32(self, *shape):
        if self.model.dry:
            return _FakeBuf(shape, torch.float32)
        return torch.empty(shape, dtype=torch.float32, device=self.model.device)

    def acc64(self, *shape):
        """fp64 accumulator zeroed at the start of every step (carved later from one flat buffer)."""
        self._zero_chunks.append((math.prod(shape), shape))
        return len(self._zero_chunks) - 1

    def carve(self, first=0):
        """One zeroed flat buffer for the accumulators from handle `first` on (they have no view yet); returns it."""
        assert first == len(self._zero_views)
        chunks = self._zero_chunks[first:]
        buf = torch.zeros(max(sum(c[0] for c in chunks), 1), dtype=torch.float64, device=self.model.device)
        off = 0
        for numel, shape in chunks:
            self._zero_views.append(buf[off:off + numel].view(shape))
            off += numel
        return buf

    def bn(self, prefix, c):
        """Buffers of a BatchNorm layer, in the form `bn_eval` names for it.  Inference form (every layer of an inference plan,
        the frozen prefix of a cut training plan): its coefficients come from the moving statistics, every such layer's in
        ONE launch at the head of the forward list (x3d_bn_eval_coef_batched over bn_eval_items); it keeps no statistics and
        is not in bn_layers.  A frozen layer of the trained region (frozen_bn) is both: coefficients as in inference form, from
        the same launch, and the backward sums and table of a trained layer -- but no forward statistics."""
        b = BNBuf(prefix, c, self.f32(c, 2), self.f32(c, 2))
        b.frozen = not self.bn_eval and prefix in self.frozen_bn
        if b.frozen:
            b.bsums = self.acc64(c, 2)
            b.coef = self.f32(c, 4)
        if not self.bn_eval and not b.frozen:
            # forward statistics: the library's replicated layout (x3d_stats_replicas copies, x3d_stats_stride apart)
            b.stats = self.acc64(self.model._stats_r * int(self.lib.x3d_stats_stride(c)))
            b.bsums = self.acc64(c, 2)
            b.coef = self.f32(c, 4)
            self.bn_layers.append(b)
        else:
            p = self.model.params
            if self.training:
                self.prefix_bn.append(prefix)
            self.bn_eval_items.append(hip.BnEvalItem(_p(p[f"{prefix}/gamma"]), _p(p[f"{prefix}/beta"]),
                                                     _p(p[f"{prefix}/moving_mean"]), _p(p[f"{prefix}/moving_variance"]),
                                                     _p(b.ss), _p(b.mi), c))
        return b

    # -- recording -------------------------------------------------------------------------------
    def rec(self, lst, name, *args):
        fn = getattr(self.lib, name)
        if fn.argtypes is not None and len(args) + 1 != len(fn.argtypes):   # (+ the stream): caught when recording, dry plans too
            raise hip.X3DHipError(f"{name}: recorded with {len(args)} arguments, the C ABI takes {len(fn.argtypes) - 1} + stream")
        conv = []
        for k, a in enumerate(args):
            if isinstance(a, (torch.Tensor, _FakeBuf)):
                self.keep.append(a)
                conv.append(a.data_ptr())
            elif isinstance(a, C.Structure):   # remember the argument struct of this launch (profiling tools read shapes from it)
                self.structs[(id(lst), len(lst))] = a
                self.keep.append(a)
                conv.append(C.byref(a))
            elif isinstance(a, _Acc):
                self._deferred.append((lambda ptr, i=len(lst), k=k: self._set_arg(lst, i, k, ptr), a.handle))
                conv.append(None)
            else:
                conv.append(a)
        lst.append((name, fn, tuple(conv)))

    @staticmethod
    def _set_arg(lst, i, k, value):
        name, fn, args = lst[i]
        lst[i] = (name, fn, args[:k] + (value,) + args[k + 1:])

    @staticmethod
    def acc(handle):
        """As a positional argument of rec(): the address of accumulator `handle` (None stays NULL)."""
        return None if handle is None else _Acc(handle)

    def defer(self, struct, **fields):
        """struct.<field> gets the address of accumulator <handle> (None: the field stays NULL).  `struct` is an argument
        struct or a host struct a launch refers to by address (x3d_bn_bwd_fold)."""
        for fname, handle in fields.items():
            if handle is not None:
                self._deferred.append((lambda ptr, f=fname: setattr(struct, f, ptr), handle))

    def resolve(self):
        """Patch in every deferred accumulator address recorded so far (all their handles have views: carve)."""
        for setter, handle in self._deferred:
            setter(self._zero_views[handle].data_ptr())
        self._deferred = []

    def precise_bn_table(self):
        """The int64 layer table [layers][PBN_COLS] of x3d_precise_bn_accum / x3d_precise_bn_final (include/x3d_hip.h) for
        this training plan, built with the first call and kept on the model's device (a dry plan: on the host, with the
        addresses of its stand-in accumulators).  Rows follow model.precise_bn_layout() -- the same for every plan of the
        model -- and add what belongs to this plan: where each layer's `stats` lies and how many elements per channel one
        forward pass sums into it.  The kernels trust the table, so it is checked here: ValueError for a layer the plan did
        not register exactly once, or registered without `stats` or `count`, and for a channel count or an accumulator size
        that disagrees with the layout."""
        if self._pbn_table is not None:
            return self._pbn_table
        if not self.training:
            raise ValueError("precise_bn_table: only a training plan accumulates BatchNorm statistics")
        lay = self.model.precise_bn_layout()
        by_prefix = {}
        for b in self.bn_layers:
            if b.prefix in by_prefix:
                raise ValueError(f"precise_bn_table: BatchNorm layer {b.prefix} registered twice")
            by_prefix[b.prefix] = b
        # (a cut plan: rows for the layers of the trained region only -- the prefix keeps no statistics and its moving
        # statistics are not to be touched.  Row r's count slot is pooled[r], r < len(rows) <= layers, and every layer's sums
        # lie at its layout offset >= layers: slots and sums cannot overlap, whichever subset a plan has)
        want_layers = [q for q in lay.prefixes if q not in set(self.prefix_bn)]
        if sorted(by_prefix) != sorted(want_layers) or len(want_layers) + len(self.prefix_bn) != len(lay.prefixes):
            odd = sorted(set(by_prefix) ^ set(want_layers))
            raise ValueError(f"precise_bn_table: the plan's BatchNorm layers are not the model's: {odd}")
        if not want_layers or min(lay.pooled_offsets) < len(lay.prefixes):
            raise ValueError("precise_bn_table: no BatchNorm layer to recompute, or pooled sums that overlap the count slots")
        rows = []
        for l, prefix in enumerate(lay.prefixes):
            if prefix not in by_prefix:
                continue
            b = by_prefix[prefix]
            if b.stats is None or b.count is None:
                raise ValueError(f"precise_bn_table: {prefix} has no {'stats' if b.stats is None else 'count'}")
            view = self._zero_views[b.stats] if b.stats < len(self._zero_views) else None
            want = self.model._stats_r * int(self.lib.x3d_stats_stride(b.c))
            if b.c != lay.channels[l] or b.count < 1 or view is None or view.numel() != want:
                raise ValueError(f"precise_bn_table: {prefix}: C = {b.c} (layout {lay.channels[l]}), count = {b.count}, "
                                 f"accumulator of {None if view is None else view.numel()} doubles (needs {want})")
            row = [0] * hip.PBN_COLS
            row[hip.PBN_STATS], row[hip.PBN_C], row[hip.PBN_COUNT] = view.data_ptr(), b.c, b.count
            row[hip.PBN_MEAN], row[hip.PBN_VAR], row[hip.PBN_POOLED] = lay.mean_offsets[l], lay.var_offsets[l], lay.pooled_offsets[l]
            rows.append(row)
        self._pbn_table = torch.tensor(rows, dtype=torch.int64).to(self.model.device)
        return self._pbn_table

    def install_backward(self, bw: Backward):
        self.backward, self.bwd, self.bwd_stage_marks = bw, bw.launches, bw.stage_marks
        self.input_slots += bw.input_slots
        self.stem_bwd_folded, self.se_scratch = bw.stem_bwd_folded, bw.se_scratch
        for B, r in zip(self.blocks, bw.blocks):
            vars(B).update(vars(r))

    def use_soft_targets(self, soft: bool, distill: bool = False, weighted=None, row_w: bool = False):
        """Which loss the head slot (fwd[grad_scale_slot]) of a training plan holds.  Single-label plans: x3d_softmax_xent on
        `labels`, as recorded, or x3d_softmax_xent_soft on the dense rows in `targets`.  The targets buffer and the second
        entry come into being with the first soft call, so a plan that never sees soft targets allocates nothing for them.
        distill: the knowledge-distillation form of that loss instead -- x3d_softmax_xent_kd on `labels` or on `targets`,
        x3d_sigmoid_bce_kd for a multi-label plan (whose one hard head takes no `soft`) -- reading the teacher's logits from
        `teacher` and writing the KD term per row to `kd_rows`; both buffers and the entries likewise come into being with
        the first distilled call.  weighted (None: whether the model has loss modifiers, X3D.set_loss): the _w entry point of
        the head -- x3d_softmax_xent_w / x3d_sigmoid_bce_w -- which covers all of the above; row_w: the step brings sample
        weights, and `row_w` [N] comes into being with the first such call (it implies weighted).  The scalars of a recorded
        entry (grad_scale, alpha, temperature, the gammas) are placeholders: the model launches the slot's entry point with
        the step's own (head_launch)."""
        m = self.model
        if weighted is None:
            weighted = m.loss_mods is not None
        weighted = bool(weighted) or bool(row_w)
        key = (bool(soft) and not m.multi_label, bool(distill)) + (("w",) if weighted else ())
        if row_w and self.row_w is None:
            self.row_w = self.f32(self.rows)
        if key not in self._heads:
            if key[0] and self.targets is None:
                self.targets = torch.zeros(self.rows, m.num_classes, dtype=torch.float32, device=m.device)
            if key[1] and self.teacher is None:
                self.teacher, self.kd_rows = self.f32(self.n, m.num_classes), self.f32(self.n)
            tmp = []
            name, args = self.head_launch(*key[:2], grad_scale=1.0 / self.n, weighted=weighted)
            self.rec(tmp, name, *args)
            self._heads[key] = tmp[0]
        self.fwd[self.grad_scale_slot] = self._heads[key]

    def head_launch(self, soft: bool, distill: bool, grad_scale, alpha=0.5, temperature=1.0, weighted=False, row_w=False):
        """(entry point, its arguments without the stream) of the loss of a training plan: the one place that says which of
        the seven a step runs and in which order it takes the plan's buffers and the scalars.  `soft` counts for single-label
        plans only; the buffers the choice needs exist (use_soft_targets).  weighted: the _w entry point of the head with the
        model's tables and gammas (X3D.set_loss; none: NULL tables, gamma 0) and, with row_w, the plan's sample weights."""
        m = self.model
        soft = bool(soft) and not m.multi_label
        ptr = hip.ptr
        size = (self.rows, m.num_classes)
        labels, targets = (None, ptr(self.targets)) if soft or m.multi_label else (ptr(self.labels), None)
        if weighted or row_w:
            mods = m.loss_mods or NO_LOSS_MODS
            kd = (ptr(self.teacher), ptr(self.kd_rows), alpha, temperature) if distill else (None, None, 0.0, 1.0)
            rw = ptr(self.row_w) if row_w else None
            outs = (ptr(self.probs), ptr(self.loss_rows), kd[1], ptr(self.dlogits), grad_scale)
            if m.multi_label:
                return "x3d_sigmoid_bce_w", (ptr(self.logits), kd[0], targets, ptr(mods.class_w), ptr(mods.pos_w), rw, *outs,
                                             mods.gamma, mods.gamma_neg, kd[2], kd[3], *size)
            return "x3d_softmax_xent_w", (ptr(self.logits), kd[0], labels, targets, ptr(mods.class_w), rw, *outs, mods.gamma,
                                          kd[2], kd[3], *size)
        if distill:
            given = (targets,) if m.multi_label else (labels, targets)
            return "x3d_sigmoid_bce_kd" if m.multi_label else "x3d_softmax_xent_kd", (
                ptr(self.logits), ptr(self.teacher), *given, ptr(self.probs), ptr(self.loss_rows), ptr(self.kd_rows),
                ptr(self.dlogits), grad_scale, alpha, temperature, *size)
        name = "x3d_sigmoid_bce" if m.multi_label else "x3d_softmax_xent_soft" if soft else "x3d_softmax_xent"
        return name, (ptr(self.logits), targets if labels is None else labels, ptr(self.probs), ptr(self.loss_rows),
                      ptr(self.dlogits), grad_scale, *size)

    def run(self, lst, start=0, stop=None):
        if self.model.dry:
            raise hip.X3DHipError("a dry plan records launches; it cannot run (no CPU fallback for the hot path)")
        s = torch.cuda.current_stream().cuda_stream
        for name, fn, args in lst[start:stop]:
            st = fn(*args, s)
            if st != 0:
                hip.check(st, name)


# forward: what the training and the inference recorder share ----------------------------------------
def _geometry(arch, h, w):
    """(stem output h, w; per block (input h, w, output h, w))"""
    h1, w1 = (h - 1) // 2 + 1, (w - 1) // 2 + 1
    geo, hh, ww = [], h1, w1
    for b in arch.blocks:
        ho, wo = same_pad(hh, 3, b.stride)[0], same_pad(ww, 3, b.stride)[0]
        geo.append((hh, ww, ho, wo))
        hh, ww = ho, wo
    return h1, w1, geo


def _bind_stem_input(model, pl, dt):
    """Where the stem reads the batch from, and whether it runs as x3d_stem_fwd / x3d_stem_bwd (one launch each way): that
    needs the in-place channels-last input (pl.x_cl) and a shape the fused kernels take (x3d_stem_fused_supported: bit 0
    forward, bit 1 backward -- a plan whose backward pass reaches the stem needs both, since the fused forward stores no
    conv_s output; a cut training plan's does not); the two-kernel path otherwise."""
    a, n, t, h, w = model.arch, pl.n, pl.t, pl.h, pl.w
    # 16-bit storage: the stem's matrix-core kernels read the caller's channels-last batch in place (x3d_hip.h K1)
    pl.x_cl = bool(pl.lib.x3d_stem_s_nthwc_supported(model.in_channels, w, a.c1, dt)) and model.opt["stem_nthwc"]
    pl.x = None if pl.x_cl else pl.act(n, model.in_channels, t, h, w)
    pl.stem_fused = False
    if pl.x_cl and model.opt["stem_fused"]:
        need = 3 if pl.training and pl.frozen_prefix == 0 else 1
        have = pl.lib.x3d_stem_fused_supported(model.in_channels, a.c1, a.c1_temp_filter, n, t, h, w, dt, 1)
        pl.stem_fused = (have & need) == need


def _rec_stem(model, pl, y, stats, ss, act, dt):
    """conv_s -> conv_t into y, with the BatchNorm statistics (training) or BN + ReLU (inference: ss, act) in the epilogue."""
    a, p, F = model.arch, model.params, pl.fwd
    n, t, h, w = pl.n, pl.t, pl.h, pl.w
    pl.input_slots.append((F, len(F)))     # (the launch reads the caller's batch in place when pl.x_cl: _bind_input)
    if pl.stem_fused:   # one launch: the conv_s output stays on chip (reference model.py:202-208)
        pl.rec(F, "x3d_stem_fwd", pl.x, p["conv1/conv_s/kernel"], p["conv1/conv_t/kernel"], y, pl.acc(stats), ss, act,
               n, model.in_channels, t, h, w, a.c1, a.c1_temp_filter, dt, 1)
    else:
        pl.rec(F, "x3d_stem_s_fwd", pl.x, p["conv1/conv_s/kernel"], pl.s_raw, n, model.in_channels, t, h, w, a.c1, dt, int(pl.x_cl))
        pl.rec(F, "x3d_dwt_fwd", pl.s_raw, p["conv1/conv_t/kernel"], y, pl.acc(stats), ss, act, n, a.c1, t,
               y.shape[3] * y.shape[4], a.c1_temp_filter, dt)


def _a_conv_args(model, pl, B, dt):
    """x3d_pw_fwd arguments of the `a` conv (1x1x1 on the block input, raw output)."""
    b, q = B.spec, f"{block_prefix(B.spec)}/bottleneck"
    sa = hip.PwFwdArgs(_p(B.x), _p(model.params[f"{q}/a/kernel"]), _p(B.a_raw), None, None, None, ACT_NONE, pl.n, b.cin,
                       b.inner, pl.t, B.hh, B.ww, 1, dt)
    sa.w_panel = model._wp(f"{q}/a/kernel")
    return sa


def _rec_dw(pl, lst, entry, st):
    """One channelwise 3x3x3 launch: the entry point itself, or -- a struct tagged with a dilation >= 2 (NETWORK.RES5_DILATION) -- its
    dilated form, which takes the dilation behind the struct.  An undilated block records what it always recorded."""
    d = hip.dw3d_dilation(st)
    if d > 1:
        pl.rec(lst, entry + "_dil", st, d)
    else:
        pl.rec(lst, entry, st)


def _rec_se(model, pl, B):
    b, p, q = B.spec, model.params, f"{block_prefix(B.spec)}/bottleneck"
    pl.rec(pl.fwd, "x3d_se_fwd", pl.acc(B.pool), float(pl.t * B.ho * B.wo), B.bn_b.ss, p[f"{q}/se_fc1/kernel"],
           p[f"{q}/se_fc1/bias"], p[f"{q}/se_fc2/kernel"], p[f"{q}/se_fc2/bias"], B.gate, B.hidden, pl.n,
           b.inner, b.se_width)


def _rec_shortcut_conv(model, pl, B, dt):
    """The shortcut conv of a stage's first block into B.r_raw (raw; training: with the BN_r statistics)."""
    b, p, F, n, t = B.spec, model.params, pl.fwd, pl.n, pl.t
    pre = block_prefix(b)
    B.bn_r = pl.bn(f"{pre}/bn_r", b.cout)
    if b.stride == 2 and B.wo % 2 == 1 and model.opt["shortcut_compact"]:
        # the pixels the strided conv samples (reference model.py:360-367), copied once per step: the conv's forward and
        # both of its gradients are then dense launches -- 16-byte coalesced rows instead of one output per 4-byte load.
        # Only where the gather is at its worst (odd output rows): measured per launch on X3D-M (profiles/
        # r06_ab_shortcut_compact.txt) the copy costs what the dense launches save at 112 / 56 / 28-wide inputs
        # (108 + 39 + 25 us against -111 / -43 / -32) and a quarter of it at 14 -> 7 (15 against -68)
        B.xs = pl.act(n, b.cin, t, B.ho, B.wo)
        pl.rec(F, "x3d_subsample2", B.x, B.xs, n * b.cin * t, B.hh, B.ww, dt)
    x_r, geom = (B.xs, (B.ho, B.wo, 1)) if B.xs is not None else (B.x, (B.hh, B.ww, b.stride))
    sr = hip.PwFwdArgs(_p(x_r), _p(p[f"{pre}/residual/kernel"]), _p(B.r_raw), None, None, None, ACT_NONE,
                       n, b.cin, b.cout, t, *geom, dt)
    sr.w_panel = model._wp(f"{pre}/residual/kernel")
    B.sr = sr
    pl.defer(sr, stats=B.bn_r.stats)
    pl.rec(F, "x3d_pw_fwd", sr)


def _conv5_args(model, pl, x_cur, hh, ww, dt):
    a, n, t = model.arch, pl.n, pl.t
    pl.P5, pl.h5, pl.w5 = t * hh * ww, hh, ww
    pl.y_last = x_cur
    s5 = hip.PwFwdArgs(_p(x_cur), _p(model.params["conv5/layer_with_weights-0/kernel"]), _p(pl.c5_raw), None, None, None,
                       ACT_NONE, n, a.stages[-1].cout, a.conv5_out, t, hh, ww, 1, dt)
    s5.w_panel = model._wp("conv5/layer_with_weights-0/kernel")
    return s5


def _rec_head_dense(model, pl, dt):
    """pool of relu(bn5(conv5)) -> fc1 -> [dropout] -> fc2: logits"""
    a, p, F, c5 = model.arch, model.params, pl.fwd, model.arch.conv5_out
    n = pl.rows                                  # (DETECTION.ENABLE: one row per box slot)
    pl.pooled = pl.f32(n, c5)
    pl.h1 = pl.f32(n, a.fc1_out)
    pl.logits = pl.f32(n, a.num_classes)
    pl.probs = pl.f32(n, a.num_classes)
    if pl.det:
        _rec_roi_pool(model, pl, dt)
    else:
        pl.rec(F, "x3d_pool_fwd", pl.c5_raw, pl.bn5.ss, pl.pooled, n, c5, pl.P5, dt)
    pl.rec(F, "x3d_dense_fwd", pl.pooled, None, 1.0, p["fc1/kernel"], None, pl.h1, ACT_RELU, n, c5, a.fc1_out)
    use_drop = pl.training and a.dropout_rate > 0
    pl.drop_mask = pl.f32(n, a.fc1_out) if use_drop else None
    pl.drop_scale = 1.0 / (1.0 - a.dropout_rate) if use_drop else 1.0
    pl.rec(F, "x3d_dense_fwd", pl.h1, pl.drop_mask, float(pl.drop_scale), p["fc2/kernel"], p["fc2/bias"],
           pl.logits, ACT_NONE, n, a.fc1_out, a.num_classes)


def _roi_args(pl):
    """(N, C, T, H, W, K, R, sampling_ratio, spatial_scale) as both ROI entry points take them"""
    d = pl.det
    return (pl.n, pl.model.arch.conv5_out, pl.t, pl.h5, pl.w5, d.max_boxes, d.resolution, d.sampling_ratio,
            1.0 / d.spatial_scale_factor)


def _rec_roi_pool(model, pl, dt):
    """x3d_roi_pool_fwd in the place of x3d_pool_fwd: pl.pooled [n * K, c5] from the plan's own boxes [n, K, 4] / num_boxes [n]
    (the model copies the caller's into them; all slots empty until then).  The shape limits are the kernel's: stated here,
    before anything is launched."""
    from .ops import roi_limits
    d, n = pl.det, pl.n
    roi_limits("DETECTION", n, pl.h5 * pl.w5, d.max_boxes, d.resolution, d.sampling_ratio, 1.0 / d.spatial_scale_factor)
    pl.boxes, pl.box_mask = pl.f32(n, d.max_boxes, 4), pl.f32(pl.rows)
    if model.dry:
        pl.num_boxes = _FakeBuf((n,), torch.int32)
        pl.roi_argmax = _FakeBuf((pl.rows, model.arch.conv5_out), torch.uint8) if pl.training else None
    else:
        pl.boxes.zero_()
        pl.box_mask.zero_()
        pl.num_boxes = torch.zeros(n, dtype=torch.int32, device=model.device)
        pl.roi_argmax = torch.zeros(pl.rows, model.arch.conv5_out, dtype=torch.uint8, device=model.device) if pl.training else None
    pl.rec(pl.fwd, "x3d_roi_pool_fwd", pl.c5_raw, pl.bn5.ss, pl.boxes, pl.num_boxes, pl.pooled, pl.roi_argmax, *_roi_args(pl), dt)


def _rec_infer_head(model, pl):
    """probabilities of the logits (softmax, or sigmoid with DATA.MULTI_LABEL), then the views x crops of every video
    combined by TEST.ENSEMBLE_METHOD (mean, or element-wise max) into pl.out [n / num_preds, classes]"""
    a, F, n = model.arch, pl.fwd, pl.rows        # (DETECTION.ENABLE: num_preds is 1, pl.out has a row per box slot)
    pl.rec(F, "x3d_sigmoid_bce" if model.multi_label else "x3d_softmax_xent", pl.logits, None, pl.probs, None, None, 1.0, n,
           a.num_classes)
    pl.out = pl.f32(n // a.num_preds, a.num_classes)
    views = "x3d_view_max" if model.ensemble_method == "max" else "x3d_view_mean"
    pl.rec(F, views, pl.probs, pl.out, n // a.num_preds, a.num_preds, a.num_classes)


# forward, inference ----------------------------------------
def record_inference(model, n, t, h, w, probs=True) -> _Plan:
    """The forward pass at training=False (reference model.py:113-127; eval.py:83-89) as its own launch list.
    probs=False (X3D.logits): the same list without its last two launches -- it ends with fc2, pl.logits [n, classes] is the
    result, and n need not be a multiple of views * crops since no views are combined.

    With the moving statistics every BatchNorm is a per-channel affine known before the first kernel, so nothing
    waits for batch statistics and the training plan's materialised intermediates disappear:
      stem     conv_s -> conv_t with BN + ReLU in its epilogue (x3d_dwt_fwd out_scale_shift): no raw t tensor, no tail
      block    a (raw) -> b (BN_a + ReLU on load; SE squeeze in the epilogue) -> [SE MLP] -> [strided shortcut conv (raw)]
               -> c with BN_b * gate -> swish on load and  relu(bn_c(acc) + shortcut)  in its epilogue
               (x3d_pw_fwd out_scale_shift / out_add / out_add_scale_shift): no c_raw, no residual-tail pass
      head     conv5 (raw) -> pool of relu(bn(.)) -> fc1 -> fc2 -> softmax -> view mean
    3 launches per block (4 with SE, +1 for a stage's first block) instead of 4-6, and 2 tensor passes of Cout*P less
    per block.  The per-layer coefficients still come from ONE batched launch at the head of the list (they depend on
    the parameters only, but parameters may change between calls).  Activation buffers are shared between blocks
    (two block outputs ping-pong; one a / b / shortcut scratch each), so a 30-view X3D-XL plan holds ~3 GB, not ~30."""
    a = model.arch
    pl = _Plan(model, n, t, h, w, False)
    dt = hip.dtype_code(model.dtype)
    F = pl.fwd
    if probs and n % a.num_preds:
        raise ValueError(f"inference batch {n} is not a multiple of views*crops={a.num_preds} "
                         "(reference model.py:125)")
    F.append(None)   # slot 0: x3d_bn_eval_coef_batched, filled in once every BN layer is known
    # ---- geometry first: the shared buffers are sized for their largest user ----------------------------------
    h1, w1, geo = _geometry(a, h, w)
    numel_y = max([n * a.c1 * t * h1 * w1] + [n * b.cout * t * g[2] * g[3] for b, g in zip(a.blocks, geo)])
    numel_a = max(n * b.inner * t * g[0] * g[1] for b, g in zip(a.blocks, geo))
    numel_b = max(n * b.inner * t * g[2] * g[3] for b, g in zip(a.blocks, geo))
    numel_r = max([1] + [n * b.cout * t * g[2] * g[3] for b, g in zip(a.blocks, geo) if b.has_shortcut_conv])
    ybuf = [pl.act(numel_y), pl.act(numel_y)]
    abuf, bbuf, rbuf = pl.act(numel_a), pl.act(numel_b), pl.act(numel_r)
    # ---- input + stem ------------------------------------------------------------------------------------------
    _bind_stem_input(model, pl, dt)
    pl.y0 = _view(ybuf[0], n, a.c1, t, h1, w1)
    pl.bn1 = pl.bn("conv1/bn", a.c1)
    pl.s_raw = None if pl.stem_fused else _view(abuf, n, a.c1, t, h1, w1)   # conv_s output: dead once conv_t has run, shares the `a` scratch
    _rec_stem(model, pl, pl.y0, None, pl.bn1.ss, ACT_RELU, dt)
    # ---- residual stages ---------------------------------------------------------------------------------------
    x_cur, cur = pl.y0, 0
    for b, (hh, ww, ho, wo) in zip(a.blocks, geo):
        B = Block(b, x_cur, hh, ww, ho, wo, a_raw=_view(abuf, n, b.inner, t, hh, ww), b_raw=_view(bbuf, n, b.inner, t, ho, wo),
                  y=_view(ybuf[1 - cur], n, b.cout, t, ho, wo),
                  r_raw=_view(rbuf, n, b.cout, t, ho, wo) if b.has_shortcut_conv else None)
        _rec_infer_block(model, pl, B, dt)
        pl.blocks.append(B)
        x_cur, cur = B.y, 1 - cur
    # ---- head --------------------------------------------------------------------------------------------------
    hh, ww = geo[-1][2], geo[-1][3]
    c5 = a.conv5_out
    pl.c5_raw = _view(abuf, n, c5, t, hh, ww) if n * c5 * t * hh * ww <= numel_a else pl.act(n, c5, t, hh, ww)
    pl.bn5 = pl.bn("conv5/layer_with_weights-1", c5)
    pl.s5 = _conv5_args(model, pl, x_cur, hh, ww, dt)
    pl.rec(F, "x3d_pw_fwd", pl.s5)
    _rec_head_dense(model, pl, dt)
    pl.out = None
    if probs:
        _rec_infer_head(model, pl)
    items = (hip.BnEvalItem * len(pl.bn_eval_items))(*pl.bn_eval_items)
    pl.bn_eval_table = torch.frombuffer(bytearray(bytes(items)), dtype=torch.uint8).to(model.device)
    F[0] = ("x3d_bn_eval_coef_batched", pl.lib.x3d_bn_eval_coef_batched,
            (pl.bn_eval_table.data_ptr(), len(pl.bn_eval_items), float(a.bn_eps)))
    pl.zero_buf = pl.carve()
    pl.resolve()
    return pl


def _rec_infer_block(model, pl, B, dt):
    b, p, F, n, t = B.spec, model.params, pl.fwd, pl.n, pl.t
    q = f"{block_prefix(b)}/bottleneck"
    B.bn_a, B.bn_b, B.bn_c = pl.bn(f"{q}/bn_a", b.inner), pl.bn(f"{q}/bn_b", b.inner), pl.bn(f"{q}/bn_c", b.cout)
    B.pool = pl.acc64(n, b.inner) if b.has_se else None
    B.gate = pl.f32(n, b.inner) if b.has_se else None
    B.hidden = pl.f32(n, b.se_width) if b.has_se else None
    B.sa = _a_conv_args(model, pl, B, dt)
    pl.rec(F, "x3d_pw_fwd", B.sa)
    B.sb = hip.dilated(hip.Dw3dFwdArgs(_p(B.a_raw), _p(p[f"{q}/b/kernel"]), _p(B.b_raw), _p(B.bn_a.ss), ACT_RELU, None, None,
                                       n, b.inner, t, B.hh, B.ww, b.stride, dt), b.dilation)
    pl.defer(B.sb, pool=B.pool)
    _rec_dw(pl, F, "x3d_dw3d_fwd", B.sb)
    if b.has_se:
        _rec_se(model, pl, B)
    if b.has_shortcut_conv:
        _rec_shortcut_conv(model, pl, B, dt)
        add, add_ss = B.r_raw, B.bn_r.ss
    else:
        add, add_ss = B.x, None
    # c: BN_b * gate -> swish on load; relu(bn_c(acc) + shortcut) on the accumulators
    B.sc = hip.PwFwdArgs(_p(B.b_raw), _p(p[f"{q}/c/kernel"]), _p(B.y), None, _p(B.bn_b.ss), _p(B.gate),
                         ACT_SWISH, n, b.inner, b.cout, t, B.ho, B.wo, 1, dt, model._wp(f"{q}/c/kernel"),
                         out_scale_shift=_p(B.bn_c.ss), out_add=_p(add), out_add_scale_shift=_p(add_ss), out_act=ACT_RELU)
    pl.rec(F, "x3d_pw_fwd", B.sc)


# forward, training ----------------------------------------
# A residual tail y = relu(bn_c(c_raw) + shortcut) (shortcut raw with its own BatchNorm r_ss, or activated) that no launch
# has built yet
# (keep: the block's row of the stochastic-depth table -- such a tail is never folded, x3d_tail_fwd_dp builds it)
_Tail = collections.namedtuple("_Tail", "c_raw c_ss shortcut r_ss y cout p_out keep", defaults=(None,))


def record_training(model, n, t, h, w, frozen_prefix=0) -> _Plan:
    """Forward list up to the loss, then the backward list.  Per block: a (raw + BN_a statistics) -> finalize -> b (BN_a + ReLU
    on load, BN_b statistics + SE squeeze in the epilogue) -> finalize -> [SE MLP] -> c (BN_b * gate -> swish on load) ->
    finalize -> [shortcut conv -> finalize]; the residual tail is left to the first reader of the block output.

    frozen_prefix = k > 0 (SOLVER.FREEZE_EVAL, finetune.frozen_prefix): a CUT plan.  Units u0..u(k-1) -- the stem, then the
    first k - 1 blocks -- are recorded with the inference recorder's launches (_rec_frozen_prefix); the first trained unit
    (block k - 1, or conv5 for k = blocks + 1) reads their output, the seam tensor, as a materialised, activated input;
    everything above is recorded as always, and the backward list ends at that unit (record_backward first_unit = k)."""
    a = model.arch
    k = int(frozen_prefix)
    if not 0 <= k <= len(a.blocks) + 1:
        raise ValueError(f"frozen_prefix must lie in [0, {len(a.blocks) + 1}] (the stem and {len(a.blocks)} blocks), "
                         f"not {frozen_prefix!r}")
    pl = _Plan(model, n, t, h, w, True, k)
    dt = hip.dtype_code(model.dtype)
    F = pl.fwd
    if k or pl.frozen_bn:
        F.append(None)   # slot 0: x3d_bn_eval_coef_batched over the prefix layers and the frozen layers above them, filled in below
    # ---- input + stem --------------------------------------------------------------------
    _bind_stem_input(model, pl, dt)
    h1, w1, geo = _geometry(a, h, w)
    if k:
        x_cur, tail = _rec_frozen_prefix(model, pl, k, h1, w1, geo, dt), None
    else:
        x_cur, tail = _rec_train_stem(model, pl, h1, w1, dt)
    # ---- residual stages -------------------------------------------------------------------
    # The residual tail of a block (y = relu(bn_c(c) + shortcut), reference model.py:381-392) is DEFERRED to the first
    # reader of y: the next block's `a` conv (or conv5) builds y on load and stores it (x3d_pw_fwd in_add / in_store) where
    # that form exists and does not cost the layer its weights-stationary kernel; otherwise x3d_tail_fwd runs first.
    # Stochastic depth (NETWORK.DROP_PATH_RATE): blocks with a rate > 0 scale bn_c's output by keep[l][n] -- 0, or 1 / (1 - rate_l)
    # -- in their residual tail.  The table [blocks][N] is drawn anew on the device before every replay (x3d_drop_path_draw,
    # model._draw_drop_path), so the lists themselves never change.  With every rate 0 nothing below differs from before.
    rates = model.drop_path_rates
    if any(r > 0.0 for r in rates):
        pl.dp_keep = pl.f32(len(a.blocks), n)
        if not model.dry:
            pl.dp_keep.fill_(1.0)
    for (l, b), (hh, ww, ho, wo) in zip(enumerate(a.blocks), geo):
        if l + 1 < k:          # a block of the frozen prefix: recorded above, never dropped
            continue
        B = Block(b, x_cur, hh, ww, ho, wo)
        if rates[l] > 0.0:
            B.dp_keep = pl.dp_keep.data_ptr() + 4 * n * l
        tail = _rec_train_block(model, pl, B, tail, dt)
        pl.blocks.append(B)
        x_cur = B.y
    # ---- head ------------------------------------------------------------------------------
    hh, ww = geo[-1][2], geo[-1][3]
    pl.c5_raw = pl.act(n, a.conv5_out, t, hh, ww)
    pl.bn5 = pl.bn("conv5/layer_with_weights-1", a.conv5_out)
    pl.s5 = _conv5_args(model, pl, x_cur, hh, ww, dt)
    if tail is not None:       # (None: conv5 reads the seam tensor of a cut plan)
        pl.s5 = _fold_pending_tail(model, pl, pl.s5, tail, dt)
    pl.defer(pl.s5, stats=pl.bn5.stats)
    pl.rec(F, "x3d_pw_fwd", pl.s5)
    _rec_bn_finalize(model, pl, pl.bn5, n * pl.P5)
    _rec_head_dense(model, pl, dt)
    pl.loss_rows = pl.f32(pl.rows)
    pl.dlogits = pl.f32(pl.rows, a.num_classes)
    pl.grad_scale_slot = len(F)
    if model.multi_label:
        pl.labels = None
        pl.targets = torch.zeros(pl.rows, a.num_classes, dtype=torch.float32, device=model.device)
    else:
        pl.labels = torch.zeros(pl.rows, dtype=torch.int32, device=model.device)
        pl.targets = None                  # soft targets: allocated by the first call that brings some (use_soft_targets)
    F.append(None)
    pl.use_soft_targets(False)             # x3d_sigmoid_bce on targets / x3d_softmax_xent on labels
    pl.install_backward(record_backward(model, pl, model.opt, first_unit=k))
    if F[0] is None:
        items = (hip.BnEvalItem * len(pl.bn_eval_items))(*pl.bn_eval_items)
        pl.bn_eval_table = torch.frombuffer(bytearray(bytes(items)), dtype=torch.uint8).to(model.device)
        F[0] = ("x3d_bn_eval_coef_batched", pl.lib.x3d_bn_eval_coef_batched,
                (pl.bn_eval_table.data_ptr(), len(pl.bn_eval_items), float(a.bn_eps)))
    pl.zero_buf = pl.carve()
    pl.resolve()
    return pl


def _rec_train_stem(model, pl, h1, w1, dt):
    """The stem in training form; returns (its output buffer, its pending BatchNorm + ReLU as a _Tail)."""
    a, n, t = model.arch, pl.n, pl.t
    # conv_s -> conv_t as one launch each way where the fused kernels take the shape: the conv_s output (616 MB at the
    # headline's size) and its gradient never exist in HBM (reference model.py:202-206: nothing between the two convs)
    pl.s_raw = None if pl.stem_fused else pl.act(n, a.c1, t, h1, w1)
    pl.t_raw = pl.act(n, a.c1, t, h1, w1)
    pl.y0 = pl.act(n, a.c1, t, h1, w1)
    pl.bn1 = pl.bn("conv1/bn", a.c1)
    _rec_stem(model, pl, pl.t_raw, pl.bn1.stats, None, ACT_NONE, dt)
    _rec_bn_finalize(model, pl, pl.bn1, n * t * h1 * w1)
    return pl.y0, _Tail(pl.t_raw, pl.bn1.ss, None, None, pl.y0, a.c1, t * h1 * w1)     # the stem's BatchNorm + ReLU (no Add)


def _rec_frozen_prefix(model, pl, k, h1, w1, geo, dt):
    """The frozen prefix of a cut training plan, units u0..u(k-1), as record_inference records them: the stem with BN + ReLU in
    its epilogue, blocks through _rec_infer_block, every BatchNorm a per-channel affine from the moving statistics (one
    x3d_bn_eval_coef_batched at slot 0 of the list, over these layers only: record_training fills it in), no statistics, no
    c_raw, no residual-tail pass.  Unit outputs ping-pong between two buffers and the a / b / shortcut scratch is shared,
    all sized for the prefix's largest user -- except the output of the LAST prefix unit, the seam tensor: the weight-gradient
    launches of the first trained unit read it again during the backward pass, so it has a buffer of its own (pl.seam) that
    nothing later writes.  Returns it, shaped."""
    a, n, t, F = model.arch, pl.n, pl.t, pl.fwd
    assert pl.bn_eval and F == [None]   # slot 0: x3d_bn_eval_coef_batched over the prefix layers (record_training reserved it)
    units = list(zip(a.blocks, geo))[:k - 1]
    outs = [(a.c1, h1, w1)] + [(b.cout, g[2], g[3]) for b, g in units]          # (channels, h, w) of every prefix unit's output
    pl.seam = pl.act(n, outs[-1][0], t, outs[-1][1], outs[-1][2])
    numel_y = max([0] + [n * c * t * hh * ww for c, hh, ww in outs[:-1]])
    ybuf = [pl.act(numel_y) for _ in range(min(len(outs) - 1, 2))]
    numel_a = max([0 if pl.stem_fused else n * a.c1 * t * h1 * w1] + [n * b.inner * t * g[0] * g[1] for b, g in units])
    numel_b = max([0] + [n * b.inner * t * g[2] * g[3] for b, g in units])
    numel_r = max([0] + [n * b.cout * t * g[2] * g[3] for b, g in units if b.has_shortcut_conv])
    abuf, bbuf, rbuf = (pl.act(m) if m else None for m in (numel_a, numel_b, numel_r))
    pl.prefix_bufs = ybuf + [buf for buf in (abuf, bbuf, rbuf) if buf is not None]

    def out_view(i):
        c, hh, ww = outs[i]
        return pl.seam if i == len(outs) - 1 else _view(ybuf[i % 2], n, c, t, hh, ww)

    pl.t_raw = None      # (the stem's raw output is never stored: BN + ReLU in the epilogue)
    pl.y0 = out_view(0)
    pl.bn1 = pl.bn("conv1/bn", a.c1)
    pl.s_raw = None if pl.stem_fused else _view(abuf, n, a.c1, t, h1, w1)   # conv_s output: dead once conv_t has run
    _rec_stem(model, pl, pl.y0, None, pl.bn1.ss, ACT_RELU, dt)
    x_cur = pl.y0
    for i, (b, (hh, ww, ho, wo)) in enumerate(units):
        B = Block(b, x_cur, hh, ww, ho, wo, a_raw=_view(abuf, n, b.inner, t, hh, ww), b_raw=_view(bbuf, n, b.inner, t, ho, wo),
                  y=out_view(i + 1), r_raw=_view(rbuf, n, b.cout, t, ho, wo) if b.has_shortcut_conv else None)
        _rec_infer_block(model, pl, B, dt)
        pl.blocks.append(B)
        x_cur = B.y
    pl.bn_eval = False   # the seam: every layer registered from here on keeps batch statistics
    return x_cur


def _rec_bn_finalize(model, pl, b: BNBuf, count):
    """after the producer kernel: turn the batch statistics into scale / shift (and update the moving statistics).  A frozen
    layer: no launch -- its coefficients are in place since slot 0, its moving statistics are not to be touched"""
    p, a = model.params, model.arch
    b.count = int(count)
    if b.frozen:
        return
    pl.rec(pl.fwd, "x3d_bn_finalize", pl.acc(b.stats), float(count), p[f"{b.prefix}/gamma"], p[f"{b.prefix}/beta"],
           p[f"{b.prefix}/moving_mean"], p[f"{b.prefix}/moving_variance"], float(a.bn_eps), float(a.bn_momentum), 1,
           b.ss, b.mi, b.c)


def _fold_pending_tail(model, pl, st, tl: _Tail, dt):
    """st: the x3d_pw_fwd arguments of the conv that reads the pending block output first.  Returns the arguments to record:
    the form that builds the tail on load, or st behind an x3d_tail_fwd launch."""
    if tl.keep is not None:
        # a block that may be dropped: the folded prologue does not carry keep (nor, backward, the tail epilogue of x3d_pw_bwd),
        # so its tail is a pass of its own, which skips the c_raw of the dropped samples
        pl.rec(pl.fwd, "x3d_tail_fwd_dp", tl.c_raw, tl.c_ss, tl.shortcut, tl.r_ss, tl.keep, tl.y, pl.n, tl.cout, tl.p_out, dt)
        return st
    ft = hip.PwFwdArgs(_p(tl.c_raw), st.w, st.y, None, _p(tl.c_ss), None, ACT_RELU, st.N, st.Cin, st.Cout, st.T, st.H, st.W,
                       1, st.dtype, st.w_panel, in_add=_p(tl.shortcut), in_add_scale_shift=_p(tl.r_ss), in_store=_p(tl.y))
    # (the fold must not cost a layer its stationary kernel: stages 4 / 5 fold where the weights-stationary kernel carries
    # the prologue itself -- x3d_pw_kernel_name of the folded form says which kernel it gets)
    if (model.opt["tail_fwd_fold"] and st.stride == 1 and pl.lib.x3d_pw_fwd_tail_supported(C.byref(ft))
            and (not hip.pw_kernel_name(st).startswith(("pw_gemm_wst", "pw_gemm_ws_kernel"))
                 or (hip.pw_kernel_name(ft).startswith("pw_gemm_wst") and model.opt["tail_fold_wst"]))):
        if pl.blocks:
            pl.blocks[-1].tail_fwd_folded = True
        else:
            pl.stem_tail_folded = True      # the stem's BatchNorm + ReLU (no Add)
        return ft
    pl.rec(pl.fwd, "x3d_tail_fwd", tl.c_raw, tl.c_ss, tl.shortcut, tl.r_ss, tl.y, pl.n, tl.cout, tl.p_out, dt)
    return st


def _rec_train_block(model, pl, B, tail: _Tail, dt) -> _Tail:
    """Allocates and records one block; `tail`: the pending tail of the block below (or the stem), None where the block input
    is already materialised and activated (the seam tensor of a cut plan).  Returns this block's."""
    b, p, F, n, t = B.spec, model.params, pl.fwd, pl.n, pl.t
    q = f"{block_prefix(b)}/bottleneck"
    P_in, P_out = t * B.hh * B.ww, t * B.ho * B.wo
    B.a_raw = pl.act(n, b.inner, t, B.hh, B.ww)
    B.b_raw = pl.act(n, b.inner, t, B.ho, B.wo)
    B.c_raw = pl.act(n, b.cout, t, B.ho, B.wo)
    B.y = pl.act(n, b.cout, t, B.ho, B.wo)
    B.bn_a, B.bn_b, B.bn_c = pl.bn(f"{q}/bn_a", b.inner), pl.bn(f"{q}/bn_b", b.inner), pl.bn(f"{q}/bn_c", b.cout)
    B.pool = pl.acc64(n, b.inner) if b.has_se else None
    B.gate = pl.f32(n, b.inner) if b.has_se else None
    B.hidden = pl.f32(n, b.se_width) if b.has_se else None
    # a: 1x1x1 on the block input -- materialised and already activated, or (16-bit storage, resident-panel kernel) built
    # on load from the raw `c` output + shortcut of the block below, whose residual tail is then not a pass of its own
    B.sa = _a_conv_args(model, pl, B, dt)
    if tail is not None:       # (None: the block reads the seam tensor of a cut plan)
        B.sa = _fold_pending_tail(model, pl, B.sa, tail, dt)
    pl.defer(B.sa, stats=B.bn_a.stats)
    pl.rec(F, "x3d_pw_fwd", B.sa)
    # b: channelwise 3x3x3, BN_a + ReLU folded into the load, BN_b statistics + SE squeeze in the epilogue
    _rec_bn_finalize(model, pl, B.bn_a, n * P_in)
    B.sb = hip.dilated(hip.Dw3dFwdArgs(_p(B.a_raw), _p(p[f"{q}/b/kernel"]), _p(B.b_raw), _p(B.bn_a.ss), ACT_RELU, None, None,
                                       n, b.inner, t, B.hh, B.ww, b.stride, dt), b.dilation)
    pl.defer(B.sb, stats=B.bn_b.stats, pool=B.pool)
    _rec_dw(pl, F, "x3d_dw3d_fwd", B.sb)
    _rec_bn_finalize(model, pl, B.bn_b, n * P_out)
    if b.has_se:
        _rec_se(model, pl, B)
    # c: 1x1x1 with BN_b * SE gate -> swish folded into the load
    B.sc = hip.PwFwdArgs(_p(B.b_raw), _p(p[f"{q}/c/kernel"]), _p(B.c_raw), None, _p(B.bn_b.ss), _p(B.gate),
                         ACT_SWISH, n, b.inner, b.cout, t, B.ho, B.wo, 1, dt)
    B.sc.w_panel = model._wp(f"{q}/c/kernel")
    pl.defer(B.sc, stats=B.bn_c.stats)
    pl.rec(F, "x3d_pw_fwd", B.sc)
    _rec_bn_finalize(model, pl, B.bn_c, n * P_out)
    if not b.has_shortcut_conv:
        return _Tail(B.c_raw, B.bn_c.ss, B.x, None, B.y, b.cout, P_out, B.dp_keep)
    B.r_raw = pl.act(n, b.cout, t, B.ho, B.wo)
    _rec_shortcut_conv(model, pl, B, dt)
    _rec_bn_finalize(model, pl, B.bn_r, n * P_out)
    return _Tail(B.c_raw, B.bn_c.ss, B.r_raw, B.bn_r.ss, B.y, b.cout, P_out, B.dp_keep)


# backward: written out explicitly (the reference relies on Keras autodiff) ----------------------------------------
@dataclass
class _BwdState:
    """What recording a backward list carries from launch to launch and from block to block (last block first)."""
    out: Backward
    opt: dict
    dt: int
    dy: Any = None                # gradient of the current block's output: a view of out.gbuf[cur]
    cur: int = 0
    tail_folded: bool = False     # the `a` backward just recorded applied the Add + ReLU backward of the block below
    pending_fin: Any = None       # (rc_sums, w, coef, dw, cout, cin): a recomputed-output dW the NEXT finalize launch finishes
    pending_reduce: Any = None    # DwReduceJob of the `a` conv's slab, added up by the next block's x3d_se_bnb_bwd
    pending_mark: Optional[int] = None   # stage whose mark waits for the launch that takes pending_fin
    slab_bufs: Dict = field(default_factory=dict)


def record_backward(model, pl: _Plan, opt: dict, first_unit: int = 0) -> Backward:
    """Records the backward pass over the forward state of `pl` under the plan options `opt` and returns it; the plan and
    its blocks are read, never written (new buffers and accumulators are allocated from the plan).

    first_unit = k > 0: the list ends at the SEAM, unit k (units: 0 the stem, 1..L the blocks, L + 1 conv5 and the head) -- the
    first unit above a frozen prefix u0..u(k-1), though the plan need not be a cut one.  The seam unit's convs that read the
    seam tensor -- a block's `a` and shortcut conv, or conv5 -- record their BatchNorm-backward finalize and x3d_pw_wgrad
    only: nobody below wants a data gradient, so there is no x3d_pw_dgrad, no fused x3d_pw_bwd and no write to gbuf / rtmp
    for them.  Nothing below the seam is recorded: no tail backward of the unit below, no stem backward; nothing is left
    pending.  stage_marks keeps every key: the seam's stage, the stages wholly below it and the stem get len(launches)."""
    n, t, a = pl.n, pl.t, model.arch
    k, L = int(first_unit), len(pl.blocks)
    if not 0 <= k <= L + 1 or k < pl.frozen_prefix:
        raise ValueError(f"record_backward: first_unit must lie in [{pl.frozen_prefix}, {L + 1}], not {first_unit!r}")
    out = Backward()
    live = pl.blocks[max(k - 1, 0):]          # the blocks this list walks
    # scratch shared by all blocks (sized for the largest user)
    max_out = max(([pl.y0.numel()] if k == 0 else [1]) + [B.y.numel() for B in live])
    max_inner_out = max([1] + [B.b_raw.numel() for B in live])
    max_inner_in = max([1] + [B.a_raw.numel() for B in live])
    max_r = max([1] + [n * B.spec.cin * t * B.ho * B.wo for B in live[1 if k else 0:] if B.spec.has_shortcut_conv])
    max_nc = max([1] + [n * B.spec.inner for B in live])
    out.gbuf = [pl.act(max_out), pl.act(max_out)]
    out.dv = pl.act(max_inner_out)
    out.ga = pl.act(max_inner_in)
    out.rtmp = pl.act(max_r)
    max_dp = max([0] + [B.y.numel() for B in live if B.dp_keep is not None])
    out.gbr = pl.act(max_dp) if max_dp else None
    out.coef_nc = pl.f32(max_nc * 4)
    out.se_scratch = pl.f32(max([1] + [n * (2 * B.spec.inner + B.spec.se_width) for B in live if B.spec.has_se]))
    out.g5 = pl.act(*pl.c5_raw.shape)
    out.dh1 = pl.f32(pl.rows, a.fc1_out)
    out.dpooled = pl.f32(pl.rows, a.conv5_out)
    out.ds = None if pl.stem_fused or k else pl.act(*pl.s_raw.shape)
    out.blocks = [BlockBackward() for _ in pl.blocks]
    s = _BwdState(out, opt, hip.dtype_code(model.dtype))
    _bwd_head(model, pl, s, seam=k == L + 1)
    # ---- residual blocks, last to first ----------------------------------------------------
    for bi in range(L - 1, max(k - 1, 0) - 1, -1):
        _bwd_block(model, pl, s, bi, seam=bi == k - 1)
    if k == 0:
        _bwd_stem(model, pl, s)
        return out
    # the seam: nothing may wait for a launch that never comes (a slab for a "next block", a dW riding on a later finalize)
    assert s.pending_fin is None and s.pending_mark is None and s.pending_reduce is None
    # the seam's stage is final behind the seam's last launch (also where the seam block is not the first of its stage), and
    # so -- trivially: their gradients stay at the step's zeros -- are the stages wholly inside the prefix and the stem.  The
    # keys are set in backward order, which forward_backward's stable sort keeps: the hooks fire once per bucket, as always
    seam_stage = pl.blocks[k - 1].spec.stage if k <= L else len(a.stages)
    for st in list(range(min(seam_stage, len(a.stages) - 1), -1, -1)) + [-1]:
        out.stage_marks.setdefault(st, len(out.launches))
    return out


def _fold_bn_bwd(pl, s, bn, count, gamma, dgamma, dbeta, consumers):
    """The BatchNorm-backward finalize (sums -> the coefficient table of dYraw = A g + B yraw + C, dgamma, dbeta) is a ~6 us launch
    between the producer of the sums and the consumers of the table.  Where EVERY consumer's kernel takes `coef_fold`
    (include/x3d_hip.h x3d_bn_bwd_fold: the persistent weights-stationary kernels and the 16-bit weight-gradient kernel
    -- stages 4 / 5 and conv5, 37 launches of an X3D-M step) the consumers derive the table themselves, the same bits, and
    one of them -- never the weight-gradient launch -- publishes dgamma / dbeta and the table; no launch is recorded.
    consumers: [(argument struct, "dgrad" | "wgrad" | "bwd")] -- every launch that reads bn.coef.  True: folded."""
    if not s.opt["coef_fold"] or not consumers:
        return False
    slot = {"dgrad": 0, "wgrad": 1, "bwd": 2}
    for st, kind in consumers:
        q3 = [None, None, None]
        q3[slot[kind]] = C.byref(st)
        if not pl.lib.x3d_pw_coef_fold_supported(*q3):
            return False
    pub = next((st for st, kind in consumers if kind != "wgrad"), None)
    if pub is None:
        return False
    for st, kind in consumers:
        f = hip.BnBwdFold(None, float(count), _p(bn.mi), _p(gamma), _p(dgamma) if st is pub else None,
                          _p(dbeta) if st is pub else None, _p(bn.coef) if st is pub else None)
        pl.keep += [f, bn.mi, gamma, dgamma, dbeta, bn.coef]
        pl.defer(f, sums=bn.bsums)
        st.coef_fold = hip.fold_address(f)
    return True


def _rec_bn_bwd_finalize(model, pl, s, bn, count, c, prep=None, consumers=None):
    """The backward finalize of `bn` in front of its consumers: folded into them (no launch), a plain launch, or -- with the
    recomputed-output backward's jobs on board -- x3d_bn_bwd_finalize_rc.  prep = (w, panel, c0, cin): build the panel of the
    recomputed-output launch that follows."""
    Bk = s.out.launches
    gamma, dgamma, dbeta = model.params[f"{bn.prefix}/gamma"], model.grads[f"{bn.prefix}/gamma"], model.grads[f"{bn.prefix}/beta"]
    if bn.frozen:
        # a negative count asks the two finalize LAUNCHES for the frozen rule: A = gamma * invstd, B = C = +0 (x3d_hip.h K3).
        # The consumers that derive their table themselves (coef_fold) have no such form: a frozen layer gets the launch.  The
        # recomputed-output jobs take the table as data and hold for B = C = 0
        count, consumers = -count, None
    if prep is None and s.pending_fin is None and _fold_bn_bwd(pl, s, bn, count, gamma, dgamma, dbeta, consumers):
        return          # (derived by the consumers: no launch)
    fin, s.pending_fin = s.pending_fin, None
    if prep is None and fin is None:
        pl.rec(Bk, "x3d_bn_bwd_finalize", pl.acc(bn.bsums), float(count), bn.mi, gamma, bn.coef, dgamma, dbeta, c)
        return
    w_, panel_, c0_, cin_ = prep if prep is not None else (None, None, None, 0)
    f_ = fin if fin is not None else (None, None, None, None, 0, 0)
    pl.rec(Bk, "x3d_bn_bwd_finalize_rc", pl.acc(bn.bsums), float(count), bn.mi, gamma, bn.coef, dgamma, dbeta, c,
           w_, panel_, c0_, cin_, pl.acc(f_[0]), f_[1], f_[2], f_[3], f_[4], f_[5], s.dt)
    if fin is not None and s.pending_mark is not None:
        # this launch finished the dW of the FIRST block of a stage (its `a` conv's pending job): only now is every
        # gradient of that stage final -- the stage's all-reduce bucket may start behind it, not before
        s.out.stage_marks[s.pending_mark], s.pending_mark = len(Bk), None


def _dw_slab_job(pl, s, st, role, dw):
    """Weight-gradient SLABS (x3d_hip.h dw_slab): the persistent fused backward kernels of stage 4 end in a flush of 256
    workgroups x [Cout][Cin] floats -- as device-scope atomics 13-24 us of a 85-105 us launch (profiles/r05_noflush.txt), as
    plain stores into a slab per workgroup a few.  The slabs are added up by extra workgroups of the NEXT x3d_se_bnb_bwd
    launch (every block has one, 12 us of latency on the critical path anyway): the `c` conv's by its own block's, the `a`
    conv's by the block below's.  Two slab buffers per role, reused by every block (stream order).
    st: the x3d_pw_bwd / x3d_pw_wgrad arguments about to be recorded; returns its reduce job (and points st at the
    slab) or None."""
    query = pl.lib.x3d_pw_wgrad_dw_parts if isinstance(st, hip.PwWgradArgs) else pl.lib.x3d_pw_bwd_dw_parts
    # (small weight gradients -- stages 2 / 3 of the unfused fp32 path -- flush a few MB: not worth a reduce job)
    parts = int(query(C.byref(st))) if (s.opt["dw_slab"] and st.Cout * st.Cin >= 8192) else 0
    if parts <= 0:
        return None
    elems = st.Cout * st.Cin
    buf = s.slab_bufs.get((role, parts * elems))
    if buf is None:
        buf = s.slab_bufs[(role, parts * elems)] = pl.f32(parts * elems)
        pl.keep.append(buf)
    st.dw_slab, st.dw_slab_parts = _p(buf), parts
    return hip.DwReduceJob(_p(buf), _p(dw), parts, elems)


def _bwd_head(model, pl, s, seam=False):
    """seam: conv5 is the seam unit -- its weight gradient only, behind a plain finalize launch"""
    a, p, g, n, t, dt = model.arch, model.params, model.grads, pl.n, pl.t, s.dt
    out, Bk, c5, b5 = s.out, s.out.launches, model.arch.conv5_out, pl.bn5
    pl.rec(Bk, "x3d_dense_bwd", pl.dlogits, None, ACT_NONE, pl.h1, pl.drop_mask, float(pl.drop_scale),
           p["fc2/kernel"], out.dh1, g["fc2/kernel"], g["fc2/bias"], pl.rows, a.fc1_out, a.num_classes)
    pl.rec(Bk, "x3d_dense_bwd", out.dh1, pl.h1, ACT_RELU, pl.pooled, None, 1.0, p["fc1/kernel"], out.dpooled,
           g["fc1/kernel"], None, pl.rows, c5, a.fc1_out)
    if pl.det:     # the same contract below it: g5 and bn5's backward sums
        pl.rec(Bk, "x3d_roi_pool_bwd", out.dpooled, pl.roi_argmax, pl.boxes, pl.num_boxes, pl.c5_raw, b5.ss, out.g5,
               pl.acc(b5.bsums), *_roi_args(pl), dt)
    else:
        pl.rec(Bk, "x3d_relu_bn_bwd_reduce", None, out.dpooled, pl.c5_raw, b5.ss, out.g5, pl.acc(b5.bsums), n, c5,
               pl.P5, dt)
    c_last = a.stages[-1].cout
    w5 = hip.PwWgradArgs(_p(out.g5), _p(pl.c5_raw), _p(b5.coef), _p(pl.y_last), None, None, ACT_NONE,
                         _p(g["conv5/layer_with_weights-0/kernel"]), n, c_last, c5, t, pl.h5, pl.w5, 1, dt)
    s.dy = out.gbuf[s.cur][:pl.y_last.numel()]
    d5 = hip.PwDgradArgs(_p(out.g5), _p(pl.c5_raw), _p(b5.coef), _p(p["conv5/layer_with_weights-0/kernel"]),
                         _p(s.dy), EPI_STORE, None, None, None, None, None, n, c_last, c5, t, pl.h5, pl.w5, dt)
    d5.w_panel = model._wp("conv5/layer_with_weights-0/kernel", True)
    if seam:
        s.dy = None
        _rec_bn_bwd_finalize(model, pl, s, b5, n * pl.P5, c5)
        pl.rec(Bk, "x3d_pw_wgrad", w5)
    else:
        _rec_bn_bwd_finalize(model, pl, s, b5, n * pl.P5, c5, consumers=[(w5, "wgrad"), (d5, "dgrad")])
        pl.rec(Bk, "x3d_pw_wgrad", w5)
        pl.rec(Bk, "x3d_pw_dgrad", d5)
    out.stage_marks[len(a.stages)] = len(Bk)   # head finished


def _bwd_block(model, pl, s, bi, seam=False):
    """One block: [tail] -> c -> SE / BN_b -> depthwise b -> [shortcut conv] -> a, which stores the gradient of the block input.
    seam: the list ends with this block -- the shortcut conv and `a` record their weight gradients only (_bwd_seam_wgrads)."""
    B, R, Bk = pl.blocks[bi], s.out.blocks[bi], s.out.launches
    b = B.spec
    R.bwd_start, R.dy_view = len(Bk), s.dy.view(B.y.shape)
    # The Add + ReLU backward of a block (g = dy * [y > 0] with the BN_c / BN_r backward sums) is applied by the kernel that
    # PRODUCES dy -- the `a`-conv backward of the next block, whose conv input is this block's y -- wherever the fused
    # x3d_pw_bwd covers that layer with its tail epilogue; x3d_tail_bwd remains for the other blocks (and tail_bwd_fold = False)
    R.tail_folded, s.tail_folded = s.tail_folded, False
    if B.dp_keep is not None:
        # stochastic depth: g in place as below (the shortcut path's gradient), and g_branch = keep * g for the `c` backward;
        # the BN_c sums are taken over g_branch as stored, so bn_c's backward coefficients belong to the tensor `c` reads
        assert not R.tail_folded
        R.g_branch = s.out.gbr[:B.y.numel()]
        pl.rec(Bk, "x3d_tail_bwd_dp", s.dy, R.g_branch, B.y, B.c_raw, B.r_raw, B.dp_keep, pl.acc(B.bn_c.bsums),
               pl.acc(B.bn_r.bsums) if B.bn_r else None, pl.n, b.cout, pl.t * B.ho * B.wo, s.dt)
    elif not R.tail_folded:
        # dy -> g = dy*[y>0] in place, with the BN_c (and BN_r) backward sums
        pl.rec(Bk, "x3d_tail_bwd", s.dy, B.y, B.c_raw, B.r_raw, pl.acc(B.bn_c.bsums),
               pl.acc(B.bn_r.bsums) if B.bn_r else None, pl.n, b.cout, pl.t * B.ho * B.wo, s.dt)
    dvv = s.out.dv[:B.b_raw.numel()]
    gaa = s.out.ga[:B.a_raw.numel()]
    c_job = _bwd_c(model, pl, s, B, R, dvv)
    _bwd_se_bnb(model, pl, s, B, R, c_job)
    _bwd_dw(model, pl, s, B, R, dvv, gaa)
    # (bn_a's backward finalize is recorded in _bwd_a, right in front of the `a` backward: whether it also builds that launch's
    # panel is known there; the shortcut launches in between do not depend on it)
    if seam:
        _bwd_seam_wgrads(model, pl, s, B, gaa)
        R.bwd_stop, s.dy = len(Bk), None
        return
    nxt = s.out.gbuf[1 - s.cur][:B.x.numel()]
    rt = _bwd_shortcut(model, pl, s, B, R) if b.has_shortcut_conv else None
    _bwd_a(model, pl, s, bi, gaa, nxt, rt)
    s.cur = 1 - s.cur
    R.bwd_stop, R.dx_view = len(Bk), nxt.view(B.x.shape)
    s.dy = nxt
    if b.index == 0:
        # a slab nobody has added up yet, in front of a point where its gradient must be final: its own small launch
        # (the next x3d_se_bnb_bwd belongs to the stage below: behind this stage's mark)
        job, s.pending_reduce = s.pending_reduce, None
        if job is not None:
            jobs = (hip.DwReduceJob * 1)(job)
            pl.keep.append(jobs)
            pl.rec(Bk, "x3d_dw_slab_reduce", jobs, 1)
        if s.pending_fin is not None:      # the dW of this block's `a` conv rides on the NEXT finalize launch:
            s.pending_mark = b.stage       # the mark is set there (_rec_bn_bwd_finalize)
        else:
            s.out.stage_marks[b.stage] = len(Bk)   # every gradient of stages >= b.stage is final


def _bwd_seam_wgrads(model, pl, s, B, gaa):
    """The two convs of the seam block that read the seam tensor B.x: the shortcut conv (on B.xs where the forward pass made
    the even-pixel copy) and `a`.  Each: the plain BatchNorm-backward finalize and x3d_pw_wgrad.  The weight gradients are
    flushed by the launches themselves (no slab: no later x3d_se_bnb_bwd would add it up) and nothing rides on a later finalize."""
    b, g, n, t, dt, Bk = B.spec, model.grads, pl.n, pl.t, s.dt, s.out.launches
    pre = block_prefix(b)
    q = f"{pre}/bottleneck"
    assert s.pending_fin is None          # (taken by bn_c's finalize of this block at the latest)
    if b.has_shortcut_conv:
        x_r, geom = (B.xs, (B.ho, B.wo, 1)) if B.xs is not None else (B.x, (B.hh, B.ww, b.stride))
        wr = hip.PwWgradArgs(_p(s.dy), _p(B.r_raw), _p(B.bn_r.coef), _p(x_r), None, None, ACT_NONE,
                             _p(g[f"{pre}/residual/kernel"]), n, b.cin, b.cout, t, *geom, dt)
        _rec_bn_bwd_finalize(model, pl, s, B.bn_r, n * t * B.ho * B.wo, b.cout)
        pl.rec(Bk, "x3d_pw_wgrad", wr)
    wa = hip.PwWgradArgs(_p(gaa), _p(B.a_raw), _p(B.bn_a.coef), _p(B.x), None, None, ACT_NONE,
                         _p(g[f"{q}/a/kernel"]), n, b.cin, b.inner, t, B.hh, B.ww, 1, dt)
    _rec_bn_bwd_finalize(model, pl, s, B.bn_a, n * t * B.hh * B.ww, b.inner)
    pl.rec(Bk, "x3d_pw_wgrad", wa)


def _bwd_c(model, pl, s, B, R, dvv):
    """The `c` conv: data gradient with the swish backward in its epilogue (into dvv, with the per-(n, c) sums the SE / BN_b
    backward needs) + weight gradient.  Returns the reduce job of its weight-gradient slab, or None."""
    b, p, g, n, t, dt = B.spec, model.params, model.grads, pl.n, pl.t, s.dt
    q, Bk, gten = f"{block_prefix(b)}/bottleneck", s.out.launches, (s.dy if R.g_branch is None else R.g_branch)
    wc = hip.PwWgradArgs(_p(gten), _p(B.c_raw), _p(B.bn_c.coef), _p(B.b_raw), _p(B.bn_b.ss), _p(B.gate),
                         ACT_SWISH, _p(g[f"{q}/c/kernel"]), n, b.inner, b.cout, t, B.ho, B.wo, 1, dt)
    R.nc_sums = pl.acc64(n, b.inner, 2)
    dc = hip.PwDgradArgs(_p(gten), _p(B.c_raw), _p(B.bn_c.coef), _p(p[f"{q}/c/kernel"]), _p(dvv),
                         EPI_SWISH_BWD, None, _p(B.b_raw), _p(B.bn_b.ss), _p(B.gate), None, n, b.inner,
                         b.cout, t, B.ho, B.wo, dt)
    dc.w_panel = model._wp(f"{q}/c/kernel", True)
    # one pass over g / c_raw / b_raw for both gradients where the fused kernel covers the layer
    fc = hip.PwBwdArgs(_p(gten), _p(B.c_raw), _p(B.bn_c.coef), dc.w_panel, _p(dvv), EPI_SWISH_BWD, None,
                       _p(B.b_raw), _p(B.bn_b.ss), _p(B.gate), None, None, _p(g[f"{q}/c/kernel"]), n, b.inner,
                       b.cout, t, B.ho, B.wo, dt)
    c_fused = bool(s.opt["fused_pw_bwd"] and pl.lib.x3d_pw_bwd_supported(C.byref(fc)))
    _rec_bn_bwd_finalize(model, pl, s, B.bn_c, n * t * B.ho * B.wo, b.cout,
                         consumers=[(fc, "bwd")] if c_fused else [(wc, "wgrad"), (dc, "dgrad")])
    if c_fused:
        c_job = _dw_slab_job(pl, s, fc, "c", g[f"{q}/c/kernel"])
        pl.defer(fc, nc_sums=R.nc_sums)
        pl.rec(Bk, "x3d_pw_bwd", fc)
    else:
        c_job = _dw_slab_job(pl, s, wc, "c", g[f"{q}/c/kernel"])
        pl.rec(Bk, "x3d_pw_wgrad", wc)
        pl.defer(dc, nc_sums=R.nc_sums)
        pl.rec(Bk, "x3d_pw_dgrad", dc)
    return c_job


def _bwd_se_bnb(model, pl, s, B, R, c_job):
    """SE + BN_b backward from the per-(n,c) sums; its spare workgroups add up the weight-gradient slabs on hand."""
    b, p, g = B.spec, model.params, model.grads
    q = f"{block_prefix(b)}/bottleneck"
    se = hip.SeBnbBwdArgs(
        None, None, float(pl.t * B.ho * B.wo) * (-1.0 if B.bn_b.frozen else 1.0), _p(B.bn_b.ss), _p(B.bn_b.mi), _p(p[f"{q}/bn_b/gamma"]),
        _p(p.get(f"{q}/se_fc1/kernel")), _p(p.get(f"{q}/se_fc1/bias")), _p(p.get(f"{q}/se_fc2/kernel")),
        _p(p.get(f"{q}/se_fc2/bias")), _p(B.gate), _p(B.hidden), _p(g.get(f"{q}/se_fc1/kernel")),
        _p(g.get(f"{q}/se_fc1/bias")), _p(g.get(f"{q}/se_fc2/kernel")), _p(g.get(f"{q}/se_fc2/bias")),
        _p(g[f"{q}/bn_b/gamma"]), _p(g[f"{q}/bn_b/beta"]), _p(s.out.coef_nc), _p(s.out.se_scratch), pl.n, b.inner,
        b.se_width)
    if c_job is not None:
        se.reduce[0] = c_job
    if s.pending_reduce is not None:      # the `a` conv of the block above (recorded just before this block)
        se.reduce[1], s.pending_reduce = s.pending_reduce, None
    pl.defer(se, nc_sums=R.nc_sums, pool_sums=B.pool)
    pl.rec(s.out.launches, "x3d_se_bnb_bwd", se)


def _bwd_dw(model, pl, s, B, R, dvv, gaa):
    """b (fused data + weight gradient), emits grad wrt BN_a output with the ReLU mask applied"""
    b, q = B.spec, f"{block_prefix(B.spec)}/bottleneck"
    R.db = hip.dilated(hip.Dw3dBwdArgs(_p(dvv), _p(B.b_raw), _p(s.out.coef_nc), _p(B.a_raw), _p(B.bn_a.ss),
                                       _p(model.params[f"{q}/b/kernel"]), _p(gaa), None, _p(model.grads[f"{q}/b/kernel"]), pl.n,
                                       b.inner, pl.t, B.hh, B.ww, b.stride, s.dt), b.dilation)
    pl.defer(R.db, a_sums=B.bn_a.bsums)
    _rec_dw(pl, s.out.launches, "x3d_dw3d_bwd", R.db)


def _bwd_shortcut(model, pl, s, B, R):
    """The shortcut conv of a stage's first block: its data gradient goes to `rt` (returned), which the `a` backward adds."""
    b, p, g, n, t, dt = B.spec, model.params, model.grads, pl.n, pl.t, s.dt
    pre, Bk, gten = block_prefix(b), s.out.launches, s.dy
    P_out = t * B.ho * B.wo
    rt = s.out.rtmp[:n * b.cin * P_out]
    # the strided shortcut conv's two gradients in ONE launch over g and the even pixels of the block input, its raw
    # output recomputed algebraically like the `a` conv's (pw_bwd_rc.hip, x_stride = 2) -- where the shape is covered
    sr = None
    per = int(pl.lib.x3d_pw_bwd_rc_panel_elems(b.cout, b.cin)) if (s.opt["fused_pw_bwd"] and s.opt["pw_bwd_rc"] and b.stride == 2
                                                                    and model.dtype != torch.float32) else 0
    xs = B.xs       # the even-pixel copy of B.x the forward pass made (option shortcut_compact), or None
    if per:
        rcr = (pl.act(per), pl.f32(b.cin), pl.acc64((int(pl.lib.x3d_pw_bwd_rc_sums_elems(b.cout, b.cin)) + 1) // 2))
        x_geom = (_p(xs),) if xs is not None else (_p(B.x), b.stride, B.hh, B.ww)      # (x, then x_stride, xH, xW of a strided x)
        sr = hip.PwBwdArgs(_p(gten), None, None, None, _p(rt), EPI_STORE, None, None, None, None, None, x_geom[0], None,
                           n, b.cin, b.cout, t, B.ho, B.wo, dt, None, None, None, None, _p(rcr[0]), _p(rcr[1]), None, *x_geom[1:])
        if not pl.lib.x3d_pw_bwd_supported(C.byref(sr)):
            sr = None
    R.r_bwd_rc = sr is not None
    w_r, g_r = p[f"{pre}/residual/kernel"], g[f"{pre}/residual/kernel"]
    if sr is not None:
        if s.opt["pw_bwd_rc_merge"]:
            _rec_bn_bwd_finalize(model, pl, s, B.bn_r, n * P_out, b.cout, prep=(w_r, rcr[0], rcr[1], b.cin))
        else:
            _rec_bn_bwd_finalize(model, pl, s, B.bn_r, n * P_out, b.cout)
            pl.rec(Bk, "x3d_pw_bwd_rc_prepare", w_r, B.bn_r.coef, rcr[0], rcr[1], b.cout, b.cin, dt)
        pl.defer(sr, rc_sums=rcr[2])
        pl.rec(Bk, "x3d_pw_bwd", sr)
        if s.opt["pw_bwd_rc_merge"]:     # (the bn_a finalize recorded next carries this dW)
            s.pending_fin = (rcr[2], w_r, B.bn_r.coef, g_r, b.cout, b.cin)
        else:
            pl.rec(Bk, "x3d_pw_bwd_rc_finish", pl.acc(rcr[2]), w_r, B.bn_r.coef, g_r, b.cout, b.cin, dt)
        return rt
    x_r, geom = (xs, (B.ho, B.wo, 1)) if xs is not None else (B.x, (B.hh, B.ww, b.stride))
    wr = hip.PwWgradArgs(_p(gten), _p(B.r_raw), _p(B.bn_r.coef), _p(x_r), None, None, ACT_NONE,
                         _p(g_r), n, b.cin, b.cout, t, *geom, dt)
    dr = hip.PwDgradArgs(_p(gten), _p(B.r_raw), _p(B.bn_r.coef), _p(w_r), _p(rt),
                         EPI_STORE, None, None, None, None, None, n, b.cin, b.cout, t, B.ho, B.wo, dt)
    dr.w_panel = model._wp(f"{pre}/residual/kernel", True)
    _rec_bn_bwd_finalize(model, pl, s, B.bn_r, n * P_out, b.cout, consumers=[(wr, "wgrad"), (dr, "dgrad")])
    pl.rec(Bk, "x3d_pw_wgrad", wr)
    pl.rec(Bk, "x3d_pw_dgrad", dr)
    return rt


def _bwd_a(model, pl, s, bi, gaa, nxt, rt):
    """The `a` conv: dx = its data gradient + the shortcut's (rt: the shortcut conv's, else the identity's dy) into `nxt`,
    and its weight gradient.  Form selection, in order of preference: fused with the tail of the block below in its epilogue
    (ft), fused with the stem's BatchNorm sums there (stem_ft), plain fused (fa) -- each as the recomputed-output form (rc)
    where that covers the layer -- else the unfused pair."""
    B, R, Bk = pl.blocks[bi], s.out.blocks[bi], s.out.launches
    prev = pl.blocks[bi - 1] if bi > 0 else None
    b, p, g, n, t, dt, opt = B.spec, model.params, model.grads, pl.n, pl.t, s.dt, s.opt
    q = f"{block_prefix(b)}/bottleneck"
    w_a, g_a = p[f"{q}/a/kernel"], g[f"{q}/a/kernel"]
    wa = hip.PwWgradArgs(_p(gaa), _p(B.a_raw), _p(B.bn_a.coef), _p(B.x), None, None, ACT_NONE,
                         _p(g_a), n, b.cin, b.inner, t, B.hh, B.ww, 1, dt)
    epi, add = (EPI_ADD_STRIDED if b.stride == 2 else EPI_ADD, rt) if rt is not None else (EPI_ADD, s.dy)
    da = hip.PwDgradArgs(_p(gaa), _p(B.a_raw), _p(B.bn_a.coef), _p(w_a), _p(nxt), epi, _p(add), None, None, None, None, n,
                         b.cin, b.inner, t, B.hh, B.ww, dt)
    da.w_panel = model._wp(f"{q}/a/kernel", True)
    # The `a` conv's raw output is linear in its input, so the BatchNorm backward dY = A g + B a_raw + C folds into the
    # GEMMs (pw_bwd_rc.hip): where that form covers the layer (stages 2-3 first blocks: Cin <= 32) the launch streams
    # g and x only -- a_raw, 2.25x the size of x, is not read here.  Per-step operands: the panel [W^T A | W^T B W] and
    # c0 (x3d_pw_bwd_rc_prepare, after bn_a's backward finalize) and the moment sums dW is finished from.
    rc = None
    pe = int(pl.lib.x3d_pw_bwd_rc_panel_elems(b.inner, b.cin)) if (opt["fused_pw_bwd"] and opt["pw_bwd_rc"] and
                                                                    model.dtype != torch.float32) else 0
    if b.inner > 127 and not opt["pw_bwd_rc_wide"]:      # (the 48 -> 216 layer unfused as before)
        pe = 0
    if pe:
        rc = (pl.act(pe), pl.f32(b.cin), pl.acc64((int(pl.lib.x3d_pw_bwd_rc_sums_elems(b.inner, b.cin)) + 1) // 2))

    def a_bwd_args(tail_c=None, tail_r=None, use_rc=True):
        if rc is not None and use_rc:
            return hip.PwBwdArgs(da.g, None, None, None, da.dx, da.epi, da.add, None, None, None, None, _p(B.x), None,
                                 n, b.cin, b.inner, t, B.hh, B.ww, dt, tail_c, tail_r, None, None, _p(rc[0]), _p(rc[1]), None)
        return hip.PwBwdArgs(da.g, da.yraw, da.coef, da.w_panel, da.dx, da.epi, da.add, None, None, None, None,
                             _p(B.x), _p(g_a), n, b.cin, b.inner, t, B.hh, B.ww, dt, tail_c, tail_r, None, None)

    def supported(st):
        return st is not None and bool(pl.lib.x3d_pw_bwd_supported(C.byref(st)))

    fa = a_bwd_args()
    if rc is not None and not supported(fa):
        rc, fa = None, a_bwd_args(use_rc=False)
    fold_tail = opt["fused_pw_bwd"] and opt["tail_bwd_fold"]
    ft = None
    # B.x is prev.y: this launch can apply prev's Add + ReLU backward to its dx (not with stochastic depth: x3d_tail_bwd_dp)
    if fold_tail and prev is not None and prev.dp_keep is None:
        ft = a_bwd_args(_p(prev.c_raw), _p(prev.r_raw))
        if not supported(ft):
            ft = None
    stem_ft = None
    if fold_tail and prev is None and opt["stem_bwd_fold"]:
        # B.x is the stem output y0 = relu(bn(t_raw)): the same epilogue masks dx with [y0 > 0] and takes the stem
        # BatchNorm's backward sums (sum dx, sum dx * t_raw) -- the x3d_relu_bn_bwd_reduce pass over dy0 / t_raw goes
        stem_ft = a_bwd_args(_p(pl.t_raw), None)
        if not supported(stem_ft):
            stem_ft = None
    if prev is None:
        s.out.stem_bwd_folded = stem_ft is not None
    chosen = ft if ft is not None else (stem_ft if stem_ft is not None else (fa if opt["fused_pw_bwd"] and supported(fa) else None))
    R.a_bwd_rc = rc is not None and chosen is not None
    # The per-step operands of the recomputed-output `a` backward ride on the BatchNorm-backward finalize launches that
    # are on the critical path anyway (x3d_bn_bwd_finalize_rc): the panel of a layer with ITS bn_a finalize, the dW of a
    # layer with the NEXT finalize recorded after its x3d_pw_bwd (pw_bwd_rc_merge = False: separate launches).
    merge_rc = opt["pw_bwd_rc_merge"]
    if R.a_bwd_rc and merge_rc:
        _rec_bn_bwd_finalize(model, pl, s, B.bn_a, n * t * B.hh * B.ww, b.inner, prep=(w_a, rc[0], rc[1], b.cin))
    else:
        _rec_bn_bwd_finalize(model, pl, s, B.bn_a, n * t * B.hh * B.ww, b.inner,
                             consumers=None if R.a_bwd_rc else ([(chosen, "bwd")] if chosen is not None else
                                                                [(wa, "wgrad"), (da, "dgrad")]))
    if R.a_bwd_rc and not merge_rc:
        pl.rec(Bk, "x3d_pw_bwd_rc_prepare", w_a, B.bn_a.coef, rc[0], rc[1], b.inner, b.cin, dt)
    # (the `a` conv's slab is added up by the NEXT block's x3d_se_bnb_bwd: not for the first block of a stage, whose
    # gradient must be final at the stage mark -- a reduce launch of its own would cost what the slab saves)
    if chosen is not None and rc is None and b.index != 0:
        s.pending_reduce = _dw_slab_job(pl, s, chosen, "a", g_a)
    if chosen is not None:
        pl.defer(chosen, rc_sums=None if rc is None else rc[2])
        if ft is not None:
            s.tail_folded = True
            pl.defer(ft, tail_sums_c=prev.bn_c.bsums, tail_sums_r=prev.bn_r.bsums if prev.bn_r else None)
        elif stem_ft is not None:
            pl.defer(stem_ft, tail_sums_c=pl.bn1.bsums)
        pl.rec(Bk, "x3d_pw_bwd", chosen)
    else:
        if b.index != 0:
            s.pending_reduce = _dw_slab_job(pl, s, wa, "a", g_a)
        pl.rec(Bk, "x3d_pw_wgrad", wa)
        pl.rec(Bk, "x3d_pw_dgrad", da)
    if R.a_bwd_rc:
        if merge_rc:    # dW rides on the next BatchNorm-backward finalize (the block below's bn_c, or the stem's)
            s.pending_fin = (rc[2], w_a, B.bn_a.coef, g_a, b.inner, b.cin)
        else:
            pl.rec(Bk, "x3d_pw_bwd_rc_finish", pl.acc(rc[2]), w_a, B.bn_a.coef, g_a, b.inner, b.cin, dt)


def _bwd_stem(model, pl, s):
    a, p, g, n, t, dt = model.arch, model.params, model.grads, pl.n, pl.t, s.dt
    out, Bk, b1, dy = s.out, s.out.launches, pl.bn1, s.dy
    P1 = t * pl.y0.shape[3] * pl.y0.shape[4]
    # sums only (g = NULL): x3d_dwt_bwd applies the ReLU mask itself on the t_raw values it loads anyway, so the masked
    # gradient of the widest tensor of the network is neither written nor read back
    if not out.stem_bwd_folded:
        pl.rec(Bk, "x3d_relu_bn_bwd_reduce", dy, None, pl.t_raw, b1.ss, None, pl.acc(b1.bsums), n, a.c1, P1, dt)
    _rec_bn_bwd_finalize(model, pl, s, b1, n * P1, a.c1)
    assert s.pending_fin is None and s.pending_mark is None and s.pending_reduce is None
    if pl.stem_fused:
        # one pass over dy, t_raw and the batch: conv_s recomputed on the matrix cores, the conv_t input gradient kept in LDS
        out.input_slots.append((Bk, len(Bk), 4))
        pl.rec(Bk, "x3d_stem_bwd", dy, pl.t_raw, b1.ss, b1.coef, pl.x, p["conv1/conv_s/kernel"], p["conv1/conv_t/kernel"],
               g["conv1/conv_s/kernel"], g["conv1/conv_t/kernel"], n, model.in_channels, t, pl.h, pl.w, a.c1,
               a.c1_temp_filter, dt, 1)
    else:
        pl.rec(Bk, "x3d_dwt_bwd", dy, pl.t_raw, b1.ss, b1.coef, pl.s_raw, p["conv1/conv_t/kernel"], out.ds,
               g["conv1/conv_t/kernel"], n, a.c1, t, pl.y0.shape[3] * pl.y0.shape[4], a.c1_temp_filter, dt)
        out.input_slots.append((Bk, len(Bk)))
        pl.rec(Bk, "x3d_stem_s_wgrad", pl.x, out.ds, g["conv1/conv_s/kernel"], n, model.in_channels, t, pl.h, pl.w,
               a.c1, dt, int(pl.x_cl))
    out.stage_marks[-1] = len(Bk)
