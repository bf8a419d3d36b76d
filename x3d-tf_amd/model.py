"""``X3D(cfg)``: the reference's model surface (reference model.py:8-132) over hand-written HIP kernels.

Same constructor argument (the config tree), same call signature (``model(input, training=False)``
with a channels-last ``[N, T, H, W, 3]`` clip batch, fp32 probabilities out, views averaged at
inference -- model.py:113-127), same attribute tree (``conv1.conv_s``, ``stages[i].stage[j].bottleneck.a``
... -- the names the released checkpoints are keyed by), ``summary(input_shape)`` and
``load_weights(path)``.  What is different is everything underneath: activations live in NCTHW, every
op is a kernel from libx3d_hip.so, BatchNorm / ReLU / swish / SE scale never touch HBM as separate
passes (they are folded into the prologue of the consuming conv and the epilogue of the producing
one), and the backward pass is written out explicitly instead of taped.

Execution model: for one (batch, clip shape, mode) a ``_Plan`` allocates every buffer once and records
the kernel launches as pre-bound C calls; a step replays the list on the current HIP stream.  Nothing in a
replay allocates or synchronises, but a replay is NOT capture-safe as it stands: with 16-bit storage the stem
launches are re-bound to the CALLER's batch on every call (`_bind_input`: the clips are read in place, forward
AND backward -- `stem_s_wgrad` reads them again, so the caller must not overwrite the batch between the two), a
captured graph would bake that pointer in.  `options={"stem_nthwc": False}` restores the static planar input
buffer (one conversion pass per step) for graph capture; replaying as a hipGraph measured no gain.
"""
import collections
import types
from typing import Dict, Optional

import torch

from . import hip, ops
from .config import FinetuneSettings, detection_settings, ensemble_method, multi_label
from .arch import Arch, ParamSpec, block_prefix, build_arch, drop_path_rates, param_specs, summary_rows
from .params import init_params
from .segments import Segment, SegTable
from .solver import RULES
from .plan import PLAN_DEFAULTS, LossMods, _FakeBuf, _Plan, _experiment_options, record_inference, record_training  # noqa: F401  (PLAN_DEFAULTS, _FakeBuf: re-exported)


# ------------------------------------------------------------------------------------------------
# thin layer objects: they own views of the flat parameter buffers and give the reference's
# attribute paths something to resolve to.  No compute happens here.
# ------------------------------------------------------------------------------------------------
class _Layer:
    def __init__(self, name):
        self.name = name

    def variables(self):
        return {k: v for k, v in vars(self).items() if isinstance(v, torch.Tensor)}


class Conv3D(_Layer):
    def __init__(self, name, kernel, bias=None, **attrs):
        super().__init__(name)
        self.kernel = kernel
        if bias is not None:
            self.bias = bias
        self.__dict__.update(attrs)


class Dense(Conv3D):
    pass


class BatchNormalization(_Layer):
    def __init__(self, name, gamma, beta, moving_mean, moving_variance, epsilon, momentum):
        super().__init__(name)
        self.gamma, self.beta = gamma, beta
        self.moving_mean, self.moving_variance = moving_mean, moving_variance
        self.epsilon, self.momentum = epsilon, momentum
        self.axis = -1


class Activation(_Layer):
    def __init__(self, kind):
        super().__init__(kind)
        self.activation = kind


class AdaptiveAvgPool3D(_Layer):
    def __init__(self, name="pool"):
        super().__init__(name)
        self.out_shape = (1, 1, 1)


class Dropout(_Layer):
    def __init__(self, rate):
        super().__init__("dropout")
        self.rate = rate


class X3D_Stem(_Layer):
    pass


class Bottleneck(_Layer):
    pass


class ResBlock(_Layer):
    pass


class ResStage(_Layer):
    pass


class _Sequential(list):
    """K.Sequential stand-in: an indexable list of layers (``layer_with_weights-i`` order)."""
    pass



PreciseBNLayout = collections.namedtuple("PreciseBNLayout", "prefixes channels mean_offsets var_offsets pooled_offsets pooled_size")


class X3D:
    """Constructs the X3D model from the model configurations (reference model.py:8-111).

    Args:
        cfg: config tree (x3d_tf_amd.config.CfgNode or anything exposing the same attributes).
        dtype: activation storage type on the GPU: torch.float32, torch.bfloat16 or torch.float16 (weights,
            statistics and accumulation stay fp32).  float16 is the reference's reduced-precision mode (Keras
            mixed_float16, utils.py:176-192: fp16 compute, fp32 variables, loss scaling in training --
            train.Trainer's `loss_scale`); bfloat16 needs no loss scaling and is the benchmark's default.
        device: a CUDA/HIP device.  There is no CPU path.  The one exception is device="dry": the model is built on
            the host with address-only stand-ins for the activation buffers, plans can be RECORDED (to enumerate
            launches and their kernel instantiations, x3d_tf_amd/dispatch.py) and every attempt to run one raises.
        seed: seed of the Glorot-uniform initialisation.
        options: overrides of PLAN_DEFAULTS (which launch list a plan records; differential tests and A/B tools).
    """

    def __init__(self, cfg, dtype=torch.float32, device="cuda", seed: int = 0, in_channels: int = 3, options: Optional[dict] = None):
        self.cfg = cfg
        self.opt = dict(PLAN_DEFAULTS, **_experiment_options())
        for k, v in (options or {}).items():
            if k not in PLAN_DEFAULTS:
                raise ValueError(f"unknown plan option {k!r} (known: {sorted(PLAN_DEFAULTS)})")
            self.opt[k] = bool(v)
        self.arch: Arch = build_arch(cfg)
        self.num_classes = self.arch.num_classes
        self._num_preds = self.arch.num_preds
        # DATA.MULTI_LABEL: sigmoid / binary cross-entropy head on [N, classes] targets instead of softmax on labels;
        # TEST.ENSEMBLE_METHOD: mean (x3d_view_mean) or max (x3d_view_max) over the views x crops of a video
        self.multi_label = multi_label(cfg)
        self.ensemble_method = ensemble_method(cfg)
        # DETECTION.ENABLE: the head classifies box slots instead of clips (x3d_roi_pool_fwd / _bwd; plan.py _rec_roi_pool); None: off
        det = detection_settings(cfg)
        self.det = det if det.enable else None
        self._bn_cfg = cfg.NETWORK.BN
        self.dtype = dtype
        self.in_channels = in_channels
        hip.dtype_code(dtype)
        self.dry = (device == "dry")
        if self.dry:
            self.device = torch.device("cpu")
        else:
            if not torch.cuda.is_available():
                raise hip.X3DHipError("X3D needs an MI355X: the HIP path has no CPU fallback")
            self.device = torch.device(device if device != "cuda" else f"cuda:{torch.cuda.current_device()}")
        hip.load()
        self._plans: Dict = {}
        self._build_params(seed)
        self._build_panels()
        self._build_layers()
        self._dropout_mask_override = None
        # stochastic depth (NETWORK.DROP_PATH_RATE): per-block rates, and -- only with a rate > 0 -- their fp32 device copy, the
        # scale 1 / (1 - rate) of a kept sample and the generator state (seed, step) of x3d_drop_path_draw
        self.drop_path_rates = drop_path_rates(self.arch)
        self._drop_path_mask_override = None
        self._dp_rates = self._dp_scale = self._dp_state = None
        if any(r > 0.0 for r in self.drop_path_rates) and not self.dry:
            r32 = torch.tensor(self.drop_path_rates, dtype=torch.float32)
            self._dp_rates = r32.to(self.device)
            self._dp_scale = (1.0 / (1.0 - r32)).to(self.device)         # fp32 arithmetic, as the draw kernel's
            self.set_drop_path_state(0)
        self.last_loss = None
        self.loss_mods = None          # class / positive weights and focal exponents of the training loss (set_loss); None: off
        self._stats_r = int(hip.load().x3d_stats_replicas())

    # ---------------------------------------------------------------------------------------------
    # parameters: one flat fp32 buffer (trainable first, then BN moving statistics), one flat
    # gradient buffer and one flat momentum buffer -- a single optimizer launch and contiguous
    # all-reduce buckets.
    # ---------------------------------------------------------------------------------------------
    def _build_params(self, seed):
        specs = param_specs(self.arch, self.in_channels)
        self.specs: Dict[str, ParamSpec] = {s.name: s for s in specs}
        order = [s for s in specs if s.trainable] + [s for s in specs if not s.trainable]
        init = init_params(self.arch, seed, self.in_channels)

        def numel(s):
            n = 1
            for d in s.shape:
                n *= d
            return n

        # pad every tensor to a multiple of 4 floats so views stay 16-byte aligned
        self._offsets = {}
        off = 0
        for s in order:
            self._offsets[s.name] = off
            off += (numel(s) + 3) // 4 * 4
            if s.trainable:
                self.n_trainable_flat = off
        self.flat_params = torch.zeros(off, dtype=torch.float32, device=self.device)
        self.flat_grads = torch.zeros(self.n_trainable_flat, dtype=torch.float32, device=self.device)
        self.flat_velocity = torch.zeros(self.n_trainable_flat, dtype=torch.float32, device=self.device)
        self.flat_second = None    # until an Adam-kind rule or an Adam checkpoint needs it (second_slot)
        self.slot_kind = None      # whose state the slot buffers hold: set by load_weights, then by the first update (_claim_slots)
        l2 = torch.zeros(self.n_trainable_flat, dtype=torch.uint8)
        self.params: Dict[str, torch.Tensor] = {}
        self.grads: Dict[str, torch.Tensor] = {}
        for s in order:
            o, n = self._offsets[s.name], numel(s)
            self.params[s.name] = self.flat_params[o:o + n].view(s.shape)
            self.params[s.name].copy_(init[s.name])
            if s.trainable:
                self.grads[s.name] = self.flat_grads[o:o + n].view(s.shape)
                if s.l2:
                    l2[o:o + n] = 1
        self.l2_mask = l2.to(self.device)
        self.param_order = [s.name for s in order]
        self.n_params = sum(numel(s) for s in order)
        self.n_trainable = sum(numel(s) for s in order if s.trainable)
        # the trainable tensors as segments of the flat buffers, in param_order: what the layer-wise optimizers (lars, adamw,
        # lamb) walk.  Their chunk table goes to the device with the first use (`seg_table`), once.
        self.segments = [Segment(s.name, self._offsets[s.name], numel(s), bool(s.l2)) for s in order if s.trainable]
        self._seg_table = None
        # fine-tuning (set_finetune): off -- every apply_* and the gradient reduction make the launches they always made
        self._ft = None
        self.tuned_segments, self.lr_scales, self.frozen_names = list(self.segments), {s.name: 1.0 for s in self.segments}, []
        self.frozen_prefix = 0     # units (stem, blocks) a training plan records in inference form (set_finetune freeze_eval)
        self.frozen_bn = ()        # BatchNorm layers a training plan normalises with their moving statistics (set_finetune freeze_bn)

    def _build_panels(self):
        """bf16 LDS-image panels of every pointwise-conv weight (x3d_pw_pack_weights): refreshed by one launch
        at the start of each forward so the GEMM workgroups copy their weight rows instead of converting them."""
        self._panels: Dict[str, tuple] = {}
        self._panel_table = None
        if self.dtype not in (torch.bfloat16, torch.float16):
            return
        lib = hip.load()
        names = [s.name for s in self.specs.values() if s.kind == "pw" and
                 (s.name.endswith(("/a/kernel", "/c/kernel", "/residual/kernel")) or s.name.startswith("conv5/"))]
        sizes = []
        for nm in names:
            cout, cin = self.specs[nm].shape
            sizes.append((lib.x3d_pw_panel_elems(cout, cin), lib.x3d_pw_panel_elems(cin, cout)))
        total = sum(a + b for a, b in sizes)
        self._panel_buf = torch.zeros(total, dtype=self.dtype, device=self.device)
        items = (hip.PwPackItem * len(names))()
        off = 0
        for i, (nm, (nf, nd)) in enumerate(zip(names, sizes)):   # panel sizes are multiples of 8 elements: 16-B aligned
            fp, dp = self._panel_buf[off:off + nf], self._panel_buf[off + nf:off + nf + nd]
            off += nf + nd
            cout, cin = self.specs[nm].shape
            items[i] = hip.PwPackItem(self.params[nm].data_ptr(), fp.data_ptr(), dp.data_ptr(), cout, cin)
            self._panels[nm] = (fp, dp)
        self._panel_table = torch.frombuffer(bytearray(bytes(items)), dtype=torch.uint8).to(self.device)
        self._n_panels = len(names)

    def _pack_panels(self):
        if self._panel_table is not None:
            hip.call("x3d_pw_pack_weights", self._panel_table.data_ptr(), self._n_panels, hip.dtype_code(self.dtype))

    def _wp(self, name, dgrad=False):
        pr = self._panels.get(name)
        return None if pr is None else pr[1 if dgrad else 0].data_ptr()

    def _bn(self, prefix):
        p = self.params
        return BatchNormalization(prefix, p[f"{prefix}/gamma"], p[f"{prefix}/beta"],
                                  p[f"{prefix}/moving_mean"], p[f"{prefix}/moving_variance"],
                                  self.arch.bn_eps, self.arch.bn_momentum)

    def _build_layers(self):
        p, a = self.params, self.arch
        self.conv1 = X3D_Stem("conv_1")
        self.conv1.conv_s = Conv3D("conv_s", p["conv1/conv_s/kernel"], kernel_size=(1, 3, 3), strides=(1, 2, 2))
        self.conv1.conv_t = Conv3D("conv_t", p["conv1/conv_t/kernel"], kernel_size=(a.c1_temp_filter, 1, 1),
                                   strides=(1, 1, 1), groups=a.c1)
        self.conv1.bn = self._bn("conv1/bn")
        self.conv1.relu = Activation("relu")
        self.stages = []
        for si, st in enumerate(a.stages):
            stage = ResStage(f"res_stage_{si + 2}")
            stage._inner_channels = st.inner
            stage.stage = _Sequential()
            for b in st.blocks:
                pre = block_prefix(b)
                q = f"{pre}/bottleneck"
                rb = ResBlock(f"ResBlock_{b.global_index - 1}")
                rb.in_channels, rb.inner_channels, rb.out_channels = b.cin, b.inner, b.cout
                if b.has_shortcut_conv:
                    rb.residual = Conv3D("residual", p[f"{pre}/residual/kernel"], kernel_size=(1, 1, 1),
                                         strides=(1, b.stride, b.stride))
                    rb.bn_r = self._bn(f"{pre}/bn_r")
                bt = Bottleneck("bottleneck")
                bt.block_index = b.global_index
                bt.a = Conv3D("a", p[f"{q}/a/kernel"], kernel_size=(1, 1, 1), strides=(1, 1, 1))
                bt.bn_a = self._bn(f"{q}/bn_a")
                bt.relu = Activation("relu")
                bt.b = Conv3D("b", p[f"{q}/b/kernel"], kernel_size=(3, 3, 3), strides=(1, b.stride, b.stride),
                              groups=b.inner, dilation_rate=(1, b.dilation, b.dilation))
                bt.bn_b = self._bn(f"{q}/bn_b")
                bt.swish = Activation("swish")
                if b.has_se:
                    bt.se_pool = AdaptiveAvgPool3D("se_pool")
                    bt.se_fc1 = Conv3D("se_fc1", p[f"{q}/se_fc1/kernel"], p[f"{q}/se_fc1/bias"])
                    bt.se_fc2 = Conv3D("se_fc2", p[f"{q}/se_fc2/kernel"], p[f"{q}/se_fc2/bias"])
                bt.c = Conv3D("c", p[f"{q}/c/kernel"], kernel_size=(1, 1, 1), strides=(1, 1, 1))
                bt.bn_c = self._bn(f"{q}/bn_c")
                rb.bottleneck = bt
                rb.add_op = Activation("add")
                rb.relu = Activation("relu")
                stage.stage.append(rb)
            self.stages.append(stage)
        self.conv5 = _Sequential([
            Conv3D("conv_5", p["conv5/layer_with_weights-0/kernel"], kernel_size=(1, 1, 1)),
            self._bn("conv5/layer_with_weights-1"), Activation("relu")])
        self.pool5 = AdaptiveAvgPool3D("pool_5")
        self.fc1 = Conv3D("fc_1", p["fc1/kernel"], kernel_size=(1, 1, 1))
        self.dropout = Dropout(a.dropout_rate)
        self.fc2 = Dense("fc_2", p["fc2/kernel"], p["fc2/bias"])
        self.softmax = Activation("softmax")

    # ---------------------------------------------------------------------------------------------
    def summary(self, input_shape, print_fn=print):
        """Same table as the reference's ``X3D.summary`` (model.py:129-132, models/X3D-*/X3D_*.txt)."""
        t, h, w, c = input_shape
        rows = summary_rows(self.arch, t, h, w, c)
        lines = ['Model: "X3D"', "_" * 65, f"{'Layer (type)':<29}{'Output Shape':<26}{'Param #':<10}", "=" * 65,
                 f"{'input_1 (InputLayer)':<29}{str([(None, t, h, w, c)]):<26}{0:<10}", "_" * 65]
        kinds = {"conv_1": "X3D_Stem", "conv_5": "Sequential", "pool_5": "AdaptiveAvgPool3D", "fc_1": "Conv3D",
                 "dropout": "Dropout", "fc_2": "Dense"}
        for name, shp, n in rows:
            kind = kinds.get(name, "ResStage")
            lines += [f"{name + ' (' + kind + ')':<29}{str((None,) + tuple(shp)):<26}{n:<10}", "_" * 65]
        lines[-1] = "=" * 65
        lines += [f"Total params: {self.n_params:,}", f"Trainable params: {self.n_trainable:,}",
                  f"Non-trainable params: {self.n_params - self.n_trainable:,}", "_" * 65]
        text = "\n".join(lines)
        if print_fn:
            print_fn(text)
        return text

    def state_dict(self):
        return {k: v.detach().clone() for k, v in self.params.items()}

    def load_state_dict(self, sd, strict=True):
        missing = [k for k in self.params if k not in sd]
        if strict and missing:
            raise KeyError(f"missing parameters: {missing[:5]}{'...' if len(missing) > 5 else ''}")
        for k, v in sd.items():
            if k in self.params:
                if tuple(v.shape) != tuple(self.params[k].shape):
                    raise ValueError(f"{k}: shape {tuple(v.shape)} vs {tuple(self.params[k].shape)}")
                self.params[k].copy_(v)
            elif strict:
                raise KeyError(f"unexpected parameter {k}")

    def load_weights(self, path, expect_partial=True, optimizer=None, skip_mismatch=False):
        """Keras-style ``load_weights`` on a TF tensor-bundle checkpoint prefix or directory
        (reference train.py:131-143, eval.py:78-81).  optimizer: "sgd" | "adam" -- the branch that will use the
        optimizer slots (slots written by the other branch are left at zero); None installs what the bundle holds.
        skip_mismatch: variables whose bundle shape differs from the model's (a 400-class fc2 loaded into a 157-class
        model) keep their current values and zero optimizer slots instead of raising; their names are returned (with one
        warning).  Returns the model, or with skip_mismatch=True the list of skipped variable names."""
        from .checkpoint import load_tf_checkpoint
        return load_tf_checkpoint(self, path, expect_partial=expect_partial, optimizer=optimizer,
                                  skip_mismatch=skip_mismatch)

    def _claim_slots(self, kind):
        """The slot buffers hold state of ONE optimizer branch (`slot_kind`: set by load_weights, then by the first update).
        An update of the other branch starts from zero slots, as a freshly built Keras optimizer does."""
        if self.slot_kind is not None and self.slot_kind != kind:
            self.zero_slots()
        self.slot_kind = kind

    def zero_slots(self):
        """Both slot buffers as a freshly built optimizer has them."""
        self.flat_velocity.zero_()
        if self.flat_second is not None:
            self.flat_second.zero_()

    def second_slot(self):
        """`flat_second`, the second slot buffer of the Adam-kind rules (v), allocated -- as zeros -- with the first use."""
        if self.flat_second is None:
            self.flat_second = torch.zeros_like(self.flat_velocity)
        return self.flat_second

    def _adam_slots(self):
        self._claim_slots("adam")
        self.second_slot()

    def save_weights(self, prefix, optimizer_hyper=None, optimizer="sgd"):
        from .checkpoint import save_tf_checkpoint
        return save_tf_checkpoint(self, prefix, optimizer_hyper, optimizer)

    # ---------------------------------------------------------------------------------------------
    # plans: recorded by plan.py, cached here
    # ---------------------------------------------------------------------------------------------
    MAX_PLANS = 3   # a plan owns every activation / gradient / scratch buffer of its shape (X3D-M, B = 64, bf16: ~16 GB)

    def _plan(self, n, t, h, w, training, logits_only=False) -> _Plan:
        """logits_only: the inference list that ends with fc2 (`logits`), a plan of its own beside the `call` one"""
        # (a training plan is recorded for one frozen prefix and one set of frozen BatchNorm layers: changing either never reuses
        # a stale plan)
        key = (n, t, h, w, False, "logits") if logits_only else ((n, t, h, w, True, self.frozen_prefix) if training and self.frozen_prefix
                                                                  else (n, t, h, w, bool(training)))
        if training and self.frozen_bn and not logits_only:
            key += (self.frozen_bn,)
        pl = self._plans.pop(key, None)
        if pl is None:
            self.release_plans(keep=self.MAX_PLANS - 1)
            if logits_only:
                pl = record_inference(self, n, t, h, w, probs=False)
            else:
                pl = record_training(self, n, t, h, w, self.frozen_prefix) if training else record_inference(self, n, t, h, w)
        self._plans[key] = pl           # most recently used last
        return pl

    def release_plans(self, keep: int = 0):
        """Drop all but the `keep` most recently used plans (their buffers return to the allocator once no launch that
        uses them is pending: the stream is synchronised first)."""
        if len(self._plans) <= keep:
            return
        if not self.dry:
            torch.cuda.synchronize(self.device)
        for key in list(self._plans)[:len(self._plans) - keep]:
            del self._plans[key]

    def _head_probs_only(self, pl: _Plan, n):
        """probabilities of a training plan's logits without a loss (call(training=True))"""
        name = "x3d_sigmoid_bce" if self.multi_label else "x3d_softmax_xent"
        hip.call(name, pl.logits.data_ptr(), None, pl.probs.data_ptr(), None, None, 1.0, n, self.num_classes)

    # ---------------------------------------------------------------------------------------------
    # execution
    # ---------------------------------------------------------------------------------------------
    def _bind_input(self, pl: _Plan, x):
        if self.dry:
            raise hip.X3DHipError("a dry model cannot run (no CPU fallback for the hot path)")
        if x.dim() != 5 or x.shape[-1] != self.in_channels:
            raise ValueError(f"expected a channels-last clip batch [N, T, H, W, {self.in_channels}], got {tuple(x.shape)}")
        if not x.is_cuda:
            x = x.to(self.device, non_blocking=True)
        x = x.contiguous()
        if x.dtype not in (torch.float32, torch.bfloat16, torch.float16) or (x.dtype != torch.float32 and x.dtype != self.dtype):
            x = x.float()
        n, t, h, w, c = x.shape
        if pl.x_cl:
            # the stem reads the batch where it lies: storage type of the model, 16-byte aligned (a copy only if it is neither)
            if x.dtype != self.dtype:
                x = x.to(self.dtype)
            if x.data_ptr() % 16:
                x = x.clone()
            for lst, i, *pos in pl.input_slots:
                k = pos[0] if pos else 0                   # (the batch is argument 0 of most stem launches, argument 4 of x3d_stem_bwd)
                name, fn, args = lst[i]
                lst[i] = (name, fn, tuple(args[:k]) + (x.data_ptr(),) + tuple(args[k + 1:]))
        else:
            hip.call("x3d_nthwc_to_ncthw", x.data_ptr(), hip.dtype_code(x.dtype), pl.x.data_ptr(),
                     hip.dtype_code(self.dtype), n, c, t * h * w)
        pl._x_keepalive = x      # (until the next batch is bound: the backward pass reads it again)

    def _draw_dropout(self, pl: _Plan):
        if pl.drop_mask is None:
            return
        if self._dropout_mask_override is not None:
            pl.drop_mask.copy_(self._dropout_mask_override.to(self.device, torch.float32))
        else:
            pl.drop_mask.bernoulli_(1.0 - self.arch.dropout_rate)

    def set_dropout_mask(self, mask: Optional[torch.Tensor]):
        """Fix the dropout keep-mask ([N, 2048] of 0/1) for reproducible parity tests; None = random."""
        self._dropout_mask_override = mask

    def _draw_drop_path(self, pl: _Plan):
        """The keep table of this replay: one x3d_drop_path_draw launch (it advances the step counter on the device: no host
        synchronisation, nothing to patch), or the override scaled by 1 / (1 - rate_l) -- then no launch, and no step."""
        if pl.dp_keep is None:
            return
        if self._drop_path_mask_override is not None:
            mask = self._drop_path_mask_override.to(self.device, torch.float32)
            if tuple(mask.shape) != tuple(pl.dp_keep.shape):
                raise ValueError(f"drop-path mask must be [blocks, N] = {tuple(pl.dp_keep.shape)}, got {tuple(mask.shape)}")
            torch.mul(mask, self._dp_scale.view(-1, 1), out=pl.dp_keep)
        else:
            hip.call("x3d_drop_path_draw", pl.dp_keep.data_ptr(), self._dp_rates.data_ptr(), self._dp_state.data_ptr(),
                     pl.dp_keep.shape[0], pl.n)

    def set_drop_path_mask(self, mask: Optional[torch.Tensor]):
        """Fix the stochastic-depth keep flags ([blocks, N] of 0/1, every residual block in network order; rows of blocks with
        rate 0 are ignored) for reproducible parity tests; the model scales them by 1 / (1 - rate_l).  None = drawn on the device."""
        self._drop_path_mask_override = mask

    def set_drop_path_state(self, seed: int, step: int = 0):
        """Seed and 64-bit step counter of the stochastic-depth draw: the table of a training replay is a function of (seed,
        step) alone, and every replay advances the step by one.  Without NETWORK.DROP_PATH_RATE there is no draw: a no-op."""
        if self._dp_rates is None:
            return
        st = ops.drop_path_state(seed, step, self.device)
        if self._dp_state is None:
            self._dp_state = st
        else:
            self._dp_state.copy_(st)

    def drop_path_step(self) -> Optional[int]:
        """The step the next draw will use (synchronises); None without NETWORK.DROP_PATH_RATE."""
        if self._dp_state is None:
            return None
        return ops.drop_path_step(self._dp_state)

    def __call__(self, input, training=False, boxes=None, num_boxes=None):
        return self.call(input, training, boxes, num_boxes)

    def call(self, input, training=False, boxes=None, num_boxes=None):
        """Forward pass (reference model.py:113-127).  Returns fp32 probabilities: ``[N, classes]`` when
        training, ``[N / (views*crops), classes]`` (views combined by TEST.ENSEMBLE_METHOD) otherwise.  With
        DATA.MULTI_LABEL the probabilities are per-class sigmoids instead of a softmax.

        DETECTION.ENABLE: boxes [N, K, 4] fp32 (x1, y1, x2, y2 in pixels of the clips as passed; K = DETECTION.MAX_BOXES) and
        num_boxes [N] (a HOST sequence or tensor: the valid count is taken from it without a device read) are required, and the
        result is ``[N, K, classes]`` with the rows of empty slots zeroed.  Boxes without the switch, or the switch without
        boxes, raise ValueError before any launch."""
        n, t, h, w, _ = input.shape
        nb = self._check_boxes(boxes, num_boxes, n)
        pl = self._plan(n, t, h, w, training)
        self._bind_input(pl, input)
        if self.det:
            self._bind_boxes(pl, boxes, nb)
        self._pack_panels()
        if training:
            pl.zero_buf.zero_()
            self._draw_dropout(pl)
            self._draw_drop_path(pl)
            # forward only: stop before the loss kernel (labels unknown); softmax (sigmoid) without labels
            pl.run(pl.fwd, 0, pl.grad_scale_slot)
            self._head_probs_only(pl, pl.rows)
            return self._box_rows(pl, pl.probs)
        pl.zero_buf.zero_()
        pl.run(pl.fwd)
        return self._box_rows(pl, pl.out)

    # -- DETECTION.ENABLE ----------------------------------------------------------------------------
    def _check_boxes(self, boxes, num_boxes, n):
        """The argument checks of the box head, before any plan is recorded or kernel launched; returns num_boxes as a host int64
        tensor [n] (None with the switch off)."""
        if self.det is None:
            if boxes is not None or num_boxes is not None:
                raise ValueError("boxes / num_boxes were given but DETECTION.ENABLE is off: this model classifies clips")
            return None
        k = self.det.max_boxes
        if boxes is None or num_boxes is None:
            raise ValueError(f"DETECTION.ENABLE: boxes [N, {k}, 4] and num_boxes [N] are required")
        if not torch.is_tensor(boxes):
            boxes = torch.as_tensor(boxes)
        if tuple(boxes.shape) != (n, k, 4) or not boxes.dtype.is_floating_point:
            raise ValueError(f"boxes must be a floating-point [{n}, {k}, 4] tensor (DETECTION.MAX_BOXES = {k}), got "
                             f"{tuple(boxes.shape)} {boxes.dtype}")
        if torch.is_tensor(num_boxes) and num_boxes.is_cuda:
            raise ValueError("num_boxes must live on the host: the number of valid boxes is taken from it without a device read")
        nb = torch.as_tensor(num_boxes).reshape(-1)
        if nb.numel() != n or nb.dtype.is_floating_point or nb.dtype == torch.bool or int(nb.min()) < 0 or int(nb.max()) > k:
            raise ValueError(f"num_boxes must be {n} integers in [0, {k}], got {nb.tolist() if nb.numel() <= 16 else tuple(nb.shape)}")
        return nb.to(torch.int64)

    def _bind_boxes(self, pl: _Plan, boxes, nb):
        """boxes / num_boxes -> the plan's own device buffers; box_mask [rows] = 1 for a filled slot.  Returns the number of
        filled slots (a host int)."""
        k = self.det.max_boxes
        if not torch.is_tensor(boxes):
            boxes = torch.as_tensor(boxes)
        if boxes.data_ptr() != pl.boxes.data_ptr():
            pl.boxes.copy_(boxes.to(self.device, non_blocking=True))
        pl.num_boxes.copy_(nb.to(torch.int32), non_blocking=True)
        mask = (torch.arange(k).view(1, k) < nb.view(-1, 1)).to(torch.float32).reshape(-1)
        pl.box_mask.copy_(mask, non_blocking=True)
        pl._box_keepalive = mask
        return int(nb.sum())

    def _box_rows(self, pl: _Plan, probs):
        """[rows, classes] -> [N, K, classes] with the rows of empty slots zeroed in place (switch off: `probs` as it is)"""
        if self.det is None:
            return probs
        probs.mul_(pl.box_mask.view(-1, 1))
        return probs.view(pl.n, self.det.max_boxes, -1)

    def logits(self, input):
        """Per-clip logits at training=False (moving statistics, no dropout): the launches of `call(input)` up to, but not
        including, the probabilities -- what a distillation teacher hands to the student's `forward_backward`.  Returns the
        plan-owned fp32 ``[N, classes]`` buffer on the device (overwritten by the next call of the same shape); N need not be
        a multiple of views * crops.  Nothing of the model's state is written."""
        n, t, h, w, _ = input.shape
        pl = self._plan(n, t, h, w, False, logits_only=True)
        self._bind_input(pl, input)
        self._pack_panels()
        pl.zero_buf.zero_()
        pl.run(pl.fwd)
        return pl.logits

    def set_loss(self, class_weights=None, pos_weight=None, focal_gamma: float = 0.0, focal_gamma_neg: float = 0.0):
        """The class-imbalance modifiers of the training loss (LOSS.* of the config; x3d_softmax_xent_w / x3d_sigmoid_bce_w in
        include/x3d_hip.h): class_weights [classes] on the hard term of either head, pos_weight [classes] on the positive
        term of the sigmoid head, the focal exponent focal_gamma (sigmoid head: of the positive term) and focal_gamma_neg (of
        the sigmoid head's negative term).  The tables (sequences, arrays or tensors) are checked here -- finite, >= 0, not
        all zero, one entry per class -- and uploaded once; every later `forward_backward` then launches the _w entry point
        of its head.  Everything at its default switches the modifiers off again: the plain entry points, launch for launch."""
        import math

        def table(what, w):
            if w is None:
                return None
            t = torch.as_tensor(w, dtype=torch.float64).detach().cpu().flatten()
            if t.numel() == 0:
                return None
            if t.numel() != self.num_classes:
                raise ValueError(f"{what} has {t.numel()} entries, the model has {self.num_classes} classes")
            if not bool(torch.isfinite(t).all()) or float(t.min()) < 0.0 or float(t.max()) <= 0.0:
                raise ValueError(f"{what} must be finite and >= 0, and not all zeros")
            return t.to(torch.float32).to(self.device)

        cw, pw = table("class_weights", class_weights), table("pos_weight", pos_weight)
        g, gneg = float(focal_gamma), float(focal_gamma_neg)
        for what, v in (("focal_gamma", g), ("focal_gamma_neg", gneg)):
            if not (0.0 <= v <= 8.0 and math.isfinite(v)):
                raise ValueError(f"{what} must lie in [0, 8], not {v}")
        if not self.multi_label and (pw is not None or gneg != 0.0):
            raise ValueError("pos_weight and focal_gamma_neg belong to the sigmoid head (DATA.MULTI_LABEL)")
        off = cw is None and pw is None and g == 0.0 and gneg == 0.0
        self.loss_mods = None if off else LossMods(cw, pw, g, gneg)

    def _bind_sample_weight(self, pl: _Plan, sample_weight, n):
        """sample weights [n] (host or device, any real type) -> pl.row_w fp32.  Host weights are checked (finite, >= 0); device
        weights by the kernel (a NaN, negative or infinite weight: NaN loss row, no gradient from the sample)."""
        w = sample_weight if torch.is_tensor(sample_weight) else torch.as_tensor(sample_weight)
        if w.numel() != n or w.dim() > 1 or w.dtype == torch.bool or w.is_complex():
            raise ValueError(f"sample_weight must be {n} real numbers, got {tuple(w.shape)} {w.dtype}")
        if not w.is_cuda:
            wd = w.double()
            if not bool(torch.isfinite(wd).all()) or float(wd.min()) < 0.0:
                raise ValueError("sample_weight must be finite and >= 0")
        if w.data_ptr() != pl.row_w.data_ptr():
            pl.row_w.copy_(w.to(self.device, non_blocking=True).reshape(n))

    def forward_backward(self, input, labels, global_batch=None, on_stage_done=None, loss_scale=1.0, teacher_logits=None,
                         distill=None, sample_weight=None, boxes=None, num_boxes=None):
        """One training forward + backward.  Fills ``self.grads`` (data gradients only; the L2 term is
        applied by the optimizer), updates BN moving statistics, returns the plan (loss_rows, probs).

        labels: [N] class indices; with DATA.MULTI_LABEL the targets [N, classes] in [0, 1] (float, uint8 or bool;
            multi-hot or soft), and the loss is Keras BinaryCrossentropy on sigmoid outputs (x3d_sigmoid_bce).
            A single-label model also takes soft targets [N, classes] (floating point, finite, >= 0: label smoothing,
            mixup / CutMix) and then runs x3d_softmax_xent_soft instead of x3d_softmax_xent; `plan.labels` is not touched.

        global_batch: divisor of the loss mean (defaults to the local batch; data-parallel callers pass
            world_size * local batch so that summing gradients over ranks gives the global mean).
        loss_scale: every gradient is multiplied by this factor (Keras LossScaleOptimizer, reference train.py:99-100:
            keeps fp16 activation gradients out of the denormal range); the optimizer step divides it out again
            (`apply_sgd(grad_scale=1 / loss_scale)`).  The backward kernels are linear in the upstream gradient.
            Also the device state of the loss scaler (ops.loss_scale_state, a [8] fp64 device tensor): the head then takes
            1 / global_batch and x3d_loss_scale_apply multiplies dlogits by the state's scale right behind it -- the scale is
            a power of two, so the backward pass sees the bits a host number would have given it -- and `unscale_norm_sq`
            divides it out again.
        on_stage_done(stage): called with "fwd" once the forward pass is on the stream, then as soon as every
            gradient of ``stage`` (4 = head, 3..0 = stages, -1 = stem) is final on the stream -- the hook gradient
            all-reduce buckets attach to.
        teacher_logits, distill=(alpha, temperature): knowledge distillation.  teacher_logits: a device fp32 [N, classes]
            tensor (a teacher's `logits(input)`); the loss of whichever head applies becomes (1 - alpha) * that loss +
            alpha * T^2 * KL(teacher || student) at temperature T (x3d_softmax_xent_kd / x3d_sigmoid_bce_kd), `plan.kd_rows`
            holds the KD term per row and `plan.teacher` the logits.  The shape is checked here, the values by the kernel
            (a non-finite teacher logit: NaN loss row, no gradient from the sample).  Without teacher_logits nothing changes.
        sample_weight: [N] weights of the samples (host or device), Keras' `(x, y, sample_weight)`: row n's loss and gradient
            are multiplied by sample_weight[n] and still divided by global_batch (SUM_OVER_BATCH_SIZE).  0 is a valid weight;
            `plan.row_w` holds them.  With it, or with `set_loss` modifiers, the head runs x3d_softmax_xent_w /
            x3d_sigmoid_bce_w; with neither nothing changes.
        boxes [N, K, 4], num_boxes [N] (host): DETECTION.ENABLE, as `call` takes them.  labels are then [N, K] class indices (with
            DATA.MULTI_LABEL: targets [N, K, classes]); those of empty slots are not used (indices are replaced by 0, targets must
            be finite).  The head runs its _w entry point on N * K rows with `plan.row_w` = N * K / max(valid, 1) for a filled
            slot and 0 for an empty one, and divides by global_batch * K: loss and gradient are the mean over this rank's valid
            boxes, and data-parallel averaging stays what it is.  A filled slot whose box is degenerate or not finite pools
            zeros and still counts.  sample_weight and teacher_logits are refused with boxes.
        """
        n, t, h, w, _ = input.shape
        nb = self._check_boxes(boxes, num_boxes, n)
        rows = n * self.det.max_boxes if self.det else n
        if self.det:
            if sample_weight is not None or teacher_logits is not None:
                raise ValueError("DETECTION.ENABLE: sample_weight / teacher_logits cannot be combined with boxes (the row weights "
                                 "carry the valid-box mean)")
            if not torch.is_tensor(labels):
                labels = torch.as_tensor(labels)
            want = (n, self.det.max_boxes) + ((self.num_classes,) if self.multi_label or labels.dim() == 3 else ())
            if tuple(labels.shape) != want:
                raise ValueError(f"DETECTION.ENABLE: labels must be {list(want)}, got {list(labels.shape)}")
            labels = labels.reshape((rows,) + want[2:])
        pl = self._plan(n, t, h, w, True)
        self._bind_input(pl, input)
        soft = (not self.multi_label and torch.is_tensor(labels) and labels.dim() == 2
                and labels.dtype.is_floating_point)
        kd = teacher_logits is not None
        if kd:
            if distill is None:
                raise ValueError("teacher_logits needs distill=(alpha, temperature)")
            kd_alpha, kd_temp = (float(v) for v in distill)
            if not torch.is_tensor(teacher_logits) or not teacher_logits.is_cuda or teacher_logits.dtype != torch.float32 \
                    or tuple(teacher_logits.shape) != (n, self.num_classes):
                got = (tuple(teacher_logits.shape), teacher_logits.dtype, teacher_logits.device) \
                    if torch.is_tensor(teacher_logits) else type(teacher_logits)
                raise ValueError(f"teacher_logits must be a device float32 [{n}, {self.num_classes}] tensor, got {got}")
        rw = sample_weight is not None or self.det is not None
        weighted = rw or self.loss_mods is not None
        pl.use_soft_targets(soft, distill=kd, weighted=weighted, row_w=rw)
        if self.det:
            valid = self._bind_boxes(pl, boxes, nb)
            torch.mul(pl.box_mask, float(rows) / max(valid, 1), out=pl.row_w)
        elif rw:
            self._bind_sample_weight(pl, sample_weight, n)
        if self.multi_label:
            self._bind_targets(pl, labels, rows)
        elif soft:
            self._bind_targets(pl, labels, rows, what="soft")
        else:
            if not labels.is_cuda:   # host labels are validated for free; device labels by the kernel (NaN loss row, zero gradient)
                used = labels.reshape(-1)[pl._box_keepalive.bool()] if self.det else labels
                if labels.numel() != rows or (used.numel() and (int(used.min()) < 0 or int(used.max()) >= self.num_classes)):
                    raise ValueError(f"labels must be {rows} class indices in [0, {self.num_classes})")
            pl.labels.copy_(labels.to(self.device, non_blocking=True).to(torch.int32))
            if self.det:             # the label of an empty slot is never an index the kernel could refuse
                pl.labels.mul_(pl.box_mask.to(torch.int32))
        # (round 4: the panel packing, the gradient-buffer zeroing and the dropout draw -- ~70 us the stem does not depend on -- on a
        # second stream beside the stem's two convolutions, joined in front of the first pointwise conv: 22.30 -> 22.63 ms per step,
        # three alternating runs on one box; the fork / join costs more than it hides.  Not kept.)
        self._pack_panels()
        pl.zero_buf.zero_()
        self.flat_grads.zero_()
        self._draw_dropout(pl)
        self._draw_drop_path(pl)
        gb = float(global_batch or n) * (self.det.max_boxes if self.det else 1)
        on_device = torch.is_tensor(loss_scale)          # the device state of the loss scaler: the head takes 1 / gb, the scale follows
        head_scale = (1.0 if on_device else float(loss_scale)) / gb
        if kd and teacher_logits.data_ptr() != pl.teacher.data_ptr():
            pl.teacher.copy_(teacher_logits)
        pl.run(pl.fwd, 0, pl.grad_scale_slot)
        name, args = pl.head_launch(soft, kd, head_scale, *((kd_alpha, kd_temp) if kd else ()),
                                    **(dict(weighted=True, row_w=rw) if weighted else {}))
        hip.call(name, *args)
        if on_device:
            ops.loss_scale_apply(pl.dlogits.view(-1), loss_scale)
        if on_stage_done is None:
            pl.run(pl.bwd)
        else:
            on_stage_done("fwd")      # forward (and the BN moving-statistics updates in it) is on the stream
            marks = sorted(pl.bwd_stage_marks.items(), key=lambda kv: kv[1])
            start = 0
            for stage, stop in marks:
                pl.run(pl.bwd, start, stop)
                on_stage_done(stage)
                start = stop
        return pl

    def _bind_targets(self, pl: _Plan, targets, n, what="multi-label"):
        """multi-label targets [n, classes] (float / uint8 / bool) -> pl.targets fp32.  Host targets are checked for shape
        and range (they are on the host anyway); device targets for shape only.  what="soft": the dense target rows of a
        single-label model (label smoothing, mixup / CutMix): finite and >= 0."""
        if not torch.is_tensor(targets):
            targets = torch.as_tensor(targets)
        if tuple(targets.shape) != (n, self.num_classes):
            raise ValueError(f"{what} targets must be [{n}, {self.num_classes}], got {tuple(targets.shape)}")
        if not (targets.dtype.is_floating_point or targets.dtype in (torch.uint8, torch.bool)):
            raise ValueError(f"{what} targets must be float, uint8 or bool, got {targets.dtype}")
        if not targets.is_cuda:
            t = targets.float()
            if what == "soft":
                if not bool(torch.isfinite(t).all()) or float(t.min()) < 0.0:
                    raise ValueError("soft targets must be finite and >= 0")
            elif not bool(torch.isfinite(t).all()) or float(t.min()) < 0.0 or float(t.max()) > 1.0:
                raise ValueError("multi-label targets must lie in [0, 1]")
        if targets.data_ptr() != pl.targets.data_ptr():     # (the trainer builds mixed targets in pl.targets itself)
            pl.targets.copy_(targets.to(self.device, non_blocking=True))

    def regularization_loss(self):
        """weight_decay * sum(w^2) over the L2-regularised kernels (reference model.py:47)."""
        acc = torch.zeros(1, dtype=torch.float64, device=self.device)
        hip.call("x3d_l2_sumsq", self.flat_params.data_ptr(), self.l2_mask.data_ptr(), acc.data_ptr(),
                 self.n_trainable_flat)
        return acc * self.arch.weight_decay

    def _solver_form(self, rule=None):
        """The one choice of where a solver launch goes, as ops.solver_launch's keywords.  set_finetune active: the tuned chunk
        table, its scales and scratch -- the _pt entry points and x3d_seg_grad_sumsq.  Otherwise the whole flat block under the
        byte mask for a rule with flat entry points and for the gradient reductions (rule None), the full `seg_table` for the
        other rules."""
        ft = self._ft
        if ft is not None:
            return dict(table=ft.table, pt=True, lr_scale=ft.scale, partials=ft.partials, q=ft.trust_ratios)
        if rule is None or rule.flat:
            return dict(mask=self.l2_mask, n=self.n_trainable_flat)
        return dict(table=self.seg_table, partials=self._seg_partials, q=self.trust_ratios)

    def _norm_buffers(self):
        """the scratch and the [2] fp64 result of the gradient reductions, allocated by the first of them"""
        if getattr(self, "_norm_out", None) is None:
            n_scratch = int(hip.load().x3d_grad_sumsq_scratch(self.n_trainable_flat))
            self._norm_scratch = torch.empty(n_scratch, dtype=torch.float64, device=self.device)
            self._norm_out = torch.zeros(2, dtype=torch.float64, device=self.device)

    def grad_norm_sq(self):
        """x3d_grad_sumsq over `flat_grads` into buffers the model keeps: the device [2] fp64 tensor (sum of squares of the
        raw gradient, number of non-finite entries) the `norm=` of the apply_* methods reads.  Two launches, no
        synchronisation; the tensor is overwritten by the next call."""
        self._norm_buffers()
        form = self._solver_form()
        if "table" in form:                   # the tuned tensors only, as clip_grad_norm_ over the requires_grad parameters
            return ops.seg_grad_sumsq(self.flat_grads, form["table"], self._norm_out, form["partials"])
        hip.call("x3d_grad_sumsq", self.flat_grads.data_ptr(), form["n"], self._norm_scratch.data_ptr(),
                 self._norm_out.data_ptr())
        return self._norm_out

    def unscale_norm_sq(self, state):
        """`grad_norm_sq` for a gradient that carries the loss scale of the device state `state` (ops.loss_scale_state):
        x3d_unscale_sumsq -- with set_finetune x3d_seg_unscale_sumsq over the tuned tensors -- divides the scale out of
        `flat_grads` in place and leaves (sum of squares of the unscaled gradient, number of non-finite entries) in the same
        device [2] fp64 tensor.  A frozen tensor's gradient keeps its (scaled) bits.  Two launches, no synchronisation."""
        self._norm_buffers()
        form = self._solver_form()
        if "table" in form:
            return ops.seg_unscale_sumsq(self.flat_grads, form["table"], state, self._norm_out, form["partials"])
        return ops.unscale_sumsq(self.flat_grads[:form["n"]], state, self._norm_out, self._norm_scratch)

    def _apply(self, rule, norm, max_norm, ema, ema_decay, **scalars):
        """One update of solver.RULES[rule], for every apply_*: claims the slot buffers for the rule's slot kind (zeroed when the
        other kind held them), checks that `ema` also holds the padding behind the last tensor -- the chunk tables end before
        it, so ops.solver_launch cannot know -- and makes the launch in the form `_solver_form` chooses.  Returns the device
        trust ratios of a rule that computes them."""
        r = RULES[rule]
        self._claim_slots(r.slot_kind)
        slots = (self.flat_velocity, self.second_slot()) if r.slot_kind == "adam" else (self.flat_velocity,)
        if ema is not None and ema.numel() < self.n_trainable_flat:
            raise ValueError(f"apply_{rule}: ema must hold at least {self.n_trainable_flat} elements, got {ema.numel()}")
        if "weight_decay" in r.scalars:       # the coupled L2 term is the architecture's (NETWORK.WEIGHT_DECAY)
            scalars["weight_decay"] = self.arch.weight_decay
        return ops.solver_launch("apply_" + rule, rule, self.flat_params, slots, self.flat_grads, norm=norm, max_norm=max_norm,
                                 ema=ema, ema_decay=ema_decay, **self._solver_form(r), **scalars)

    def apply_sgd(self, lr, momentum=0.9, grad_scale=1.0, norm=None, max_norm=0.0, ema=None, ema_decay=0.0):
        """SGD(momentum, nesterov=True) + L2 (reference train.py:89-92, model.py:47), one launch.
        norm (grad_norm_sq()) + max_norm: the gradient is clipped to that global L2 norm and a non-finite gradient skips
        the update, both decided on the device; ema: a flat fp32 buffer that receives ema_decay * ema + (1 - ema_decay) * w
        in the same pass (x3d_sgd_nesterov_ex).  With neither this is the x3d_sgd_nesterov launch it always was."""
        self._apply("sgd", norm, max_norm, ema, ema_decay, lr=lr, momentum=momentum, grad_scale=grad_scale)

    def apply_adam(self, lr, step, beta1=0.9, beta2=0.999, eps=1e-7, grad_scale=1.0, norm=None, max_norm=0.0, ema=None,
                   ema_decay=0.0):
        """Adam + L2 (reference train.py:93-95: tf.optimizers.Adam(learning_rate), Keras defaults), one launch.  The first
        moment lives in `flat_velocity` (the slot the SGD branch uses for momentum), the second in `flat_second`.
        norm / max_norm / ema / ema_decay: as apply_sgd (x3d_adam_ex)."""
        self._apply("adam", norm, max_norm, ema, ema_decay, lr=lr, step=step, beta1=beta1, beta2=beta2, eps=eps,
                    grad_scale=grad_scale)

    # -- the layer-wise optimizers: a fixed number of launches over the chunk table, per-tensor trust ratios on the device --
    def apply_lars(self, lr, momentum=0.9, trust_coef=0.001, eps=1e-8, clip=False, grad_scale=1.0, norm=None, max_norm=0.0,
                   ema=None, ema_decay=0.0):
        """LARS: SGD(momentum, nesterov=True) + L2 with the update of every conv / dense kernel scaled by its trust ratio
        q_t = trust_coef ||w_t|| / (c ||g_t|| + 2 wd ||w_t|| + eps) (clip: min(q_t / lr, 1)); BatchNorm and bias tensors take
        q_t = 1 (x3d_lars, the rule is in include/x3d_hip.h).  Slot and checkpoint layout: SGD's.  Three launches, no
        synchronisation.  norm / max_norm / ema / ema_decay: as apply_sgd.  Returns the device [nseg] fp32 trust ratios (in
        `segments` order), overwritten by the next call."""
        return self._apply("lars", norm, max_norm, ema, ema_decay, lr=lr, momentum=momentum, trust_coef=trust_coef, eps=eps,
                           clip=clip, grad_scale=grad_scale)

    def apply_adamw(self, lr, step, beta1=0.9, beta2=0.999, eps=1e-7, decay=0.0, grad_scale=1.0, norm=None, max_norm=0.0,
                    ema=None, ema_decay=0.0):
        """Adam with DECOUPLED weight decay: apply_adam's step without the coupled L2 term (NETWORK.WEIGHT_DECAY plays no part),
        then w -= lr * decay * w_old on the conv / dense kernels (x3d_adamw).  Slots and checkpoint layout: Adam's.  One launch."""
        self._apply("adamw", norm, max_norm, ema, ema_decay, lr=lr, step=step, beta1=beta1, beta2=beta2, eps=eps, decay=decay,
                    grad_scale=grad_scale)

    def apply_lamb(self, lr, step, beta1=0.9, beta2=0.999, eps=1e-6, decay=0.0, grad_scale=1.0, norm=None, max_norm=0.0,
                   ema=None, ema_decay=0.0):
        """LAMB: Adam's moments, u = r_k m / (sqrt(v) + eps) + decay w, and w -= lr q_t u with q_t = ||w_t|| / ||u_t|| on the conv
        / dense kernels, 1 elsewhere (x3d_lamb).  NETWORK.WEIGHT_DECAY plays no part.  Slots and checkpoint layout: Adam's.
        Three launches, no synchronisation.  Returns the device [nseg] fp32 trust ratios, overwritten by the next call."""
        return self._apply("lamb", norm, max_norm, ema, ema_decay, lr=lr, step=step, beta1=beta1, beta2=beta2, eps=eps,
                           decay=decay, grad_scale=grad_scale)

    @property
    def seg_table(self):
        """segments.SegTable of `self.segments`, on the model's device (built and copied once)."""
        if self._seg_table is None:
            self._seg_table = SegTable(self.segments).to(self.device)
            self._seg_partials = torch.empty(2 * self._seg_table.nchunk, dtype=torch.float64, device=self.device)
            self.trust_ratios = torch.ones(self._seg_table.nseg, dtype=torch.float32, device=self.device)
        return self._seg_table

    def set_finetune(self, freeze=(), lr_mult=(), layer_decay=1.0, freeze_eval=False, freeze_bn=()):
        """Fine-tuning (SOLVER.FREEZE / LR_MULT / LAYER_DECAY, finetune.py): freeze the trainable tensors whose names start with
        a prefix of `freeze`, and give every other ("tuned") tensor the learning rate lr * scale, scale = layer_decay ** (D -
        depth group) * factor of the longest `lr_mult` prefix ([(prefix, factor), ...]).  Builds and keeps the chunk table of
        the tuned segments and their fp32 scales on the device, `tuned_segments`, `lr_scales` (name -> scale, frozen names
        absent) and `frozen_names`.  While set, apply_sgd / adam / lars / adamw / lamb make the x3d_*_pt launches, grad_norm_sq
        makes x3d_seg_grad_sumsq's and grads_finite reads its count: a frozen tensor's weights, slots and EMA are never read or
        written and its gradient is in neither the norm nor the finite check; the trust ratios apply_lars / apply_lamb return
        are [len(tuned_segments)], in that order.  Without arguments: cleared, every method makes the launches it always made.
        By itself this does not change the forward and backward passes: frozen tensors' gradients are still computed, BatchNorm
        in frozen layers still uses batch statistics and updates its moving statistics.
        freeze_eval (SOLVER.FREEZE_EVAL): the passes are cut for the frozen PREFIX, `frozen_prefix` = finetune.frozen_prefix --
        the stem and the blocks behind it as far as every trainable tensor is frozen.  Training plans recorded from now on run
        those units as training=False runs them (moving statistics, not updated; never dropped by NETWORK.DROP_PATH_RATE;
        nothing kept) and end their backward list at the first unit above them: the prefix tensors' slices of `flat_grads`
        stay at the zero forward_backward writes.  Frozen tensors outside the prefix behave as described above.  ValueError
        when the stem is not fully frozen (an empty prefix), naming the first tensor that breaks the run.
        freeze_bn (SOLVER.FREEZE_BN): name prefixes of BatchNorm layers (finetune.frozen_bn_layers; "" = every layer) that training
        plans recorded from now on normalise with their moving statistics, which the step then leaves bit-identical; their
        backward pass is dYraw = gamma * invstd * g, gamma and beta still get their gradients.  Independent of
        the other arguments: the layers it names may be trained or frozen, inside or outside a prefix (a prefix layer is in that
        form anyway).  `frozen_bn`: the layers, in layout order.  ValueError for a prefix that matches no BatchNorm layer."""
        from .finetune import _prefix_break, frozen_bn_layers, lr_scales
        if isinstance(freeze_bn, str) or not all(isinstance(p, str) for p in freeze_bn):
            raise ValueError(f"set_finetune: freeze_bn must be a sequence of name prefixes (str), not {freeze_bn!r}")
        fbn = frozen_bn_layers([self.specs[n] for n in self.param_order], tuple(freeze_bn))
        st = FinetuneSettings(float(layer_decay), tuple((str(p), float(f)) for p, f in lr_mult), tuple(freeze))
        if not 0.0 < st.layer_decay <= 1.0 or not all(f > 0.0 and f < float("inf") for _, f in st.lr_mult):
            raise ValueError(f"set_finetune: layer_decay must lie in (0, 1] and every factor must be finite and > 0, not "
                             f"{layer_decay}, {list(lr_mult)}")
        if st == FinetuneSettings(1.0, (), ()):
            if freeze_eval:
                raise ValueError("set_finetune: freeze_eval needs a `freeze` list that freezes the stem (conv1/) at least")
            self._ft, self.frozen_prefix, self.frozen_bn = None, 0, fbn
            self.tuned_segments, self.lr_scales, self.frozen_names = list(self.segments), {s.name: 1.0 for s in self.segments}, []
            return
        tuned, scales, frozen = lr_scales(self.arch, [self.specs[n] for n in self.param_order], st)
        if not set(tuned) <= set(self.segments):
            raise RuntimeError("finetune.flat_segments and the model's parameter layout disagree")
        k = 0
        if freeze_eval:
            k, broke = _prefix_break(self.arch, [self.specs[n] for n in self.param_order], frozen)
            if k == 0:
                raise ValueError(f"set_finetune: freeze_eval needs a frozen prefix, but {broke} (the stem) is not frozen by "
                                 f"{list(st.freeze)}: nothing would run in inference form")
        ft = types.SimpleNamespace()
        ft.table = SegTable(tuned)
        if not self.dry:
            ft.table.to(self.device)
            ft.scale = torch.tensor(scales, dtype=torch.float32).to(self.device)
            ft.partials = torch.empty(2 * ft.table.nchunk, dtype=torch.float64, device=self.device)
            ft.trust_ratios = torch.ones(ft.table.nseg, dtype=torch.float32, device=self.device)
        self._ft, self.frozen_prefix, self.frozen_bn = ft, k, fbn
        self.tuned_segments, self.lr_scales, self.frozen_names = tuned, {s.name: c for s, c in zip(tuned, scales)}, frozen

    def grads_finite(self) -> bool:
        """True when every entry of the flat gradient buffer is finite (x3d_all_finite; synchronises).  With set_finetune:
        every entry of the TUNED tensors' gradients -- the count x3d_seg_grad_sumsq leaves in grad_norm_sq()'s result."""
        if "table" in self._solver_form():
            return float(self.grad_norm_sq()[1].item()) == 0.0
        if getattr(self, "_finite_flag", None) is None:
            self._finite_flag = torch.ones(1, dtype=torch.int32, device=self.device)
        self._finite_flag.fill_(1)
        hip.call("x3d_all_finite", self.flat_grads.data_ptr(), self.n_trainable_flat, self._finite_flag.data_ptr())
        return bool(self._finite_flag.item())

    def grad_bucket(self, stage):
        """Contiguous slice of the flat gradient buffer holding the gradients of one stage
        (4 = conv5 + head, 0..3 = residual stages, -1 = stem)."""
        names = [k for k in self.param_order if k in self.grads]
        if stage == -1:
            sel = [k for k in names if k.startswith("conv1/")]
        elif stage == len(self.arch.stages):
            sel = [k for k in names if k.startswith(("conv5/", "fc1/", "fc2/"))]
        else:
            sel = [k for k in names if k.startswith(f"stages/{stage}/")]
        lo = self._offsets[sel[0]]
        last = sel[-1]
        hi = self._offsets[last] + (self.params[last].numel() + 3) // 4 * 4
        return self.flat_grads[lo:hi]

    def moving_stats_flat(self):
        return self.flat_params[self.n_trainable_flat:]

    def trained_moving_stats_flat(self):
        """`moving_stats_flat()` without the statistics of a frozen prefix in inference form, which no training step writes:
        what data-parallel training averages over the ranks (x + x + x over three ranks, divided by three, need not give x
        back; the prefix is to stay bit-identical).  The moving statistics lie in network order, so the prefix's are the
        head of the block; without a prefix this is the whole block."""
        if not self.frozen_prefix:
            return self.moving_stats_flat()
        from .finetune import depth_groups
        group, _ = depth_groups(self.arch)
        stats = [k for k in self.param_order if not self.specs[k].trainable]
        cut = next((i for i, k in enumerate(stats) if group(k) >= self.frozen_prefix), len(stats))
        if any(group(k) < self.frozen_prefix for k in stats[cut:]):
            raise RuntimeError("the moving statistics are not laid out in network order")
        lo = self._offsets[stats[cut]] if cut < len(stats) else self.flat_params.numel()
        return self.flat_params[lo:]

    def precise_bn_layout(self):
        """Where precise BatchNorm (precise_bn.update_bn_stats) keeps and writes each layer's statistics: a PreciseBNLayout of
        parallel tuples over the BatchNorm layers, in `param_order` of their moving means -- `prefixes`, `channels`,
        `mean_offsets` / `var_offsets` (elements into `flat_params`), `pooled_offsets` (elements into the fp64 pooled buffer:
        the layer's [C][2] sums, behind one count slot per layer) -- and `pooled_size`, that buffer's length.  A function of
        the architecture alone: plans of different (N, T, H, W) share one pooled buffer (_Plan.precise_bn_table)."""
        if getattr(self, "_pbn_layout", None) is None:
            prefixes = [k[:-len("/moving_mean")] for k in self.param_order if k.endswith("/moving_mean")]
            channels = [self.params[f"{q}/moving_mean"].numel() for q in prefixes]
            pooled, off = [], len(prefixes)
            for c in channels:
                pooled.append(off)
                off += 2 * c
            self._pbn_layout = PreciseBNLayout(tuple(prefixes), tuple(channels),
                                               tuple(self._offsets[f"{q}/moving_mean"] for q in prefixes),
                                               tuple(self._offsets[f"{q}/moving_variance"] for q in prefixes), tuple(pooled), off)
        return self._pbn_layout
