"""SOLVER.DEVICE_LOSS_SCALE on the device: the four entry points of the loss scaler against fp64 on the host, against their
sibling kernels (x3d_grad_sumsq / x3d_seg_grad_sumsq) and against tests/loss_scale_ref.py, and a trainer with the switch on
against the same trainer with it off -- bit for bit, because the scale is a power of two.

Exactness.  With S = 2^k every product g * S and g * (1 / S) is exact unless it falls below the smallest normal fp32; the data
here keeps all of them normal (magnitudes in [1e-6, 1e3], S <= 2^40).  So `g` after the launch is exactly g * 2^-k, every fp64
square is the sibling's times 2^-2k, and -- the walks adding in the same fixed order -- out[0] * S^2 has the sibling's bits.
Against fp64 on the host (math.fsum, exact) the kernel's sum of n non-negative fp64 terms, each a rounded FMA, is within
(n + 1) * 2^-52 relative, whatever the order.

The trainer pairs: the on arm divides S out of the gradient where the off arm hands 1 / S to the update as grad_scale, and the
clip factor is the same fp64 quantity in both.  Weights, slots, EMA, moving statistics, the scale, the counters: equal after
every step, no tolerance.  One thing has to be arranged for that: training is not reproducible to the bit from one run to the
next (fp32 atomics in some weight-gradient kernels), so two trainers that each run their own backward pass differ in
last bits whatever the switch says.  `_Twin` therefore hands every backward result of the on arm -- the scaled gradient and the
moving statistics, as forward_backward left them -- to the off arm, which has run its own forward_backward on the same batch
and adopts them in its place; everything behind that point is deterministic and compared as it stands.  That the on arm's
backward pass starts from the bits the off arm's would have started from (the head at 1 / batch, then x3d_loss_scale_apply,
against the head at S / batch) is checked on its own, on dlogits."""
import collections
import importlib.util
import json
import math
import os

import numpy as np
import pytest
import torch

import x3d_tf_amd as x
from x3d_tf_amd import hip, ops
from x3d_tf_amd.segments import SegTable

from tests import loss_scale_ref as R

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LENGTHS = (1, 3, 4, 5, 1023, 1024, 1025, 70001)
SCALES = (1.0, 2.0 ** 15, 2.0 ** 40)
GUARD = 8              # sentinel floats on either side of a gradient
SENTINEL = 7.0
INVALID = 1            # X3D_ERR_INVALID


def _gradient(n, seed):
    """n seeded normal values with magnitudes clamped into [1e-6, 1e3] (fp32, host)"""
    gen = torch.Generator().manual_seed(seed)
    g = torch.randn(n, generator=gen) * torch.pow(10.0, torch.empty(n).uniform_(-3.0, 1.0, generator=gen))
    return torch.sign(g) * g.abs().clamp(1e-6, 1e3) + (g == 0).float() * 1e-3


def _poison(g):
    """a few inf / nan entries; returns their number"""
    n = g.numel()
    at = sorted({0, n // 2, n - 1})
    for k, i in enumerate(at):
        g[i] = (float("inf"), float("nan"), float("-inf"))[k % 3]
    return len(at)


def _place(values, offset, gpu):
    """`values` on the device at `offset` floats behind a 16-byte aligned base, sentinels around it: (buffer, view)"""
    buf = torch.full((offset + values.numel() + 2 * GUARD,), SENTINEL, dtype=torch.float32)
    buf[offset + GUARD:offset + GUARD + values.numel()] = values
    buf = buf.to(gpu)
    assert buf.data_ptr() % 16 == 0
    return buf, buf[offset + GUARD:offset + GUARD + values.numel()]


def _bits(t):
    return t.detach().cpu().contiguous().view(torch.int32 if t.dtype == torch.float32 else torch.int64)


def _same_bits(a, b):
    """equal bit for bit; NaNs only have to be NaNs in the same places"""
    a, b = a.detach().cpu(), b.detach().cpu()
    nan = torch.isnan(a)
    return bool(torch.equal(nan, torch.isnan(b)) and torch.equal(_bits(a)[~nan], _bits(b)[~nan]))


def _host_sumsq(g):
    """(exact fp64 sum of squares of the finite entries, number of non-finite ones)"""
    d = g.double().numpy()
    fin = np.isfinite(d)
    return math.fsum((d[fin] * d[fin]).tolist()), int((~fin).sum())


# ---- x3d_unscale_sumsq ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", LENGTHS)
def test_unscale_sumsq(gpu, n):
    for scale in SCALES:
        for offset in (0, 1):                       # 16-byte aligned (vectors of four), and one float behind it (by element)
            for poisoned in (False, True):
                g = _gradient(n, 100 + n)
                bad = _poison(g) if poisoned else 0
                scaled = g * scale                  # exact: what the backward pass leaves
                state = ops.loss_scale_state(scale, gpu)
                buf, view = _place(scaled, offset, gpu)
                out = ops.unscale_sumsq(view, state)
                again_buf, again_view = _place(scaled, offset, gpu)
                again = ops.unscale_sumsq(again_view, state)
                sib_buf, sib_view = _place(scaled, offset, gpu)
                sib = ops.grad_sumsq(sib_view)
                tag = f"n={n} S={scale} offset={offset} poisoned={poisoned}"
                # g after: exactly g * 2^-k (for S = 1: its own bits), nothing outside it written
                assert _same_bits(view, scaled * (1.0 / scale)), tag
                assert _same_bits(view, g), tag
                assert _same_bits(sib_view, scaled), tag                        # the sibling reads only
                head, tail = buf[:offset + GUARD].cpu(), buf[offset + GUARD + n:].cpu()
                assert bool((head == SENTINEL).all() and (tail == SENTINEL).all()), tag
                # the count, and the sum against fp64 on the host
                want, want_bad = _host_sumsq(g)
                got = out.cpu().tolist()
                assert got[1] == want_bad == bad, tag
                print(f"unscale_sumsq {tag}: out {got}, host {want}, rel {abs(got[0] - want) / max(want, 1e-300):.3e}")
                assert abs(got[0] - want) <= (n + 1) * 2.0 ** -52 * want, tag
                # against the sibling over the scaled gradient: out[0] * S^2 has its bits; S = 1: out has its bits
                assert torch.equal(_bits(out * torch.tensor([scale * scale, 1.0], dtype=torch.float64, device=gpu)), _bits(sib)), tag
                # the same input twice: the same bits
                assert torch.equal(_bits(out), _bits(again)) and _same_bits(view, again_view), tag


# ---- x3d_seg_unscale_sumsq --------------------------------------------------------------------------------------------------
SEG_LENGTHS = (1, 5, 1024, 1025, 2049)
LEFT_OUT = 2           # the segment no chunk covers: the frozen tensor


def _segments():
    """(offset, length, l2) with padding between the segments; offsets are multiples of 4"""
    segs, at = [], 4
    for n in SEG_LENGTHS:
        segs.append((at, n, True))
        at += (n + 3) // 4 * 4 + 8
    return segs, at


@pytest.mark.parametrize("scale", SCALES)
def test_seg_unscale_sumsq(gpu, scale):
    segs, total = _segments()
    tuned = [s for i, s in enumerate(segs) if i != LEFT_OUT]
    table = SegTable(tuned).to(gpu)
    for offset in (0, 1):
        for poisoned in (False, True):
            flat = torch.full((total,), SENTINEL)           # the padding between the segments
            bad = 0
            for i, (at, n, _) in enumerate(segs):
                g = _gradient(n, 200 + n)
                if poisoned and i in (1, 4):
                    bad += _poison(g)
                flat[at:at + n] = g * scale
            flat[segs[LEFT_OUT][0] + 7] = float("inf")      # the frozen tensor holds an inf: neither counted nor rewritten
            state = ops.loss_scale_state(scale, gpu)
            buf, view = _place(flat, offset, gpu)
            out = ops.seg_unscale_sumsq(view, table, state)
            again_buf, again_view = _place(flat, offset, gpu)
            again = ops.seg_unscale_sumsq(again_view, table, state)
            sib_buf, sib_view = _place(flat, offset, gpu)
            sib = ops.seg_grad_sumsq(sib_view, table)
            tag = f"S={scale} offset={offset} poisoned={poisoned}"
            want = flat.clone()
            inside = torch.zeros(total, dtype=torch.bool)
            for at, n, _ in tuned:
                inside[at:at + n] = True
            want[inside] = flat[inside] * (1.0 / scale)
            assert _same_bits(view, want), tag              # tuned: exactly g * 2^-k; frozen tensor and padding: their bits
            assert _same_bits(view[~inside.to(gpu)], flat[~inside]), tag
            assert bool((buf[:offset + GUARD] == SENTINEL).all() and (buf[offset + GUARD + total:] == SENTINEL).all()), tag
            host, host_bad = _host_sumsq(want[inside])
            got = out.cpu().tolist()
            assert got[1] == host_bad == bad, tag
            nin = int(inside.sum())
            print(f"seg_unscale_sumsq {tag}: out {got}, host {host}, rel {abs(got[0] - host) / host:.3e}")
            assert abs(got[0] - host) <= (nin + 1) * 2.0 ** -52 * host, tag
            assert torch.equal(_bits(out * torch.tensor([scale * scale, 1.0], dtype=torch.float64, device=gpu)), _bits(sib)), tag
            assert torch.equal(_bits(out), _bits(again)) and _same_bits(view, again_view), tag


# ---- x3d_loss_scale_apply / x3d_loss_scale_update ---------------------------------------------------------------------------
@pytest.mark.parametrize("n", LENGTHS)
def test_loss_scale_apply_is_exact(gpu, n):
    for scale in SCALES:
        state = ops.loss_scale_state(scale, gpu)
        for offset in (0, 1):
            g = _gradient(n, 300 + n)
            buf, view = _place(g, offset, gpu)
            ops.loss_scale_apply(view, state)
            assert _same_bits(view, g * scale), (n, scale, offset)
            assert bool((buf[:offset + GUARD] == SENTINEL).all() and (buf[offset + GUARD + n:] == SENTINEL).all())


def test_loss_scale_update_follows_the_rule(gpu):
    script = [0, 0, 0, 0, 1, 0, 0, 0, 0, 0, 1, 1, 0, 0, 0, 1]          # finite / non-finite blocks, growth_steps = 3
    state = ops.loss_scale_state(2.0 ** 15, gpu)
    blocks = torch.tensor([[123.25, float(3 * b)] for b in script], dtype=torch.float64, device=gpu)
    seen = []
    for i in range(len(script)):
        ops.loss_scale_update(state, blocks[i], 3)
        seen.append(state.clone())
    got = torch.stack(seen).cpu().tolist()
    want = R.run(R.initial(2.0 ** 15), script, 3)
    assert got == want
    assert {s[R.SCALE] for s in want} >= {2.0 ** 14, 2.0 ** 15, 2.0 ** 16}        # the script halves and doubles
    # the floor at 1, and no doubling into a scale that is no float32
    low = ops.loss_scale_state(1.0, gpu)
    ops.loss_scale_update(low, blocks[4], 3)
    assert low.cpu().tolist() == R.update(R.initial(1.0), True, 3)
    top = ops.loss_scale_state(2.0 ** 127, gpu)
    ops.loss_scale_update(top, blocks[0], 1)
    assert top.cpu().tolist() == R.update(R.initial(2.0 ** 127), False, 1)


def test_refusals_write_nothing(gpu):
    lib = hip.load()
    st = hip.stream_ptr()
    g = torch.full((64,), 2.0, dtype=torch.float32, device=gpu)
    state = ops.loss_scale_state(4.0, gpu)
    scratch = torch.full((16,), 5.0, dtype=torch.float64, device=gpu)
    out = torch.full((2,), 6.0, dtype=torch.float64, device=gpu)
    norm = torch.tensor([1.0, 1.0], dtype=torch.float64, device=gpu)
    table = SegTable([(0, 5, True), (8, 40, False)]).to(gpu)
    G, S, SC, O, N = (t.data_ptr() for t in (g, state, scratch, out, norm))
    CH, SG, nc, ns = table.d_chunks.data_ptr(), table.d_segs.data_ptr(), table.nchunk, table.nseg
    bad = [
        lib.x3d_loss_scale_apply(None, 64, S, st), lib.x3d_loss_scale_apply(G, 64, None, st),
        lib.x3d_loss_scale_apply(G, 0, S, st), lib.x3d_loss_scale_apply(G, -1, S, st),
        lib.x3d_loss_scale_apply(G + 2, 32, S, st), lib.x3d_loss_scale_apply(G, 64, S + 4, st),
        lib.x3d_unscale_sumsq(None, 64, S, SC, O, st), lib.x3d_unscale_sumsq(G, 64, None, SC, O, st),
        lib.x3d_unscale_sumsq(G, 64, S, None, O, st), lib.x3d_unscale_sumsq(G, 64, S, SC, None, st),
        lib.x3d_unscale_sumsq(G, 0, S, SC, O, st), lib.x3d_unscale_sumsq(G + 2, 32, S, SC, O, st),
        lib.x3d_unscale_sumsq(G, 64, S + 4, SC, O, st), lib.x3d_unscale_sumsq(G, 64, S, SC + 4, O, st),
        lib.x3d_unscale_sumsq(G, 64, S, SC, O + 4, st),
        lib.x3d_seg_unscale_sumsq(None, CH, nc, SG, ns, S, SC, O, st), lib.x3d_seg_unscale_sumsq(G, None, nc, SG, ns, S, SC, O, st),
        lib.x3d_seg_unscale_sumsq(G, CH, nc, None, ns, S, SC, O, st), lib.x3d_seg_unscale_sumsq(G, CH, nc, SG, ns, None, SC, O, st),
        lib.x3d_seg_unscale_sumsq(G, CH, nc, SG, ns, S, None, O, st), lib.x3d_seg_unscale_sumsq(G, CH, nc, SG, ns, S, SC, None, st),
        lib.x3d_seg_unscale_sumsq(G, CH, 0, SG, ns, S, SC, O, st), lib.x3d_seg_unscale_sumsq(G, CH, nc, SG, 0, S, SC, O, st),
        lib.x3d_seg_unscale_sumsq(G, CH, 1, SG, 2, S, SC, O, st),                 # more segments than chunks
        lib.x3d_seg_unscale_sumsq(G, CH + 2, nc, SG, ns, S, SC, O, st), lib.x3d_seg_unscale_sumsq(G + 2, CH, nc, SG, ns, S, SC, O, st),
        lib.x3d_seg_unscale_sumsq(G, CH, nc, SG, ns, S + 4, SC, O, st), lib.x3d_seg_unscale_sumsq(G, CH, nc, SG, ns, S, SC + 4, O, st),
        lib.x3d_seg_unscale_sumsq(G, CH, nc, SG, ns, S, SC, O + 4, st),
        lib.x3d_loss_scale_update(None, N, 3, st), lib.x3d_loss_scale_update(S, None, 3, st),
        lib.x3d_loss_scale_update(S, N, 0, st), lib.x3d_loss_scale_update(S, N, -2, st),
        lib.x3d_loss_scale_update(S + 4, N, 3, st), lib.x3d_loss_scale_update(S, N + 4, 3, st),
    ]
    assert bad == [INVALID] * len(bad), bad
    torch.cuda.synchronize()
    assert bool((g == 2.0).all() and (scratch == 5.0).all() and (out == 6.0).all())
    assert state.cpu().tolist() == R.initial(4.0) and norm.cpu().tolist() == [1.0, 1.0]
    with pytest.raises(ValueError):
        ops.loss_scale_state(3.0, gpu)              # not a power of two
    with pytest.raises(ValueError):
        ops.loss_scale_update(state, norm, 0)


# ---- the trainer, switch on against switch off ------------------------------------------------------------------------------
BASE = ["NETWORK.NUM_CLASSES", 11]
CLIP = ["SOLVER.CLIP_GRAD_L2NORM", 0.05]
FT = ["SOLVER.FREEZE", ["conv1/", "stages/0/"], "SOLVER.LAYER_DECAY", 0.9]
LR = 0.01


def _batches(gpu):
    """the clips of test_trainer_fp16_loss_scaling_and_adam, and a second batch to alternate with"""
    gen = torch.Generator().manual_seed(3)
    out = []
    for _ in range(2):
        clips = torch.randn(2, 4, 64, 64, 3, generator=gen).to(gpu)
        out.append((clips, torch.randint(0, 11, (2,), generator=gen).to(gpu)))
    return out


def _trainer(gpu, opts, on):
    from x3d_tf_amd.model import X3D
    from x3d_tf_amd.train import Trainer
    cfg = x.get_config("XS", BASE + opts + (["SOLVER.DEVICE_LOSS_SCALE", True] if on else []))
    m = X3D(cfg, dtype=torch.float16, device=gpu, seed=5)
    m.set_dropout_mask(torch.ones(2, x.build_arch(cfg).fc1_out))
    tr = Trainer(m, cfg)
    tr.growth_steps = 3
    assert tr.dynamic_scale and (tr._dls is not None) == on
    return tr


class _Twin:
    """the off arm adopts what the on arm's forward_backward left: in step order, one entry per call (module docstring)"""

    def __init__(self, off, on):
        self.queue = collections.deque()
        real_on, real_off = on.model.forward_backward, off.model.forward_backward

        def fb_on(*args, **kw):
            pl = real_on(*args, **kw)
            self.queue.append((on.model.flat_grads.clone(), on.model.moving_stats_flat().clone()))
            return pl

        def fb_off(*args, **kw):
            pl = real_off(*args, **kw)
            grads, stats = self.queue.popleft()
            off.model.flat_grads.copy_(grads)
            off.model.moving_stats_flat().copy_(stats)
            return pl
        on.model.forward_backward, off.model.forward_backward = fb_on, fb_off


def _slots(tr):
    m = tr.model
    out = dict(params=m.flat_params, velocity=m.flat_velocity)
    if tr.slot_kind == "adam":
        out["second"] = m.second_slot()
    if tr.ema is not None:
        out["ema"] = tr.ema
    return out


def _assert_arms_agree(off, on, scale_used, tag):
    """after a step: weights + moving statistics, slots, EMA, the scaler and the gradient (on = off / S on the tuned tensors)"""
    a, b = _slots(off), _slots(on)
    for k in a:
        assert _same_bits(a[k], b[k]), f"{tag}: {k} differs in {int((_bits(a[k]) != _bits(b[k])).sum())} elements"
    assert (on.loss_scale, on.skipped_steps, on.opt_step) == (off.loss_scale, off.skipped_steps, off.opt_step), tag
    g_off, g_on = off.model.flat_grads.cpu(), on.model.flat_grads.cpu()
    want = g_off.clone()
    for s in off.model.tuned_segments:                  # (without set_finetune: every segment)
        want[s.offset:s.offset + s.length] = g_off[s.offset:s.offset + s.length] * (1.0 / scale_used)
    assert _same_bits(g_on, want), f"{tag}: flat_grads is not the off arm's / {scale_used}"


CASES = {
    "sgd": ["TRAIN.OPTIMIZER", "sgd"],
    "adam": ["TRAIN.OPTIMIZER", "adam"],
    "lamb": ["TRAIN.OPTIMIZER", "lamb", "OPTIM.WEIGHT_DECAY", 0.01],
    "adamw_finetune": ["TRAIN.OPTIMIZER", "adamw", "OPTIM.WEIGHT_DECAY", 0.01] + FT,
    "sgd_clip_ema": ["TRAIN.OPTIMIZER", "sgd", "SOLVER.EMA_DECAY", 0.5] + CLIP,
    "adam_clip": ["TRAIN.OPTIMIZER", "adam"] + CLIP,
    "lamb_clip_finetune": ["TRAIN.OPTIMIZER", "lamb", "OPTIM.WEIGHT_DECAY", 0.01] + CLIP + FT,
}


def _run_pair(gpu, case, opts, steps, poke_at, growth_steps=3):
    """`steps` steps of both arms on alternating batches, compared after every one; the scale is set to 2^40 before step
    `poke_at`, so that both arms skip there.  Returns the off arm."""
    off, on = _trainer(gpu, opts, False), _trainer(gpu, opts, True)
    off.growth_steps = on.growth_steps = growth_steps
    _Twin(off, on)
    batches = _batches(gpu)
    assert _same_bits(off.model.flat_params, on.model.flat_params)
    trace = []
    for step in range(1, steps + 1):
        if step == poke_at:
            off.loss_scale = on.loss_scale = 2.0 ** 40
        used, applied = off.loss_scale, off.opt_step
        clips, labels = batches[(step - 1) % 2]
        on.step(clips, labels, LR)
        off.step(clips, labels, LR)
        _assert_arms_agree(off, on, used, f"{case} step {step}")
        if off._clip and off.opt_step != applied:       # an applied step: the norm of the unscaled gradient, the same fp64 number
            assert _same_bits(off.last_grad_norm.reshape(1), on.last_grad_norm.reshape(1)), f"{case} step {step}"
        if step == poke_at:
            assert off.skipped_steps >= 1 and off.loss_scale == 2.0 ** 39
        trace.append(math.log2(off.loss_scale))
    assert off.opt_step + off.skipped_steps == steps
    print(f"{case}: applied {off.opt_step}, skipped {off.skipped_steps}, log2 of the scale after each step {trace}")
    return off


@pytest.mark.parametrize("case", list(CASES))
def test_trainer_on_matches_off(gpu, case):
    """8 steps on alternating batches, the scale set to 2^40 before step 3 so that both arms skip there"""
    off = _run_pair(gpu, case, CASES[case], 8, 3)
    assert off.opt_step >= 2


def test_trainer_on_matches_off_while_the_scale_grows(gpu):
    """no skip forced, growth_steps = 2: both arms double after every second finite step (and halve alike if 2^16 or 2^17 overflow)"""
    off = _run_pair(gpu, "growth", CASES["sgd_clip_ema"], 5, None, growth_steps=2)
    assert off.loss_scale != 2.0 ** 15 or off.skipped_steps > 0


@pytest.mark.parametrize("scale", [2.0 ** 15, 2.0 ** 40])
def test_the_backward_pass_starts_from_the_scaled_dlogits(gpu, scale):
    """device mode: dlogits, as the head at 1 / batch and x3d_loss_scale_apply leave it, has the bits of the head at S / batch on
    the same logits -- what the off arm launches"""
    tr = _trainer(gpu, ["TRAIN.OPTIMIZER", "sgd"], True)
    tr.loss_scale = scale
    clips, labels = _batches(gpu)[0]
    pl = tr.step(clips, labels, LR)
    probs, rows, want = torch.empty_like(pl.probs), torch.empty_like(pl.loss_rows), torch.empty_like(pl.dlogits)
    ops.softmax_xent(pl.logits, pl.labels, probs, rows, want, grad_scale=scale / 2.0)
    assert _same_bits(pl.dlogits, want) and _same_bits(pl.probs, probs) and bool(torch.isfinite(want).all())
    assert float(want.abs().max()) > 0.01 * scale


def test_trainer_accumulation_matches_off(gpu):
    """ACCUM_STEPS = 2: the scale is one value inside an accumulation, the update every second micro-batch matches the off arm"""
    opts = ["TRAIN.OPTIMIZER", "sgd", "SOLVER.ACCUM_STEPS", 2] + CLIP
    off, on = _trainer(gpu, opts, False), _trainer(gpu, opts, True)
    _Twin(off, on)
    batches = _batches(gpu)
    for micro in range(1, 9):
        if micro == 3:
            off.loss_scale = on.loss_scale = 2.0 ** 40
        used = off.loss_scale
        clips, labels = batches[(micro - 1) % 2]
        on.step(clips, labels, LR)
        off.step(clips, labels, LR)
        if micro % 2 == 0:
            _assert_arms_agree(off, on, used, f"accum micro-batch {micro}")
        else:                                           # inside an accumulation: nothing but the gradient has moved
            assert _same_bits(off.model.flat_params, on.model.flat_params) and on.loss_scale == used == off.loss_scale
            assert _same_bits(off.model.flat_grads, on.model.flat_grads)      # still scaled, in both arms
    assert off.opt_step + off.skipped_steps == 4 and off.skipped_steps >= 1


def test_adam_bias_correction_does_not_count_a_skipped_step(gpu):
    """Clip on, a skipped step, then a finite one: the on arm's update is Adam's at bias-correction step 1 (fp64 restatement from
    the unscaled gradient the step left in flat_grads; the tolerance of test_trainer_fp16_loss_scaling_and_adam: fp32 roundings
    of an update of weights of magnitude <= 1), and NOT the one at step 2, which a count that ran ahead would give."""
    tr = _trainer(gpu, ["TRAIN.OPTIMIZER", "adam"] + CLIP, True)
    m = tr.model
    (clips, labels), _ = _batches(gpu)
    tr.loss_scale = 2.0 ** 40
    w0 = m.flat_params[:m.n_trainable_flat].clone()
    tr.step(clips, labels, LR)
    assert (tr.skipped_steps, tr.opt_step, tr.loss_scale) == (1, 0, 2.0 ** 39)
    assert _same_bits(w0, m.flat_params[:m.n_trainable_flat])
    tr.loss_scale = 2.0 ** 15
    tr.step(clips, labels, LR)
    assert (tr.skipped_steps, tr.opt_step) == (1, 1)
    g = m.flat_grads[:m.n_trainable_flat].double().cpu().numpy()
    norm = float(tr.last_grad_norm.item())
    assert abs(norm - math.sqrt(float((g * g).sum()))) <= 1e-9 * norm          # last_grad_norm: of the unscaled gradient
    c = min(1.0, 0.05 / (norm + 1e-6))
    assert c < 1.0                                      # the clip acts
    l2 = m.l2_mask[:m.n_trainable_flat].double().cpu().numpy()
    zeros = np.zeros_like(g)
    got = m.flat_params[:m.n_trainable_flat].double().cpu().numpy()
    tol = 2e-6 * max(1.0, float(np.abs(got).max()))
    for step, ok in ((1, True), (2, False)):
        want, _, _ = R.adam_step(w0.double().cpu().numpy(), zeros, zeros, g, l2, LR, step, m.arch.weight_decay, c=c)
        err = float(np.abs(got - want).max())
        print(f"adam restated at step {step}: max |got - want| = {err:.3e} (tolerance {tol:.1e})")
        assert (err <= tol) == ok, (step, err, tol)


class _HostWaits:
    """counts what makes the host wait for the device: Tensor.item / tolist / cpu / numpy, torch.cuda.synchronize, and event and
    stream synchronisations (which event, for the former)"""

    def __init__(self, monkeypatch):
        self.reads, self.syncs, self.events = [], 0, []
        for name in ("item", "tolist", "cpu", "numpy"):
            real = getattr(torch.Tensor, name)

            def spy(t, *a, _real=real, _name=name, **kw):
                if t.is_cuda:
                    self.reads.append((_name, tuple(t.shape), t.dtype))
                return _real(t, *a, **kw)
            monkeypatch.setattr(torch.Tensor, name, spy)
        real_sync, real_ev, real_st = torch.cuda.synchronize, torch.cuda.Event.synchronize, torch.cuda.Stream.synchronize

        def sync(*a, **kw):
            self.syncs += 1
            return real_sync(*a, **kw)

        def ev_sync(ev):
            self.events.append(ev)
            return real_ev(ev)

        def st_sync(s):
            self.syncs += 1
            return real_st(s)
        monkeypatch.setattr(torch.cuda, "synchronize", sync)
        monkeypatch.setattr(torch.cuda.Event, "synchronize", ev_sync)
        monkeypatch.setattr(torch.cuda.Stream, "synchronize", st_sync)

    def clear(self):
        self.reads, self.syncs, self.events = [], 0, []


@pytest.mark.parametrize("opt", ["sgd", "adam"])
def test_a_step_does_not_wait_for_the_device(gpu, opt, monkeypatch):
    """device mode: no .item() (nor any other read) and no synchronisation in Trainer.step; at most one event wait, for the event
    the PREVIOUS step recorded behind its update (adam: exactly that one, for the bias-correction step; sgd: none)"""
    tr = _trainer(gpu, ["TRAIN.OPTIMIZER", opt] + CLIP, True)
    batches = _batches(gpu)
    tr.step(*batches[0], LR)                            # (the first step records the plan and allocates)
    waits = _HostWaits(monkeypatch)
    ds = tr._dls
    for step in range(2, 6):
        previous = ds.events[ds.pending]
        tr.step(*batches[(step - 1) % 2], LR)
        assert waits.reads == [] and waits.syncs == 0, (step, waits.reads, waits.syncs)
        assert waits.events == ([previous] if opt == "adam" else []), step
        assert ds.pending is not None and ds.events[ds.pending] is not previous      # this step's, which nobody has waited for
        waits.clear()
    assert tr.opt_step == 5 and waits.reads == [("tolist", (8,), torch.float64)]         # the property is the explicit read
    # the off arm does read: grads_finite is what decides there
    off = _trainer(gpu, ["TRAIN.OPTIMIZER", opt] + CLIP, False)
    off.step(*batches[0], LR)
    waits.clear()
    off.step(*batches[1], LR)
    assert any(name == "item" for name, _, _ in waits.reads)


def test_fit_reads_the_state_once_per_epoch(gpu, monkeypatch):
    """2 epochs x 4 steps, the first steps skipped (scale 2^40): history["loss_scale"] / ["skipped_steps"] / ["grad_norm"] of the on
    arm are the off arm's attributes at the ends of the epochs, from one read of the 8-double state per epoch"""
    import itertools
    opts = ["TRAIN.OPTIMIZER", "sgd"] + CLIP
    off, on = _trainer(gpu, opts, False), _trainer(gpu, opts, True)
    batches = _batches(gpu)
    _Twin(off, on)
    off.loss_scale = on.loss_scale = 2.0 ** 40
    ends, count = [], itertools.count(1)

    def on_step(tr, pl):
        if next(count) % 4 == 0:
            ends.append((tr.loss_scale, tr.skipped_steps))
    waits = _HostWaits(monkeypatch)
    on.fit(itertools.cycle(batches), epochs=2, steps_per_epoch=4)
    reads = list(waits.reads)
    off.fit(itertools.cycle(batches), epochs=2, steps_per_epoch=4, on_step=on_step)
    waits.reads = reads
    state_reads = [r for r in waits.reads if r[1:] == ((8,), torch.float64)]
    assert len(state_reads) == 2, waits.reads
    assert on.history["loss_scale"] == [s for s, _ in ends]
    assert on.history["skipped_steps"] == [ends[0][1], ends[1][1] - ends[0][1]] and sum(on.history["skipped_steps"]) >= 1
    assert on.history["grad_norm"] == off.history["grad_norm"]
    assert on.history["loss"] == pytest.approx(off.history["loss"], rel=1e-5)      # (each arm's own forward pass: fp32 rows)
    assert "loss_scale" not in off.history and "skipped_steps" not in off.history
    assert _same_bits(off.model.flat_params, on.model.flat_params)


# ---- the default path -------------------------------------------------------------------------------------------------------
def test_switch_off_makes_the_recorded_launches(gpu, monkeypatch):
    """With the switch off an fp16 step makes the solver launches tests/golden/solver_launches.json pins (x3d_all_finite first:
    grads_finite is still what decides) and none of the new ones"""
    from x3d_tf_amd.model import X3D
    spec = importlib.util.spec_from_file_location("solver_launches", os.path.join(ROOT, "tools", "solver_launches.py"))
    tool = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(tool)
    with open(os.path.join(ROOT, "tests", "golden", "solver_launches.json")) as fh:
        golden = json.load(fh)["cases"]
    gen = torch.Generator().manual_seed(5)
    batches = [(torch.randn(2, 4, 32, 32, 3, generator=gen).to(gpu), torch.randint(0, 10, (2,), generator=gen).to(gpu))
               for _ in range(tool.STEPS)]
    asked, new = [], []
    real_finite, real_call = X3D.grads_finite, hip.call

    def finite(self):
        asked.append(1)
        return real_finite(self)

    def call(name, *args):
        if "loss_scale" in name or "unscale" in name:
            new.append(name)
        return real_call(name, *args)
    monkeypatch.setattr(X3D, "grads_finite", finite)
    monkeypatch.setattr(hip, "call", call)
    for case in ("fp16/sgd/none/plain", "fp16/adamw/clip/ft"):
        opts, dtype = tool.cases()[case]
        assert dtype == torch.float16
        assert tool._one_case(opts, dtype, gpu, batches) == golden[case], case
    assert len(asked) == 2 * tool.STEPS and new == []
    assert golden["fp16/sgd/none/plain"][0][0][0] == "x3d_all_finite"
