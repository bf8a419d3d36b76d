"""Stochastic depth (NETWORK.DROP_PATH_RATE) on the GPU: the device draw bit for bit against the host Philox, the two tail kernels
against fp64, the model against the CPU oracle with drop-path (tests/drop_path_ref.py), and the trainer."""

import numpy as np
import pytest
import torch

from tests import drop_path_ref as R
from tests.util import hip_relu_masks, rel_l2, relu_mask_mismatch, report

pytestmark = pytest.mark.gpu

DTYPES = [torch.float32, torch.bfloat16, torch.float16]
ULP_HALF = {torch.float32: 2.0 ** -24, torch.bfloat16: 2.0 ** -8, torch.float16: 2.0 ** -11}
U32 = 2.0 ** -24          # unit roundoff of fp32
SEED = 0x0123456789ABCDEF


# ---- 1. the draw ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("L,N,rates", [(3, 5, [0.0, 0.25, 0.5]), (55, 64, [0.5 * l / 54 for l in range(55)])])
def test_draw_matches_host_philox(gpu, L, N, rates):
    """Two launches from (seed, step): the tables of step and step + 1 bit for bit, every value 0 or fp32(1 / (1 - rate_l)), a
    rate-0 row all ones, and the state left at step + 2."""
    from x3d_tf_amd import ops
    step = 41
    rd = torch.from_numpy(R.rates32(rates)).to(gpu)
    state = ops.drop_path_state(SEED, step, gpu)
    got = []
    for _ in range(2):
        keep = torch.full((L, N), float("nan"), device=gpu)
        ops.drop_path_draw(keep, rd, state)
        got.append(keep.cpu().numpy())
    assert ops.drop_path_step(state) == step + 2
    assert state.tolist()[:2] == ops.drop_path_state(SEED, 0, "cpu").tolist()[:2]      # the seed is left alone
    sc = R.keep_scale(rates)
    for k, t in enumerate(got):
        want = R.keep_table(SEED, step + k, rates, N)
        assert t.dtype == np.float32 and np.array_equal(t.view(np.uint32), want.view(np.uint32)), f"table of step {step + k}"
        for l in range(L):
            assert set(np.unique(t[l]).tolist()) <= {0.0, float(sc[l])}
        assert (t[0] == 1.0).all()
    assert not np.array_equal(got[0], got[1])


def test_draw_step_carries_into_the_high_word(gpu):
    from x3d_tf_amd import ops
    rates = [0.0, 0.5]
    rd = torch.from_numpy(R.rates32(rates)).to(gpu)
    state = ops.drop_path_state(SEED, 2 ** 32 - 1, gpu)
    keep = torch.empty(2, 64, device=gpu)
    ops.drop_path_draw(keep, rd, state)
    assert ops.drop_path_step(state) == 2 ** 32
    assert np.array_equal(keep.cpu().numpy(), R.keep_table(SEED, 2 ** 32 - 1, rates, 64))
    ops.drop_path_draw(keep, rd, state)
    assert ops.drop_path_step(state) == 2 ** 32 + 1
    assert np.array_equal(keep.cpu().numpy(), R.keep_table(SEED, 2 ** 32, rates, 64))


# ---- 2. / 3. the tail kernels -------------------------------------------------------------------------------------------------
# (N, C, P, misaligned): the scalar path; the vector path across the 256 x 8 x 4-element workgroup boundary; a small plane; a
# pointer one element off alignment (scalar path, with a ragged last chunk)
TAIL_CASES = [(3, 5, 7, False), (2, 3, 8200, False), (4, 6, 392, False), (2, 3, 8201, True)]
KEEP_PATTERN = [1.0 / (1.0 - 0.25), 0.0, 1.0, 2.0, 0.0, 1.0 / (1.0 - 0.1), 1.0, 0.0, 2.0]


def _keep(n):
    return torch.tensor(KEEP_PATTERN[:n], dtype=torch.float32)


def _dev(t, gpu, off=False):
    """t on the GPU; off: one element past a 16-byte boundary"""
    if not off:
        return t.to(gpu)
    base = torch.zeros(t.numel() + 8, dtype=t.dtype, device=gpu)
    v = base[1:1 + t.numel()].view(t.shape)
    v.copy_(t)
    assert v.data_ptr() % 16 != 0
    return v


def _ss(c, gen):
    return torch.stack([torch.rand(c, generator=gen) + 0.5, torch.randn(c, generator=gen)], 1).contiguous()


@pytest.mark.parametrize("conv_shortcut", [False, True])
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("n,c,p,off", TAIL_CASES)
def test_tail_fwd_dp(gpu, n, c, p, off, dtype, conv_shortcut):
    """y = relu(keep[n] (s_c c + t_c) + shortcut) against fp64 on the stored inputs.  Bound: the kernel evaluates the four terms
    k s_c c, k t_c, s_r r, t_r in fp32 with at most 6 roundings (two multiply-adds, the scale by keep, the sum; each at most
    2^-24 of the magnitudes involved), so |y32 - y64| <= 8 * 2^-24 * M with M = k (|s_c c| + |t_c|) + |s_r r| + |t_r| (8: a few
    roundings, with room for the order); a 16-bit store adds half an ulp of the storage type, <= 2^-8 (bf16) / 2^-11 (fp16) of
    the fp32 value.  The c_raw of every dropped sample is NaN: it must not be loaded -- y finite, and bit for bit relu(x) for
    the identity shortcut."""
    from x3d_tf_amd import ops
    gen = torch.Generator().manual_seed(n * 1000 + c * 10 + p)
    keep = _keep(n)
    c_raw = torch.randn(n, c, p, generator=gen).to(dtype)
    sh = torch.randn(n, c, p, generator=gen).to(dtype)
    c_ss, r_ss = _ss(c, gen), (_ss(c, gen) if conv_shortcut else None)
    c_poison = c_raw.clone()
    c_poison[keep == 0] = float("nan")
    y = _dev(torch.full((n, c, p), float("nan")).to(dtype), gpu, off)
    ops.tail_fwd_dp(c_poison.to(gpu), c_ss.to(gpu), _dev(sh, gpu, off), None if r_ss is None else r_ss.to(gpu), keep.to(gpu), y)
    got = y.cpu()
    assert torch.isfinite(got.float()).all()
    col = lambda t, j: t[:, j].double().view(1, -1, 1)
    k = keep.double().view(-1, 1, 1)
    branch = k * (col(c_ss, 0) * c_raw.double() + col(c_ss, 1))
    short = col(r_ss, 0) * sh.double() + col(r_ss, 1) if conv_shortcut else sh.double()
    ref = torch.relu(branch + short)
    mag = k * ((col(c_ss, 0) * c_raw.double()).abs() + col(c_ss, 1).abs()) + \
        ((col(r_ss, 0) * sh.double()).abs() + col(r_ss, 1).abs() if conv_shortcut else sh.double().abs())
    f32 = 8 * U32 * mag
    tol = f32 + (ULP_HALF[dtype] * (ref.abs() + f32) if dtype != torch.float32 else 0.0)
    err = (got.double() - ref).abs()
    print(f"tail_fwd_dp {dtype} {(n, c, p)} conv={conv_shortcut}: max err/tol {(err / tol.clamp_min(1e-300)).max().item():.3f}")
    assert (err <= tol).all(), f"max err {err.max().item():.3e}, worst err/tol {(err / tol.clamp_min(1e-300)).max().item():.3f}"
    if not conv_shortcut:
        dropped = keep == 0
        assert torch.equal(got[dropped], torch.relu(sh[dropped].float()).to(dtype))


def _wg_elems(n, p, dtype, aligned):
    """elements one workgroup of x3d_tail_bwd_dp sums in fp32 before its fp64 atomics (elem.hip, the DP form of tail_bwd_kernel:
    256 threads x 4 iterations x the vector width; small 16-bit planes: nb samples of one channel)"""
    full = 4 if dtype == torch.float32 else 8
    vec = full if aligned and p % full == 0 else 1
    if dtype != torch.float32 and vec == 8 and p // 8 < 256:
        return min(n, 16, 4 * 256 // (p // 8)) * p
    return min(p, 256 * vec * 4)


@pytest.mark.parametrize("conv_shortcut", [False, True])
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("n,c,p,off", TAIL_CASES + [(9, 4, 392, False)])
def test_tail_bwd_dp(gpu, n, c, p, off, dtype, conv_shortcut):
    """g = dy [y > 0] in place and g_branch = round(keep g), both bit for bit (g is dy or 0; g_branch the same two roundings as
    (keep.float() * g.float()).to(dtype)); sums_c over the STORED g_branch, sums_r over g, added to what the buffers held.
    Bound on a sum: a workgroup adds W = _wg_elems terms in fp32 (each product rounded once) before its fp64 atomic, so its
    error is at most (W + 1) 2^-24 times the sum of the magnitudes of its terms; over the workgroups of a channel that is
    (W + 1) * 2^-24 * sum |term| (the fp64 additions are 2^-29 of that).  (9, 4, 392) in 16-bit takes the several-samples-per-
    workgroup form with N > 4.  NaN in the c_raw of dropped samples: the sums stay finite."""
    from x3d_tf_amd import ops
    gen = torch.Generator().manual_seed(n * 1000 + c * 10 + p + 1)
    keep = _keep(n)
    dy = torch.randn(n, c, p, generator=gen).to(dtype)
    y = torch.relu(torch.randn(n, c, p, generator=gen)).to(dtype)
    c_raw = torch.randn(n, c, p, generator=gen).to(dtype)
    r_raw = torch.randn(n, c, p, generator=gen).to(dtype) if conv_shortcut else None
    c_poison = c_raw.clone()
    c_poison[keep == 0] = float("nan")
    dyg = dy.to(gpu)
    gbr = _dev(torch.full((n, c, p), float("nan")).to(dtype), gpu, off)      # (the misaligned pointer is the one x3d_tail_bwd has not)
    sums_c = torch.full((c, 2), 0.25, dtype=torch.float64, device=gpu)
    sums_r = torch.full((c, 2), 0.25, dtype=torch.float64, device=gpu) if conv_shortcut else None
    ops.tail_bwd_dp(dyg, gbr, y.to(gpu), c_poison.to(gpu), None if r_raw is None else r_raw.to(gpu), keep.to(gpu), sums_c, sums_r)
    g_ref = torch.where(y.float() > 0, dy, torch.zeros_like(dy))
    gb_ref = (keep.view(-1, 1, 1) * g_ref.float()).to(dtype)
    assert torch.equal(dyg.cpu(), g_ref)
    assert torch.equal(gbr.cpu(), gb_ref)
    bound = (_wg_elems(n, p, dtype, not off) + 1) * U32
    kept = (keep != 0).view(-1, 1, 1)
    t_c = torch.where(kept, gb_ref.double() * c_raw.double(), torch.zeros((), dtype=torch.float64))
    checks = [("sums_c[0]", sums_c[:, 0], gb_ref.double()), ("sums_c[1]", sums_c[:, 1], t_c)]
    if conv_shortcut:
        checks += [("sums_r[0]", sums_r[:, 0], g_ref.double()), ("sums_r[1]", sums_r[:, 1], g_ref.double() * r_raw.double())]
    for name, got, terms in checks:
        got = got.cpu() - 0.25
        assert torch.isfinite(got).all(), name
        ref, tol = terms.sum((0, 2)), bound * terms.abs().sum((0, 2)) + 1e-15
        err = (got - ref).abs()
        print(f"tail_bwd_dp {dtype} {(n, c, p)} {name}: max err/tol {(err / tol).max().item():.3f}")
        assert (err <= tol).all(), f"{name}: err {err.max().item():.3e} against {tol.min().item():.3e}"


# ---- 4. the model in fp32 against the oracle with drop-path -----------------------------------------------------------------
def _setup(name, overrides=None):
    import x3d_tf_amd as x
    from x3d_tf_amd.params import init_params, randomize_bn_
    cfg = x.get_config(name, overrides)
    arch = x.build_arch(cfg)
    return cfg, arch, randomize_bn_(init_params(arch, seed=3), seed=4)


def _model(cfg, params, dtype, gpu):
    from x3d_tf_amd.model import X3D
    m = X3D(cfg, dtype=dtype, device=gpu, seed=0)
    m.load_state_dict(params)
    return m


def _scaled(name, got, ref, rel):
    return report(name, got, ref, 0, rel * (ref.detach().abs().max().item() + 1e-30))


def _mask01(rates, n, all_dropped, seed=11):
    """[L][N] of 0/1: every block with a rate keeps some samples and drops some; block `all_dropped` drops them all"""
    gen = torch.Generator().manual_seed(seed)
    m = torch.ones(len(rates), n)
    for l, r in enumerate(rates):
        if r > 0:
            row = (torch.rand(n, generator=gen) >= 0.5).float()
            row[l % n] = 0.0
            row[(l + 1) % n] = 1.0
            m[l] = row
    m[all_dropped] = 0.0
    return m


@pytest.mark.parametrize("name,n,t,s", [("XS", 4, 4, 64), ("S", 3, 5, 96)])
def test_train_step_fp32_with_drop_path(gpu, name, n, t, s):
    """Forward + backward at DROP_PATH_RATE = 0.5 under a fixed keep mask against tests/drop_path_ref.py, at the limits of
    test_model_gpu.test_train_step_fp32: block outputs 2e-4 of the tensor's maximum, logits and probabilities 1e-4, loss 1e-5,
    each gradient below 1e-3 relative L2 with the device's ReLU masks handed to the reference.  One block drops every sample:
    its a / b / c / SE weights (and BatchNorm parameters) get a gradient of exactly zero."""
    from oracle import x3d_oracle as O
    from x3d_tf_amd.arch import block_prefix, drop_path_rates
    cfg, arch, params = _setup(name, ["NETWORK.DROP_PATH_RATE", 0.5])
    rates = drop_path_rates(arch)
    torch.manual_seed(1)
    x = torch.randn(n, t, s, s, 3)
    labels = torch.randint(0, arch.num_classes, (n,))
    mask = (torch.rand(n, arch.fc1_out) >= arch.dropout_rate).float()
    gone = 6                                  # an identity-shortcut block of the second stage, with SE
    assert not arch.blocks[gone].has_shortcut_conv and arch.blocks[gone].has_se and rates[gone] > 0
    dp01 = _mask01(rates, n, gone)
    keep = R.scaled_mask(dp01, rates)

    m = _model(cfg, params, torch.float32, gpu)
    m.set_dropout_mask(mask)
    m.set_drop_path_mask(dp01)
    pl = m.forward_backward(x.to(gpu), labels.to(gpu))
    torch.cuda.synchronize()
    assert torch.equal(pl.dp_keep.cpu(), keep)
    assert sum(it[0] == "x3d_tail_fwd_dp" for it in pl.fwd) == sum(it[0] == "x3d_tail_bwd_dp" for it in pl.bwd) == len(rates) - 1

    taps, st, free_masks = {}, O.BNState(), O.RecordMasks()
    probs_free = R.forward_dp({k: v.clone() for k, v in params.items()}, x, arch, keep, rates, dropout_mask=mask, state=st,
                              taps=taps, relu_masks=free_masks)
    _scaled("conv1/out", pl.y0, taps["conv1/out"], 2e-5)
    for B in pl.blocks:
        pre = O.block_prefix(B.spec)
        _scaled(pre + "/out", B.y, taps[pre + "/out"], 2e-4)
    _scaled("logits", pl.logits, taps["logits"], 1e-4)
    report("probs", pl.probs, probs_free, 0, 1e-4)
    for k, v in st.new_moving.items():
        report(k, m.params[k], v, 1e-4, 1e-5)

    dev_masks = hip_relu_masks(pl)
    frac, bad, tot = relu_mask_mismatch(dev_masks, free_masks)
    assert frac <= 1e-5, f"{bad} of {tot} ReLU signs differ between the device and the free-running reference"
    r = R.train_step_dp({k: v.clone() for k, v in params.items()}, x, labels, arch, keep, rates, dropout_mask=mask,
                        relu_masks=dev_masks)
    loss = pl.loss_rows.mean() + m.regularization_loss().float()
    report("loss", loss.view(1), r["loss"].view(1), 1e-5, 1e-5)
    worst = 0.0
    for k, g_ref in r["grads"].items():
        g = m.grads[k].cpu().double()
        if m.specs[k].l2:
            g = g + 2 * arch.weight_decay * params[k].double()
        if g_ref.norm().item() == 0.0:
            assert g.abs().max().item() == 0.0, f"grad {k}: the reference is exactly zero"
            continue
        e = rel_l2(g, g_ref)
        worst = max(worst, e)
        assert e < 1e-3, f"grad {k}: relative L2 error {e:.3e}"
    print(f"{name}: worst gradient relative L2 {worst:.3e}")
    q = block_prefix(arch.blocks[gone]) + "/bottleneck/"
    zero = [k for k in m.grads if k.startswith(q)]
    assert {k[len(q):] for k in zero} >= {"a/kernel", "b/kernel", "c/kernel", "se_fc1/kernel", "se_fc2/kernel", "bn_c/gamma"}
    for k in zero:
        assert m.grads[k].abs().max().item() == 0.0, f"{k}: every sample of the block is dropped, the gradient must be zero"


# ---- 5. 16-bit storage: the drop-path gradients are as close to fp32 as the parent's path is -------------------------------------
_FP32_RUNS = {}


def _grads_of(gpu, dtype, rate, n=2, t=4, s=128):
    """gradients of one X3D-M step (as fp64 on the host), dropout and keep masks fixed"""
    from x3d_tf_amd.arch import drop_path_rates
    cfg, arch, params = _setup("M", ["NETWORK.DROP_PATH_RATE", rate])
    rates = drop_path_rates(arch)
    torch.manual_seed(2)
    x = torch.randn(n, t, s, s, 3).to(torch.bfloat16).float()         # (representable in all three storage types' input path)
    labels = torch.randint(0, arch.num_classes, (n,))
    mask = (torch.rand(n, arch.fc1_out) >= arch.dropout_rate).float()
    m = _model(cfg, params, dtype, gpu)
    m.set_dropout_mask(mask)
    if rate > 0:
        dp01 = torch.ones(len(rates), n)
        for l in range(1, len(rates)):
            dp01[l, l % n] = 0.0                                          # every block with a rate keeps one sample, drops one
        m.set_drop_path_mask(dp01)
    ls = 1024.0 if dtype == torch.float16 else 1.0                       # as test_train_step_half_block_by_block
    m.forward_backward(x.to(gpu), labels.to(gpu), loss_scale=ls)
    torch.cuda.synchronize()
    out = {k: v.detach().cpu().double() / ls for k, v in m.grads.items()}
    assert all(torch.isfinite(v).all() for v in out.values())
    return out


def _fp32_run(gpu, rate):
    if rate not in _FP32_RUNS:
        _FP32_RUNS[rate] = _grads_of(gpu, torch.float32, rate)
    return _FP32_RUNS[rate]


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16])
def test_half_gradients_no_further_from_fp32_than_without_drop_path(gpu, dtype):
    """X3D-M n=2, t=4, s=128: per gradient tensor the relative L2 distance between the 16-bit device run and the fp32 device run
    (pinned to the reference by test_train_step_fp32_with_drop_path), at DROP_PATH_RATE = 0.5 and -- in this same test -- at 0, the
    parent's code path.  Required: maximum over tensors <= 2x, median <= 1.5x the rate-0 figures (the margin is for the smaller
    effective batch of a dropped branch).
    On an MI355X (profiles/tail_refactor_mi355x.txt): bf16 ratios max 0.599, median 0.671; fp16 max 1.532, median 0.574.  The test
    prints the four figures and both ratios before it asserts."""
    dist = {}
    for rate in (0.0, 0.5):
        ref, got = _fp32_run(gpu, rate), _grads_of(gpu, dtype, rate)
        dist[rate] = torch.tensor([rel_l2(got[k], ref[k]) for k in ref if ref[k].norm().item() > 0])
    mx0, md0 = dist[0.0].max().item(), dist[0.0].median().item()
    mx1, md1 = dist[0.5].max().item(), dist[0.5].median().item()
    print(f"DP_HALF {dtype}: rate 0 max {mx0:.4e} median {md0:.4e}; rate 0.5 max {mx1:.4e} median {md1:.4e}; "
          f"ratios max {mx1 / mx0:.3f} median {md1 / md0:.3f}")
    assert mx1 <= 2.0 * mx0, f"max relative L2 distance {mx1:.3e} with drop-path against {mx0:.3e} without"
    assert md1 <= 1.5 * md0, f"median relative L2 distance {md1:.3e} with drop-path against {md0:.3e} without"


# ---- 6. the trainer -----------------------------------------------------------------------------------------------------------
CLASSES = 10
OPTS = ["DATA.TEMP_DURATION", 4, "DATA.TRAIN_CROP_SIZE", 32, "DATA.TEST_CROP_SIZE", 32, "TEST.NUM_TEMPORAL_VIEWS", 1,
        "TEST.NUM_SPATIAL_CROPS", 3, "TEST.BATCH_SIZE", 2, "NETWORK.NUM_CLASSES", CLASSES, "NETWORK.DROPOUT_RATE", 0.0,
        "TRAIN.BATCH_SIZE", 2, "TRAIN.DATASET_SIZE", 4, "TRAIN.EPOCHS", 2]


def _cfg(*extra):
    import x3d_tf_amd as x
    return x.get_config("XS", OPTS + list(extra))


def _batches(k, gpu, seed=5, views=1):
    gen = torch.Generator().manual_seed(seed)
    return [(torch.randn(2 * views, 4, 32, 32, 3, generator=gen).to(gpu), torch.randint(0, CLASSES, (2,), generator=gen).to(gpu))
            for _ in range(k)]


def test_trainer_fit_draws_a_new_table_every_step(gpu, tmp_path):
    """X3D-XS bf16 at DROP_PATH_RATE = 0.3 through Trainer.fit: finite losses; the table read after step k is the host
    reference's for (seed, k) and differs from step to step; the eval plan records no *_dp launch and gives, bit for bit, the
    probabilities of a rate-0 model holding the same weights; resume() continues the step counter."""
    from x3d_tf_amd.arch import drop_path_rates
    from x3d_tf_amd.model import X3D
    from x3d_tf_amd.train import Trainer
    cfg = _cfg("NETWORK.DROP_PATH_RATE", 0.3)
    m = X3D(cfg, dtype=torch.bfloat16, device=gpu, seed=1)
    rates = drop_path_rates(m.arch)
    seed = 77
    tr = Trainer(m, cfg, drop_path_seed=seed)
    assert m.drop_path_step() == 0
    tables = []

    def on_step(trainer, pl):
        tables.append((m.drop_path_step(), pl.dp_keep.cpu().numpy().copy()))
    run = str(tmp_path / "run")
    val = _batches(1, gpu, seed=9, views=3)
    hist = tr.fit(iter(_batches(4, gpu)), model_dir=run, validation_data=lambda: val, metrics=(), on_step=on_step)
    assert len(hist) == 2 and all(np.isfinite(h) for h in hist) and np.isfinite(tr.history["val_loss"]).all()
    assert [s for s, _ in tables] == [1, 2, 3, 4]
    for k, (_, t) in enumerate(tables):
        assert np.array_equal(t, R.keep_table(seed, k, rates, 2)), f"table of step {k}"
    assert any(not np.array_equal(tables[0][1], t) for _, t in tables[1:])
    # inference: the plan of the validation above has no drop-path launch, and equals the rate-0 model bit for bit
    ev = m._plans[(6, 4, 32, 32, False)]
    assert not any("_dp" in it[0] for it in ev.fwd if it is not None) and ev.dp_keep is None
    m0 = X3D(_cfg(), dtype=torch.bfloat16, device=gpu, seed=2)
    m0.load_state_dict(m.state_dict())
    assert torch.equal(m(val[0][0], training=False), m0(val[0][0], training=False))
    # a resumed run goes on from the number of forward_backward calls made
    m2 = X3D(cfg, dtype=torch.bfloat16, device=gpu, seed=3)
    tr2 = Trainer(m2, cfg, drop_path_seed=seed)
    assert tr2.resume(run) == 2 and tr2.opt_step == 4
    assert m2.drop_path_step() == 4
    pl = tr2.step(*_batches(1, gpu, seed=6)[0], lr=0.01)
    assert np.array_equal(pl.dp_keep.cpu().numpy(), R.keep_table(seed, 4, rates, 2)) and m2.drop_path_step() == 5


def test_trainer_accumulation_draws_per_micro_batch(gpu):
    """SOLVER.ACCUM_STEPS = 2: every micro-batch draws anew, so the step counter advances twice per optimizer update."""
    from x3d_tf_amd.arch import drop_path_rates
    from x3d_tf_amd.model import X3D
    from x3d_tf_amd.train import Trainer
    cfg = _cfg("NETWORK.DROP_PATH_RATE", 0.3, "SOLVER.ACCUM_STEPS", 2)
    m = X3D(cfg, dtype=torch.bfloat16, device=gpu, seed=1)
    rates = drop_path_rates(m.arch)
    tr = Trainer(m, cfg, drop_path_seed=5)
    seen = []
    for k, (clips, labels) in enumerate(_batches(4, gpu)):
        pl = tr.step(clips, labels, lr=0.01)
        seen.append(pl.dp_keep.cpu().numpy().copy())
        assert np.array_equal(seen[-1], R.keep_table(5, k, rates, 2))
        assert m.drop_path_step() == k + 1 and tr.opt_step == (k + 1) // 2
    assert torch.isfinite(pl.loss_rows).all()
