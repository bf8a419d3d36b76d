"""Multi-label (Charades-style) training on the GPU: x3d_sigmoid_bce / x3d_view_max / x3d_multilabel_ap against fp64
restatements, the sigmoid head of the model against the oracle's autograd, fine-tuning from a checkpoint with another
class count, the multi-label input pipeline and Trainer.fit with mAP validation."""
import math
import os
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import x3d_tf_amd as x  # noqa: E402
from x3d_tf_amd import dataloader as DL  # noqa: E402
from x3d_tf_amd import hip, ops  # noqa: E402
from test_multilabel import ap_ref_all  # noqa: E402


def _bce_ref(logits, targets, grad_scale):
    z = logits.double()
    y = targets.double()
    p = torch.sigmoid(z)
    rows = (z.clamp(min=0) - z * y + torch.log1p(torch.exp(-z.abs()))).mean(1)
    return p, rows, grad_scale * (p - y) / z.shape[1]


# ---- x3d_sigmoid_bce --------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("n", [1, 7, 64, 130])
@pytest.mark.parametrize("m", [1, 157, 400])
def test_sigmoid_bce_matches_fp64(gpu, n, m):
    g = torch.Generator().manual_seed(n * 1000 + m)
    z = torch.randn(n, m, generator=g) * 4
    far = torch.rand(n, m, generator=g)
    z[far < 0.05] = 1e4
    z[(far >= 0.05) & (far < 0.1)] = -1e4
    z[(far >= 0.1) & (far < 0.15)] *= 30
    y = torch.rand(n, m, generator=g)
    y[y < 0.3] = 0.0
    y[y > 0.8] = 1.0
    gs = 0.37
    probs = torch.empty(n, m, device=gpu)
    rows = torch.empty(n, device=gpu)
    dl = torch.empty(n, m, device=gpu)
    ops.sigmoid_bce(z.to(gpu), y.to(gpu), probs, rows, dl, gs)
    torch.cuda.synchronize()
    p_ref, r_ref, d_ref = _bce_ref(z, y, gs)
    assert torch.isfinite(dl).all() and torch.isfinite(rows).all()
    assert (probs.cpu().double() - p_ref).abs().max().item() <= 1e-6
    assert ((rows.cpu().double() - r_ref).abs() / r_ref.abs().clamp(min=1e-30)).max().item() <= 1e-6
    assert (dl.cpu().double() - d_ref).abs().max().item() <= 1e-6 * d_ref.abs().max().item() + 1e-30


@pytest.mark.gpu
def test_sigmoid_bce_nan_rows_and_probs_only(gpu):
    n, m = 5, 157
    g = torch.Generator().manual_seed(7)
    z = torch.randn(n, m, generator=g)
    y = (torch.rand(n, m, generator=g) < 0.1).float()
    z[2, 17] = float("nan")
    probs = torch.empty(n, m, device=gpu)
    rows = torch.empty(n, device=gpu)
    dl = torch.empty(n, m, device=gpu)
    ops.sigmoid_bce(z.to(gpu), y.to(gpu), probs, rows, dl, 1.0)
    torch.cuda.synchronize()
    rows, dl, probs = rows.cpu(), dl.cpu(), probs.cpu()
    assert math.isnan(rows[2].item()) and torch.isfinite(rows[[0, 1, 3, 4]]).all()
    assert math.isnan(dl[2, 17].item()) and math.isnan(probs[2, 17].item())
    assert int(torch.isnan(dl).sum()) == 1 and int(torch.isnan(probs).sum()) == 1
    # targets = None (loss_rows / dlogits NULL too): the same probabilities; a loss without targets is refused
    rows2 = torch.empty(n, device=gpu)
    p2 = torch.empty(n, m, device=gpu)
    hip.call("x3d_sigmoid_bce", z.to(gpu).data_ptr(), None, p2.data_ptr(), None, None, 1.0, n, m)
    torch.cuda.synchronize()
    torch.testing.assert_close(p2.cpu(), probs, rtol=0, atol=0, equal_nan=True)
    with pytest.raises(hip.X3DHipError):
        hip.call("x3d_sigmoid_bce", p2.data_ptr(), None, p2.data_ptr(), rows2.data_ptr(), None, 1.0, n, m)


# ---- x3d_view_max -----------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("videos, views, m", [(1, 1, 1), (3, 6, 157), (4, 30, 400), (2, 10, 401)])
def test_view_max_is_torch_amax(gpu, videos, views, m):
    g = torch.Generator().manual_seed(videos * views + m)
    p = torch.rand(videos * views, m, generator=g)
    p[p < 0.01] = float("nan")
    out = torch.empty(videos, m, device=gpu)
    ops.view_max(p.to(gpu), out, views)
    torch.cuda.synchronize()
    ref = p.view(videos, views, m).amax(1)
    torch.testing.assert_close(out.cpu(), ref, rtol=0, atol=0, equal_nan=True)


# ---- x3d_multilabel_ap ------------------------------------------------------------------------------------------------
def _ap_inputs(n, m, seed, rate=0.2):
    rng = np.random.default_rng(seed)
    s = (np.floor(rng.random((n, m)) * 8) / 7).astype(np.float32)      # 8 levels: ties everywhere
    t = (rng.random((n, m)) < rate).astype(np.float32)
    if m > 2:
        t[:, 0] = 0.0                                                   # a class without positives
        s[n // 2, 1] = np.nan                                           # a column with a NaN
        soft = rng.random(n) < 0.3
        t[soft, 2] = rng.choice(np.array([0.3, 0.5, 0.7], np.float32), int(soft.sum()))   # soft targets (>= 0.5: positive)
    return s, t


def _check_ap(ap, npos, s, t):
    want = ap_ref_all(s, t)
    got = ap.cpu().numpy()
    assert np.array_equal(np.isnan(got), np.isnan(want))
    ok = ~np.isnan(want)
    assert np.abs(got[ok] - want[ok]).max(initial=0.0) <= 1e-12
    assert npos.cpu().numpy().tolist() == (t >= 0.5).sum(0).tolist()


@pytest.mark.gpu
@pytest.mark.parametrize("n", [1, 63, 1863, 20000])
@pytest.mark.parametrize("m", [1, 157, 400])
def test_multilabel_ap_matches_fp64(gpu, n, m):
    s, t = _ap_inputs(n, m, seed=n + m)
    S, T = torch.from_numpy(s).to(gpu), torch.from_numpy(t).to(gpu)
    ap, npos = ops.multilabel_ap(S, T)
    ap2, _ = ops.multilabel_ap(S, T)
    torch.cuda.synchronize()
    _check_ap(ap, npos, s, t)
    assert torch.equal(torch.nan_to_num(ap, nan=-1.0), torch.nan_to_num(ap2, nan=-1.0))   # bit-identical


@pytest.mark.gpu
@pytest.mark.parametrize("n, rate", [(20000, 0.6), (32768, 0.9), (40000, None)])
def test_multilabel_ap_many_positives(gpu, n, rate):
    """more positives than one histogram chunk holds (several passes), up to X3D_AP_MAX_POSITIVES"""
    s, t = _ap_inputs(n, 2, seed=5, rate=rate or 0.0)
    if rate is None:       # exactly the most positives a class may have, and exactly one histogram chunk (7168)
        rng = np.random.default_rng(9)
        t[rng.permutation(n)[:hip.AP_MAX_POSITIVES], 0] = 1.0
        t[rng.permutation(n)[:7168], 1] = 1.0
    else:
        t[: n // 3, 1] = 1.0
    ap, npos = ops.multilabel_ap(torch.from_numpy(s).to(gpu), torch.from_numpy(t).to(gpu))
    torch.cuda.synchronize()
    _check_ap(ap, npos, s, t)


@pytest.mark.gpu
def test_multilabel_ap_refusals(gpu):
    s = torch.rand(40000, 2, device=gpu)
    t = torch.zeros(40000, 2, device=gpu)
    t[:33000, 1] = 1.0                                   # more positives than the kernel holds: refused, not truncated
    with pytest.raises(ValueError, match="positives"):
        ops.multilabel_ap(s, t)
    ap, npos = ops.multilabel_ap(s, t, check=False)
    torch.cuda.synchronize()
    assert npos.cpu().tolist() == [0, -33000] and math.isnan(ap[1].item())
    with pytest.raises(ValueError):
        ops.multilabel_ap(s.double(), t)
    with pytest.raises(ValueError):
        ops.multilabel_ap(s, t[:, :1].contiguous())
    small = torch.zeros(4, device=gpu)
    lib = hip.load()
    for n, m in ((0, 4), (4, 0), (1 << 16, 1 << 15)):    # refused before any launch
        assert lib.x3d_multilabel_ap(small.data_ptr(), small.data_ptr(), n, m, small.data_ptr(), small.data_ptr(),
                                     hip.stream_ptr()) != 0


@pytest.mark.gpu
def test_device_map_in_chunks_equals_one_call(gpu):
    from x3d_tf_amd.evaluate import DeviceMAP
    s, t = _ap_inputs(1863, 157, seed=3)
    s = np.nan_to_num(s, nan=0.5)
    S, T = torch.from_numpy(s).to(gpu), torch.from_numpy(t).to(gpu)
    dm = DeviceMAP(0.25)
    for a, b in zip(torch.tensor_split(S, 5), torch.tensor_split(T, 5)):
        dm.update(a, b)
    r = dm.result()
    ap, npos = ops.multilabel_ap(S, T)
    ap, npos = ap.cpu(), npos.cpu()
    have = npos > 0
    assert r["videos"] == 1863 and r["classes"] == int(have.sum()) == 156
    assert r["mAP"] == float(ap[have].mean())
    q = np.clip(s.astype(np.float64), 1e-7, 1 - 1e-7)
    t64 = t.astype(np.float64)
    want = float(np.mean(-(t64 * np.log(q) + (1 - t64) * np.log(1 - q)))) + 0.25
    assert abs(r["loss"] - want) <= 1e-12 * want
    want_map = np.nanmean(ap_ref_all(s, t)[npos.numpy() > 0])
    assert abs(r["mAP"] - want_map) <= 1e-12


# ---- the model --------------------------------------------------------------------------------------------------------
def _setup(name, overrides=None):
    from x3d_tf_amd.params import init_params, randomize_bn_
    cfg = x.get_config(name, overrides)
    arch = x.build_arch(cfg)
    return cfg, arch, randomize_bn_(init_params(arch, seed=3), seed=4)


def _model(cfg, params, dtype, gpu):
    from x3d_tf_amd.model import X3D
    m = X3D(cfg, dtype=dtype, device=gpu, seed=0)
    m.load_state_dict(params)
    return m


@pytest.mark.gpu
def test_multilabel_train_step_fp32_matches_oracle(gpu):
    from oracle import x3d_oracle as O
    from util import hip_relu_masks, rel_l2
    cfg, arch, params = _setup("XS", ["DATA.MULTI_LABEL", True])
    n, t, s = 4, 4, 64
    torch.manual_seed(1)
    clips = torch.randn(n, t, s, s, 3)
    y = (torch.rand(n, arch.num_classes) < 0.05).float()
    y[0, :7] = torch.tensor([0.2, 0.9, 0.5, 1.0, 0.0, 0.7, 0.33])        # soft targets
    mask = (torch.rand(n, arch.fc1_out) >= arch.dropout_rate).float()
    m = _model(cfg, params, torch.float32, gpu)
    m.set_dropout_mask(mask)
    pl = m.forward_backward(clips.to(gpu), y)
    torch.cuda.synchronize()
    assert pl.labels is None and pl.targets.shape == (n, arch.num_classes)

    names = O.trainable_names(params)
    leaf = {k: (v.detach().clone().requires_grad_(True) if k in names else v.clone()) for k, v in params.items()}
    probs, logits = O.forward(leaf, clips, arch, training=True, dropout_mask=mask, state=O.BNState(),
                              relu_masks=hip_relu_masks(pl), return_logits=True)
    z = logits.double()
    yd = y.double()
    bce = (z.clamp(min=0) - z * yd + torch.log1p(torch.exp(-z.abs()))).mean(1).mean()
    reg = sum((leaf[k].double() ** 2).sum() for k in O.l2_names(leaf)) * arch.weight_decay
    loss = bce + reg
    grads = dict(zip(names, torch.autograd.grad(loss, [leaf[k] for k in names])))
    got_loss = pl.loss_rows.double().mean().item() + m.regularization_loss().item()
    assert abs(got_loss - loss.item()) <= 1e-5, (got_loss, loss.item())
    assert (pl.probs.cpu().double() - torch.sigmoid(z)).abs().max().item() <= 1e-4
    for k, g_ref in grads.items():
        g = m.grads[k].cpu().double()
        if m.specs[k].l2:
            g = g + 2 * arch.weight_decay * params[k].double()
        e = rel_l2(g, g_ref.double())
        assert e < 1e-3, f"grad {k}: relative L2 error {e:.3e}"
    # call(training=True) returns the sigmoid probabilities of the same forward pass
    p2 = m(clips.to(gpu), training=True)
    torch.cuda.synchronize()
    assert (p2.cpu().double() - torch.sigmoid(z)).abs().max().item() <= 1e-4
    # host targets are checked
    with pytest.raises(ValueError):
        m.forward_backward(clips.to(gpu), y * 2)
    with pytest.raises(ValueError):
        m.forward_backward(clips.to(gpu), y[:, :5])
    pl = m.forward_backward(clips.to(gpu), (y >= 0.5))          # bool targets
    torch.cuda.synchronize()
    assert torch.equal(pl.targets.cpu(), (y >= 0.5).float())


@pytest.mark.gpu
@pytest.mark.parametrize("multi", [True, False])
def test_inference_max_ensemble_matches_oracle(gpu, multi):
    from oracle import x3d_oracle as O
    over = ["TEST.NUM_TEMPORAL_VIEWS", 2, "TEST.NUM_SPATIAL_CROPS", 3, "TEST.ENSEMBLE_METHOD", "max"]
    if multi:
        over += ["DATA.MULTI_LABEL", True]
    cfg, arch, params = _setup("XS", over)
    torch.manual_seed(2)
    clips = torch.randn(12, 4, 64, 64, 3)
    m = _model(cfg, params, torch.float32, gpu)
    out = m(clips.to(gpu), training=False)
    torch.cuda.synchronize()
    _, logits = O.forward({k: v.clone() for k, v in params.items()}, clips, arch, training=False, return_logits=True)
    p = torch.sigmoid(logits.double()) if multi else torch.softmax(logits.double(), -1)
    want = p.view(2, 6, -1).amax(1)
    assert out.shape == want.shape
    assert (out.cpu().double() - want).abs().max().item() <= 1e-4


@pytest.mark.gpu
def test_bf16_x3d_s_loss_goes_down(gpu):
    cfg, arch, params = _setup("S", ["DATA.MULTI_LABEL", True, "NETWORK.NUM_CLASSES", 157])
    torch.manual_seed(5)
    clips = torch.randn(4, 4, 64, 64, 3).to(gpu)
    y = (torch.rand(4, 157) < 0.05).float().to(gpu)
    m = _model(cfg, params, torch.bfloat16, gpu)
    m.set_dropout_mask((torch.rand(4, arch.fc1_out) >= arch.dropout_rate).float())
    losses = []
    for _ in range(5):
        pl = m.forward_backward(clips, y)
        losses.append(float(pl.loss_rows.double().mean()))
        m.apply_sgd(1.0, 0.9)
    torch.cuda.synchronize()
    assert all(np.isfinite(losses)), losses
    assert losses[-1] < losses[0], losses


# ---- fine-tuning from a checkpoint with another class count -----------------------------------------------------------
@pytest.mark.gpu
def test_skip_mismatch_fine_tuning(gpu, tmp_path):
    from x3d_tf_amd.model import X3D
    from x3d_tf_amd.train import Trainer
    src = X3D(x.get_config("XS"), dtype=torch.float32, device=gpu, seed=1)
    src.flat_velocity.copy_(torch.randn(src.flat_velocity.shape, generator=torch.Generator().manual_seed(0)))
    os.makedirs(tmp_path / "k400")
    prefix = src.save_weights(str(tmp_path / "k400" / "ckpt-7"))
    cfg = x.get_config("XS", ["NETWORK.NUM_CLASSES", 157, "DATA.MULTI_LABEL", True])
    dst = X3D(cfg, dtype=torch.float32, device=gpu, seed=2)
    before = dst.state_dict()
    with pytest.raises(ValueError):
        dst.load_weights(prefix)
    dst = X3D(cfg, dtype=torch.float32, device=gpu, seed=2)
    with pytest.warns(UserWarning, match="fc2"):
        skipped = dst.load_weights(prefix, optimizer="sgd", skip_mismatch=True)
    assert sorted(skipped) == ["fc2/bias", "fc2/kernel"]
    from x3d_tf_amd.checkpoint import _flat_slot
    for k, v in dst.params.items():
        if k.startswith("fc2/"):
            assert torch.equal(v, before[k]), k
            if k in dst.grads:
                assert not bool(_flat_slot(dst, dst.flat_velocity, k).any()), k
        else:
            assert torch.equal(v, src.params[k]), k
            if k in dst.grads:
                assert torch.equal(_flat_slot(dst, dst.flat_velocity, k), _flat_slot(src, src.flat_velocity, k)), k
    # Trainer.resume: the flag reaches the pretrained fallback
    dst2 = X3D(cfg, dtype=torch.float32, device=gpu, seed=2)
    tr = Trainer(dst2, cfg)
    with pytest.warns(UserWarning):
        assert tr.resume(str(tmp_path / "empty"), pretrained_ckpt=str(tmp_path / "k400"), skip_mismatch=True) == 0
    assert sorted(tr.skipped_keys) == ["fc2/bias", "fc2/kernel"]
    assert torch.equal(dst2.params["conv5/layer_with_weights-0/kernel"], src.params["conv5/layer_with_weights-0/kernel"])
    with pytest.raises(ValueError):
        Trainer(X3D(cfg, dtype=torch.float32, device=gpu, seed=2), cfg).resume(str(tmp_path / "empty"),
                                                                                pretrained_ckpt=str(tmp_path / "k400"))


# ---- input pipeline and Trainer.fit -----------------------------------------------------------------------------------
CLASSES = 10
OPTS = ["DATA.TEMP_DURATION", 4, "DATA.TRAIN_CROP_SIZE", 32, "DATA.TRAIN_JITTER_SCALES", [34, 40], "DATA.FRAME_RATE", 1,
        "DATA.TEST_CROP_SIZE", 32, "TEST.NUM_TEMPORAL_VIEWS", 1, "TEST.NUM_SPATIAL_CROPS", 3, "TEST.BATCH_SIZE", 2,
        "NETWORK.NUM_CLASSES", CLASSES, "TRAIN.BATCH_SIZE", 2, "TRAIN.DATASET_SIZE", 4, "TRAIN.EPOCHS", 2]


def _write(dirpath, n, seed, bad=None, per_file=2):
    """n smooth synthetic videos with 1-3 labels each as TFRecords; video `bad` gets the class id CLASSES"""
    os.makedirs(dirpath, exist_ok=True)
    rng = np.random.default_rng(seed)
    recs = []
    for i in range(n):
        f = int(rng.integers(5, 9))
        yy, xx = np.mgrid[0:40, 0:48]
        base = np.sin(yy / 5.0 + i + seed)[..., None] * 60 + np.cos(xx[..., None] / 7.0 + np.arange(3) + i) * 60 + 128
        vid = np.stack([np.clip(base + 10 * t, 0, 255) for t in range(f)]).astype(np.uint8)
        labels = [int(c) for c in rng.choice(CLASSES, int(rng.integers(1, 4)), replace=False)]
        if i == bad:
            labels.append(CLASSES)
        recs.append(DL.make_sequence_example(vid, labels))
    for k in range(0, n, per_file):
        DL.write_tfrecords(os.path.join(dirpath, f"part-{k // per_file}.tfrecord"), recs[k:k + per_file])
    return os.path.join(dirpath, "part-*.tfrecord")


def _cfg(multi=True):
    return x.get_config("XS", OPTS + (["DATA.MULTI_LABEL", True] if multi else []))


@pytest.mark.gpu
@pytest.mark.parametrize("training", [True, False])
def test_reader_multi_hot_targets_host_and_device_decode(gpu, tmp_path, training):
    pattern = _write(str(tmp_path / "d"), 6, seed=2)
    cfg, single = _cfg(), _cfg(multi=False)
    bs = 2
    its = [DL.InputReader(c, training, True, device=gpu, seed=4, jpeg_decode=mode)(pattern, bs)
           for c, mode in ((cfg, "host"), (cfg, "device"), (single, "host"))]
    n = 0
    try:
        for (ch, th), (cd, td), (cs, ls) in zip(*its):
            assert th.shape == (bs, CLASSES) and th.dtype == torch.float32 and th.is_cuda
            assert torch.equal(ch, cd) and torch.equal(th, td)
            # the single-label reader on the same records: the same clips (draws, order) and its label among the targets
            assert torch.equal(ch, cs)
            assert bool((th[torch.arange(bs), ls.to(th.device)] == 1.0).all())
            assert bool(((th == 0) | (th == 1)).all()) and bool((th.sum(1) >= 1).all())
            n += 1
            if n == 3:
                break
    finally:
        for it in its:
            it.close()
    assert n == 3


@pytest.mark.gpu
@pytest.mark.parametrize("mode", ["host", "device"])
def test_reader_refuses_out_of_range_class(gpu, tmp_path, mode):
    pattern = _write(str(tmp_path / "bad"), 6, seed=3, bad=1)     # the second record of the first of three files
    it = DL.InputReader(_cfg(), False, True, device=gpu, jpeg_decode=mode)(pattern, 2)
    with pytest.raises(ValueError, match=r"part-0\.tfrecord#1"):
        for _ in it:
            pass


@pytest.mark.gpu
def test_fit_with_map_validation(gpu, tmp_path):
    from x3d_tf_amd.evaluate import evaluate_dataset
    from x3d_tf_amd.model import X3D
    from x3d_tf_amd.train import Trainer
    cfg = _cfg()
    train_pattern = _write(str(tmp_path / "train"), 4, seed=4)
    val_pattern = _write(str(tmp_path / "val"), 5, seed=8)

    def val():
        return DL.InputReader(cfg, False, True, device=gpu)(val_pattern, cfg.TEST.BATCH_SIZE)

    m = X3D(cfg, dtype=torch.float32, device=gpu, seed=1)
    tr = Trainer(m, cfg)
    with pytest.raises(ValueError):
        tr.fit(iter(()), epochs=1, steps_per_epoch=1, metrics=("acc",))
    ds = DL.InputReader(cfg, True, True, device=gpu, seed=3)(train_pattern, cfg.TRAIN.BATCH_SIZE)
    hist = tr.fit(ds, validation_data=val)
    ds.close()
    h = tr.history
    assert set(h) == {"loss", "lr", "mAP", "val_loss", "val_mAP"}
    assert all(len(v) == 2 for v in h.values()) and h["loss"] == hist
    for k in ("loss", "mAP", "val_loss", "val_mAP"):
        assert np.isfinite(h[k]).all(), (k, h[k])
    assert all(0.0 < v <= 1.0 for v in h["mAP"] + h["val_mAP"])
    r = evaluate_dataset(m, cfg, val())
    assert r["videos"] == 4
    assert abs(h["val_mAP"][-1] - r["mAP"]) <= 1e-12 and abs(h["val_loss"][-1] - r["loss"]) <= 1e-9
    assert tr.validate(val())["mAP"] == r["mAP"]
