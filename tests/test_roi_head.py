"""The ROI head for action detection on the host: tests/roi_ref.py against a second formulation (torch grid_sample + autograd), the
DETECTION.* config section, dry plans with the switch on and off, the two entry points' declarations, and the refusals of the ops
wrappers (the kernels, the model and the trainer are in test_roi_head_gpu.py)."""
import os
import re
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import x3d_tf_amd as x  # noqa: E402
from x3d_tf_amd.config import detection_settings  # noqa: E402
import roi_ref as R  # noqa: E402

SCALE = 1.0 / 32
DEFAULTS = dict(ENABLE=False, MAX_BOXES=8, ROI_XFORM_RESOLUTION=7, SPATIAL_SCALE_FACTOR=32, ROI_SAMPLING_RATIO=0)


# ---- the reference against torch ------------------------------------------------------------------------------------------
def _grid_sample_head(x, ss, boxes, num_boxes, r, sr):
    """torch fp64: mean_t relu(s x + t) -> per box and bin, grid_sample(bilinear, border, align_corners) at the sample points in
    pixel coordinates -> mean over the sample grid -> max over the bins.  Returns (pooled [N*K][C] with grad, bins, valid)."""
    n_, c_, _, H, W = x.shape
    K = boxes.shape[1]
    m = torch.relu(ss[:, 0].view(1, -1, 1, 1, 1) * x + ss[:, 1].view(1, -1, 1, 1, 1)).mean(2)         # [N][C][H][W]
    pooled, bins_all, valid = [], [], []
    for n in range(n_):
        for k in range(K):
            geom = R.box_geometry(boxes[n, k], k < num_boxes[n], SCALE, H, W, r, sr)
            if geom is None:
                pooled.append(torch.zeros(c_, dtype=torch.float64))
                bins_all.append(torch.zeros(c_, r * r, dtype=torch.float64))
                valid.append(False)
                continue
            x1, y1, bw, bh, gh, gw = geom
            ys = torch.from_numpy(R.sample_coords(y1, bh, gh, r))          # [R][gh]
            xs = torch.from_numpy(R.sample_coords(x1, bw, gw, r))          # [R][gw]
            ny = 2 * ys / (H - 1) - 1 if H > 1 else torch.zeros_like(ys)
            nx = 2 * xs / (W - 1) - 1 if W > 1 else torch.zeros_like(xs)
            gy = ny.view(r, 1, gh, 1).expand(r, r, gh, gw)
            gx = nx.view(1, r, 1, gw).expand(r, r, gh, gw)
            grid = torch.stack([gx, gy], -1).reshape(1, r * r, gh * gw, 2)
            v = torch.nn.functional.grid_sample(m[n:n + 1], grid, mode="bilinear", padding_mode="border", align_corners=True)
            b = v.mean(-1)[0]                                               # [C][R*R]
            bins_all.append(b)
            pooled.append(b.max(dim=1).values)
            valid.append(True)
    return torch.stack(pooled), torch.stack(bins_all), np.array(valid)


@pytest.mark.parametrize("sr", [0, 2])
@pytest.mark.parametrize("thw", [(4, 7, 7), (3, 5, 3), (2, 8, 10)], ids=lambda s: "x".join(map(str, s)))
def test_reference_against_grid_sample(thw, sr):
    t, h, w = thw
    c, n, k, r = 3, 2, 6, 3
    g = torch.Generator().manual_seed(7)
    xt = torch.randn(n, c, t, h, w, generator=g, dtype=torch.float64)
    ss = torch.stack([0.5 + torch.rand(c, generator=g, dtype=torch.float64), 0.25 + torch.rand(c, generator=g, dtype=torch.float64)], 1)
    ss[1, 0] = -ss[1, 0]
    boxes = R.box_mix(n, k, 32 * h, 32 * w, seed=11)        # all six kinds in each sample
    nb = [k, 3]                                             # sample 1: the last three slots are empty whatever they hold
    pooled, bins, argmax, valid = R.forward(xt.numpy(), ss.numpy(), boxes, nb, r, sr, SCALE)
    xg = xt.clone().requires_grad_(True)
    t_pooled, t_bins, t_valid = _grid_sample_head(xg, ss, boxes, nb, r, sr)
    assert (valid == t_valid).all() and valid.sum() == 4 + 3      # inside, touching, beyond, sub-pixel; not: zero width, NaN, empty
    assert np.abs(pooled - t_pooled.detach().numpy()).max() < 1e-12
    assert np.abs(bins - t_bins.detach().numpy()).max() < 1e-12
    top2 = np.sort(bins[valid], axis=2)[:, :, -2:]
    assert (top2[:, :, 1] - top2[:, :, 0]).min() > 1e-9, "a maximal bin is not unique: draw other boxes"
    assert (pooled[~valid] == 0).all() and (argmax[~valid] == 0).all()
    dp = torch.randn(n * k, c, generator=g, dtype=torch.float64)
    (t_pooled * dp).sum().backward()
    gref, _ = R.backward(dp.numpy(), argmax, boxes, nb, xt.numpy(), ss.numpy(), r, sr, SCALE)
    assert np.abs(gref * ss.numpy()[None, :, 0, None, None, None] - xg.grad.numpy()).max() < 1e-12     # (g is the gradient wrt s x + t)


# ---- config ---------------------------------------------------------------------------------------------------------------
ONE_VIEW = ["TEST.NUM_SPATIAL_CROPS", 1, "TEST.NUM_TEMPORAL_VIEWS", 1]


def test_config_defaults_and_a_tree_without_the_section():
    assert dict(x.get_default_config().DETECTION) == DEFAULTS
    s = detection_settings(x.get_config("XS"))
    assert s == (False, 8, 7, 32.0, 0) and not s.enable
    c = x.get_config("XS", ONE_VIEW + ["DETECTION.ENABLE", True, "DETECTION.MAX_BOXES", 5, "DETECTION.ROI_XFORM_RESOLUTION", 4,
                                       "DETECTION.SPATIAL_SCALE_FACTOR", 16, "DETECTION.ROI_SAMPLING_RATIO", 2])
    s = detection_settings(c)
    assert s == (True, 5, 4, 16.0, 2)
    assert (s.enable, s.max_boxes, s.resolution, s.spatial_scale_factor, s.sampling_ratio) == tuple(s)
    old = c.clone()
    old.defrost()
    del old["DETECTION"]
    assert detection_settings(old) == (False, 8, 7, 32.0, 0)
    assert set(c) == set(old) | {"DETECTION"}


@pytest.mark.parametrize("over, key", [
    (["DETECTION.MAX_BOXES", 0], "DETECTION.MAX_BOXES"), (["DETECTION.MAX_BOXES", 65], "DETECTION.MAX_BOXES"),
    (["DETECTION.ROI_XFORM_RESOLUTION", 0], "DETECTION.ROI_XFORM_RESOLUTION"),
    (["DETECTION.ROI_XFORM_RESOLUTION", 16], "DETECTION.ROI_XFORM_RESOLUTION"),
    (["DETECTION.SPATIAL_SCALE_FACTOR", 0], "DETECTION.SPATIAL_SCALE_FACTOR"),
    (["DETECTION.SPATIAL_SCALE_FACTOR", -4], "DETECTION.SPATIAL_SCALE_FACTOR"),
    (["DETECTION.ROI_SAMPLING_RATIO", -1], "DETECTION.ROI_SAMPLING_RATIO"),
])
def test_config_value_refusals_name_the_key(over, key):
    with pytest.raises(ValueError, match=re.escape(key)):
        x.get_config("XS", over)
    cfg = x.get_config("XS", freeze=False)
    cfg.merge_from_list(over)
    with pytest.raises(ValueError, match=re.escape(key)):
        detection_settings(cfg)


@pytest.mark.parametrize("over, word", [
    (ONE_VIEW + ["MIXUP.ENABLE", True], "MIXUP.ENABLE"),
    (ONE_VIEW + ["DISTILL.ENABLE", True, "DISTILL.TEACHER", "M"], "DISTILL.ENABLE"),
    (["TEST.NUM_SPATIAL_CROPS", 3, "TEST.NUM_TEMPORAL_VIEWS", 1], "TEST.NUM_SPATIAL_CROPS"),
    (["TEST.NUM_SPATIAL_CROPS", 1, "TEST.NUM_TEMPORAL_VIEWS", 10], "TEST.NUM_SPATIAL_CROPS"),
])
def test_config_refused_combinations(over, word):
    x.get_config("XS", over)                                       # fine with the switch off
    with pytest.raises(ValueError, match=re.escape(word)):
        x.get_config("XS", over + ["DETECTION.ENABLE", True])


# ---- dry plans ------------------------------------------------------------------------------------------------------------
BASE = ["DATA.TEMP_DURATION", 4] + ONE_VIEW
K = 3


def _dry_plan(cfg, training):
    from x3d_tf_amd.model import X3D
    return X3D(cfg, dtype=torch.float32, device="dry")._plan(2, 4, 64, 64, training)


def _names(pl):
    return [e[0] for e in pl.fwd], [e[0] for e in pl.bwd]


@pytest.mark.parametrize("training", [True, False])
def test_dry_plans_switch_off_is_the_section_absent(training):
    absent = x.get_config("XS", BASE, freeze=False)
    del absent["DETECTION"]
    off = x.get_config("XS", BASE + ["DETECTION.ENABLE", False, "DETECTION.MAX_BOXES", K])
    assert _names(_dry_plan(absent, training)) == _names(_dry_plan(off, training))
    assert "x3d_roi_pool_fwd" not in _names(_dry_plan(off, training))[0]


@pytest.mark.parametrize("training", [True, False])
def test_dry_plans_switch_on_changes_one_name_each_way(training):
    off = _dry_plan(x.get_config("XS", BASE), training)
    on = _dry_plan(x.get_config("XS", BASE + ["DETECTION.ENABLE", True, "DETECTION.MAX_BOXES", K]), training)
    (f0, b0), (f1, b1) = _names(off), _names(on)
    assert len(f0) == len(f1) and [(a, b) for a, b in zip(f0, f1) if a != b] == [("x3d_pool_fwd", "x3d_roi_pool_fwd")]
    assert len(b0) == len(b1)
    if training:
        assert [(a, b) for a, b in zip(b0, b1) if a != b] == [("x3d_relu_bn_bwd_reduce", "x3d_roi_pool_bwd")]
    # the dense launches carry 2 * K rows (x3d_dense_fwd: N is argument 7; x3d_dense_bwd: argument 10)
    for lst, name, pos in ((on.fwd, "x3d_dense_fwd", 7), (on.bwd, "x3d_dense_bwd", 10)):
        rows = [e[2][pos] for e in lst if e[0] == name]
        assert rows == ([2 * K, 2 * K] if lst is on.fwd or training else []), (name, rows)
    assert on.rows == 2 * K and off.rows == 2
    assert tuple(on.pooled.shape) == (2 * K, on.model.arch.conv5_out) and tuple(on.logits.shape)[0] == 2 * K
    assert tuple(on.boxes.shape) == (2, K, 4) and tuple(on.num_boxes.shape) == (2,)
    if training:
        from x3d_tf_amd import dispatch
        assert tuple(on.dlogits.shape)[0] == 2 * K and tuple(on.roi_argmax.shape) == tuple(on.pooled.shape)
        acc = [a for a in dispatch.scratch_accesses(on) if a[1] == "x3d_roi_pool_bwd"]
        i = b1.index("x3d_roi_pool_bwd")
        assert acc == [(i, "x3d_roi_pool_bwd", "bsums", on.bwd[i][2][7], "W")] and on.bwd[i][2][7]
        assert dispatch.scratch_hazards(on) == []
    else:
        assert on.roi_argmax is None and on.fwd[f1.index("x3d_roi_pool_fwd")][2][5] is None


def test_dry_plan_refuses_what_the_kernel_would():
    from x3d_tf_amd.model import X3D
    m = X3D(x.get_config("XS", BASE + ["DETECTION.ENABLE", True, "DETECTION.MAX_BOXES", 64]), dtype=torch.float32, device="dry")
    with pytest.raises(ValueError, match="N\\*K"):
        m._plan(33, 4, 64, 64, True)


# ---- ABI ------------------------------------------------------------------------------------------------------------------
def test_abi_version_struct_count_and_the_two_signatures():
    from x3d_tf_amd import hip
    lib = hip.load()
    assert hip.ABI_VERSION == 138 == lib.x3d_version()
    with open(os.path.join(ROOT, "include", "x3d_hip.h")) as f:
        header = " ".join(f.read().split())
    assert len(re.findall(r"typedef\s+struct", header)) == 16
    fwd = ("int x3d_roi_pool_fwd(const void* x_raw, const float* scale_shift, const float* boxes, const int* num_boxes, "
           "float* pooled, unsigned char* argmax, int N, int C, int T, int H, int W, int K, int R, "
           "int sampling_ratio, float spatial_scale, int dtype, void* stream);")
    bwd = ("int x3d_roi_pool_bwd(const float* dpooled, const unsigned char* argmax, const float* boxes, const int* num_boxes, "
           "const void* yraw, const float* scale_shift, void* g, double* sums, int N, int C, int T, int H, "
           "int W, int K, int R, int sampling_ratio, float spatial_scale, int dtype, void* stream);")
    assert fwd in header and bwd in header
    for name, nargs in (("x3d_roi_pool_fwd", 17), ("x3d_roi_pool_bwd", 19)):
        assert name in hip.exported_symbols() and len(getattr(lib, name).argtypes) == nargs


def test_library_refusals_come_before_any_launch():
    from x3d_tf_amd import hip
    lib = hip.load()
    A = [0x10000 * (i + 1) for i in range(8)]            # addresses that are never touched

    def fwd(n=2, c=3, t=4, h=7, w=7, k=3, r=7, sr=0, scale=SCALE):
        return lib.x3d_roi_pool_fwd(A[0], A[1], A[2], A[3], A[4], A[5], n, c, t, h, w, k, r, sr, scale, hip.F32, None)

    def bwd(n=2, c=3, t=4, h=7, w=7, k=3, r=7, sr=0, scale=SCALE):
        return lib.x3d_roi_pool_bwd(A[0], A[1], A[2], A[3], A[4], A[5], A[6], A[7], n, c, t, h, w, k, r, sr, scale, hip.F32, None)

    for kw, word in ((dict(h=33, w=32), b"H*W"), (dict(r=16), b"R ="), (dict(r=0), b"R ="), (dict(k=65), b"K ="), (dict(k=0), b"K ="),
                     (dict(n=64, k=33), b"N*K"), (dict(sr=-1), b"sampling_ratio"), (dict(scale=0.0), b"spatial_scale"),
                     (dict(scale=-1.0), b"spatial_scale")):
        for call, who in ((fwd, b"roi_pool_fwd"), (bwd, b"roi_pool_bwd")):
            assert call(**kw) != 0
            msg = lib.x3d_last_error()
            assert word in msg and who in msg, msg


# ---- ops wrappers -----------------------------------------------------------------------------------------------------------
def _host_args(n=2, c=3, t=4, h=7, w=7, k=3):
    return dict(x=torch.zeros(n, c, t, h, w), ss=torch.zeros(c, 2), boxes=torch.zeros(n, k, 4),
                nb=torch.zeros(n, dtype=torch.int32), rows=torch.zeros(n * k, c), argmax=torch.zeros(n * k, c, dtype=torch.uint8),
                sums=torch.zeros(c, 2, dtype=torch.float64))


@pytest.mark.parametrize("change, word", [
    (lambda a: a.update(boxes=torch.zeros(2, 3, 5)), "boxes"),
    (lambda a: a.update(boxes=torch.zeros(3, 3, 4)), "boxes"),
    (lambda a: a.update(boxes=torch.zeros(2, 3, 4, dtype=torch.float64)), "boxes"),
    (lambda a: a.update(nb=torch.zeros(2, dtype=torch.int64)), "num_boxes"),
    (lambda a: a.update(nb=torch.zeros(3, dtype=torch.int32)), "num_boxes"),
    (lambda a: a.update(_host_args(n=33, k=64)), "N*K"),
    (lambda a: a.update(r=16), "resolution"),
    (lambda a: a.update(_host_args(h=33, w=32)), "H*W"),
    (lambda a: a.update(rows=torch.zeros(6, 4)), "pooled"),
    (lambda a: a.update(argmax=torch.zeros(6, 3, dtype=torch.int32)), "argmax"),
], ids=["box-last-dim", "box-batch", "box-dtype", "num_boxes-dtype", "num_boxes-shape", "rows", "R16", "HW", "pooled-shape", "argmax-dtype"])
def test_ops_wrapper_refusals_name_the_argument(change, word):
    """host tensors throughout: a call that got as far as the library would fail on them differently (X3DHipError)"""
    from x3d_tf_amd import ops
    a = dict(_host_args(), r=7)
    change(a)
    with pytest.raises(ValueError, match=re.escape(word)):
        ops.roi_pool_fwd(a["x"], a["ss"], a["boxes"], a["nb"], a["rows"], a["argmax"], resolution=a["r"])
    word_b = "dpooled" if word == "pooled" else word
    with pytest.raises(ValueError, match=re.escape(word_b)):
        ops.roi_pool_bwd(a["rows"], a["argmax"], a["boxes"], a["nb"], a["x"], a["ss"], torch.zeros_like(a["x"]), a["sums"],
                         resolution=a["r"])


def test_model_refuses_boxes_with_the_switch_off_and_the_switch_without_boxes():
    from x3d_tf_amd.model import X3D
    clips = torch.zeros(2, 4, 64, 64, 3)
    off = X3D(x.get_config("XS", BASE), dtype=torch.float32, device="dry")
    with pytest.raises(ValueError, match="DETECTION.ENABLE"):
        off.call(clips, boxes=torch.zeros(2, 3, 4), num_boxes=[1, 1])
    on = X3D(x.get_config("XS", BASE + ["DETECTION.ENABLE", True, "DETECTION.MAX_BOXES", K]), dtype=torch.float32, device="dry")
    with pytest.raises(ValueError, match="boxes"):
        on.call(clips)
    with pytest.raises(ValueError, match="boxes"):
        on.forward_backward(clips, torch.zeros(2, K, dtype=torch.int64))
    with pytest.raises(ValueError, match="boxes"):
        on.call(clips, boxes=torch.zeros(2, K + 1, 4), num_boxes=[1, 1])
    with pytest.raises(ValueError, match="num_boxes"):
        on.call(clips, boxes=torch.zeros(2, K, 4), num_boxes=[1, K + 1])
    with pytest.raises(ValueError, match="sample_weight"):
        on.forward_backward(clips, torch.zeros(2, K, dtype=torch.int64), boxes=torch.zeros(2, K, 4), num_boxes=[1, 1],
                            sample_weight=torch.ones(2))
    assert not on._plans and not off._plans           # nothing was recorded, let alone launched


# ---- the edge table of the GPU suite ----------------------------------------------------------------------------------------
def test_roi_edge_table_runs_every_class():
    """shapes.ROI_EDGE, over the three storage types, holds a case of every loop and dispatch class of roi.hip (roi_classes.CLASSES);
    a class loses its cases -> its name is reported; and the constants the table was built for are still roi.hip's"""
    import roi_classes as RC
    from shapes import ROI_EDGE, roi_edge_id
    assert RC.roi_defines() == RC.ROI
    assert RC.ROI["ROI_STAGE"] // RC.ROI["ROI_MAX_HW"] >= 8            # (what keeps `if (tc < q) tc = q` out of reach)
    ids = [roi_edge_id(c) for c in ROI_EDGE]
    assert len(set(ids)) == len(ids)
    cov = RC.covered(ROI_EDGE)
    assert RC.missing(ROI_EDGE) == [], f"no case of ROI_EDGE runs: {RC.missing(ROI_EDGE)}"
    for name, labels in cov.items():                                   # the check has teeth: without its cases a class is reported
        rest = [c for c in ROI_EDGE if c[0] not in labels]
        assert name in RC.missing(rest), name
    assert all(any(c[0] in labels for labels in cov.values()) for c in ROI_EDGE), "a case that runs no class"
    for c in ROI_EDGE:                                                 # what the library and the GPU test's timing accept
        _, (t, h, w), ch, k, nb, r, sr, den, boxes, offs, extra = c
        assert h * w <= RC.ROI["ROI_MAX_HW"] and 1 <= r <= 15 and 1 <= k <= 64 and len(nb) == 2 and all(0 <= v <= k for v in nb)
        assert (ch <= 3 or (t, h, w) == (16, 7, 7)) and boxes in ("grid", "offgrid") and extra in ("", "poison")
    assert sum(c[10] == "poison" and max(RC.form(c, "float32")["bwd_rounds"]) >= 2 for c in ROI_EDGE) == 1


def test_roi_reference_is_quick_on_the_edge_table():
    """the fp64 reference of every ROI_EDGE case, forward and backward, in under two seconds (the GPU test runs it three times)"""
    import time
    import roi_classes as RC
    from shapes import ROI_EDGE
    worst = 0.0
    for i, c in enumerate(ROI_EDGE):
        _, (t, h, w), ch, k, nb, r, sr, den, kind, _, _ = c
        scale = float(np.float32(1.0 / den))
        rng = np.random.default_rng(i)
        xx = rng.standard_normal((2, ch, t, h, w))
        ss = np.stack([np.full(ch, 0.7), np.full(ch, 0.5)], 1)
        boxes = RC.case_boxes(i, c)
        t0 = time.perf_counter()
        pooled, bins, am, valid = R.forward(xx, ss, boxes, nb, r, sr, scale)
        R.backward(rng.standard_normal((2 * k, ch)), am, boxes, nb, xx, ss, r, sr, scale)
        worst = max(worst, time.perf_counter() - t0)
        assert valid.any() and (k < 4 or not valid.all()), c[0]
        per_sample = valid.reshape(2, k)
        assert all(per_sample[a].any() for a in range(2) if nb[a] >= 3), c[0]
        if c[10] == "poison":
            assert per_sample[:, 4:].any(), "the poison case needs a valid box in its second round"
        if r in (9, 15):
            assert valid.any()
    print(f"slowest case: {worst:.3f} s")
    assert worst < 2.0


def test_offgrid_boxes_keep_the_kinds_and_leave_the_grid():
    b = R.box_mix_offgrid(2, 6, 168, 168, seed=3)
    g = R.box_mix(2, 6, 168, 168, seed=3)
    fin = np.isfinite(b).all(axis=2)
    assert (fin == np.isfinite(g).all(axis=2)).all() and (~fin).sum() == 2          # the NaN slots are the same
    assert b.dtype == np.float32 and np.abs(b[fin] - g[fin]).max() <= 1.0 / 16      # the grid version is this one rounded
    assert (b[fin] * 8 != np.round(b[fin] * 8)).mean() > 0.5                        # most coordinates are off the 1/8 grid
    assert (b[:, 4, 0] == b[:, 4, 2]).all()                                          # zero width stays exactly zero
    valid = [R.box_geometry(b[0, k], True, float(np.float32(1 / 24)), 7, 7, 7, 0) is not None for k in range(6)]
    assert valid == [True, True, True, True, False, False]
