"""x3d_train_clips_aug / views.make_train_batch_aug on the GPU: the "jitter" rows against x3d_train_clip bit for bit, the
random-resized crop and the colour chain against fp64 restatements (tests/aug_ref.py) with bounds derived from the fp32
operation counts, random erasing, reproducibility, argument errors, and InputReader / Trainer with AUG.ENABLE."""
import itertools
import math
import os

import numpy as np
import pytest
import torch

import x3d_tf_amd as x
from x3d_tf_amd import aug, hip, views
from x3d_tf_amd import dataloader as DL

from tests import aug_ref as R

EPS = 2.0 ** -24          # unit roundoff of fp32
DTYPES = [torch.float32, torch.bfloat16, torch.float16]
MEAN, STD = [0.45, 0.40, 0.50], [0.225, 0.25, 0.2]


def _cfg(t, s, rate=1, *over):
    return x.get_config("XS", ["DATA.TEMP_DURATION", t, "DATA.TRAIN_CROP_SIZE", s, "DATA.FRAME_RATE", rate, "DATA.MEAN", MEAN,
                               "DATA.STD", STD, "AUG.ENABLE", True] + list(over))


def _noise_video(f, h, w, seed):
    """uniform noise: neighbouring pixels differ by up to 255, the worst case for the interpolation weights"""
    return np.random.default_rng(seed).integers(0, 256, (f, h, w, 3), dtype=np.uint8)


def _name(dt):
    return str(dt).split(".")[-1]


# ---- 1. anchor -----------------------------------------------------------------------------------------------------
def _jitter_params(videos, size, jitters, flips, starts, corner):
    out = []
    for v, j, fl, st, co in zip(videos, jitters, flips, starts, corner):
        nh, nw = views.train_resized_hw(v.shape[1], v.shape[2], j)
        y0, x0 = [(0, 0), (nh - size, nw - size), ((nh - size) // 2, nw - size), (nh - size, (nw - size) // 3)][co]
        out.append(aug.neutral_params("jitter", st, j, y0, x0, flip=fl))
    return out


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", DTYPES, ids=_name)
def test_jitter_rows_are_bit_identical_to_train_clip(gpu, dtype):
    cases = [
        # T, S, rate, videos (F, H, W), jitters, flips, starts
        (4, 16, 3, [(5, 240, 320), (7, 340, 256), (3, 17, 33), (4, 33, 17), (6, 17, 33)], [20.7, 18.2, 17.0, 21.9, 16.0],
         [True, False, True, False, False], [4, 6, 2, 0, 5]),
        (3, 112, 2, [(4, 240, 320), (5, 340, 256), (2, 240, 320)], [240.0, 182.5, 227.99], [False, True, True], [3, 1, 1]),
        (2, 15, 1, [(3, 17, 33), (2, 33, 17)], [17.0, 19.3], [True, True], [0, 1]),     # T*S*S % 8 != 0: element-wise stores
        (1, 6, 1, [(3, 17, 33), (2, 33, 17)], [17.0, 8.5], [False, True], [2, 1]),      # ... and a partial run after wide ones (fp32)
    ]
    for t, s, rate, shapes, jitters, flips, starts in cases:
        cfg = _cfg(t, s, rate)
        vids = [torch.from_numpy(_noise_video(*sh, seed=i)).to(gpu) for i, sh in enumerate(shapes)]
        params = _jitter_params(vids, s, jitters, flips, starts, [i % 4 for i in range(len(vids))])
        assert any(views.train_resized_hw(v.shape[1], v.shape[2], p.jitter) == tuple(v.shape[1:3]) for v, p in zip(vids, params))
        assert t == 1 or any(p.start + (t - 1) * rate >= v.shape[0] for v, p in zip(vids, params))      # the frame index wraps
        got = views.make_train_batch_aug(vids, cfg, params_list=params, dtype=dtype)
        for i, (v, p) in enumerate(zip(vids, params)):
            want = views.make_train_clip(v, cfg, params=dict(start=p.start, jitter=p.jitter, y0=p.y0, x0=p.x0, flip=p.flip),
                                         dtype=dtype)
            torch.cuda.synchronize()
            assert torch.equal(got[i], want), (t, s, i)
        # a view that is not 16-byte aligned takes the element-wise stores: the same bits
        buf = torch.empty(got.numel() + 1, dtype=dtype, device=gpu)
        got2 = views.make_train_batch_aug(vids, cfg, params_list=params, out=buf[1:].view(got.shape))
        torch.cuda.synchronize()
        assert torch.equal(got2, got)


# ---- 2. random-resized crop ----------------------------------------------------------------------------------------
def _interp_bound(box_side, dtype):
    """|kernel - exact| on the NORMALISED scale for a pixel whose neighbours differ by up to 255.
    source coordinate: sy = bh / S, (y + 0.5) * sy - 0.5 and the weight fy - iy0: four fp32 roundings on magnitudes <= the box
    side -> 4 EPS side per axis; a weight error w moves the value by <= 255 w, two axes.
    the three lerps a + (b - a) l: three roundings each on magnitudes <= 255, top and bottom errors enter the third: 12 EPS 255.
    normalise: x / 255, - mean, / std: the 0-255 error scaled by 1 / (255 std) plus three roundings on magnitudes <=
    (1 + mean) / std.   storage: half an ulp of the stored value (added per element by the caller)."""
    smin = min(STD)
    return _interp_e255(box_side) / (255.0 * smin) + 3 * EPS * (1.0 + max(MEAN)) / smin


def _interp_e255(box_side):
    """the interpolation part of `_interp_bound`, on the 0-255 scale (before normalisation)"""
    return 255.0 * 2 * 4 * EPS * box_side + 12 * EPS * 255.0


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", DTYPES, ids=_name)
def test_rrc_geometry_against_fp64_and_interpolate(gpu, dtype):
    t, s, rate = 3, 40, 2
    cfg = _cfg(t, s, rate, "AUG.CROP", "rrc")
    shapes = [(5, 240, 320), (4, 340, 256), (3, 17, 33), (2, 33, 17), (3, 240, 320), (2, 340, 256)]
    boxes = [(13, 21, 200, 290), (0, 0, 340, 256), (2, 5, 9, 20), (0, 3, 33, 1), (100, 150, 7, 11), (300, 0, 40, 40)]
    flips = [False, True, True, False, True, False]
    starts = [4, 0, 2, 1, 1, 1]
    vids_np = [_noise_video(*sh, seed=10 + i) for i, sh in enumerate(shapes)]
    vids = [torch.from_numpy(v).to(gpu) for v in vids_np]
    params = [aug.neutral_params("rrc", st, box=b, flip=fl) for st, b, fl in zip(starts, boxes, flips)]
    got = views.make_train_batch_aug(vids, cfg, params_list=params, dtype=dtype).float().cpu().double().numpy()
    worst = worst_t = 0.0
    for i, (v, p) in enumerate(zip(vids_np, params)):
        want = R.normalize(R.rrc_clip(v, p.box, p.start, rate, t, s, p.flip), MEAN, STD)
        bound = _interp_bound(max(p.box[2:]), dtype)
        err = np.abs(got[i] - want)
        assert (err <= bound + R.ulp_half(_name(dtype)) * np.abs(want)).all(), (i, err.max(), bound)
        worst = max(worst, err.max() / (bound + R.ulp_half(_name(dtype)) * np.abs(want).max()))
        # second opinion: torch's own bilinear resize of the CPU crop (fp32, so it carries the same kind of error: 2 x bound)
        ry0, rx0, rh, rw = p.box
        crop = torch.from_numpy(v[R.frame_indices(p.start, rate, t, v.shape[0]), ry0:ry0 + rh, rx0:rx0 + rw].astype(np.float32))
        ti = torch.nn.functional.interpolate(crop.permute(0, 3, 1, 2), size=(s, s), mode="bilinear", align_corners=False)
        ti = ti.permute(0, 2, 3, 1).double().numpy()
        ti = R.normalize(ti[:, :, ::-1] if p.flip else ti, MEAN, STD)
        err_t = np.abs(got[i] - ti)
        assert (err_t <= 2 * bound + R.ulp_half(_name(dtype)) * np.abs(ti)).all(), (i, err_t.max(), bound)
        worst_t = max(worst_t, err_t.max() / (2 * bound + R.ulp_half(_name(dtype)) * np.abs(ti).max()))
    print(f"rrc {_name(dtype)}: largest error / bound = {worst:.3f} (fp64), {worst_t:.3f} (interpolate)")


# ---- 3. colour -----------------------------------------------------------------------------------------------------
def _color_bound(p, n_px):
    """|kernel - exact| on the 0-255 scale for the folded chain v = M x + K m on exact inputs x (uint8 values).
    M, K are rounded to fp32 (EPS each), every product and sum is one rounding: 6 EPS on magnitudes <= (A + |K|) 255 with
    A the largest absolute row sum of M.  m: the gray of a pixel is three products and two sums of fp32-rounded weights
    (6 EPS 255); the T S S of them are added in fp64 (n 2^-53 255) and the mean rounded to fp32 (EPS 255)."""
    m, k = aug.fold_color(p)
    a = np.abs(m).sum(1).max()
    e_mean = (6 * EPS + n_px * 2.0 ** -53 + EPS) * 255.0
    return (a + abs(k)) * 255.0 * 6 * EPS + abs(k) * e_mean


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", DTYPES, ids=_name)
def test_colour_chain_against_the_sequential_definition(gpu, dtype):
    t, s = 3, 24
    cfg = _cfg(t, s, 1)
    chains = [(o, g, 1.27, 0.71, 0.83) for o in itertools.permutations(aug.COLOR_OPS) for g in (False, True)]
    chains += [(aug.COLOR_OPS, False, 1.0, 1.36, 1.0), (aug.COLOR_OPS, True, 1.0, 0.62, 1.0),     # contrast alone
               (aug.COLOR_OPS, False, 0.8, 1.0, 1.3), (aug.COLOR_OPS, True, 1.0, 1.0, 1.0)]        # no mean pass / gray only
    vids_np = [_noise_video(4, 24, 24 + (i % 3), seed=30 + i) // (1 + i % 2) for i in range(len(chains))]     # different means
    vids = [torch.from_numpy(v).to(gpu) for v in vids_np]
    # identity-size "jitter" geometry (short side 24 == jitter): the geometric output is the uint8 crop itself
    params = [aug.neutral_params("jitter", i % 4, 24.0, 0, i % 3 if v.shape[2] - 24 >= i % 3 else 0, flip=bool(i & 1))
              ._replace(order=o, gray=g, brightness=b, contrast=c, saturation=sa)
              for i, (v, (o, g, b, c, sa)) in enumerate(zip(vids_np, chains))]
    got = views.make_train_batch_aug(vids, cfg, params_list=params, dtype=dtype).float().cpu().double().numpy()
    smin = min(STD)
    worst = 0.0
    for i, (v, p) in enumerate(zip(vids_np, params)):
        geo = v[R.frame_indices(p.start, 1, t, 4), :, p.x0:p.x0 + s].astype(np.float64)
        geo = geo[:, :, ::-1] if p.flip else geo
        seq = R.color_chain_sequential(geo, p)
        want = R.normalize(seq, MEAN, STD)
        bound = _color_bound(p, t * s * s) / (255.0 * smin) + 3 * EPS * (np.abs(seq).max() / 255.0 + max(MEAN)) / smin
        err = np.abs(got[i] - want)
        assert (err <= bound + R.ulp_half(_name(dtype)) * np.abs(want)).all(), (i, p, err.max(), bound)
        worst = max(worst, err.max() / (bound + R.ulp_half(_name(dtype)) * np.abs(want).max()))
    print(f"colour {_name(dtype)}: largest error / bound = {worst:.3f}")


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", DTYPES, ids=_name)
def test_colour_chain_on_interpolated_geometry(gpu, dtype):
    """The chain and the mean pass on geometric outputs that are NOT the uint8 source: "rrc" rows (fp32, non-integer values)
    against R.rrc_clip + the sequential chain, and "jitter" rows that resize and truncate.
    Bound for the rrc rows: the inputs of the chain carry the interpolation error e <= _interp_e255 each; the affine map
    v = M x + K m moves by <= (A + |K|) e (A the largest absolute row sum of M; m is a mean of grays, and the gray weights
    sum to 1, so m moves by <= e); on top, `_color_bound` for the map's own roundings and the mean.
    The jitter rows truncate to uint8, which no fp64 restatement follows through a value that lands within rounding of an
    integer; their geometric output is taken from x3d_train_clip (the anchor test pins the batched kernel to it bit for
    bit): uint8 values recovered exactly from its fp32 result, so the bound is `_color_bound` on exact inputs, as above."""
    t, s, rate = 3, 24, 2
    cfg = _cfg(t, s, rate)
    chains = [(("contrast", "brightness", "saturation"), False, 1.27, 0.71, 0.83),
              (("saturation", "contrast", "brightness"), True, 0.77, 1.33, 1.21),
              (aug.COLOR_OPS, False, 1.0, 1.36, 1.0)]                                     # contrast alone
    shapes = [(5, 60, 80), (4, 47, 33), (3, 17, 33)]
    boxes = [(3, 7, 50, 61), (0, 0, 47, 33), (2, 5, 9, 20)]
    jitters = [31.7, 26.4, 25.0]                                                          # none is the identity size
    smin = min(STD)
    vids_np = [_noise_video(*sh, seed=40 + i) // (1 + i % 2) for i, sh in enumerate(shapes)]
    vids = [torch.from_numpy(v).to(gpu) for v in vids_np]
    params, geos, e_in = [], [], []
    for i, (v, (o, g, b, c, sa)) in enumerate(zip(vids_np, chains)):
        col = dict(order=o, gray=g, brightness=b, contrast=c, saturation=sa)
        params.append(aug.neutral_params("rrc", i, box=boxes[i], flip=bool(i & 1))._replace(**col))
        geos.append(R.rrc_clip(v, boxes[i], i, rate, t, s, bool(i & 1)))
        e_in.append(_interp_e255(max(boxes[i][2:])))
    for i, (v, (o, g, b, c, sa)) in enumerate(zip(vids_np, chains)):
        col = dict(order=o, gray=g, brightness=b, contrast=c, saturation=sa)
        nh, nw = views.train_resized_hw(v.shape[1], v.shape[2], jitters[i])
        assert (nh, nw) != v.shape[1:3]
        d = dict(start=i, jitter=jitters[i], y0=(nh - s) // 2, x0=nw - s, flip=bool(i & 1))
        params.append(aug.neutral_params("jitter", **d)._replace(**col))
        ref = views.make_train_clip(vids[i], cfg, params=d).cpu().double().numpy()       # fp32: (u8 / 255 - mean) / std
        u8 = (ref * np.asarray(STD) + np.asarray(MEAN)) * 255.0
        assert np.abs(u8 - np.rint(u8)).max() < 1e-3                                      # recovered exactly
        geos.append(np.rint(u8))
        e_in.append(0.0)
    got = views.make_train_batch_aug(vids + vids, cfg, params_list=params, dtype=dtype).float().cpu().double().numpy()
    worst = 0.0
    for i, (p, geo, e) in enumerate(zip(params, geos, e_in)):
        seq = R.color_chain_sequential(geo, p)
        want = R.normalize(seq, MEAN, STD)
        m, k = aug.fold_color(p)
        b255 = (np.abs(m).sum(1).max() + abs(k)) * e + _color_bound(p, t * s * s)
        bound = b255 / (255.0 * smin) + 3 * EPS * (np.abs(seq).max() / 255.0 + max(MEAN)) / smin
        err = np.abs(got[i] - want)
        assert (err <= bound + R.ulp_half(_name(dtype)) * np.abs(want)).all(), (i, p, err.max(), bound)
        worst = max(worst, err.max() / (bound + R.ulp_half(_name(dtype)) * np.abs(want).max()))
    print(f"colour on rrc / resized jitter {_name(dtype)}: largest error / bound = {worst:.3f}")


# ---- 4. erase ------------------------------------------------------------------------------------------------------
def _erase_setup(gpu, mode, n=4, t=4, s=64):
    cfg = _cfg(t, s, 1, "AUG.CROP", "rrc", "AUG.RE_MODE", mode)
    vids = [torch.from_numpy(_noise_video(5, 80, 96, seed=50 + i)).to(gpu) for i in range(n)]
    base = [aug.neutral_params("rrc", i, box=(3 + i, 2, 70, 90), flip=bool(i & 1))._replace(contrast=1.2) for i in range(n)]
    return cfg, vids, base


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", DTYPES, ids=_name)
def test_erase_const(gpu, dtype):
    cfg, vids, base = _erase_setup(gpu, "const")
    boxes = [(0, 64, 0, 64), (5, 17, 60, 64), (63, 64, 0, 1), (10, 50, 3, 44)]
    plain = views.make_train_batch_aug(vids, cfg, params_list=base, dtype=dtype)
    got = views.make_train_batch_aug(vids, cfg, params_list=[p._replace(erase=b) for p, b in zip(base, boxes)], dtype=dtype)
    torch.cuda.synchronize()
    for i, (y0, y1, x0, x1) in enumerate(boxes):
        inside = torch.zeros(got.shape[1:], dtype=torch.bool, device=gpu)
        inside[:, y0:y1, x0:x1] = True
        assert (got[i][inside] == 0).all()
        assert torch.equal(got[i][~inside], plain[i][~inside])


@pytest.mark.gpu
def test_erase_pixel_noise(gpu):
    cfg, vids, base = _erase_setup(gpu, "pixel")
    box = (8, 56, 4, 52)                                           # 48 x 48 x 4 frames x 3 channels x 4 clips = 110 592 samples
    params = [p._replace(erase=box) for p in base]
    seeded = lambda seeds: [p._replace(seed=sd) for p, sd in zip(params, seeds)]
    big = 2 ** 63 - 5                                              # a seed that uses the high word
    plain = views.make_train_batch_aug(vids, cfg, params_list=base)
    a = views.make_train_batch_aug(vids, cfg, params_list=seeded([7, 7, 7, 7]))      # one seed: only the clip index differs
    b = views.make_train_batch_aug(vids, cfg, params_list=seeded([7, 7, 7, 7]))
    c = views.make_train_batch_aug(vids, cfg, params_list=seeded([8, 8, 8, 8]))
    d = views.make_train_batch_aug(vids, cfg, params_list=seeded([7, 7, big, 7]))    # every clip is keyed by its OWN seed
    d2 = views.make_train_batch_aug(vids, cfg, params_list=seeded([7, 7, big - 2 ** 32, 7]))     # the high word counts
    torch.cuda.synchronize()
    inside = torch.zeros(a.shape, dtype=torch.bool, device=gpu)
    inside[:, :, box[0]:box[1], box[2]:box[3]] = True
    assert torch.equal(a[~inside], plain[~inside])
    assert torch.equal(a, b)
    for i in (0, 1, 3):
        assert torch.equal(d[i], a[i]) and torch.equal(d2[i], a[i])
    assert (d[2][inside[2]] != a[2][inside[2]]).double().mean().item() > 0.999
    assert (d[2][inside[2]] != d2[2][inside[2]]).double().mean().item() > 0.999
    na, nc = a[inside].double(), c[inside].double()
    assert bool(torch.isfinite(na).all())
    assert (na != nc).double().mean().item() > 0.999                # another seed: other noise
    per_clip = na.view(4, -1)
    for i, j in itertools.combinations(range(4), 2):                # another clip index: other noise
        assert (per_clip[i] != per_clip[j]).double().mean().item() > 0.999
    # the same clip at another index of the batch keeps its picture and changes its noise
    e = views.make_train_batch_aug([vids[1], vids[0]], cfg, params_list=seeded([7, 7])[1::-1])
    torch.cuda.synchronize()
    assert torch.equal(e[1][~inside[0]], a[0][~inside[0]]) and not torch.equal(e[1][inside[0]], a[0][inside[0]])
    # moments of n standard normal samples: the mean has standard deviation 1 / sqrt(n), the variance sqrt(2 / n)
    n = na.numel()
    assert n >= 100000
    mean, var = na.mean().item(), na.var(unbiased=True).item()
    print(f"erase noise: n = {n}, mean = {mean:.5f} (bound {4 / math.sqrt(n):.5f}), var - 1 = {var - 1:.5f} "
          f"(bound {4 * math.sqrt(2 / n):.5f})")
    assert abs(mean) <= 4.0 / math.sqrt(n)
    assert abs(var - 1.0) <= 4.0 * math.sqrt(2.0 / n)
    # bf16 storage: the same noise rounded once
    h = views.make_train_batch_aug(vids, cfg, params_list=seeded([7, 7, 7, 7]), dtype=torch.bfloat16)
    torch.cuda.synchronize()
    assert torch.equal(h, a.to(torch.bfloat16))


# ---- 5. reproducibility --------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_full_call_is_reproducible(gpu):
    t, s = 8, 112
    cfg = _cfg(t, s, 2, "AUG.CROP", "rrc", "AUG.RE_PROB", 1.0, "AUG.GRAYSCALE_PROB", 0.3)
    shapes = [(9, 240, 320), (12, 340, 256)] * 4
    vids = [torch.from_numpy(_noise_video(*sh, seed=70 + i)).to(gpu) for i, sh in enumerate(shapes)]
    rng = np.random.default_rng(3)
    params = [aug.draw_aug_params(cfg, *sh, rng) for sh in shapes]
    assert all(p.contrast != 1.0 for p in params) and any(p.erase != aug.NO_ERASE for p in params)
    runs = [views.make_train_batch_aug(vids, cfg, params_list=params, dtype=torch.bfloat16) for _ in range(3)]
    torch.cuda.synchronize()
    assert torch.equal(runs[0], runs[1]) and torch.equal(runs[0], runs[2])
    assert bool(torch.isfinite(runs[0].float()).all())
    # drawn from a generator: the same seed, the same batch
    r1 = views.make_train_batch_aug(vids, cfg, rng=np.random.default_rng(3), dtype=torch.bfloat16)
    torch.cuda.synchronize()
    assert torch.equal(r1, runs[0])


# ---- 6. argument errors --------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_argument_errors_launch_nothing(gpu):
    t, s = 2, 16
    cfg = _cfg(t, s, 1)
    vids = [torch.from_numpy(_noise_video(3, 40, 48, seed=i)).to(gpu) for i in range(2)]
    shapes = [(3, 40, 48)] * 2
    good = [aug.neutral_params("rrc", 0, box=(1, 2, 30, 40))._replace(erase=(2, 9, 3, 12), contrast=1.1),
            aug.neutral_params("jitter", 1, 20.0, 2, 3)]
    geom0, color0 = views.aug_tables(shapes, good, cfg)
    G = hip.AUG_G
    lib = hip.load()
    out = torch.full((2, t, s, s, 3), -7.0, device=gpu)
    scratch = torch.empty(int(lib.x3d_train_clips_aug_scratch(2, t, s)), dtype=torch.uint8, device=gpu)
    mean, std = (hip._f * 3)(*MEAN), (hip._f * 3)(*STD)

    def call(geom=geom0, color=color0, n=2, null=None, erase_mode=hip.AUG_ERASE_CONST, dtype=hip.F32):
        addrs = torch.tensor([v.data_ptr() for v in vids], dtype=torch.int64, device=gpu)
        dg, dc = torch.from_numpy(geom).to(gpu), torch.from_numpy(color).to(gpu)
        args = dict(videos=addrs.data_ptr(), geom=dg.data_ptr(), color=dc.data_ptr(), host_geom=geom.ctypes.data,
                    host_color=color.ctypes.data)
        if null:
            args[null] = None
        rc = lib.x3d_train_clips_aug(args["videos"], args["geom"], args["color"], args["host_geom"], args["host_color"],
                                     out.data_ptr(), scratch.data_ptr(), n, t, 1, s, mean, std, erase_mode, dtype,
                                     hip.stream_ptr())
        torch.cuda.synchronize()
        return rc, (lib.x3d_last_error() or b"").decode()

    def edited(col, value, row=0, table="geom"):
        g, c = geom0.copy(), color0.copy()
        (g if table == "geom" else c)[row, col] = value
        return dict(geom=g, color=c)

    bad = {
        "rrc box below the frame": edited(G["BH"], 40),                    # 1 + 40 > 40
        "rrc box right of the frame": edited(G["X0"], 9),                  # 9 + 40 > 48
        "rrc box with a negative corner": edited(G["Y0"], -1),
        "empty rrc box": edited(G["BW"], 0),
        "jitter crop outside the resized frame": edited(G["Y0"], 5, row=1),   # resized 20 x 24, crop 16: y0 <= 4
        "jitter frame smaller than the crop": edited(G["NH"], 15, row=1),
        "erase box outside the crop": edited(G["EY1"], 17),
        "erase box reversed": edited(G["EX0"], 13),
        "start outside the video": edited(G["START"], 3),
        "unknown crop mode": edited(G["MODE"], 2),
        "non-finite colour": edited(hip.AUG_C_K, float("nan"), table="color"),
        "N = 0": dict(n=0),
        "N < 0": dict(n=-1),
        "null videos": dict(null="videos"),
        "null geom": dict(null="geom"),
        "null color": dict(null="color"),
        "null host_geom": dict(null="host_geom"),
        "null host_color": dict(null="host_color"),
        "unknown erase mode": dict(erase_mode=2),
        "unknown dtype": dict(dtype=9),
    }
    for what, kw in bad.items():
        rc, msg = call(**kw)
        assert rc != 0 and "train_clips_aug" in msg, what
        assert bool((out == -7.0).all()), what                     # nothing was launched
    rc, _ = call()
    assert rc == 0 and bool((out != -7.0).all())
    # the Python wrapper raises with the library's message
    with pytest.raises(hip.X3DHipError, match="outside"):
        views.make_train_batch_aug(vids, cfg, params_list=[good[0]._replace(box=(1, 2, 40, 40)), good[1]])
    with pytest.raises(ValueError):
        views.make_train_batch_aug(vids, cfg, params_list=good[:1])
    with pytest.raises(ValueError):
        views.make_train_batch_aug([], cfg)


# ---- 7. end to end -------------------------------------------------------------------------------------------------
CLASSES = 10
E2E = ["DATA.TEMP_DURATION", 4, "DATA.TRAIN_CROP_SIZE", 32, "DATA.TRAIN_JITTER_SCALES", [34, 40], "DATA.FRAME_RATE", 2,
       "NETWORK.NUM_CLASSES", CLASSES, "TRAIN.BATCH_SIZE", 2, "TRAIN.DATASET_SIZE", 4, "TRAIN.EPOCHS", 1]
AUG_ON = ["AUG.ENABLE", True, "AUG.CROP", "rrc", "AUG.RE_PROB", 0.7, "AUG.GRAYSCALE_PROB", 0.3]


def _smooth_video(h, w, f, seed):
    rng = np.random.default_rng(seed)
    yy, xx = np.mgrid[0:h, 0:w]
    base = np.sin(yy / 5.0 + seed)[..., None] * 60 + np.cos(xx[..., None] / 7.0 + np.arange(3)) * 60 + 128
    return np.stack([np.clip(base + 9 * t + rng.normal(0, 6, base.shape), 0, 255) for t in range(f)]).astype(np.uint8)


def _write(dirpath, n, seed):
    """n videos of 5-19 frames in three sizes, video i labelled i: a batch's labels name its videos.  Returns the pattern and
    the videos as the host decoder sees them."""
    os.makedirs(dirpath, exist_ok=True)
    rng = np.random.default_rng(seed)
    recs, decoded = [], []
    for i in range(n):
        h, w = [(41, 50), (40, 48), (37, 61)][i % 3]
        jpegs = [DL.encode_jpeg(f) for f in _smooth_video(h, w, int(rng.integers(5, 20)), seed * 100 + i)]
        decoded.append(np.stack([DL.decode_jpeg(j) for j in jpegs]))
        recs.append(DL.make_sequence_example(None, i, encoded=jpegs))
    for k in range(0, n, 3):
        DL.write_tfrecords(os.path.join(dirpath, f"part-{k // 3}.tfrecord"), recs[k:k + 3])
    return os.path.join(dirpath, "part-*.tfrecord"), decoded


@pytest.mark.gpu
@pytest.mark.parametrize("crop", ["rrc", "jitter"])
def test_reader_modes_agree_and_batches_replay_from_the_params(gpu, tmp_path, crop):
    cfg = x.get_config("XS", E2E + AUG_ON + ["AUG.CROP", crop])
    pattern, decoded = _write(str(tmp_path / "train"), 7, seed=3)
    kw = dict(device=gpu, seed=11, mixed_precision=True, dtype=torch.bfloat16)
    rh = DL.InputReader(cfg, True, True, **kw)
    rd = DL.InputReader(cfg, True, True, jpeg_decode="device", **kw)
    ih, idv = rh(pattern, 2), rd(pattern, 2)
    seen = []
    try:
        for step, ((ch, lh), (cd, ld)) in enumerate(zip(ih, idv)):
            assert ch.dtype == torch.bfloat16 and tuple(ch.shape) == (2, 4, 32, 32, 3)
            assert torch.equal(ch, cd) and torch.equal(lh, ld), step
            params = rh.last_params
            assert params == rd.last_params and all(isinstance(p, aug.AugParams) and p.crop == crop for p in params)
            vids = [torch.from_numpy(decoded[int(i)]).to(gpu) for i in lh.tolist()]
            replay = views.make_train_batch_aug(vids, cfg, params_list=params, dtype=torch.bfloat16)
            torch.cuda.synchronize()
            assert torch.equal(replay, ch), step
            seen += params
            if step == 7:                                      # more than one pass over the 7 videos
                break
    finally:
        ih.close()
        idv.close()
    assert len(seen) == 16 and len(set(seen)) == 16
    assert {p.flip for p in seen} == {False, True} and any(p.erase != aug.NO_ERASE for p in seen)
    # the same seed repeats the draws
    r2 = DL.InputReader(cfg, True, True, **kw)
    it = r2(pattern, 2)
    next(it)
    assert r2.last_params == seen[:2]
    it.close()


@pytest.mark.gpu
def test_reader_without_aug_is_the_per_clip_path(gpu, tmp_path):
    cfg_off = x.get_config("XS", E2E)
    cfg_flag = x.get_config("XS", E2E + ["AUG.ENABLE", False, "AUG.CROP", "rrc", "AUG.FLIP_PROB", 0.1])
    pattern, decoded = _write(str(tmp_path / "train"), 7, seed=5)
    for mode in ("host", "device"):
        batches = []
        for cfg in (cfg_off, cfg_flag):
            r = DL.InputReader(cfg, True, True, device=gpu, seed=4, jpeg_decode=mode)
            it = r(pattern, 2)
            for step, (clips, labels) in enumerate(it):
                params = r.last_params
                assert all(isinstance(p, dict) and p["flip"] is True for p in params)
                for k, (i, p) in enumerate(zip(labels.tolist(), params)):
                    want = views.make_train_clip(torch.from_numpy(decoded[int(i)]).to(gpu), cfg, params=p)
                    torch.cuda.synchronize()
                    assert torch.equal(clips[k], want)
                batches.append((clips.clone(), labels.clone(), params))
                if step == 4:
                    break
            it.close()
        for (c0, l0, p0), (c1, l1, p1) in zip(batches[:5], batches[5:]):      # the other AUG keys are inert
            assert torch.equal(c0, c1) and torch.equal(l0, l1) and p0 == p1


@pytest.mark.gpu
def test_trainer_steps_with_aug_and_mixup(gpu, tmp_path):
    from x3d_tf_amd.model import X3D
    from x3d_tf_amd.train import Trainer
    cfg = x.get_config("XS", E2E + AUG_ON + ["MIXUP.ENABLE", True])
    pattern, _ = _write(str(tmp_path / "train"), 4, seed=9)
    m = X3D(cfg, dtype=torch.float32, device=gpu, seed=1)
    tr = Trainer(m, cfg, mix_seed=2)
    it = DL.InputReader(cfg, True, True, device=gpu, seed=3, jpeg_decode="device")(pattern, cfg.TRAIN.BATCH_SIZE)
    losses = []
    for step, (clips, labels) in enumerate(it):
        pl = tr.step(clips, labels, 0.01)
        torch.cuda.synchronize()
        losses.append(pl.loss_rows.float().cpu())
        if step == 2:
            break
    it.close()
    assert len(losses) == 3 and all(bool(torch.isfinite(l).all()) for l in losses)
