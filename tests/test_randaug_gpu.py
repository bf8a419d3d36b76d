"""x3d_randaug_clips on the GPU: every op against the NumPy restatement (tests/randaug_ref.py, itself checked against Pillow in
tests/test_randaug.py) bit for bit, chains, edge frames, the batched training path, InputReader, and the refusals."""
import os

import numpy as np
import pytest
import torch

import x3d_tf_amd as x
from x3d_tf_amd import aug, hip, ops, views
from x3d_tf_amd import dataloader as DL

from tests import randaug_ref as R

Op = aug.RandAugOp
NONE = aug.RANDAUG_NONE
FILL = (115, 102, 128)
# F=5 17x23, F=3 40x56, F=2 33x18: rows of 69, 168 and 54 bytes; T = 4, rate = 2: the looping sampler wraps in all three
SHAPES = [(5, 17, 23), (3, 40, 56), (2, 33, 18)]
STARTS = [3, 1, 1]
T, RATE = 4, 2


def _videos(shapes=SHAPES, seed=0):
    return [np.random.default_rng(seed + i).integers(0, 256, s + (3,), dtype=np.uint8) for i, s in enumerate(shapes)]


VIDEOS = _videos()


def _run(gpu, videos, ra, t=T, rate=RATE, starts=STARTS, fill=FILL):
    dev = [torch.from_numpy(v).to(gpu) for v in videos]
    got = ops.randaug_clips(dev, ra, t, rate, starts, fill)
    torch.cuda.synchronize()
    return [g.cpu().numpy() for g in got]


def _want(videos, ra, t=T, rate=RATE, starts=STARTS, fill=FILL):
    return [R.apply_clip(v, o, t, rate, s, fill) for v, o, s in zip(videos, ra, starts)]


def _px(op, h, w):
    """Translate ops carry pixels: the stated fraction of this clip's frame"""
    if op.name == "TranslateXRel":
        return Op(op.name, op.arg * w)
    if op.name == "TranslateYRel":
        return Op(op.name, op.arg * h)
    return op


# every op at two arguments
ALONE = [Op("AutoContrast", None), Op("Equalize", None), Op("Invert", None), Op("Rotate", 21.0), Op("Rotate", -30.0),
         Op("Posterize", 2), Op("Posterize", 0), Op("Solarize", 77), Op("Solarize", 256), Op("SolarizeAdd", 55),
         Op("SolarizeAdd", 110), Op("Color", 0.1), Op("Color", 1.9), Op("Contrast", 0.55), Op("Contrast", 1.45),
         Op("Brightness", 0.1), Op("Brightness", 1.63), Op("Sharpness", 0.1), Op("Sharpness", 1.9), Op("ShearX", 0.21),
         Op("ShearX", -0.3), Op("ShearY", 0.3), Op("ShearY", -0.13), Op("TranslateXRel", 0.315), Op("TranslateXRel", -0.2),
         Op("TranslateYRel", 0.45), Op("TranslateYRel", -0.1), Op("Posterize", 8), Op("Solarize", 0), Op("Invert", None)]


@pytest.mark.gpu
def test_every_op_alone_mixed_within_the_layer(gpu):
    """30 one-layer batches: in batch k the three clips take ops k, k + 1, k + 2 of ALONE (cyclically), so every op meets
    every clip extent and every launch holds mixed ops"""
    assert {o.name for o in ALONE} == set(aug.RANDAUG_OPS)
    for k in range(len(ALONE)):
        ra = [(_px(ALONE[(k + i) % len(ALONE)], h, w),) for i, (_, h, w) in enumerate(SHAPES)]
        got = _run(gpu, VIDEOS, ra)
        for i, (g, w_) in enumerate(zip(got, _want(VIDEOS, ra))):
            assert g.shape == w_.shape and g.dtype == np.uint8
            np.testing.assert_array_equal(g, w_, err_msg=f"batch {k} clip {i}: {ra[i]}")
        again = _run(gpu, VIDEOS, ra)
        assert all(np.array_equal(a, b) for a, b in zip(got, again)), k          # the same bits on a second run


@pytest.mark.gpu
def test_three_layer_chain(gpu):
    h1, w1 = SHAPES[1][1:]
    ra = [(Op("Equalize", None), NONE, Op("Contrast", 1.45)),                    # two statistics ops in different layers
          (Op("Rotate", 12.5), Op("AutoContrast", None), Op("Sharpness", 1.7)),
          (NONE, Op("Color", 0.4), Op("TranslateXRel", 0.2 * SHAPES[2][2]))]
    got = _run(gpu, VIDEOS, ra)
    for i, (g, w_) in enumerate(zip(got, _want(VIDEOS, ra))):
        np.testing.assert_array_equal(g, w_, err_msg=f"clip {i}")
    # op tuples of different lengths, a clip with no applied op (copied by the gather), four layers of ping-pong
    ra = [(NONE, NONE), (Op("Invert", None), Op("ShearY", 0.2), Op("Solarize", 100), Op("Equalize", None)), ()]
    got = _run(gpu, VIDEOS, ra)
    for i, (g, w_) in enumerate(zip(got, _want(VIDEOS, ra))):
        np.testing.assert_array_equal(g, w_, err_msg=f"clip {i}")
    assert h1 * w1 * 3 % 16 == 0 and SHAPES[0][1] * SHAPES[0][2] * 3 % 16 != 0     # aligned and unaligned frame strides


@pytest.mark.gpu
def test_larger_than_one_workgroup_and_untouched_clip(gpu):
    """80 x 70 = 5600 pixels: two chunks per frame, the second partial; a clip whose video already is its T frames and that no
    layer touches comes back as the very tensor that went in"""
    vids = _videos([(4, 80, 70), (4, 9, 7)], seed=20)
    dev = [torch.from_numpy(v).to(gpu) for v in vids]
    for op in (Op("Equalize", None), Op("Color", 1.3), Op("Sharpness", 0.3), Op("Rotate", -17.0), Op("AutoContrast", None),
               Op("Contrast", 0.2)):
        got = ops.randaug_clips(dev, [(op,), (NONE,)], 4, 1, [0, 0], FILL)
        torch.cuda.synchronize()
        np.testing.assert_array_equal(got[0].cpu().numpy(), R.apply_clip(vids[0], (op,), 4, 1, 0, FILL), err_msg=str(op))
        assert got[1] is dev[1]
    got = ops.randaug_clips(dev, [(NONE,), (NONE,)], 4, 1, [0, 1], FILL)           # start 1: the gather copies
    torch.cuda.synchronize()
    assert got[0] is dev[0] and got[1] is not dev[1]
    np.testing.assert_array_equal(got[1].cpu().numpy(), vids[1][[1, 2, 3, 0]])


@pytest.mark.gpu
def test_edge_frames(gpu):
    rng = np.random.default_rng(5)
    v1, v2 = rng.integers(0, 256, (2, 1, 1, 3), dtype=np.uint8), rng.integers(0, 256, (2, 2, 2, 3), dtype=np.uint8)
    vc = rng.integers(0, 256, (2, 17, 23, 3), dtype=np.uint8)
    vc[..., 1] = 77                                             # a constant channel: hi <= lo, a single bin
    vids, starts = [v1, v2, vc], [0, 1, 0]
    every = [Op("Sharpness", 1.9), Op("AutoContrast", None), Op("Equalize", None), Op("Contrast", 0.3), Op("Color", 1.7),
             Op("Rotate", 30.0), Op("ShearX", 0.3), Op("Invert", None)]
    for op in every:
        ra = [(op,)] * 3
        got = _run(gpu, vids, ra, t=2, rate=1, starts=starts)
        for i, (g, w_) in enumerate(zip(got, _want(vids, ra, t=2, rate=1, starts=starts))):
            np.testing.assert_array_equal(g, w_, err_msg=f"{op} clip {i}")
    sharp = _run(gpu, vids, [(Op("Sharpness", 1.9),)] * 3, t=2, rate=1, starts=starts)
    np.testing.assert_array_equal(sharp[0], v1)                 # all border
    np.testing.assert_array_equal(sharp[1], v2[[1, 0]])
    for op in (Op("Rotate", 0.0), Op("TranslateXRel", 0.0), Op("TranslateYRel", 0.0)):
        got = _run(gpu, VIDEOS, [(op,)] * 3)
        for g, v, s in zip(got, VIDEOS, STARTS):
            np.testing.assert_array_equal(g, v[[(s + j * RATE) % v.shape[0] for j in range(T)]], err_msg=str(op))


# ---- the batched training path -----------------------------------------------------------------------------------------
MEAN, STD = [0.45, 0.40, 0.50], [0.225, 0.25, 0.2]


def _cfg(*over):
    return x.get_config("XS", ["DATA.TEMP_DURATION", T, "DATA.TRAIN_CROP_SIZE", 16, "DATA.FRAME_RATE", RATE, "DATA.MEAN", MEAN,
                               "DATA.STD", STD, "DATA.TRAIN_JITTER_SCALES", [18, 22], "AUG.ENABLE", True] + list(over))


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["fp32", "bf16"])
def test_make_train_batch_aug_with_randaug(gpu, dtype):
    cfg = _cfg("AUG.CROP", "rrc")
    assert views.randaug_fill(cfg) == (115, 102, 128)
    dev = [torch.from_numpy(v).to(gpu) for v in VIDEOS]
    rng = np.random.default_rng(3)
    params = [aug.draw_aug_params(cfg, f, h, w, rng)._replace(start=s) for (f, h, w), s in zip(SHAPES, STARTS)]
    ra = [(Op("Equalize", None), Op("Rotate", -14.0)), (NONE, Op("Sharpness", 1.6)), (Op("Posterize", 3), NONE)]
    got = views.make_train_batch_aug(dev, cfg, params_list=params, dtype=dtype, randaug_list=ra)
    # x3d_train_clips_aug on the restatement's frames: videos of T frames, start 0, rate 1
    frames = [torch.from_numpy(w_).to(gpu) for w_ in _want(VIDEOS, ra)]
    want = views.make_train_batch_aug(frames, cfg, params_list=[p._replace(start=0) for p in params], dtype=dtype, rate=1)
    torch.cuda.synchronize()
    assert torch.equal(got, want)
    # all "none": the call without randaug_list
    plain = views.make_train_batch_aug(dev, cfg, params_list=params, dtype=dtype)
    none = views.make_train_batch_aug(dev, cfg, params_list=params, dtype=dtype, randaug_list=[(NONE, NONE)] * 3)
    torch.cuda.synchronize()
    assert torch.equal(plain, none) and not torch.equal(plain, got)
    # AA_TYPE in the config: drawn from rng after the AugParams
    cfg_aa = _cfg("AUG.CROP", "rrc", "AUG.AA_TYPE", "rand-m9-n3-p1")
    a = views.make_train_batch_aug(dev, cfg_aa, rng=np.random.default_rng(8), dtype=dtype)
    r = np.random.default_rng(8)
    p2 = [aug.draw_aug_params(cfg_aa, f, h, w, r) for f, h, w in SHAPES]
    ra2 = [aug.draw_randaug(x.config.randaug_settings(cfg_aa), h, w, r) for _, h, w in SHAPES]
    b = views.make_train_batch_aug(dev, cfg_aa, params_list=p2, dtype=dtype, randaug_list=ra2)
    torch.cuda.synchronize()
    assert torch.equal(a, b) and all(o.name != "none" for t_ in ra2 for o in t_)
    with pytest.raises(ValueError):
        views.make_train_batch_aug(dev, cfg, params_list=params, randaug_list=ra[:2])


# ---- InputReader -------------------------------------------------------------------------------------------------------
E2E = ["DATA.TEMP_DURATION", 4, "DATA.TRAIN_CROP_SIZE", 32, "DATA.TRAIN_JITTER_SCALES", [34, 40], "DATA.FRAME_RATE", 2,
       "NETWORK.NUM_CLASSES", 10, "TRAIN.BATCH_SIZE", 2, "TRAIN.DATASET_SIZE", 4, "TRAIN.EPOCHS", 1]
AUG_ON = ["AUG.ENABLE", True, "AUG.CROP", "rrc", "AUG.RE_PROB", 0.7]


def _smooth_video(h, w, f, seed):
    rng = np.random.default_rng(seed)
    yy, xx = np.mgrid[0:h, 0:w]
    base = np.sin(yy / 5.0 + seed)[..., None] * 60 + np.cos(xx[..., None] / 7.0 + np.arange(3)) * 60 + 128
    return np.stack([np.clip(base + 9 * t + rng.normal(0, 6, base.shape), 0, 255) for t in range(f)]).astype(np.uint8)


def _write(dirpath, n, seed):
    os.makedirs(dirpath, exist_ok=True)
    rng = np.random.default_rng(seed)
    recs, decoded = [], []
    for i in range(n):
        h, w = [(41, 50), (40, 48), (37, 61)][i % 3]
        jpegs = [DL.encode_jpeg(f) for f in _smooth_video(h, w, int(rng.integers(5, 12)), seed * 100 + i)]
        decoded.append(np.stack([DL.decode_jpeg(j) for j in jpegs]))
        recs.append(DL.make_sequence_example(None, i, encoded=jpegs))
    for k in range(0, n, 3):
        DL.write_tfrecords(os.path.join(dirpath, f"part-{k // 3}.tfrecord"), recs[k:k + 3])
    return os.path.join(dirpath, "part-*.tfrecord"), decoded


@pytest.mark.gpu
def test_reader_modes_agree_with_aa_type(gpu, tmp_path):
    cfg = x.get_config("XS", E2E + AUG_ON + ["AUG.AA_TYPE", "rand-m7-n3-mstd0.5-inc1"])
    pattern, decoded = _write(str(tmp_path / "train"), 5, seed=3)
    kw = dict(device=gpu, seed=11)
    rh = DL.InputReader(cfg, True, True, **kw)
    rd = DL.InputReader(cfg, True, True, jpeg_decode="device", **kw)
    ih, idv = rh(pattern, 2), rd(pattern, 2)
    seen = []
    try:
        for step, ((ch, lh), (cd, ld)) in enumerate(zip(ih, idv)):
            assert torch.equal(ch, cd) and torch.equal(lh, ld), step
            assert rh.last_params == rd.last_params and rh.last_randaug == rd.last_randaug
            ra = rh.last_randaug
            assert len(ra) == 2 and all(len(r) == 3 and all(isinstance(o, Op) for o in r) for r in ra)
            vids = [torch.from_numpy(decoded[int(i)]).to(gpu) for i in lh.tolist()]
            replay = views.make_train_batch_aug(vids, cfg, params_list=rh.last_params, randaug_list=ra)
            torch.cuda.synchronize()
            assert torch.equal(replay, ch), step
            seen += ra
            if step == 3:
                break
    finally:
        ih.close()
        idv.close()
    names = {o.name for r in seen for o in r}
    assert "none" in names and len(names) > 3
    # the RandAugment generator is its own: the AugParams are those of a reader without the policy
    r0 = DL.InputReader(x.get_config("XS", E2E + AUG_ON), True, True, **kw)
    r1 = DL.InputReader(cfg, True, True, **kw)
    i0, i1 = r0(pattern, 2), r1(pattern, 2)
    next(i0), next(i1)
    assert r0.last_params == r1.last_params and r0.last_randaug == [] and r1.last_randaug == seen[:2]
    i0.close()
    i1.close()


@pytest.mark.gpu
def test_reader_with_empty_aa_type_is_the_reader_without_the_key(gpu, tmp_path):
    cfg_new = x.get_config("XS", E2E + AUG_ON)
    assert cfg_new.AUG.AA_TYPE == ""
    cfg_old = x.get_config("XS", E2E + AUG_ON, freeze=False)
    del cfg_old["AUG"]["AA_TYPE"]
    cfg_old.freeze()
    pattern, _ = _write(str(tmp_path / "train"), 5, seed=6)
    for mode in ("host", "device"):
        out = []
        for cfg in (cfg_new, cfg_old):
            r = DL.InputReader(cfg, True, True, device=gpu, seed=4, jpeg_decode=mode)
            it = r(pattern, 2)
            for step, (clips, labels) in enumerate(it):
                out.append((clips.clone(), labels.clone(), r.last_params, r.last_randaug))
                if step == 2:
                    break
            it.close()
        for (c0, l0, p0, a0), (c1, l1, p1, a1) in zip(out[:3], out[3:]):
            assert torch.equal(c0, c1) and torch.equal(l0, l1) and p0 == p1 and a0 == a1 == []


# ---- refusals ----------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_refusals_launch_nothing(gpu):
    dev = [torch.from_numpy(v).to(gpu) for v in VIDEOS]
    ra = [(Op("Posterize", 3), Op("Rotate", 10.0)), (Op("Color", 1.2), Op("Equalize", None)), (NONE, Op("Invert", None))]
    clips0, ops0, xform0, work_bytes, _ = views.randaug_tables(SHAPES, STARTS, ra, T, RATE)
    lib = hip.load()
    work = torch.full((work_bytes,), 201, dtype=torch.uint8, device=gpu)
    scratch = torch.empty(int(lib.x3d_randaug_scratch(3, T)), dtype=torch.uint8, device=gpu)
    addrs = torch.tensor([v.data_ptr() for v in dev], dtype=torch.int64, device=gpu)

    def call(clips=clips0, ops_=ops0, xform=xform0, n=3, t=T, rate=RATE, layers=2, null=None, wb=work_bytes, fill=FILL):
        dc, do, dx = torch.from_numpy(clips).to(gpu), torch.from_numpy(ops_).to(gpu), torch.from_numpy(xform).to(gpu)
        a = dict(videos=addrs.data_ptr(), clips=dc.data_ptr(), ops=do.data_ptr(), xform=dx.data_ptr(), host_clips=clips.ctypes.data,
                 host_ops=ops_.ctypes.data, host_xform=xform.ctypes.data, work=work.data_ptr(), scratch=scratch.data_ptr())
        if null:
            a[null] = None
        rc = lib.x3d_randaug_clips(a["videos"], a["clips"], a["ops"], a["xform"], a["host_clips"], a["host_ops"], a["host_xform"],
                                   a["work"], wb, a["scratch"], n, t, rate, layers, fill[0], fill[1], fill[2], hip.stream_ptr())
        torch.cuda.synchronize()
        return rc, (lib.x3d_last_error() or b"").decode()

    def edited(table, index, value):
        c, o, xf = clips0.copy(), ops0.copy(), xform0.copy()
        dict(clips=c, ops=o, xform=xf)[table][index] = value
        return dict(clips=c, ops_=o, xform=xf)

    size0 = T * 17 * 23 * 3
    nan = int(np.array([np.nan], np.float32).view(np.int32)[0])
    inf = int(np.array([np.inf], np.float32).view(np.int32)[0])
    bad = {
        "null videos": dict(null="videos"), "null clips": dict(null="clips"), "null ops": dict(null="ops"),
        "null xform": dict(null="xform"), "null host_clips": dict(null="host_clips"), "null host_ops": dict(null="host_ops"),
        "null host_xform": dict(null="host_xform"), "null work": dict(null="work"), "null scratch": dict(null="scratch"),
        "N = 0": dict(n=0), "N < 0": dict(n=-2),
        "T = 0": dict(t=0), "rate = 0": dict(rate=0), "layers = 0": dict(layers=0),
        "F = 0": edited("clips", (0, 0), 0), "H < 0": edited("clips", (1, 1), -4), "W = 0": edited("clips", (2, 2), 0),
        "start = F": edited("clips", (0, 3), 5), "start < 0": edited("clips", (1, 3), -1),
        "unknown op": edited("ops", (0, 0, hip.RA_O_OP), 17), "negative op": edited("ops", (2, 1, hip.RA_O_OP), -1),
        "NaN factor": edited("ops", (1, 0, hip.RA_O_FARG), nan), "infinite factor": edited("ops", (1, 0, hip.RA_O_FARG), inf),
        "posterize bits 9": edited("ops", (0, 0, hip.RA_O_IARG), 9), "posterize bits -1": edited("ops", (0, 0, hip.RA_O_IARG), -1),
        "destination past the work area": edited("xform", (0, 1, hip.RA_X_DST), work_bytes - size0 + 1),
        "negative destination": edited("xform", (0, 0, hip.RA_X_DST), -16),
        "source past the work area": edited("xform", (0, 1, hip.RA_X_SRC), work_bytes - size0 + 1),
        "source below -1": edited("xform", (0, 1, hip.RA_X_SRC), -2),
        "work area too small": dict(wb=work_bytes - 16),
        "source and destination overlap": edited("xform", (0, 1, hip.RA_X_DST), int(xform0[0, 1, hip.RA_X_SRC]) + size0 - 1),
        "in place": edited("xform", (0, 1, hip.RA_X_DST), int(xform0[0, 1, hip.RA_X_SRC])),
        "fill colour 256": dict(fill=(0, 256, 0)),
    }
    for what, kw in bad.items():
        rc, msg = call(**kw)
        assert rc == 1 and "randaug_clips" in msg, what         # X3D_ERR_INVALID
        assert bool((work == 201).all()), what                   # nothing was launched
    rc, _ = call()
    assert rc == 0 and not bool((work == 201).all())
    # the Python wrapper raises with the library's message
    with pytest.raises(hip.X3DHipError, match="posterize bits"):
        ops.randaug_clips(dev, [(Op("Posterize", 12),), (NONE,), (NONE,)], T, RATE, STARTS, FILL)
    with pytest.raises(hip.X3DHipError, match="not finite"):
        ops.randaug_clips(dev, [(Op("Color", float("inf")),), (NONE,), (NONE,)], T, RATE, STARTS, FILL)
    with pytest.raises(ValueError):
        ops.randaug_clips(dev, [(NONE,)], T, RATE, STARTS, FILL)
    with pytest.raises(ValueError):
        ops.randaug_clips([], [], T)
