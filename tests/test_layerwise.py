"""The layer-wise optimizers on the host: the OPTIM.* config section, the additive C ABI, the chunk-table builder (property
test) and the argument checks of the new entry points, which refuse before any launch and so need no device (the kernels and
the trainer are held to fp64 references in test_layerwise_gpu.py)."""
import os
import re
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import x3d_tf_amd as x  # noqa: E402
from x3d_tf_amd import hip  # noqa: E402
from x3d_tf_amd.config import optim_settings  # noqa: E402
from x3d_tf_amd.segments import SegTable, Segment, build_chunk_table  # noqa: E402

NEW_SYMBOLS = ("x3d_seg_sumsq", "x3d_lars", "x3d_adamw", "x3d_lamb")
DEFAULTS = dict(LARS_TRUST_COEF=0.001, LARS_EPS=1e-8, LARS_CLIP=False, WEIGHT_DECAY=0.0, LAMB_EPS=1e-6)


# ---- config -----------------------------------------------------------------------------------------------------------
def test_config_defaults_and_overrides():
    assert dict(x.get_default_config().OPTIM) == DEFAULTS
    s = optim_settings(x.get_config("M"))
    assert s == (0.001, 1e-8, False, 0.0, 1e-6)
    assert (s.lars_trust_coef, s.lars_eps, s.lars_clip, s.weight_decay, s.lamb_eps) == (0.001, 1e-8, False, 0.0, 1e-6)
    c = x.get_config("M", ["OPTIM.LARS_TRUST_COEF", 0.02, "OPTIM.LARS_EPS", 0.0, "OPTIM.LARS_CLIP", True,
                           "OPTIM.WEIGHT_DECAY", 0.05, "OPTIM.LAMB_EPS", 1e-8, "TRAIN.OPTIMIZER", "LAMB"])
    assert optim_settings(c) == (0.02, 0.0, True, 0.05, 1e-8)


def test_config_without_the_section_takes_the_defaults_and_other_sections_are_unchanged():
    m = x.get_config("M")
    old = m.clone()
    old.defrost()
    del old["OPTIM"]
    assert optim_settings(old) == optim_settings(m) == tuple(DEFAULTS.values())
    assert set(m) == set(old) | {"OPTIM"}
    assert set(m.SOLVER) == {"CLIP_GRAD_L2NORM", "ACCUM_STEPS", "EMA_DECAY", "EMA_EVAL"}
    assert set(m.TRAIN) == {"DATASET_SIZE", "BATCH_SIZE", "EPOCHS", "OPTIMIZER", "MOMENTUM", "BASE_LR", "WARMUP_EPOCHS",
                            "WARMUP_LR", "LABEL_SMOOTHING"}
    from x3d_tf_amd.config import SolverSettings
    assert SolverSettings._fields == ("clip_grad_l2norm", "accum_steps", "ema_decay", "ema_eval")


@pytest.mark.parametrize("over", [
    ["OPTIM.LARS_TRUST_COEF", 0.0], ["OPTIM.LARS_TRUST_COEF", -0.001], ["OPTIM.LARS_TRUST_COEF", float("inf")],
    ["OPTIM.LARS_TRUST_COEF", float("nan")],
    ["OPTIM.LARS_EPS", -1e-8], ["OPTIM.LARS_EPS", float("nan")],
    ["OPTIM.WEIGHT_DECAY", -0.01], ["OPTIM.WEIGHT_DECAY", float("inf")], ["OPTIM.WEIGHT_DECAY", float("nan")],
    ["OPTIM.LAMB_EPS", 0.0], ["OPTIM.LAMB_EPS", -1e-6], ["OPTIM.LAMB_EPS", float("nan")],
])
def test_config_rejects(over):
    with pytest.raises(ValueError, match=over[0]):
        x.get_config("M", over)


def test_optimizer_names():
    """the five names, case-insensitive; anything else is NotImplementedError before the trainer touches the model"""
    from x3d_tf_amd.config import OPTIMIZERS, SLOT_KIND
    from x3d_tf_amd.train import Trainer
    assert OPTIMIZERS == ("sgd", "adam", "lars", "adamw", "lamb")
    assert SLOT_KIND == dict(sgd="sgd", lars="sgd", adam="adam", adamw="adam", lamb="adam")
    with pytest.raises(NotImplementedError, match="rmsprop"):
        Trainer(None, x.get_config("XS", ["TRAIN.OPTIMIZER", "rmsprop"]))
    for name in ("LARS", "AdamW", "lamb"):      # accepted: the constructor gets past the check and trips over the missing model
        with pytest.raises(AttributeError):
            Trainer(None, x.get_config("XS", ["TRAIN.OPTIMIZER", name]))


# ---- ABI --------------------------------------------------------------------------------------------------------------
def test_abi_is_additive_and_the_new_symbols_are_declared_exported_and_typed():
    assert hip.ABI_VERSION == 138
    lib = hip.load()
    assert lib.x3d_version() == 138
    declared = hip.exported_symbols()
    header = open(os.path.join(ROOT, "include", "x3d_hip.h")).read()
    assert len(re.findall(r"typedef struct", re.sub(r"/\*.*?\*/", "", header, flags=re.S))) == 16     # no new struct
    assert hip.SEG_CHUNK == 1024 and hip.SEG_CHUNK % 4 == 0
    from ctypes import c_float as f, c_int as i, c_longlong as ll, c_void_p as vp
    sigs = {
        "x3d_seg_sumsq": ([vp, vp, i, vp, i, vp, vp, vp], i),
        "x3d_lars": ([vp, vp, vp, vp, i, vp, i, f, f, f, f, f, f, i, vp, f, vp, f, vp, vp, vp], i),
        "x3d_adamw": ([vp, vp, vp, vp, vp, i, vp, i, f, f, f, f, f, f, ll, vp, f, vp, f, vp], i),
        "x3d_lamb": ([vp, vp, vp, vp, vp, i, vp, i, f, f, f, f, f, f, ll, vp, f, vp, f, vp, vp, vp], i),
    }
    assert set(sigs) == set(NEW_SYMBOLS)
    for name, (argtypes, restype) in sigs.items():
        assert name in declared, name
        fn = getattr(lib, name)
        assert (list(fn.argtypes), fn.restype) == (argtypes, restype), name


def test_argument_checks_need_no_gpu():
    """bad arguments are refused with X3D_ERR_INVALID before any launch (so also without a device)"""
    lib = hip.load()
    a = 4096                                   # any aligned non-null address: nothing is dereferenced on the refused paths
    odd, odd8 = a + 2, a + 4                   # not 4-byte / not 8-byte aligned

    def lars(w=a, v=a, g=a, ch=a, nch=4, sg=a, nsg=2, lr=.1, mom=.9, wd=5e-5, gs=1., eta=1e-3, eps=1e-8, clip=0, norm=None,
             mx=0., ema=None, dec=0., part=a, q=a):
        return ("x3d_lars", (w, v, g, ch, nch, sg, nsg, lr, mom, wd, gs, eta, eps, clip, norm, mx, ema, dec, part, q))

    def adamw(w=a, m=a, v=a, g=a, ch=a, nch=4, sg=a, nsg=2, lr=.1, b1=.9, b2=.999, eps=1e-7, decay=0., gs=1., step=1,
              norm=None, mx=0., ema=None, dec=0.):
        return ("x3d_adamw", (w, m, v, g, ch, nch, sg, nsg, lr, b1, b2, eps, decay, gs, step, norm, mx, ema, dec))

    def lamb(w=a, m=a, v=a, g=a, ch=a, nch=4, sg=a, nsg=2, lr=.1, b1=.9, b2=.999, eps=1e-6, decay=0., gs=1., step=1,
             norm=None, mx=0., ema=None, dec=0., part=a, q=a):
        return ("x3d_lamb", (w, m, v, g, ch, nch, sg, nsg, lr, b1, b2, eps, decay, gs, step, norm, mx, ema, dec, part, q))

    def sumsq(x_=a, ch=a, nch=4, sg=a, nsg=2, part=a, out=a):
        return ("x3d_seg_sumsq", (x_, ch, nch, sg, nsg, part, out))

    inf, nan = float("inf"), float("nan")
    bad = [
        sumsq(x_=None), sumsq(ch=None), sumsq(sg=None), sumsq(part=None), sumsq(out=None), sumsq(nsg=0), sumsq(nsg=-1),
        sumsq(nch=0), sumsq(part=odd8), sumsq(out=odd8), sumsq(x_=odd),
        lars(w=None), lars(v=None), lars(g=None), lars(ch=None), lars(sg=None), lars(part=None), lars(q=None), lars(nsg=0),
        lars(nch=0), lars(eta=0.), lars(eta=-1e-3), lars(eta=inf), lars(eta=nan), lars(eps=-1e-8), lars(eps=nan),
        lars(part=odd8), lars(norm=odd8, mx=1.), lars(norm=a, mx=0.), lars(norm=a, mx=-1.), lars(ema=a, dec=1.0), lars(w=odd),
        adamw(w=None), adamw(m=None), adamw(v=None), adamw(g=None), adamw(ch=None), adamw(sg=None), adamw(nsg=0),
        adamw(decay=-0.1), adamw(decay=inf), adamw(decay=nan), adamw(step=0), adamw(norm=odd8, mx=1.), adamw(norm=a, mx=0.),
        adamw(ema=a, dec=-0.1),
        lamb(w=None), lamb(m=None), lamb(v=None), lamb(g=None), lamb(ch=None), lamb(sg=None), lamb(part=None), lamb(q=None),
        lamb(nsg=0), lamb(decay=-0.1), lamb(decay=nan), lamb(eps=0.), lamb(eps=-1e-6), lamb(eps=nan), lamb(step=0),
        lamb(part=odd8), lamb(norm=odd8, mx=1.), lamb(norm=a, mx=0.), lamb(ema=a, dec=1.5),
    ]
    for name, args in bad:
        assert getattr(lib, name)(*args, None) == 1, (name, args)      # X3D_ERR_INVALID
        assert lib.x3d_last_error()


# ---- the chunk table ---------------------------------------------------------------------------------------------------
def _check_table(segments, chunk):
    """every element of every segment in exactly one chunk; no chunk leaves its segment; padding in none; the layout the
    kernels rely on (vector-aligned starts, a segment's chunks adjacent and ascending, counts in [1, chunk])"""
    chunks, segs = build_chunk_table(segments, chunk)
    assert chunks.dtype == np.int32 and segs.dtype == np.int32 and chunks.shape[1] == 3 and segs.shape == (len(segments), 3)
    total = max(o + n for o, n, _ in segments) + 8
    cover = np.zeros(total, np.int64)
    owner = np.full(total, -1, np.int64)
    for t, (o, n, _) in enumerate(segments):
        owner[o:o + n] = t
    for seg, first, cnt in chunks:
        assert 1 <= cnt <= chunk and first % 4 == 0
        o, n, _ = segments[seg]
        assert o <= first and first + cnt <= o + n                              # inside its segment
        assert cnt == chunk or first + cnt == o + n                             # short only where the segment ends
        cover[first:first + cnt] += 1
    assert np.array_equal(cover, (owner >= 0).astype(np.int64))                 # exact cover; padding never covered
    at = 0
    for t, (c0, nc, l2) in enumerate(segs):
        assert c0 == at and nc == -(-segments[t][1] // chunk) and l2 == int(bool(segments[t][2]))
        mine = chunks[c0:c0 + nc]
        assert np.all(mine[:, 0] == t) and np.all(np.diff(mine[:, 1]) == chunk)
        assert mine[0, 1] == segments[t][0]
        at += nc
    assert at == len(chunks)
    return chunks, segs


def _random_segments(rng, chunk, must):
    lengths = list(must) + [int(v) for v in rng.integers(1, 3 * chunk + 7, size=rng.integers(1, 12))]
    rng.shuffle(lengths)
    segments, off = [], int(rng.integers(0, 3)) * 4
    for n in lengths:
        segments.append((off, n, bool(rng.integers(0, 2))))
        off += (n + 3) // 4 * 4 + int(rng.integers(0, 3)) * 4                   # the model's padding, sometimes more
    return segments


@pytest.mark.parametrize("chunk", [4, 8, 64, 1024])
def test_chunk_table_properties(chunk):
    rng = np.random.default_rng(chunk)
    must = [1, 3, 4, 5, max(chunk - 1, 1), chunk, chunk + 1, 2 * chunk, 2 * chunk + 3]
    for _ in range(25):
        _check_table(_random_segments(rng, chunk, must), chunk)
    chunks, segs = _check_table([(0, 1, True)], chunk)
    assert chunks.tolist() == [[0, 0, 1]] and segs.tolist() == [[0, 1, 1]]


def test_chunk_table_default_chunk_and_segtable():
    tb = SegTable([Segment("a", 0, 1025, True), Segment("b", 1028, 3, False)])
    assert tb.chunks.tolist() == [[0, 0, 1024], [0, 1024, 1], [1, 1028, 3]] and tb.segs.tolist() == [[0, 2, 1], [2, 1, 0]]
    assert (tb.nchunk, tb.nseg, tb.end) == (3, 2, 1031) and tb.d_chunks is None


@pytest.mark.parametrize("segments,chunk", [
    ([], 8), ([(0, 0, True)], 8), ([(2, 5, True)], 8), ([(-4, 5, True)], 8), ([(0, 9, True), (8, 4, False)], 8),
    ([(16, 4, True), (0, 4, False)], 8), ([(0, 4, True)], 6), ([(0, 4, True)], 0), ([(0, 2 ** 31, True)], 1024),
])
def test_chunk_table_rejects(segments, chunk):
    with pytest.raises(ValueError):
        build_chunk_table(segments, chunk)


def test_model_segments_cover_the_trainable_tensors():
    """a dry model (no device): `segments` = the trainable tensors in param_order with the l2 flag of their spec, and its
    chunk table covers exactly the l2 mask's support where l2 is set"""
    from x3d_tf_amd.model import X3D
    m = X3D(x.get_config("XS", ["NETWORK.NUM_CLASSES", 11]), device="dry")
    names = [k for k in m.param_order if m.specs[k].trainable]
    assert [s.name for s in m.segments] == names
    assert all(s.offset == m._offsets[s.name] and s.length == m.params[s.name].numel() and s.l2 == bool(m.specs[s.name].l2)
               for s in m.segments)
    chunks, segs = _check_table([(s.offset, s.length, s.l2) for s in m.segments], hip.SEG_CHUNK)
    l2 = np.zeros(m.n_trainable_flat, np.uint8)
    for seg, first, cnt in chunks:
        if segs[seg, 2]:
            l2[first:first + cnt] = 1
    assert np.array_equal(l2, m.l2_mask.numpy())
