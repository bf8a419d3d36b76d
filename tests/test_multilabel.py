"""Multi-label (Charades-style) training on the host: the config switches, multi-label SequenceExamples and text lines,
and the fp64 average-precision reference the GPU tests (test_multilabel_gpu.py) hold x3d_multilabel_ap to."""
import math
import os
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import x3d_tf_amd as x  # noqa: E402
from x3d_tf_amd import dataloader as DL  # noqa: E402


def ap_ref(scores, targets):
    """sklearn.metrics.average_precision_score restated in fp64 NumPy for one class: sum over the distinct thresholds
    (descending) of (recall step) * precision.  A target >= 0.5 is a positive; no positive or a NaN score -> NaN."""
    s = np.asarray(scores, dtype=np.float64).ravel()
    y = np.asarray(targets, dtype=np.float64).ravel() >= 0.5
    p = int(y.sum())
    if p == 0 or np.isnan(s).any():
        return float("nan")
    order = np.argsort(-s, kind="mergesort")
    s, y = s[order], y[order]
    last = np.r_[np.nonzero(np.diff(s))[0], len(s) - 1]     # last index of every threshold (-0 == +0: diff is 0)
    tps = np.cumsum(y)[last].astype(np.float64)
    prec = tps / (last + 1)
    rec = tps / p
    return float(np.sum(np.diff(np.r_[0.0, rec]) * prec))


def ap_ref_all(scores, targets):
    """[M] per-class ap_ref of [N, M] arrays"""
    s = np.asarray(scores)
    t = np.asarray(targets)
    return np.array([ap_ref(s[:, c], t[:, c]) for c in range(s.shape[1])])


# ---- config -----------------------------------------------------------------------------------------------------------
def test_config_defaults_and_overrides():
    d = x.get_default_config()
    assert d.DATA.MULTI_LABEL is False and d.TEST.ENSEMBLE_METHOD == "mean"
    m = x.get_config("M")
    assert m.DATA.MULTI_LABEL is False and m.TEST.ENSEMBLE_METHOD == "mean"
    c = x.get_config("M", ["NETWORK.NUM_CLASSES", 157, "DATA.MULTI_LABEL", True, "TEST.ENSEMBLE_METHOD", "max"])
    assert c.NETWORK.NUM_CLASSES == 157 and c.DATA.MULTI_LABEL is True and c.TEST.ENSEMBLE_METHOD == "max"
    assert x.build_arch(c).num_classes == 157
    with pytest.raises(ValueError):
        x.get_config("M", ["TEST.ENSEMBLE_METHOD", "median"])
    with pytest.raises(ValueError):
        x.get_config("M", ["DATA.MULTI_LABEL", 1])          # type mismatch: a bool switch


def test_single_label_dry_plans_are_unchanged_and_multi_label_records_the_new_head():
    """the launch lists of dry plans: the default config records softmax + view mean exactly as before; MULTI_LABEL swaps
    in the sigmoid head, ENSEMBLE_METHOD=max the view max -- nothing else moves"""
    import torch
    from x3d_tf_amd.model import X3D
    base = ["DATA.TEMP_DURATION", 4, "TEST.NUM_TEMPORAL_VIEWS", 2, "TEST.NUM_SPATIAL_CROPS", 3]

    def names(over, training):
        m = X3D(x.get_config("XS", base + over), dtype=torch.float32, device="dry")
        pl = m._plan(6 if not training else 2, 4, 64, 64, training)
        return [e[0] for e in pl.fwd], [e[0] for e in pl.bwd]

    for training in (False, True):
        f0, b0 = names([], training)
        f1, b1 = names(["DATA.MULTI_LABEL", True], training)
        head0 = "x3d_softmax_xent"
        assert head0 in f0 and "x3d_sigmoid_bce" not in f0
        assert f1 == [("x3d_sigmoid_bce" if n == head0 else n) for n in f0]
        assert b1 == b0
    f2, _ = names(["TEST.ENSEMBLE_METHOD", "max"], False)
    f0, _ = names([], False)
    assert f2 == [("x3d_view_max" if n == "x3d_view_mean" else n) for n in f0]


# ---- records and text lines -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("labels", [[], [7], [3, 150, 42]])
def test_sequence_example_round_trip(labels):
    frames = np.zeros((2, 8, 8, 3), np.uint8)
    rec = DL.make_sequence_example(frames, labels)
    jpegs, nf, got = DL.parse_sequence_example_labels(rec)
    assert got == labels and nf == 2 and len(jpegs) == 2
    _, _, first = DL.parse_sequence_example(rec)
    assert first == (labels[0] if labels else -1)


def test_single_label_record_is_byte_identical():
    frames = np.zeros((1, 8, 8, 3), np.uint8)
    enc = [DL.encode_jpeg(frames[0])]
    assert DL.make_sequence_example(None, 5, encoded=enc) == DL.make_sequence_example(None, np.int64(5), encoded=enc)
    assert DL.parse_sequence_example_labels(DL.make_sequence_example(None, 5, encoded=enc))[2] == [5]
    # a one-element list is the same int64 list on the wire
    assert DL.make_sequence_example(None, [5], encoded=enc) == DL.make_sequence_example(None, 5, encoded=enc)


def test_multi_label_record_wire_format():
    rec = DL.make_sequence_example(None, [3, 150, 42], encoded=[b"\xff\xd8x"])
    # video/class/label is a packed varint list: 3, 150 (two bytes), 42
    assert b"\x0a\x04\x03\x96\x01\x2a" in rec


def test_text_lines_and_multi_hot():
    assert DL.parse_label_list("3,150,42") == [3, 150, 42]
    assert DL.parse_label_list("7") == [7] and DL.parse_label_list("") == []
    t = DL.multi_hot([[0, 2], [], [1]], 3)
    assert t.dtype == torch.float32 and t.tolist() == [[1, 0, 1], [0, 0, 0], [0, 1, 0]]
    with pytest.raises(ValueError, match="clip-b"):
        DL.multi_hot([[0], [3]], 3, names=["clip-a", "clip-b"])
    with pytest.raises(ValueError):
        DL.multi_hot([[-1]], 3)


def test_reader_parses_multi_label_text_lines():
    cfg = x.get_config("XS", ["DATA.MULTI_LABEL", True, "NETWORK.NUM_CLASSES", 157])
    r = DL.InputReader(cfg, False, False, device="cpu", decoder=lambda p: np.zeros((4, 8, 8, 3), np.uint8))
    video, labels = r.decode_video("videos/abc.mp4 3,150,42\n")
    assert labels == [3, 150, 42] and video.shape == (4, 8, 8, 3)
    single = DL.InputReader(x.get_config("XS"), False, False, device="cpu", decoder=lambda p: np.zeros((4, 8, 8, 3), np.uint8))
    assert single.decode_video("videos/abc.mp4 17")[1] == 17


# ---- the AP reference -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("scores, targets, want", [
    ([0.9, 0.8, 0.7, 0.6], [1, 0, 1, 0], 0.5 + 0.5 * 2 / 3),
    ([0.5, 0.5, 0.2], [1, 1, 0], 1.0),                              # ties among positives
    ([0.5, 0.5, 0.2], [1, 0, 1], 0.5 * 0.5 + 0.5 * 2 / 3),          # a positive tied with a negative
    ([0.3, 0.3, 0.3, 0.3], [1, 0, 0, 1], 0.5),                      # every score equal
    ([0.1, 0.4, 0.35, 0.8], [0, 0, 1, 0], 1 / 3),                   # a single positive
    ([0.2, 0.9, 0.4], [1, 1, 1], 1.0),                              # all positives
    ([-0.0, 0.0, 1.0], [1, 0, 0], 1 / 3),                           # -0 and +0 are one threshold
    ([0.6, 0.6, 0.6, 0.1, 0.1], [0.5, 0.0, 1.0, 0.49, 1.0], 2 / 3 * 2 / 3 + 1 / 3 * 3 / 5),   # soft targets: >= 0.5 positive
])
def test_ap_reference_hand_worked(scores, targets, want):
    assert abs(ap_ref(scores, targets) - want) < 1e-15


def test_ap_reference_without_positives_or_with_nan():
    assert math.isnan(ap_ref([0.1, 0.2], [0, 0]))
    assert math.isnan(ap_ref([0.1, float("nan")], [1, 0]))


def test_ap_reference_matches_sklearn_when_installed():
    try:
        from sklearn.metrics import average_precision_score
    except ImportError:
        return
    rng = np.random.default_rng(0)
    for _ in range(20):
        n = int(rng.integers(1, 300))
        s = np.round(rng.random(n) * 7) / 7           # 8 levels: ties everywhere
        y = (rng.random(n) < 0.3).astype(np.float64)
        if y.sum() == 0:
            y[0] = 1
        assert abs(ap_ref(s, y) - average_precision_score(y, s)) < 1e-12


@pytest.mark.parametrize("training", [False, True])
def test_reader_names_every_record_by_its_own_file(tmp_path, training):
    """multi-label mode carries "<file>#<index>" with every record (the out-of-range class error names it): the name
    must be that of the file the record came from, in file order and after the training shuffle alike"""
    cfg = x.get_config("XS", ["DATA.MULTI_LABEL", True, "NETWORK.NUM_CLASSES", 157])
    for k in range(3):
        recs = [DL.make_sequence_example(None, [k, 10 + i], encoded=[b"\xff\xd8x"]) for i in range(k + 2)]
        DL.write_tfrecords(str(tmp_path / f"part-{k}.tfrecord"), recs)
    r = DL.InputReader(cfg, training, True, device="cpu", seed=1)
    seen = []
    for name, rec in r._records(str(tmp_path / "part-*.tfrecord"), 2):
        k, i = DL.parse_sequence_example_labels(rec)[2]
        assert name == f"{tmp_path / f'part-{k}.tfrecord'}#{i - 10}"
        seen.append(name)
    assert len(seen) == 2 + 3 + 4
