"""The device JPEG decoder (jpeg.decode_jpeg_batch -> x3d_jpeg_decode) against Pillow: every fixture of
tests/golden/jpeg/ bit-identical to its host decode, alone and in one mixed batch; the out-of-scope fixture through the
host fall-back; a cut entropy segment reported for its frame only; a batch of >= 1,024 frames equal to one at a time;
the small-size sweep (every chroma width and height at which the upsampling changes its rule, every MCU edge, all samplings
and encodings, flat and saturated frames) against a live Pillow decode; the damaged corpus of tests/golden/jpeg_damaged/
against the statuses and pixels its manifest records."""
import io
import json
import os

import numpy as np
import pytest
import torch

from tests import jpeg_replay_util as U
from tests.aux_checks import _Bands
from x3d_tf_amd import hip
from x3d_tf_amd.dataloader import decode_jpeg, encode_jpeg
from x3d_tf_amd.jpeg import JpegDecodeError, decode_jpeg_batch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden", "jpeg")
MANIFEST = json.load(open(os.path.join(GOLD, "manifest.json")))


def _case(name):
    return open(os.path.join(GOLD, name + ".jpg"), "rb").read(), np.load(os.path.join(GOLD, name + ".npy"))


@pytest.mark.gpu
@pytest.mark.parametrize("case", MANIFEST, ids=[c["name"] for c in MANIFEST])
def test_fixture_alone_is_bit_identical(gpu, case):
    data, want = _case(case["name"])
    got = decode_jpeg_batch([data], gpu)
    assert got.shape == (1,) + want.shape and got.dtype == torch.uint8
    assert torch.equal(got[0].cpu(), torch.from_numpy(want)), case["name"]


@pytest.mark.gpu
def test_mixed_batch_of_every_fixture(gpu):
    cases = [_case(c["name"]) for c in MANIFEST] * 3                # different sizes, samplings, tables; repeated
    slots = [torch.full(w.shape, 77, dtype=torch.uint8, device=gpu) for _, w in cases]
    out = decode_jpeg_batch([d for d, _ in cases], gpu, out=slots)
    assert out is not None
    for i, ((_, want), s) in enumerate(zip(cases, slots)):
        assert torch.equal(s.cpu(), torch.from_numpy(want)), MANIFEST[i % len(MANIFEST)]["name"]


@pytest.mark.gpu
def test_progressive_frame_falls_back_to_the_host(gpu):
    name = next(c["name"] for c in MANIFEST if not c["supported"])
    data, want = _case(name)
    same = [c["name"] for c in MANIFEST if c["supported"] and (c["height"], c["width"]) == want.shape[:2]]
    other, other_want = _case(same[0])
    got = decode_jpeg_batch([other, data, other], gpu)
    assert torch.equal(got[1].cpu(), torch.from_numpy(np.array(decode_jpeg(data))))
    assert torch.equal(got[1].cpu(), torch.from_numpy(want))
    assert torch.equal(got[0].cpu(), torch.from_numpy(other_want)) and torch.equal(got[2].cpu(), torch.from_numpy(other_want))


@pytest.mark.gpu
def test_cut_entropy_segment_is_reported_for_its_frame_only(gpu):
    data, want = _case("420_256x340_q90_opt")
    cut = data[:len(data) // 2]                                     # header intact, the scan ends half way
    sentinel = 91
    slots = [torch.full(want.shape, sentinel, dtype=torch.uint8, device=gpu) for _ in range(5)]
    with pytest.raises(JpegDecodeError) as ei:
        decode_jpeg_batch([data, data, cut, data, cut[:-7]], gpu, out=slots)
    e = ei.value
    assert isinstance(e, hip.X3DHipError)
    assert e.frames == [2, 4] and "frame(s) [2, 4]" in str(e)
    assert e.status == [hip.JPEG_OK, hip.JPEG_OK, hip.JPEG_CORRUPT, hip.JPEG_OK, hip.JPEG_CORRUPT]
    for i in (0, 1, 3):
        assert torch.equal(slots[i].cpu(), torch.from_numpy(want))
    assert bool((slots[2] == sentinel).all())                       # a corrupt frame's slot is not written
    # a wrong restart marker is corrupt data too
    rdata, rwant = _case("420_45x70_q90_opt_rst")
    k = rdata.index(b"\xff\xd1")
    bad = rdata[:k] + b"\xff\xd5" + rdata[k + 2:]
    with pytest.raises(JpegDecodeError) as ei:
        decode_jpeg_batch([rdata, bad], gpu)
    assert ei.value.frames == [1]
    assert torch.equal(ei.value.output[0].cpu(), torch.from_numpy(rwant))


@pytest.mark.gpu
def test_large_batch_equals_one_frame_at_a_time(gpu):
    rng = np.random.default_rng(5)
    frames = []
    for i in range(1100):
        h, w = [(48, 64), (40, 56), (17, 33)][i % 3]
        y, x = np.mgrid[0:h, 0:w]
        img = np.stack([x * 4 + i, y * 5 + 2 * i, (x * y) % 256], -1) + rng.normal(0, 10, (h, w, 3))
        frames.append(encode_jpeg(np.clip(img, 0, 255).astype(np.uint8), quality=int(rng.integers(50, 100))))
    slots = [torch.empty(decode_jpeg(f).shape, dtype=torch.uint8, device=gpu) for f in frames]
    decode_jpeg_batch(frames, gpu, out=slots)
    for i in range(0, len(frames), 7):
        one = decode_jpeg_batch([frames[i]], gpu)[0]
        assert torch.equal(slots[i], one), i
    for i in range(len(frames)):
        assert torch.equal(slots[i].cpu(), torch.from_numpy(np.array(decode_jpeg(frames[i])))), i


@pytest.mark.gpu
def test_frames_of_different_sizes_need_slots(gpu):
    a, _ = _case("420_17x33_q90_opt")
    b, _ = _case("420_33x17_q90_opt")
    with pytest.raises(ValueError, match="different sizes"):
        decode_jpeg_batch([a, b], gpu)
    with pytest.raises(ValueError, match="does not fit"):
        decode_jpeg_batch([a], gpu, out=[torch.empty((33, 17, 3), dtype=torch.uint8, device=gpu)])


# widths 1-6: downsampled chroma widths 1, 2 | 3 (replication | triangle filter); heights 1-5: chroma heights 1, 2, 3 (both
# vertical neighbours clamped, one, none); 8 | 9 and 16 | 17: the MCU edges of 4:4:4 / grey and of 4:2:0; 15, 31 | 33
SWEEP_SIZES = [1, 2, 3, 4, 5, 6, 8, 9, 15, 16, 17, 31, 33]
_SWEEP = []


def _sweep():
    """[(label, jpeg bytes, Pillow's decode)], made once: every height x width x sampling with the five encodings in turn,
    and all five on the frames of at most 5 x 6; every 7th frame is 0 / 255 noise, every 11th flat"""
    if not _SWEEP:
        index = 0
        for h in SWEEP_SIZES:
            for w in SWEEP_SIZES:
                for kind in U.KINDS:
                    small = h <= 5 and w <= 6
                    for enc in (list(U.ENCODINGS) if small else [list(U.ENCODINGS)[index % 5]]):
                        data = U.legal_stream(h, w, kind, enc, index)
                        _SWEEP.append((f"{kind}_{h}x{w}_{enc}#{index}", data, U.golden.decode(data)))
                        index += 1
    return _SWEEP


@pytest.mark.gpu
@pytest.mark.parametrize("part,off", [(0, 0), (1, 5)])
def test_small_size_sweep_equals_the_host_decode(gpu, part, off):
    """one mixed batch per half of the sweep, every frame into its own slot: a view (16-byte aligned in one half, not in
    the other) between bands of a sentinel that must still stand afterwards"""
    sweep = _sweep()
    assert len(sweep) >= 1000
    kinds = {(n.split("_")[0], n.split("#")[0].split("_", 2)[2]) for n, _, _ in sweep}
    assert len(kinds) == len(U.KINDS) * len(U.ENCODINGS)                    # every sampling with every encoding
    mine = sweep[part::2]
    bands = _Bands(gpu, off)
    slots = [bands(want.shape, torch.uint8) for _, _, want in mine]
    decode_jpeg_batch([d for _, d, _ in mine], gpu, out=slots)
    bands.check()
    got = [s.cpu().numpy() for s in slots]
    wrong = [n for (n, _, want), g in zip(mine, got) if not np.array_equal(g, want)]
    assert not wrong, (len(wrong), wrong[:8])


@pytest.mark.gpu
def test_damaged_corpus_matches_its_manifest(gpu):
    """tests/golden/jpeg_damaged/ in one batch: the statuses and the accepted frames are what the host replay of the
    decoder recorded (and verified against Pillow where it accepted), the slot of every corrupt frame keeps its sentinel"""
    manifest = json.load(open(os.path.join(U.DAMAGED, "manifest.json")))
    datas = [open(os.path.join(U.DAMAGED, m["name"] + ".jpg"), "rb").read() for m in manifest]
    bands = _Bands(gpu)
    slots = [bands((m["height"], m["width"], 3), torch.uint8) for m in manifest]
    sentinel = int(slots[0].flatten()[0])
    with pytest.raises(JpegDecodeError) as ei:
        decode_jpeg_batch(datas, gpu, out=slots)
    bands.check()
    assert ei.value.status == [m["status"] for m in manifest]
    assert ei.value.frames == [i for i, m in enumerate(manifest) if m["status"] == hip.JPEG_CORRUPT]
    for m, s in zip(manifest, slots):
        if m["status"] == hip.JPEG_OK:
            assert np.array_equal(s.cpu().numpy(), np.load(os.path.join(U.DAMAGED, m["name"] + ".npy"))), m["name"]
        else:
            assert bool((s == sentinel).all()), m["name"]
