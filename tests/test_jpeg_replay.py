"""The device JPEG decoder's stages run on the host.  Every stage function of csrc/jpeg.hip is __host__ __device__;
tests/jpeg_replay.cpp includes the file and runs parse -> Huffman tables -> entropy decode -> IDCT -> colour serially, with
every buffer a heap allocation of exactly the device's size.  No GPU: the arithmetic, the refusal rules and the memory
accesses of the decoder are checked wherever hipcc exists.

  - every fixture of tests/golden/jpeg/ equals its .npy;
  - the small-size sweep (10 heights x 16 widths x 4 samplings x 5 encodings = 3200 legal streams) equals a live Pillow
    decode and is never refused; so do 576 streams at q1 to q20, whose quantiser steps reach 255;
  - a build with AddressSanitizer and UBSan decodes 2304 + 1152 seeded damaged streams, as a child process of its own,
    without a report;
  - the contract for damaged entropy data: whatever the decoder accepts equals the host decode of the same bytes,
    everything else is X3D_JPEG_CORRUPT, and more than half is accepted;
  - the committed damaged corpus (tests/golden/jpeg_damaged/) is what the replay makes of it."""
import collections
import json
import os

import numpy as np
import pytest

from tests import jpeg_replay_util as U

pytestmark = pytest.mark.skipif(U.hipcc() is None, reason="hipcc not available")

MANIFEST = json.load(open(os.path.join(U.GOLD, "manifest.json")))
DAMAGED = json.load(open(os.path.join(U.DAMAGED, "manifest.json")))


@pytest.fixture(scope="module")
def replay(tmp_path_factory):
    return U.build_replay(tmp_path_factory.mktemp("jpeg_replay"))


@pytest.fixture(scope="module")
def replay_san(tmp_path_factory):
    return U.build_replay(tmp_path_factory.mktemp("jpeg_replay_san"), sanitize=True)


def test_every_fixture_is_bit_identical(replay, tmp_path):
    cases = [c for c in MANIFEST if c["supported"]]
    datas = [open(os.path.join(U.GOLD, c["name"] + ".jpg"), "rb").read() for c in cases]
    res = U.run_replay(replay, datas, tmp_path / "w")
    for c, (status, px) in zip(cases, res):
        assert status == U.JPEG_OK, c["name"]
        assert np.array_equal(px, np.load(os.path.join(U.GOLD, c["name"] + ".npy"))), c["name"]
    other = [c for c in MANIFEST if not c["supported"]]
    res = U.run_replay(replay, [open(os.path.join(U.GOLD, c["name"] + ".jpg"), "rb").read() for c in other], tmp_path / "u")
    assert [s for s, _ in res] == [U.JPEG_UNSUPPORTED] * len(other)


def test_legal_sweep_equals_the_host_decode(replay, tmp_path):
    sweep = U.legal_sweep()
    assert len(sweep) == 3200
    res = U.run_replay(replay, [d for _, d in sweep], tmp_path / "w")
    refused = [n for (n, _), (s, _) in zip(sweep, res) if s != U.JPEG_OK]
    assert not refused, (len(refused), refused[:8])
    wrong = [n for (n, d), (_, px) in zip(sweep, res) if not np.array_equal(px, U.golden.decode(d))]
    assert not wrong, (len(wrong), wrong[:8], U.host_versions())


def test_low_quality_streams_are_not_refused(replay, tmp_path):
    """q1 to q20: quantiser steps up to 255, the largest quantisation errors a legal stream has, so the samples before the
    clamp come nearest to the [-512, 511] limit of the IDCT range rule.  None may be refused, all equal the host decode."""
    items, index = [], 0
    for q in [1, 2, 3, 5, 8, 10, 15, 20]:
        for kind in U.KINDS:
            for (h, w) in [(8, 8), (16, 16), (17, 33), (33, 31), (5, 6), (3, 4)]:
                for c in (7, 11, 1):                                       # 0 / 255 noise, flat, gradient with hard edges
                    items.append((f"{kind}_{h}x{w}_q{q}_c{c}", U.golden.encode(U.content(h, w, 9000 + index, c), kind, q, False)))
                    index += 1
    assert len(items) == 576
    res = U.run_replay(replay, [d for _, d in items], tmp_path / "w")
    refused = [n for (n, _), (s, _) in zip(items, res) if s != U.JPEG_OK]
    assert not refused, (len(refused), refused[:8])
    wrong = [n for (n, d), (_, px) in zip(items, res) if not np.array_equal(px, U.golden.decode(d))]
    assert not wrong, (len(wrong), wrong[:8], U.host_versions())


def test_damaged_streams_under_the_sanitizers(replay_san, tmp_path):
    """bit flips, truncation, injected RSTn and runs of random bytes anywhere in the file, and the entropy-segment set of
    the contract test: the sanitizer build, a stand-alone child process, exits 0 and reports nothing (run_replay asserts
    both)"""
    mutants = U.file_mutants() + U.ecs_mutants()
    kinds = collections.Counter(n.split(".")[1].rstrip("0123456789") for n, _ in U.file_mutants())
    assert len(mutants) >= 2000 and len({n.split(".")[0] for n, _ in mutants}) >= 50
    assert sorted(kinds) == sorted(U.FILE_KINDS) and min(kinds.values()) >= 500
    res = U.run_replay(replay_san, [d for _, d in mutants], tmp_path / "w", want_pixels=False)
    by_status = collections.Counter(s for s, _ in res)
    print(f"{len(mutants)} damaged streams under ASan + UBSan: {dict(by_status)}")
    assert set(by_status) <= {U.JPEG_OK, U.JPEG_UNSUPPORTED, U.JPEG_MALFORMED, U.JPEG_CORRUPT, U.TOO_LARGE}
    assert by_status[U.JPEG_OK] > 0 and by_status[U.JPEG_CORRUPT] > 0 and by_status[U.JPEG_MALFORMED] > 0
    # the committed corpus went through this build when it was made; it still does
    corpus = [open(os.path.join(U.DAMAGED, m["name"] + ".jpg"), "rb").read() for m in DAMAGED]
    U.run_replay(replay_san, corpus, tmp_path / "c", want_pixels=False)


def test_damaged_entropy_data_is_refused_or_decoded_as_the_host_does(replay, tmp_path):
    """1152 streams damaged inside the entropy-coded segment only (1-2 bit flips, one byte replaced, one byte deleted; 12 of
    each of 96 sources): status X3D_JPEG_OK means "equal to the host decode of the same bytes", anything else is
    X3D_JPEG_CORRUPT.  Before the decoder refused blocks outside the range in which the host decoders agree and markers left
    behind the last MCU, 778 of these were accepted and 25 of those differed from Pillow 12.2.0 / libjpeg-turbo 3.1.4.1;
    now 679 are accepted and none differs.  More than half must stay accepted: a decoder that refuses everything is not one."""
    mutants = U.ecs_mutants()
    assert len(mutants) == 1152
    res = U.run_replay(replay, [d for _, d in mutants], tmp_path / "w")
    accepted = corrupt = host_only = 0
    other, differ = [], []
    for (n, d), (status, px) in zip(mutants, res):
        if status == U.JPEG_OK:
            accepted += 1
            host = U.host_decode(d)
            if host is None or host.shape != px.shape or not np.array_equal(host, px):
                differ.append(n)
        elif status == U.JPEG_CORRUPT:
            corrupt += 1
            host_only += U.host_decode(d) is not None
        else:
            other.append((n, status))
    print(f"{len(mutants)} entropy-segment mutants: {accepted} accepted, {corrupt} corrupt, {len(differ)} accepted but unlike the "
          f"host decode, {host_only} refused that the host decodes without complaint ({U.host_versions()})")
    assert not other, other[:8]
    assert 2 * accepted >= len(mutants), (accepted, len(mutants))
    if U.host_is_libjpeg_turbo():            # (another libjpeg: tests/golden/jpeg_damaged/ carries the check)
        assert not differ, (len(differ), differ[:8], U.host_versions())


def test_damaged_corpus_is_what_the_replay_makes_of_it(replay, tmp_path):
    assert 48 <= len(DAMAGED) <= 80 and len({m["name"] for m in DAMAGED}) == len(DAMAGED)
    for cls in ["422_5x1_q30", "422_15x9_q30", "422_17x9_q30", "gray_15x15_q75_rstrow"]:
        assert any(m["source"] == cls for m in DAMAGED), cls
    assert {"bitflip", "replace", "delete", "truncate", "rst", "wrongrst"} <= {m["damage"] for m in DAMAGED}
    assert {"range", "marker", "restart"} <= {m["rule"] for m in DAMAGED}
    datas = [open(os.path.join(U.DAMAGED, m["name"] + ".jpg"), "rb").read() for m in DAMAGED]
    assert max(len(d) for d in datas) < 2048
    res = U.run_replay(replay, datas, tmp_path / "w")
    for m, d, (status, px) in zip(DAMAGED, datas, res):
        assert status == m["status"] and status in (U.JPEG_OK, U.JPEG_CORRUPT), m["name"]
        assert os.path.exists(os.path.join(U.DAMAGED, m["name"] + ".npy")) == (status == U.JPEG_OK), m["name"]
        if status == U.JPEG_OK:
            assert px.shape == (m["height"], m["width"], 3)
            assert np.array_equal(px, np.load(os.path.join(U.DAMAGED, m["name"] + ".npy"))), m["name"]
            if U.host_is_libjpeg_turbo():
                assert np.array_equal(px, U.host_decode(d)), m["name"]
