"""Regenerates the damaged-stream corpus of tests/test_jpeg_gpu.py:   python tests/golden/jpeg_damaged/make_jpeg_damaged.py

About 64 damaged JPEG streams chosen from the seeded mutant sets of tests/jpeg_replay_util.py (the sets that
tests/test_jpeg_replay.py runs), each with what the device decoder must make of it.  The expectation comes from the host
replay of the decoder (tests/jpeg_replay.cpp, built here with AddressSanitizer and UBSan: a stream goes into the corpus
only if that run is clean), and every accepted stream is verified equal to Pillow's decode of the same bytes here.

  <name>.jpg      the damaged stream; its header parses (the device sees the frame)
  <name>.npy      uint8 [H, W, 3], for accepted streams only
  manifest.json   per stream: name, source, damage, height, width, status (X3D_JPEG_OK 0 | X3D_JPEG_CORRUPT 3), rule

Chosen:
  - streams the decoder accepted before it refused blocks outside the range in which the host decoders agree, with
    pixels that differed from the host's (4:2:2 5x1, 15x9, 17x9 and others): now X3D_JPEG_CORRUPT;
  - entropy-segment damage (bit flips, one byte replaced, one byte deleted) of 4:2:2 5x1 / 15x9 / 17x9 at q30 and of grey
    15x15 with a restart per MCU row, accepted and refused ones;
  - a marker the bit flip made inside the entropy data, after the last MCU (the host fails on it);
  - truncations, injected (extra) RSTn, and RSTn with the wrong number.

FORMER_DISAGREEMENTS are the former disagreements of this seeded set; it found none in 4:2:2 5x1 at q30 or in grey 15x15
with restart rows (its 4:2:2 5x1 one is the restart-row source).  Those two classes are in the corpus through the CLASSES
picks alone, with rule null: the corpus pins their statuses and pixels, not a former disagreement of each class."""
import json
import os
import sys
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(HERE))))
from tests import jpeg_replay_util as U   # noqa: E402
from x3d_tf_amd.jpeg import jpeg_info      # noqa: E402

# accepted with pixels unlike the host's before the IDCT range rule (found with Pillow 12.2.0 / libjpeg-turbo 3.1.4.1)
FORMER_DISAGREEMENTS = [
    "422_5x1_q75_rstrow.delete5", "444_15x9_q30.bitflip9", "444_15x9_q75_rstrow.bitflip0", "422_15x9_q30.bitflip9",
    "420_15x9_q30.replace1", "444_17x9_q75_rstrow.bitflip0", "422_17x9_q30.delete5", "422_15x15_q30.replace1",
    "420_15x15_q30.replace4", "420_3x4_q30.replace1", "422_8x17_q30.bitflip6", "420_16x33_q30.delete2",
    "444_9x18_q30.delete2", "gray_9x18_q75_rstrow.bitflip3"]
CLASSES = ["422_5x1_q30", "422_15x9_q30", "422_17x9_q30", "gray_15x15_q75_rstrow"]
TRAILING_MARKER = ["gray_5x1_q30.bitflip75", "422_8x17_q75_rstrow.bitflip81"]     # of ecs_mutants(120, seed=9)


def wrong_rst(data, which, number):
    """restart marker `which` (0-based) of the stream renumbered to RST<number>"""
    lo, hi = U.ecs_range(data)
    k = lo - 2
    for _ in range(which + 1):
        k = next(i for i in range(k + 2, hi) if data[i] == 0xFF and 0xD0 <= data[i + 1] <= 0xD7)
    assert data[k + 1] != 0xD0 + number
    return data[:k + 1] + bytes([0xD0 + number]) + data[k + 2:]


def main():
    ecs = U.ecs_mutants()
    by_name = dict(ecs)
    chosen = [(n, by_name[n], "range") for n in FORMER_DISAGREEMENTS]
    for cls in CLASSES:
        chosen += [(n, d, None) for n, d in ecs if n.startswith(cls + ".") and n not in FORMER_DISAGREEMENTS][:6]
    wide = dict(U.ecs_mutants(per_source=120, seed=9))
    chosen += [(n, wide[n], "marker") for n in TRAILING_MARKER]
    sources = dict(U.mutant_sources())
    chosen += [("422_16x33_q75_rstrow.wrongrst0", wrong_rst(sources["422_16x33_q75_rstrow"], 0, 5), "restart"),
               ("gray_15x15_q75_rstrow.wrongrst0", wrong_rst(sources["gray_15x15_q75_rstrow"], 0, 1), "restart"),
               ("420_17x9_q75_rstrow.wrongrst0", wrong_rst(sources["420_17x9_q75_rstrow"], 0, 7), "restart")]
    names = {n for n, _, _ in chosen}
    with tempfile.TemporaryDirectory() as tmp:
        exe = U.build_replay(tmp, sanitize=True)
        files = [(n, d) for n, d in U.file_mutants() if ".truncate" in n or ".rst" in n]
        res = U.run_replay(exe, [d for _, d in files], os.path.join(tmp, "f"), want_pixels=False)
        seen = {}
        for (n, d), (s, _) in zip(files, res):          # the frames whose header still parses, a few of each kind and status
            key = (n.split(".")[1].rstrip("0123456789"), s)
            if s == U.JPEG_OK and U.host_decode(d) is None:
                continue        # cut after its last MCU: it decodes, while Pillow reports the missing EOI; nothing to verify
            if s in (U.JPEG_OK, U.JPEG_CORRUPT) and seen.get(key, 0) < (5 if s == U.JPEG_OK else 6) and n not in names:
                seen[key] = seen.get(key, 0) + 1
                chosen.append((n, d, None))
        res = U.run_replay(exe, [d for _, d, _ in chosen], os.path.join(tmp, "c"))     # clean under the sanitizers, or it raises
    for f in os.listdir(HERE):
        if f.endswith((".jpg", ".npy")):
            os.remove(os.path.join(HERE, f))
    manifest = []
    for (n, d, rule), (s, px) in zip(chosen, res):
        assert s in (U.JPEG_OK, U.JPEG_CORRUPT), (n, s)
        assert rule is None or s == U.JPEG_CORRUPT, (n, rule, s)
        name = n.replace(".", "_")
        host = U.host_decode(d)
        if s == U.JPEG_OK:
            assert U.host_is_libjpeg_turbo() and host is not None and np.array_equal(host, px), n
        with open(os.path.join(HERE, name + ".jpg"), "wb") as f:
            f.write(d)
        if s == U.JPEG_OK:
            np.save(os.path.join(HERE, name + ".npy"), px)
        h, w = jpeg_info(d)[:2]
        manifest.append(dict(name=name, source=n.split(".")[0], damage=n.split(".")[1].rstrip("0123456789"), height=h,
                             width=w, status=s, rule=rule, host_decodes=host is not None))
    with open(os.path.join(HERE, "manifest.json"), "w") as f:
        json.dump(manifest, f, indent=1)
    ok = sum(m["status"] == U.JPEG_OK for m in manifest)
    print(f"{len(manifest)} damaged streams: {ok} accepted, {len(manifest) - ok} corrupt; host: {U.host_versions()}")


if __name__ == "__main__":
    main()
