"""Regenerates the JPEG fixtures of tests/test_jpeg.py / tests/test_jpeg_gpu.py:   python tests/golden/jpeg/make_jpeg_golden.py

Every <name>.jpg is written by Pillow (libjpeg-turbo) from a seeded synthetic frame -- a smooth gradient, sharp edges
(IDCT overshoot, clamping) and noise -- and <name>.npy is its decode by Pillow on the same host (dataloader.decode_jpeg,
the host path the device decoder must reproduce bit for bit).  manifest.json lists each file's extents, components,
sampling factors (of the first component), restart interval and whether the device decoder takes it.

The small 4:2:2 / 4:2:0 frames pin the chroma upsampling edges whatever Pillow the test machine has: widths 4 | 5, 6 are
downsampled chroma widths 2 | 3, where replication gives way to the triangle filter, and heights 3 and 2 are chroma heights
2 and 1, where both vertical neighbours are the edge row.  The `_rst1` frames restart after every MCU (12 MCUs: the marker
numbers wrap past RST7); `_flat` is one colour (DC coefficients only), `_noise` is 0 / 255 per sample (the largest ones)."""
import io
import json
import os

import numpy as np
from PIL import Image

HERE = os.path.dirname(os.path.abspath(__file__))
SUBSAMPLING = {"444": 0, "422": 1, "420": 2}
LUMA = {"444": (1, 1), "422": (2, 1), "420": (2, 2), "gray": (1, 1)}


def frame(h, w, seed):
    rng = np.random.default_rng(seed)
    y, x = np.mgrid[0:h, 0:w].astype(np.float32)
    img = np.stack([255 * x / max(w - 1, 1), 255 * y / max(h - 1, 1), 128 + 100 * np.sin((x + 2 * y) / 5)], -1)
    img[(x // 6 + y // 4) % 3 == 0] = [250, 10, 240]          # hard edges: overshoot past 0 / 255 after the IDCT
    img += rng.normal(0, 12, img.shape)
    return np.clip(img, 0, 255).astype(np.uint8)


def encode(img, kind, quality, optimize, **kw):
    buf = io.BytesIO()
    if kind == "gray":
        Image.fromarray(img).convert("L").save(buf, "JPEG", quality=quality, optimize=optimize, **kw)
    else:
        Image.fromarray(img, "RGB").save(buf, "JPEG", quality=quality, optimize=optimize,
                                         subsampling=SUBSAMPLING[kind], **kw)
    return buf.getvalue()


def decode(data):
    with Image.open(io.BytesIO(data)) as im:
        return np.asarray(im.convert("RGB"), dtype=np.uint8)


def main():
    cases = []
    for (h, w) in [(1, 1), (7, 9), (17, 33), (33, 17)]:
        for kind in ["444", "422", "420", "gray"]:
            cases.append(dict(h=h, w=w, kind=kind, q=90, opt=True))
    for kind in ["444", "422", "420", "gray"]:
        cases += [dict(h=17, w=33, kind=kind, q=50, opt=False), dict(h=33, w=17, kind=kind, q=100, opt=True),
                  dict(h=33, w=17, kind=kind, q=100, opt=False)]
    cases += [dict(h=256, w=340, kind="420", q=90, opt=True), dict(h=240, w=320, kind="422", q=90, opt=True),
              dict(h=240, w=320, kind="444", q=50, opt=False), dict(h=256, w=340, kind="gray", q=100, opt=True)]
    cases += [dict(h=45, w=70, kind="420", q=90, opt=True, restart=dict(restart_marker_blocks=3)),
              dict(h=40, w=33, kind="444", q=75, opt=False, restart=dict(restart_marker_rows=1))]
    cases += [dict(h=33, w=17, kind="420", q=90, opt=True, progressive=True)]
    for kind in ["422", "420"]:
        cases += [dict(h=h, w=w, kind=kind, q=90, opt=True) for (h, w) in [(3, 4), (3, 5), (2, 6)]]
    cases += [dict(h=17, w=49, kind="422", q=75, opt=False, restart=dict(restart_marker_blocks=1), tag="_rst1"),
              dict(h=17, w=25, kind="gray", q=75, opt=False, restart=dict(restart_marker_blocks=1), tag="_rst1"),
              dict(h=16, w=17, kind="420", q=90, opt=False, content="flat", tag="_flat"),
              dict(h=9, w=15, kind="444", q=100, opt=False, content="noise", tag="_noise")]
    manifest = []
    for i, c in enumerate(cases):
        img = frame(c["h"], c["w"], seed=100 + i)
        if c.get("content") == "flat":
            img[:] = [201, 37, 118]
        elif c.get("content") == "noise":
            img = (np.random.default_rng(100 + i).integers(0, 2, img.shape) * 255).astype(np.uint8)
        kw = dict(c.get("restart", {}))
        if c.get("progressive"):
            kw["progressive"] = True
        data = encode(img, c["kind"], c["q"], c["opt"], **kw)
        suffix = c.get("tag") or ("_rst" if "restart" in c else "") + ("_prog" if c.get("progressive") else "")
        name = f"{c['kind']}_{c['h']}x{c['w']}_q{c['q']}{'_opt' if c['opt'] else ''}{suffix}"
        with open(os.path.join(HERE, name + ".jpg"), "wb") as f:
            f.write(data)
        np.save(os.path.join(HERE, name + ".npy"), decode(data))
        manifest.append(dict(name=name, height=c["h"], width=c["w"], components=1 if c["kind"] == "gray" else 3,
                             luma_sampling=list(LUMA[c["kind"]]), restart="restart" in c,
                             supported=not c.get("progressive")))
    with open(os.path.join(HERE, "manifest.json"), "w") as f:
        json.dump(manifest, f, indent=1)
    print(f"{len(manifest)} fixtures")


if __name__ == "__main__":
    main()
