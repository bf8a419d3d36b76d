"""Shared by tests/test_jpeg_replay.py, tests/test_jpeg_gpu.py and tests/golden/jpeg_damaged/make_jpeg_damaged.py: the
host replay of the device JPEG decoder (tests/jpeg_replay.cpp: build, run), the seeded legal streams of the small-size
sweep, and the seeded damaged streams (mutants)."""
import importlib.util
import io
import os
import shutil
import subprocess

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden", "jpeg")
DAMAGED = os.path.join(ROOT, "tests", "golden", "jpeg_damaged")

JPEG_OK, JPEG_UNSUPPORTED, JPEG_MALFORMED, JPEG_CORRUPT = 0, 1, 2, 3
TOO_LARGE = -1                      # jpeg_replay.cpp: a (damaged) header claims more pixels than the replay allocates

SAN_FLAGS = ["-g", "-Xarch_host", "-fsanitize=address,undefined", "-Xarch_host", "-fno-sanitize-recover=undefined"]


def _golden():
    spec = importlib.util.spec_from_file_location("make_jpeg_golden", os.path.join(GOLD, "make_jpeg_golden.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


golden = _golden()


def hipcc():
    exe = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    return exe if os.path.exists(exe) else None


def build_replay(out_dir, sanitize=False):
    """compiles tests/jpeg_replay.cpp (which includes csrc/jpeg.hip) into out_dir; the path of the executable"""
    exe = os.path.join(str(out_dir), "jpeg_replay_san" if sanitize else "jpeg_replay")
    cmd = [hipcc(), "-x", "hip", "--offload-arch=gfx950", "-O1"] + (SAN_FLAGS if sanitize else []) + \
          [os.path.join(ROOT, "tests", "jpeg_replay.cpp"), "-o", exe]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    return exe


def run_replay(exe, datas, work_dir, want_pixels=True):
    """every byte string of `datas` through the replay, as one child process -> [(status, uint8 [H, W, 3] or None)].
    The child must exit 0 and print nothing (a sanitizer report goes to stderr and changes the exit code)."""
    work_dir = str(work_dir)
    os.makedirs(work_dir, exist_ok=True)
    lines = []
    for i, d in enumerate(datas):
        with open(os.path.join(work_dir, f"{i}.jpg"), "wb") as f:
            f.write(d)
        lines.append(f"{os.path.join(work_dir, f'{i}.jpg')} {os.path.join(work_dir, f'{i}.bin')}\n")
    lst = os.path.join(work_dir, "list.txt")
    with open(lst, "w") as f:
        f.writelines(lines)
    r = subprocess.run([exe, lst], capture_output=True, text=True)
    assert r.returncode == 0 and not r.stderr.strip(), f"exit {r.returncode}\n{r.stderr[-4000:]}"
    out = []
    for i in range(len(datas)):
        raw = open(os.path.join(work_dir, f"{i}.bin"), "rb").read()
        status, h, w = np.frombuffer(raw[:12], np.int32).tolist()
        px = None
        if status == JPEG_OK:
            assert len(raw) == 12 + h * w * 3, (i, len(raw), h, w)
            if want_pixels:
                px = np.frombuffer(raw[12:], np.uint8).reshape(h, w, 3)
        else:
            assert len(raw) == 12, (i, status, len(raw))
        out.append((status, px))
    shutil.rmtree(work_dir)
    return out


# ------------------------------------------------------------------------------------------------
# legal streams
# ------------------------------------------------------------------------------------------------
KINDS = ["444", "422", "420", "gray"]
ENCODINGS = {                       # name -> (quality, optimize, extra Pillow save arguments)
    "q90_opt": (90, True, {}),
    "q100": (100, False, {}),
    "q30": (30, False, {}),
    "q75_rstmcu": (75, False, dict(restart_marker_blocks=1)),
    "q75_rstrow": (75, False, dict(restart_marker_rows=1)),
}
SWEEP_H = [1, 2, 3, 4, 5, 8, 9, 15, 16, 17]
SWEEP_W = [1, 2, 3, 4, 5, 6, 7, 8, 9, 15, 16, 17, 18, 31, 32, 33]


def content(h, w, seed, index):
    """the frame of sweep position `index`: every 7th 0/255 noise (the largest coefficients), every 11th flat (DC only),
    the others make_jpeg_golden.frame (gradient, hard edges, noise)"""
    if index % 7 == 0:
        return (np.random.default_rng(seed).integers(0, 2, (h, w, 3)) * 255).astype(np.uint8)
    if index % 11 == 0:
        return np.broadcast_to(np.random.default_rng(seed).integers(0, 256, 3).astype(np.uint8), (h, w, 3)).copy()
    return golden.frame(h, w, seed)


def legal_stream(h, w, kind, enc, index):
    q, opt, kw = ENCODINGS[enc]
    return golden.encode(content(h, w, 1000 + index, index), kind, q, opt, **kw)


def legal_sweep(hs=SWEEP_H, ws=SWEEP_W, kinds=KINDS, encs=tuple(ENCODINGS)):
    """[(label, jpeg bytes)] over hs x ws x kinds x encs; `index` (which decides content and seed) counts the full product"""
    out, index = [], 0
    for h in hs:
        for w in ws:
            for kind in kinds:
                for enc in encs:
                    out.append((f"{kind}_{h}x{w}_{enc}#{index}", legal_stream(h, w, kind, enc, index)))
                    index += 1
    return out


def host_decode(data):
    """Pillow's decode of `data` as the input pipeline's host path does it -> (uint8 [H, W, 3] or None if Pillow raises)"""
    import warnings
    try:
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            return golden.decode(data)
    except Exception:
        return None


def host_is_libjpeg_turbo():
    from PIL import features
    return bool(features.check_feature("libjpeg_turbo"))


def host_versions():
    import PIL
    from PIL import features
    turbo = features.version_feature("libjpeg_turbo") if host_is_libjpeg_turbo() else None
    return f"Pillow {PIL.__version__}, " + (f"libjpeg-turbo {turbo}" if turbo else f"libjpeg {features.version('jpg')}")


# ------------------------------------------------------------------------------------------------
# damaged streams
# ------------------------------------------------------------------------------------------------
def ecs_range(data):
    """(first byte of the entropy-coded segment, its end = the last EOI) of a single-scan stream"""
    k = data.index(b"\xff\xda")
    return k + 2 + ((data[k + 2] << 8) | data[k + 3]), data.rindex(b"\xff\xd9")


ECS_KINDS = ["bitflip", "replace", "delete"]
FILE_KINDS = ["bitflip", "truncate", "rst", "run"]


def ecs_mutant(data, kind, rng):
    """damage inside the entropy-coded segment only: 1-2 bit flips, one byte replaced, or one byte deleted"""
    lo, hi = ecs_range(data)
    b = bytearray(data)
    if kind == "bitflip":
        for _ in range(int(rng.integers(1, 3))):
            b[int(rng.integers(lo, hi))] ^= 1 << int(rng.integers(0, 8))
    elif kind == "replace":
        b[int(rng.integers(lo, hi))] = int(rng.integers(0, 256))
    elif kind == "delete":
        del b[int(rng.integers(lo, hi))]
    else:
        raise ValueError(kind)
    return bytes(b)


def file_mutant(data, kind, rng):
    """damage anywhere in the file: bit flips, truncation, an injected RSTn, a run of random bytes"""
    b = bytearray(data)
    n = len(b)
    if kind == "bitflip":
        for _ in range(int(rng.integers(1, 4))):
            b[int(rng.integers(0, n))] ^= 1 << int(rng.integers(0, 8))
    elif kind == "truncate":
        del b[int(rng.integers(0, n)):]
    elif kind == "rst":
        k = int(rng.integers(0, n + 1))
        b[k:k] = bytes([0xFF, 0xD0 + int(rng.integers(0, 8))])
    elif kind == "run":
        k, m = int(rng.integers(0, n)), int(rng.integers(1, 9))
        b[k:k + m] = rng.integers(0, 256, m).astype(np.uint8).tobytes()
    else:
        raise ValueError(kind)
    return bytes(b)


def mutant_sources():
    """[(label, bytes)]: 96 legal streams, all samplings and encodings, among them the classes in which the decoder once
    accepted a damaged stream that the host decodes differently (4:2:2 5x1 / 15x9 / 17x9 at q30, grey 15x15 with a
    restart per MCU row)"""
    sizes = [(5, 1), (15, 9), (17, 9), (15, 15), (3, 4), (8, 17), (16, 33), (9, 18)]
    out, i = [], 0
    for (h, w) in sizes:
        for kind in KINDS:
            for enc in ["q30", "q75_rstrow", "q90_opt"]:
                img = content(h, w, 5000 + i, 7 if i % 8 == 7 else 1)      # every 8th source is 0/255 noise
                q, opt, kw = ENCODINGS[enc]
                out.append((f"{kind}_{h}x{w}_{enc}", golden.encode(img, kind, q, opt, **kw)))
                i += 1
    return out


def ecs_mutants(per_source=12, seed=2024):
    """[(label, bytes)]: per_source entropy-segment mutants of every source, the three kinds in turn"""
    rng = np.random.default_rng(seed)
    out = []
    for name, data in mutant_sources():
        for j in range(per_source):
            kind = ECS_KINDS[j % 3]
            out.append((f"{name}.{kind}{j}", ecs_mutant(data, kind, rng)))
    return out


def file_mutants(per_source=24, seed=77):
    """[(label, bytes)]: per_source whole-file mutants of every source, the four kinds in turn"""
    rng = np.random.default_rng(seed)
    out = []
    for name, data in mutant_sources():
        for j in range(per_source):
            kind = FILE_KINDS[j % 4]
            out.append((f"{name}.{kind}{j}", file_mutant(data, kind, rng)))
    return out
