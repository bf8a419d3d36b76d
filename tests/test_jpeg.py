"""JPEG header parsing of the device decoder (x3d_jpeg_parse, host only): extents, sampling and support flags of the
fixtures under tests/golden/jpeg/, and truncated / garbled headers reported as errors without reading past the buffer."""
import ctypes
import json
import mmap
import os
import re

import numpy as np
import pytest

from x3d_tf_amd import hip
from x3d_tf_amd.jpeg import jpeg_info, parse_headers

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden", "jpeg")
MANIFEST = json.load(open(os.path.join(GOLD, "manifest.json")))


def _data(name):
    return open(os.path.join(GOLD, name + ".jpg"), "rb").read()


@pytest.mark.parametrize("case", MANIFEST, ids=[c["name"] for c in MANIFEST])
def test_header_of_every_fixture(case):
    data = _data(case["name"])
    h, w, comps, supported = jpeg_info(data)
    assert (h, w, comps, supported) == (case["height"], case["width"], case["components"], case["supported"])
    assert np.load(os.path.join(GOLD, case["name"] + ".npy")).shape == (h, w, 3)
    im = parse_headers([data])[0][0]
    if not supported:
        assert im.status == hip.JPEG_UNSUPPORTED
        return
    assert im.status == hip.JPEG_OK
    assert (im.restart_interval > 0) == case["restart"]
    if comps == 3:
        assert [im.hs[0], im.vs[0]] == case["luma_sampling"]
        assert [im.hs[1], im.vs[1], im.hs[2], im.vs[2]] == [1, 1, 1, 1]
        hm, vm = case["luma_sampling"]
        assert (im.mcux, im.mcuy) == (-(-w // (8 * hm)), -(-h // (8 * vm)))
    else:
        assert (im.mcux, im.mcuy) == (-(-w // 8), -(-h // 8))
    assert 0 < im.ecs_off < im.ecs_end <= len(data)
    assert data[im.ecs_end:im.ecs_end + 2] == b"\xff\xd9"


def test_progressive_is_rejected():
    name = next(c["name"] for c in MANIFEST if not c["supported"])
    assert "prog" in name
    assert jpeg_info(_data(name))[3] is False


def test_scratch_layout_covers_every_supported_image():
    datas = [_data(c["name"]) for c in MANIFEST]
    imgs, total = parse_headers(datas)
    end = 0
    for im in imgs[:len(datas)]:
        if im.status != hip.JPEG_OK:
            continue
        blocks = sum(im.bw[c] * im.bh[c] for c in range(im.ncomp))
        assert im.coef_off % 256 == 0 and im.plane_off % 256 == 0
        assert im.coef_off + blocks * 128 <= im.plane_off + 0 and im.plane_off + blocks * 64 <= total
        end = max(end, im.plane_off + blocks * 64)
    assert end <= total


def _guarded(data: bytes):
    """`data` placed so that its last byte ends a readable page and the next page is inaccessible: a parser that reads
    one byte past the buffer faults instead of passing"""
    page = mmap.PAGESIZE
    size = -(-max(len(data), 1) // page) * page
    m = mmap.mmap(-1, size + page, prot=mmap.PROT_READ | mmap.PROT_WRITE)
    base = ctypes.addressof(ctypes.c_char.from_buffer(m))
    libc = ctypes.CDLL(None, use_errno=True)
    libc.mprotect.argtypes = [ctypes.c_void_p, ctypes.c_size_t, ctypes.c_int]
    assert libc.mprotect(base + size, page, 0) == 0
    start = base + size - len(data)
    ctypes.memmove(start, data, len(data))
    return m, start


def _parse_at(addr, n):
    imgs = (hip.JpegImage * 1)()
    ptrs = (ctypes.c_void_p * 1)(addr)
    lens = (ctypes.c_int * 1)(n)
    total = ctypes.c_longlong(0)
    hip.check(hip.load().x3d_jpeg_parse(ctypes.cast(ptrs, ctypes.c_void_p), ctypes.cast(lens, ctypes.c_void_p), 1, imgs,
                                        ctypes.byref(total)), "x3d_jpeg_parse")
    return imgs[0]


def test_truncated_headers_are_errors_and_stay_inside_the_buffer():
    for name in ["420_256x340_q90_opt", "gray_7x9_q90_opt", "444_40x33_q75_rst"]:
        data = _data(name)
        ecs = parse_headers([data])[0][0].ecs_off
        for cut in range(0, ecs):
            with pytest.raises(ValueError):
                jpeg_info(data[:cut])
            m, addr = _guarded(data[:cut])
            assert _parse_at(addr, cut).status == hip.JPEG_MALFORMED, (name, cut)
            m.close()
        assert jpeg_info(data[:ecs])[3]          # the header is complete: the entropy data is the device's to check


def test_garbled_headers_are_errors_or_parse_within_the_buffer():
    rng = np.random.default_rng(7)
    data = _data("422_17x33_q90_opt")
    ecs = parse_headers([data])[0][0].ecs_off
    errors = 0
    for _ in range(400):
        b = bytearray(data[:ecs])
        for _ in range(int(rng.integers(1, 4))):
            b[int(rng.integers(0, ecs))] = int(rng.integers(0, 256))
        m, addr = _guarded(bytes(b))
        im = _parse_at(addr, len(b))
        m.close()
        assert im.status in (hip.JPEG_OK, hip.JPEG_UNSUPPORTED, hip.JPEG_MALFORMED)
        if im.status == hip.JPEG_OK:
            assert 0 < im.ecs_off <= im.ecs_end <= len(b)
            assert all(-1 <= o < len(b) for o in im.huff_off)
        errors += im.status == hip.JPEG_MALFORMED
    assert errors > 0
    for junk in [b"", b"\xff", b"\xff\xd8", b"\xff\xd8\xff", b"\xff\xd8\xff\xc0\x00", b"GIF89a", b"\xff\xd8\xff\xd9"]:
        with pytest.raises(ValueError):
            jpeg_info(junk)


def test_descriptor_layout_matches_header():
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "x3d_hip.h")).read(), flags=re.S)
    for cname, cls in [("x3d_jpeg_image", hip.JpegImage), ("x3d_jpeg_decode_args", hip.JpegDecodeArgs)]:
        body = re.search(r"typedef struct \{([^{}]*)\} " + cname + ";", text).group(1)
        fields = []
        for decl in filter(None, (d.strip() for d in body.split(";"))):
            names = decl.split(",")
            fields.append(names[0].split()[-1])
            fields += [n.strip() for n in names[1:]]
        fields = [re.sub(r"(\[\d+\])+$", "", f).lstrip("*") for f in fields]
        assert fields == [f[0] for f in cls._fields_], cname


def test_reader_mode_is_checked():
    import x3d_tf_amd as x
    from x3d_tf_amd.dataloader import InputReader
    cfg = x.get_config("XS")
    with pytest.raises(ValueError, match="jpeg_decode"):
        InputReader(cfg, True, True, device="cpu", jpeg_decode="gpu")
    with pytest.raises(ValueError, match="use_tfrecord"):
        InputReader(cfg, True, False, device="cpu", jpeg_decode="device")
    assert InputReader(cfg, True, True, device="cpu")._jpeg_decode == "host"
