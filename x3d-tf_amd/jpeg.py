"""JPEG frames decoded on the GPU (include/x3d_hip.h: x3d_jpeg_parse / x3d_jpeg_decode, csrc/jpeg.hip).

The TFRecord input pipeline stores every frame of a video as a JPEG string (reference create_tfrecords.py:64-65) and
decodes them with tf.image.decode_jpeg (dataloader.py:80-88); `dataloader.decode_jpeg` does that on the host.  This
module decodes a batch of such strings on the device instead, bit-identical to `decode_jpeg`: the library parses the
headers on the host, then three launches decode every supported frame straight into its uint8 [H, W, 3] slot.

Frames the device decoder does not take (progressive or arithmetic coding, 12-bit samples, CMYK / RGB colour, other
sampling factors, malformed headers) are decoded by `decode_jpeg` on the host, so the result never differs from the
host decode.  That holds for damaged frames too: the device reports X3D_JPEG_CORRUPT, and writes nothing, for
entropy-coded data that is cut short or holds an invalid code or a misplaced restart marker, for a marker left over
behind the last MCU, and for a block whose values leave the IDCT range (dequantised coefficients beyond +-4095, values
between the IDCT passes beyond +-16383, samples before the + 128 outside [-512, 511]), where libjpeg's C and SIMD builds
stop agreeing with each other.  Such a frame raises `JpegDecodeError` naming it (or, with `on_corrupt="host"`, goes to
the host decoder as well, which decodes it its way or reports it as the host path would).  Whatever the device accepts
is what the host decodes from the same bytes.  One difference remains: a frame complete but for its EOI marker decodes
here, while Pillow calls the file truncated."""
import ctypes as C
from typing import List, Sequence, Tuple, Union

import numpy as np
import torch

from . import hip

MAX_PER_LAUNCH = 16384     # images per x3d_jpeg_decode call (the launches index images by grid.y < 65536)


class JpegDecodeError(hip.X3DHipError):
    """entropy-coded data of `frames` is corrupt; `status` holds every frame's X3D_JPEG_* code, `output` what was
    decoded (the slots of the named frames are not written)."""

    def __init__(self, msg: str, frames: List[int], status: List[int], output):
        super().__init__(msg)
        self.frames, self.status, self.output = frames, status, output


def _as_bytes(data) -> bytes:
    return data if isinstance(data, bytes) else bytes(data)


def parse_headers(frames: Sequence[bytes]):
    """x3d_jpeg_parse over `frames` (host only) -> (JpegImage array, scratch bytes the decode of the supported ones needs)"""
    n = len(frames)
    imgs = (hip.JpegImage * max(n, 1))()
    scratch = C.c_longlong(0)
    if n:
        ptrs = (C.c_char_p * n)(*frames)
        lens = (C.c_int * n)(*[len(f) for f in frames])
        hip.check(hip.load().x3d_jpeg_parse(C.cast(ptrs, C.c_void_p), C.cast(lens, C.c_void_p), n, imgs, C.byref(scratch)),
                  "x3d_jpeg_parse")
    return imgs, int(scratch.value)


def jpeg_info(data: bytes) -> Tuple[int, int, int, bool]:
    """(height, width, components, supported by the device decoder) from the header alone; ValueError for a header that
    cannot be parsed (truncated, garbled, not a JPEG)."""
    imgs, _ = parse_headers([_as_bytes(data)])
    im = imgs[0]
    if im.status == hip.JPEG_MALFORMED:
        raise ValueError("not a parseable JPEG header")
    return int(im.height), int(im.width), int(im.ncomp), im.status == hip.JPEG_OK


def _host_decode(data: bytes) -> np.ndarray:
    from .dataloader import decode_jpeg
    return decode_jpeg(data)


def _put(slot: torch.Tensor, arr: np.ndarray, i: int):
    if tuple(slot.shape) != arr.shape:
        raise ValueError(f"frame {i}: decoded shape {arr.shape} does not fit its slot {tuple(slot.shape)}")
    slot.copy_(torch.from_numpy(np.array(arr)))     # PIL's arrays are read-only


def decode_jpeg_batch(frames: Sequence[bytes], device=None, out: Union[None, torch.Tensor, Sequence[torch.Tensor]] = None,
                      on_corrupt: str = "raise"):
    """Decode `frames` (JPEG byte strings) on `device` (default: the current CUDA device), on the current stream.

    out=None: all frames must share one size; returns uint8 [N, H, W, 3].  Otherwise `out` is a uint8 [N, H, W, 3] tensor
    or a list of N contiguous uint8 [H_i, W_i, 3] device tensors (frame slots, e.g. views into per-video buffers), which
    are filled and returned.  Waits for the decode (its status words decide the host fall-backs) but not for other work.
    on_corrupt: "raise" -> JpegDecodeError naming the frames whose entropy-coded data is corrupt (after every other frame
    has been written); "host" -> decode those with the host decoder too."""
    if on_corrupt not in ("raise", "host"):
        raise ValueError(f"on_corrupt must be 'raise' or 'host', not {on_corrupt!r}")
    frames = [_as_bytes(f) for f in frames]
    n = len(frames)
    device = torch.device(device if device is not None else "cuda")
    if device.type != "cuda":
        raise hip.X3DHipError("decode_jpeg_batch decodes on the GPU (no CPU fallback); use dataloader.decode_jpeg")
    imgs, _ = parse_headers(frames)
    host = {i: _host_decode(frames[i]) for i in range(n) if imgs[i].status != hip.JPEG_OK}   # out-of-scope frames
    out_t = None
    if out is None:
        sizes = {(int(imgs[i].height), int(imgs[i].width)) if i not in host else host[i].shape[:2] for i in range(n)}
        if len(sizes) > 1:
            raise ValueError(f"frames of different sizes {sorted(sizes)}: pass out= a list of frame slots")
        h, w = sizes.pop() if sizes else (0, 0)
        out_t = torch.empty((n, h, w, 3), dtype=torch.uint8, device=device)
        slots = list(out_t)
    elif isinstance(out, torch.Tensor):
        out_t = out
        slots = list(out)
    else:
        slots = list(out)
    if len(slots) != n:
        raise ValueError(f"{len(slots)} output slots for {n} frames")
    for i, s in enumerate(slots):
        if not s.is_cuda or s.dtype != torch.uint8 or not s.is_contiguous() or s.dim() != 3 or s.shape[-1] != 3:
            raise hip.X3DHipError(f"frame {i}: the slot must be a contiguous uint8 [H, W, 3] GPU tensor")
        if i not in host and tuple(s.shape) != (imgs[i].height, imgs[i].width, 3):
            raise ValueError(f"frame {i}: {imgs[i].height}x{imgs[i].width} does not fit its slot {tuple(s.shape)}")

    status = [int(imgs[i].status) for i in range(n)]
    for lo in range(0, n, MAX_PER_LAUNCH):
        hi = min(n, lo + MAX_PER_LAUNCH)
        status[lo:hi] = _decode_chunk(frames[lo:hi], slots[lo:hi], device)
    for i, a in host.items():
        _put(slots[i], a, i)
    bad = [i for i in range(n) if status[i] == hip.JPEG_CORRUPT]
    if bad and on_corrupt == "host":
        for i in bad:
            _put(slots[i], _host_decode(frames[i]), i)
    elif bad:
        raise JpegDecodeError(f"corrupt JPEG data in frame(s) {bad[:16]}{' ...' if len(bad) > 16 else ''} "
                              f"of the batch of {n}", bad, status, out_t if out_t is not None else slots)
    return out_t if out_t is not None else slots


def _decode_chunk(frames: List[bytes], slots: List[torch.Tensor], device) -> List[int]:
    n = len(frames)
    imgs, scratch_bytes = parse_headers(frames)
    lens = [len(f) for f in frames]
    offs = np.zeros(n + 1, np.int64)
    np.cumsum(lens, out=offs[1:])
    packed = torch.empty(int(offs[-1]), dtype=torch.uint8, pin_memory=True)
    if n:
        packed.numpy()[:] = np.frombuffer(b"".join(frames), np.uint8)
    for i in range(n):
        im = imgs[i]
        im.data_off, im.data_len = int(offs[i]), lens[i]
        im.out = slots[i].data_ptr() if im.status == hip.JPEG_OK else None
    desc = torch.empty(C.sizeof(hip.JpegImage) * n, dtype=torch.uint8, pin_memory=True)
    C.memmove(desc.data_ptr(), C.addressof(imgs), desc.numel())
    d_data = packed.to(device, non_blocking=True)
    d_desc = desc.to(device, non_blocking=True)
    scratch = torch.empty(max(scratch_bytes, 256), dtype=torch.uint8, device=device)
    status = torch.empty(n, dtype=torch.int32, device=device)
    a = hip.JpegDecodeArgs(d_data.data_ptr(), d_desc.data_ptr(), C.addressof(imgs), n, scratch.data_ptr(), scratch_bytes,
                           status.data_ptr())
    hip.check(hip.load().x3d_jpeg_decode(C.byref(a), hip.stream_ptr()), "x3d_jpeg_decode")
    return status.cpu().tolist()     # synchronises this stream only; the pinned staging buffers are free after it
