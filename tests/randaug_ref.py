"""NumPy restatement of the RandAugment ops of x3d_randaug_clips (include/x3d_hip.h) for the tests: integers, plus the stated
fp32 steps of the ImageEnhance blend and the fp64 steps of autocontrast and the contrast mean.  Frames are [H, W, 3] uint8."""
import numpy as np

from x3d_tf_amd import aug

FRAC_BITS = 32


def luma(f):
    v = f.astype(np.int64)
    return (19595 * v[..., 0] + 38470 * v[..., 1] + 7471 * v[..., 2] + 32768) >> 16


def blend(v, d, factor):
    """d + f (v - d): t = fl32(f * fl32(v - d)), r = fl32(d + t); 0 if r <= 0, 255 if r >= 255, else trunc(r)"""
    f = np.float32(factor)
    diff = (np.asarray(v, np.int64) - np.asarray(d, np.int64)).astype(np.float32)
    t = (f * diff).astype(np.float32)
    r = (np.asarray(d, np.int64).astype(np.float32) + t).astype(np.float32)
    return np.where(r <= 0, 0, np.where(r >= 255, 255, np.trunc(r))).astype(np.uint8)


def apply_lut(f, luts):
    return np.stack([np.asarray(luts[c], np.uint8)[f[..., c]] for c in range(3)], axis=-1)


def autocontrast_lut(h):
    nz = np.nonzero(h)[0]
    lo, hi = int(nz[0]), int(nz[-1])
    if hi <= lo:
        return np.arange(256)
    scale = 255.0 / (hi - lo)
    i = np.arange(256, dtype=np.float64)
    return np.clip(np.trunc(i * scale - lo * scale), 0, 255).astype(np.int64)


def equalize_lut(h):
    h = [int(x) for x in h]
    nz = [x for x in h if x]
    if len(nz) < 2:
        return np.arange(256)
    step = (sum(h) - nz[-1]) // 255
    if step == 0:
        return np.arange(256)
    lut, n = [], step // 2
    for i in range(256):
        lut.append(min(255, n // step))
        n += h[i]
    return np.array(lut)


def smooth(f):
    """(sum k v + 6) // 13, k = 1 except 5 at the centre; the one-pixel border copied"""
    v = f.astype(np.int64)
    out = v.copy()
    h, w = f.shape[:2]
    if h >= 3 and w >= 3:
        s = 4 * v[1:-1, 1:-1]
        for dy in range(3):
            for dx in range(3):
                s = s + v[dy:h - 2 + dy, dx:w - 2 + dx]
        out[1:-1, 1:-1] = (s + 6) // 13
    return out


def affine(f, m, fill):
    """m: six fixed-point integers (aug.randaug_fixed_matrix), the half-pixel centres folded in"""
    h, w = f.shape[:2]
    one = 1 << FRAC_BITS
    a, b, c, d, e, ff = (int(k) for k in m)
    yy, xx = np.mgrid[0:h, 0:w].astype(np.int64)
    sx, sy = a * xx + b * yy + c, d * xx + e * yy + ff
    inside = (sx >= 0) & (sy >= 0) & (sx < w * one) & (sy < h * one)
    sx, sy = sx - one // 2, sy - one // 2
    ix, iy = sx >> FRAC_BITS, sy >> FRAC_BITS                      # floor
    fx, fy = ((sx >> (FRAC_BITS - 8)) & 255)[..., None], ((sy >> (FRAC_BITS - 8)) & 255)[..., None]
    x0, x1 = np.clip(ix, 0, w - 1), np.clip(ix + 1, 0, w - 1)
    y0, y1 = np.clip(iy, 0, h - 1), np.clip(iy + 1, 0, h - 1)
    v = f.astype(np.int64)
    top = v[y0, x0] * (256 - fx) + v[y0, x1] * fx
    bot = v[y1, x0] * (256 - fx) + v[y1, x1] * fx
    out = (top * (256 - fy) + bot * fy + 32768) >> 16
    return np.where(inside[..., None], out, np.asarray(fill, np.int64)).astype(np.uint8)


def apply_op(f, op, fill=(0, 0, 0)):
    """one aug.RandAugOp on one frame"""
    name, arg = op.name, op.arg
    i = np.arange(256)
    if name in ("none", "copy"):
        return f.copy()
    if name == "Invert":
        return apply_lut(f, [255 - i] * 3)
    if name == "Solarize":
        return apply_lut(f, [np.where(i < arg, i, 255 - i)] * 3)
    if name == "SolarizeAdd":
        return apply_lut(f, [np.where(i < 128, np.minimum(255, i + arg), i)] * 3)
    if name == "Posterize":
        return apply_lut(f, [i if arg >= 8 else i & ~((1 << (8 - arg)) - 1) & 255] * 3)
    if name == "AutoContrast":
        return apply_lut(f, [autocontrast_lut(np.bincount(f[..., c].ravel(), minlength=256)) for c in range(3)])
    if name == "Equalize":
        return apply_lut(f, [equalize_lut(np.bincount(f[..., c].ravel(), minlength=256)) for c in range(3)])
    if name == "Brightness":
        return blend(f, 0, arg)
    if name == "Color":
        return blend(f, luma(f)[..., None], arg)
    if name == "Contrast":
        d = int(np.trunc(float(int(luma(f).sum())) / float(f.shape[0] * f.shape[1]) + 0.5))
        return blend(f, d, arg)
    if name == "Sharpness":
        return blend(f, smooth(f), arg)
    if name in aug.RANDAUG_GEOMETRIC:
        return affine(f, aug.randaug_fixed_matrix(op, f.shape[0], f.shape[1], FRAC_BITS), fill)
    raise ValueError(name)


def apply_clip(video, ops, t_len, rate=1, start=0, fill=(0, 0, 0)):
    """video [F, H, W, 3] uint8 -> [T, H, W, 3]: frames (start + j * rate) mod F through `ops` in order, frame by frame"""
    frames = [video[(start + j * rate) % video.shape[0]] for j in range(t_len)]
    for op in ops:
        frames = [apply_op(f, op, fill) for f in frames]
    return np.stack(frames)
