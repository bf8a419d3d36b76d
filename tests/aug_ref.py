"""fp64 NumPy restatements of the batched training augmentation (include/x3d_hip.h, x3d_train_clips_aug) for the tests:
the random-resized-crop resampling, the colour chain applied op by op, normalisation."""
import numpy as np

GRAY = np.array([0.299, 0.587, 0.114])


def frame_indices(start, rate, t_len, num_frames):
    return [(start + j * rate) % num_frames for j in range(t_len)]


def rrc_clip(video_u8: np.ndarray, box, start: int, rate: int, t_len: int, size: int, flip: bool) -> np.ndarray:
    """video [F, H, W, 3] uint8 -> [T, size, size, 3] float64 on the 0-255 scale: the box resampled with half-pixel-centre
    bilinear weights, source coordinate clamped below at 0, taps clamped to the box; mirrored last."""
    ry0, rx0, rh, rw = box
    crop = video_u8[frame_indices(start, rate, t_len, video_u8.shape[0]), ry0:ry0 + rh, rx0:rx0 + rw].astype(np.float64)

    def taps(n_in):
        src = np.maximum((np.arange(size) + 0.5) * (n_in / size) - 0.5, 0.0)
        i0 = np.minimum(np.floor(src).astype(np.int64), n_in - 1)
        i1 = np.minimum(i0 + 1, n_in - 1)
        return i0, i1, np.minimum(src - i0, 1.0)
    y0, y1, ly = taps(rh)
    x0, x1, lx = taps(rw)
    lx_, ly_ = lx[None, None, :, None], ly[None, :, None, None]
    top = crop[:, y0][:, :, x0] * (1 - lx_) + crop[:, y0][:, :, x1] * lx_
    bot = crop[:, y1][:, :, x0] * (1 - lx_) + crop[:, y1][:, :, x1] * lx_
    out = top * (1 - ly_) + bot * ly_
    return out[:, :, ::-1] if flip else out


def color_chain_sequential(clip: np.ndarray, p) -> np.ndarray:
    """PySlowFast's colour jitter on a clip [T, S, S, 3] (0-255 scale, float64), op by op in p.order, nothing clamped; the
    contrast mean is taken over the whole clip at the moment contrast is applied; grayscale last."""
    x = np.asarray(clip, dtype=np.float64).copy()
    for op in p.order:
        if op == "brightness":
            x = p.brightness * x
        elif op == "contrast":
            m = (x @ GRAY).mean()
            x = p.contrast * x + (1.0 - p.contrast) * m
        elif op == "saturation":
            x = p.saturation * x + (1.0 - p.saturation) * (x @ GRAY)[..., None]
        else:
            raise ValueError(op)
    if p.gray:
        x = np.repeat((x @ GRAY)[..., None], 3, axis=-1)
    return x


def normalize(x: np.ndarray, mean, std) -> np.ndarray:
    return (x / 255.0 - np.asarray(mean, np.float64)) / np.asarray(std, np.float64)


def ulp_half(dtype_name: str) -> float:
    """half an ulp of the storage type relative to the value (round to nearest): 2^-(p+1), p explicit mantissa bits"""
    return {"float32": 2.0 ** -24, "bfloat16": 2.0 ** -8, "float16": 2.0 ** -11}[dtype_name]
