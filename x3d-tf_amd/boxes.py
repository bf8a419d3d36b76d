"""Person boxes through the crops of the input pipeline (action detection; the clips are built by x3d_train_clips_aug,
x3d_train_clip and x3d_eval_views, the boxes are mapped here, on the host: N * K * 4 numbers per batch, and the model takes
`boxes` / `num_boxes` from the host anyway).

Convention: a box is (x1, y1, x2, y2) in pixels, pixel i covers [i, i + 1) and its centre is i + 0.5 -- the ROI head's (aligned
ROIAlign samples at x * scale - 0.5).  All arithmetic is fp64; `clip_and_pack` casts to fp32 as its last step.

Where the maps come from.  Every kernel samples with half-pixel centres: output pixel (y', x') of a resized frame reads the source
at  fx = (rx + 0.5) * W / nw - 0.5  (csrc/views.hip eval_views_kernel, csrc/aug.hip aug_geom_px), rx = x' + x0 the column in the
resized frame.  In edge coordinates (centre + 0.5 on both sides) that is  x_src = (x' + x0) * W / nw  with no constant left over,
so the map of an edge is exactly linear:

    short-side resize + crop      x' = x * nw / W - x0          y' = y * nh / H - y0
    random-resized crop           x' = (x - rx0) * S / rw       y' = (y - ry0) * S / rh      (fx = (x' + 0.5) * rw / S - 0.5 inside
                                                                                             the box, whose corner is (ry0, rx0))
    mirror, after either          (x1', x2') -> (S - x2', S - x1')                            (the kernels read column S - 1 - x')

Colour, grayscale and random erasing move no box.  Each rule is written once below."""
import numpy as np


def _as_boxes(boxes) -> np.ndarray:
    return np.array(boxes, dtype=np.float64).reshape(-1, 4)


def resize_crop(boxes, height: int, width: int, nh: int, nw: int, y0: int, x0: int) -> np.ndarray:
    """boxes of an H x W frame -> the frame resized to nh x nw and cropped at origin (y0, x0)"""
    b = _as_boxes(boxes)
    sx, sy = float(nw) / float(width), float(nh) / float(height)
    return np.stack([b[:, 0] * sx - x0, b[:, 1] * sy - y0, b[:, 2] * sx - x0, b[:, 3] * sy - y0], 1)


def resized_crop(boxes, box, size: int) -> np.ndarray:
    """boxes of the source frame -> the crop `box` = (ry0, rx0, rh, rw) resized to size x size"""
    b = _as_boxes(boxes)
    ry0, rx0, rh, rw = (float(v) for v in box)
    sx, sy = float(size) / rw, float(size) / rh
    return np.stack([(b[:, 0] - rx0) * sx, (b[:, 1] - ry0) * sy, (b[:, 2] - rx0) * sx, (b[:, 3] - ry0) * sy], 1)


def mirror(boxes, size: int) -> np.ndarray:
    """left-right mirror of a size-wide crop"""
    b = _as_boxes(boxes)
    return np.stack([size - b[:, 2], b[:, 1], size - b[:, 0], b[:, 3]], 1)


def eval_geometry(height: int, width: int, size: int):
    """(nh, nw, y0, x0) of x3d_eval_views' centre crop (csrc/views.hip: sidx == 1, the only one with one crop): the short side is
    resized to `size` -- the library's own arithmetic, `views.train_resized_hw` with the target `size` -- and the crop origin is
    yoff[1] = (nh - size + 1) / 2, xoff[1] = (nw - size + 1) / 2 in integers: ceil((n - size) / 2)."""
    from .views import train_resized_hw
    nh, nw = train_resized_hw(height, width, float(size))
    return nh, nw, (nh - size + 1) // 2, (nw - size + 1) // 2


def boxes_through_train(boxes, height: int, width: int, params: dict, size: int) -> np.ndarray:
    """boxes of an H x W video -> the clip x3d_train_clip builds with `params` (views.draw_train_params: jitter, y0, x0, flip)"""
    from .views import train_resized_hw
    nh, nw = train_resized_hw(height, width, params["jitter"])
    out = resize_crop(boxes, height, width, nh, nw, int(params["y0"]), int(params["x0"]))
    return mirror(out, size) if params.get("flip", True) else out


def boxes_through_aug(boxes, height: int, width: int, params, size: int) -> np.ndarray:
    """boxes of an H x W video -> the clip x3d_train_clips_aug builds with `params` (aug.AugParams: crop "jitter" | "rrc", flip;
    its colour chain and erase box move nothing)"""
    if params.crop == "jitter":
        from .views import train_resized_hw
        nh, nw = train_resized_hw(height, width, params.jitter)
        out = resize_crop(boxes, height, width, nh, nw, int(params.y0), int(params.x0))
    elif params.crop == "rrc":
        out = resized_crop(boxes, params.box, size)
    else:
        raise ValueError(f"unknown crop mode {params.crop!r}")
    return mirror(out, size) if params.flip else out


def boxes_through_eval(boxes, height: int, width: int, size: int) -> np.ndarray:
    """boxes of an H x W video -> the single centre-crop view of x3d_eval_views (size = DATA.TEST_CROP_SIZE)"""
    nh, nw, y0, x0 = eval_geometry(height, width, size)
    return resize_crop(boxes, height, width, nh, nw, y0, x0)


def clip_and_pack(boxes, labels, size: int, max_boxes: int, min_size: float = 1.0, stats: dict = None):
    """Mapped boxes [n, 4] (+ their label rows [n, classes], or None) -> the fixed slots of one clip.  Every coordinate is clamped
    to [0, size]; a box whose clamped width or height is below `min_size` pixels, or that has a non-finite coordinate, is dropped
    (a filled slot with a degenerate box would pool zeros and still count in the loss); the survivors keep their order and fill
    the first slots, the empty slots are zero.  More than `max_boxes` survivors: the first `max_boxes` stay, the rest are counted
    in stats["boxes_dropped"] (`stats` given).  Returns (boxes fp32 [max_boxes, 4], labels [max_boxes, classes] in the dtype of
    `labels` or None, num_boxes, the kept indices into the input)."""
    b = _as_boxes(boxes)
    k = int(max_boxes)
    finite = np.isfinite(b).all(axis=1)
    c = np.clip(np.where(finite[:, None], b, 0.0), 0.0, float(size))
    keep = finite & (c[:, 2] - c[:, 0] >= min_size) & (c[:, 3] - c[:, 1] >= min_size)
    kept = np.nonzero(keep)[0]
    if len(kept) > k:
        if stats is not None:
            stats["boxes_dropped"] = stats.get("boxes_dropped", 0) + len(kept) - k
        kept = kept[:k]
    out = np.zeros((k, 4), np.float32)
    out[:len(kept)] = c[kept].astype(np.float32)          # the cast is the last step
    packed = None
    if labels is not None:
        lab = np.asarray(labels)
        if lab.ndim != 2 or lab.shape[0] != b.shape[0]:
            raise ValueError(f"labels must be [{b.shape[0]}, classes] for {b.shape[0]} boxes, got {lab.shape}")
        packed = np.zeros((k, lab.shape[1]), lab.dtype)
        packed[:len(kept)] = lab[kept]
    return out, packed, int(len(kept)), kept
