"""Eval-side view construction on the GPU: what the reference's eval input pipeline does to one
decoded video before `model(clips, training=False)` -- temporal looping sampler (transforms.py:48-65), short-side
resize to TEST_CROP_SIZE with the cast back to uint8 (:112-147), uniform crop (:149-190), normalisation
(utils.py:42-72) and the [crops][views] clip order the model's view averaging expects (dataloader.py:107-116,
model.py:123-127).  One HIP launch (`x3d_eval_views`); there is no CPU path.

Train-side clip construction (the device half of the training input pipeline -- decoding stays on the
host): `make_train_clip` / `make_train_batch` do what `TemporalTransforms` / `SpatialTransforms` do to one decoded
video in training mode (transforms.py:31-47, 112-147, 199-206, utils.py:42-72), one HIP launch per clip
(`x3d_train_clip`).  `make_train_batch_aug` builds the whole batch with the AUG.* augmentations (aug.py) in one call of
`x3d_train_clips_aug`, after `x3d_randaug_clips` (RandAugment on the uint8 frames) when AUG.AA_TYPE is set."""
import ctypes

import numpy as np
import torch

from . import hip


def num_views(cfg) -> int:
    return int(cfg.TEST.NUM_TEMPORAL_VIEWS) * int(cfg.TEST.NUM_SPATIAL_CROPS)


def make_eval_views(video_u8: torch.Tensor, cfg, dtype=torch.float32, out: torch.Tensor = None) -> torch.Tensor:
    """video_u8: decoded video [F, H, W, 3] uint8 on the GPU (contiguous).
    Returns clips [crops * views, T, S, S, 3] (channels-last) with T = cfg.DATA.TEMP_DURATION,
    S = cfg.DATA.TEST_CROP_SIZE, views = cfg.TEST.NUM_TEMPORAL_VIEWS, crops = cfg.TEST.NUM_SPATIAL_CROPS."""
    if not video_u8.is_cuda or video_u8.dtype != torch.uint8 or not video_u8.is_contiguous():
        raise hip.X3DHipError("make_eval_views needs a contiguous uint8 GPU tensor [F, H, W, 3] (no CPU fallback)")
    if video_u8.dim() != 4 or video_u8.shape[-1] != int(cfg.DATA.NUM_INPUT_CHANNELS) or video_u8.shape[-1] != 3:
        raise ValueError(f"expected [F, H, W, 3], got {tuple(video_u8.shape)}")
    f, h, w, _ = video_u8.shape
    t, s = int(cfg.DATA.TEMP_DURATION), int(cfg.DATA.TEST_CROP_SIZE)
    v, c = int(cfg.TEST.NUM_TEMPORAL_VIEWS), int(cfg.TEST.NUM_SPATIAL_CROPS)
    if out is None:
        out = torch.empty((c * v, t, s, s, 3), dtype=dtype, device=video_u8.device)
    mean = (hip._f * 3)(*[float(m) for m in cfg.DATA.MEAN])
    std = (hip._f * 3)(*[float(m) for m in cfg.DATA.STD])
    a = hip.EvalViewsArgs(video_u8.data_ptr(), out.data_ptr(), f, h, w, t, v, c, s, mean, std, hip.dtype_code(out.dtype))
    hip.call_struct("x3d_eval_views", a)
    return out


# ---- training clips ---------------------------------------------------------------------------------------------
def train_resized_hw(height: int, width: int, jitter: float):
    """Extents after random_short_side_resize with target `jitter` (transforms.py:126-141); computed by the library."""
    nh, nw = ctypes.c_int(0), ctypes.c_int(0)
    hip.check(hip.load().x3d_train_resized_hw(int(height), int(width), float(jitter), ctypes.byref(nh), ctypes.byref(nw)),
              "x3d_train_resized_hw")
    return nh.value, nw.value


def draw_train_params(num_video_frames: int, height: int, width: int, cfg, generator: torch.Generator = None) -> dict:
    """The random draws of one training clip: start ~ U{0..F-1} (transforms.py:33), jitter ~ U[min, max) float32
    (:124), crop offsets uniform over the valid positions of the resized frame (tf.image.random_crop, :199-203).
    Drawn from a torch CPU generator: TF's random streams are not reproduced [TF-3p]."""
    lo, hi = (float(v) for v in cfg.DATA.TRAIN_JITTER_SCALES)
    crop = int(cfg.DATA.TRAIN_CROP_SIZE)
    start = int(torch.randint(0, int(num_video_frames), (1,), generator=generator))
    u = torch.rand((), generator=generator, dtype=torch.float32)
    jitter = float((torch.tensor(lo, dtype=torch.float32) + u * torch.tensor(hi - lo, dtype=torch.float32)).item())
    nh, nw = train_resized_hw(height, width, jitter)
    if nh < crop or nw < crop:
        raise ValueError(f"resized frame {nh}x{nw} is smaller than TRAIN_CROP_SIZE {crop}")
    y0 = int(torch.randint(0, nh - crop + 1, (1,), generator=generator))
    x0 = int(torch.randint(0, nw - crop + 1, (1,), generator=generator))
    return dict(start=start, jitter=jitter, y0=y0, x0=x0, flip=True)   # flip: every training clip (transforms.py:205-206)


def make_train_clip(video_u8: torch.Tensor, cfg, params: dict = None, generator: torch.Generator = None,
                    dtype=torch.float32, out: torch.Tensor = None, rate: int = None) -> torch.Tensor:
    """video_u8: decoded video [F, H, W, 3] uint8 on the GPU (contiguous).  Returns one clip [T, S, S, 3]
    (channels-last) with T = cfg.DATA.TEMP_DURATION, S = cfg.DATA.TRAIN_CROP_SIZE, every cfg.DATA.FRAME_RATE-th frame
    from a random start, the video looped.  `params` (see draw_train_params) fixes the random draws.  `rate` overrides
    cfg.DATA.FRAME_RATE (a video holding just the clip's frames is read with start = 0, rate = 1)."""
    if not video_u8.is_cuda or video_u8.dtype != torch.uint8 or not video_u8.is_contiguous():
        raise hip.X3DHipError("make_train_clip needs a contiguous uint8 GPU tensor [F, H, W, 3] (no CPU fallback)")
    if video_u8.dim() != 4 or video_u8.shape[-1] != 3:
        raise ValueError(f"expected [F, H, W, 3], got {tuple(video_u8.shape)}")
    f, h, w, _ = video_u8.shape
    if params is None:
        params = draw_train_params(f, h, w, cfg, generator)
    t, s = int(cfg.DATA.TEMP_DURATION), int(cfg.DATA.TRAIN_CROP_SIZE)
    if out is None:
        out = torch.empty((t, s, s, 3), dtype=dtype, device=video_u8.device)
    mean = (hip._f * 3)(*[float(m) for m in cfg.DATA.MEAN])
    std = (hip._f * 3)(*[float(m) for m in cfg.DATA.STD])
    a = hip.TrainClipArgs(video_u8.data_ptr(), out.data_ptr(), f, h, w, t, int(cfg.DATA.FRAME_RATE if rate is None else rate), int(params["start"]),
                          float(params["jitter"]), s, int(params["y0"]), int(params["x0"]), 1 if params.get("flip", True) else 0,
                          mean, std, hip.dtype_code(out.dtype))
    hip.call_struct("x3d_train_clip", a)
    return out


def make_train_batch(videos, cfg, generator: torch.Generator = None, dtype=torch.float32) -> torch.Tensor:
    """One augmented clip per decoded video -> [B, T, S, S, 3], the tensor `Trainer.step` takes (dataloader.py:96-104)."""
    t, s = int(cfg.DATA.TEMP_DURATION), int(cfg.DATA.TRAIN_CROP_SIZE)
    if not videos:
        raise ValueError("make_train_batch: empty batch")
    out = torch.empty((len(videos), t, s, s, 3), dtype=dtype, device=videos[0].device)
    for i, v in enumerate(videos):
        make_train_clip(v, cfg, generator=generator, dtype=dtype, out=out[i])
    return out


# ---- batched, augmented training clips (AUG.*) ----------------------------------------------------------------------
def aug_tables(shapes, params_list, cfg):
    """The host tables of x3d_train_clips_aug for clips with `params_list` (aug.AugParams) from videos of `shapes` (F, H, W):
    (geom int32 [N, AUG_GEOM_COLS], color float32 [N, AUG_COLOR_COLS]), columns as include/x3d_hip.h names them."""
    from .aug import fold_color
    n = len(params_list)
    geom = np.zeros((n, hip.AUG_GEOM_COLS), np.int32)
    color = np.zeros((n, hip.AUG_COLOR_COLS), np.float32)
    G = hip.AUG_G
    for i, ((f, h, w), p) in enumerate(zip(shapes, params_list)):
        g = geom[i]
        g[G["F"]], g[G["H"]], g[G["W"]], g[G["START"]], g[G["FLIP"]] = f, h, w, p.start, 1 if p.flip else 0
        if p.crop == "jitter":
            g[G["MODE"]] = hip.AUG_CROP_JITTER
            g[G["NH"]], g[G["NW"]] = train_resized_hw(h, w, p.jitter)
            g[G["Y0"]], g[G["X0"]] = p.y0, p.x0
        elif p.crop == "rrc":
            g[G["MODE"]] = hip.AUG_CROP_RRC
            g[G["Y0"]], g[G["X0"]], g[G["BH"]], g[G["BW"]] = p.box
        else:
            raise ValueError(f"unknown crop mode {p.crop!r}")
        g[G["EY0"]], g[G["EY1"]], g[G["EX0"]], g[G["EX1"]] = p.erase
        seed = int(p.seed) & 0xFFFFFFFFFFFFFFFF
        g[G["SEED_LO"]], g[G["SEED_HI"]] = np.array([seed & 0xFFFFFFFF, seed >> 32], np.uint32).view(np.int32)
        m, k = fold_color(p)
        color[i, :9] = m.reshape(9)
        color[i, hip.AUG_C_K] = k
    return geom, color


# ---- RandAugment on the uint8 frames (AUG.AA_TYPE) --------------------------------------------------------------------
def randaug_fill(cfg):
    """the fill colour of the geometric ops: round(255 * DATA.MEAN[c])"""
    return tuple(min(max(int(round(255.0 * float(m))), 0), 255) for m in cfg.DATA.MEAN)


def randaug_tables(shapes, starts, randaug_list, t: int, rate: int):
    """The host tables of x3d_randaug_clips for clips with the ops `randaug_list` (one tuple of aug.RandAugOp per clip) read
    from videos of `shapes` (F, H, W) at `starts`: (clips int32 [N, RA_CLIP_COLS], ops int32 [N, L, RA_OP_COLS],
    xform int64 [N, L, RA_X_COLS], work_bytes, result) -- columns as include/x3d_hip.h names them, L the longest op tuple
    (at least 1).  An op keeps its layer; "none" layers are X3D_RA_NONE.  Each clip ping-pongs between two 16-byte-aligned
    ranges of its own in the work area (one when a single layer touches it); the first layer that touches it reads the video
    (SRC = -1).  A clip without an applied op is copied by the gather (X3D_RA_COPY in layer 0) unless its video already is
    its T sampled frames, in which case nothing touches it.  result[i]: offset of clip i's frames in the work area, None for
    an untouched clip."""
    from .aug import RANDAUG_ENHANCE, RANDAUG_GEOMETRIC, randaug_fixed_matrix
    n = len(shapes)
    layers = max([len(r) for r in randaug_list] + [1])
    clips = np.zeros((n, hip.RA_CLIP_COLS), np.int32)
    ops = np.zeros((n, layers, hip.RA_OP_COLS), np.int32)
    xform = np.zeros((n, layers, hip.RA_X_COLS), np.int64)
    result, top = [], 0
    for i, ((f, h, w), start, ra) in enumerate(zip(shapes, starts, randaug_list)):
        clips[i] = (f, h, w, start)
        todo = [(l, op) for l, op in enumerate(ra) if op.name != "none"]
        if not todo and [(start + j * rate) % f for j in range(t)] != list(range(t)):
            from .aug import RandAugOp
            todo = [(0, RandAugOp("copy", None))]
        size = (t * h * w * 3 + 15) // 16 * 16
        bufs = [top, top + size]
        top += size * min(len(todo), 2)
        src = -1
        for k, (l, op) in enumerate(todo):
            if op.name not in hip.RA_OPS:
                raise ValueError(f"unknown RandAugment op {op.name!r}")
            ops[i, l, hip.RA_O_OP] = hip.RA_OPS[op.name]
            if op.name in RANDAUG_ENHANCE:
                ops[i, l, hip.RA_O_FARG] = np.array([op.arg], np.float32).view(np.int32)[0]
            elif op.name in RANDAUG_GEOMETRIC:
                xform[i, l, hip.RA_X_A:hip.RA_X_A + 6] = randaug_fixed_matrix(op, h, w, hip.RA_FRAC_BITS)
            elif op.arg is not None:
                ops[i, l, hip.RA_O_IARG] = int(op.arg)
            xform[i, l, hip.RA_X_SRC], xform[i, l, hip.RA_X_DST] = src, bufs[k % 2]
            src = bufs[k % 2]
        result.append(src if todo else None)
    return clips, ops, xform, top, result


def _check_videos(what, videos):
    for v in videos:
        if not v.is_cuda or v.dtype != torch.uint8 or not v.is_contiguous():
            raise hip.X3DHipError(f"{what} needs contiguous uint8 GPU tensors [F, H, W, 3] (no CPU fallback)")
        if v.dim() != 4 or v.shape[-1] != 3:
            raise ValueError(f"expected [F, H, W, 3], got {tuple(v.shape)}")


def randaug_clips(videos, randaug_list, t: int, rate: int, starts, fill, extra=()):
    """x3d_randaug_clips on `videos` (uint8 GPU tensors [F_i, H_i, W_i, 3]): clip i = frames (starts[i] + j * rate) mod F_i,
    j < t, sent through randaug_list[i].  Returns (frames, tables, offsets): frames[i] the uint8 tensor [t, H_i, W_i, 3] of
    clip i -- a view of the call's work area, or videos[i] itself for an untouched clip (randaug_tables).  `extra`: a function
    (frames) -> list of uint8 host arrays uploaded behind the call's own tables in the same copy (make_train_batch_aug's);
    tables is then the device tensor and offsets[k] where extra array k starts in it."""
    videos = list(videos)
    n, dev = len(videos), videos[0].device
    shapes = [tuple(int(d) for d in v.shape[:3]) for v in videos]
    clips, ops, xform, work_bytes, result = randaug_tables(shapes, starts, randaug_list, t, rate)
    work = torch.empty((max(work_bytes, 16),), dtype=torch.uint8, device=dev)
    frames = [v if off is None else work[off:off + t * h * w * 3].view(t, h, w, 3)
              for v, off, (_, h, w) in zip(videos, result, shapes)]
    addrs = np.array([v.data_ptr() for v in videos], np.int64)
    parts = [addrs.view(np.uint8), xform.reshape(-1).view(np.uint8), clips.reshape(-1).view(np.uint8),
             ops.reshape(-1).view(np.uint8)] + [np.ascontiguousarray(e).reshape(-1).view(np.uint8) for e in (extra(frames) if extra else [])]
    starts_, pos = [], 0
    for k, p in enumerate(parts):         # the int64 tables lead; everything behind them is padded to 8 bytes
        pos = (pos + 7) // 8 * 8
        starts_.append(pos)
        pos += p.nbytes
    host = np.zeros((pos,), np.uint8)
    for o, p in zip(starts_, parts):
        host[o:o + p.nbytes] = p
    tables = torch.from_numpy(host).to(dev)
    if work_bytes:
        lib = hip.load()
        scratch = torch.empty((int(lib.x3d_randaug_scratch(n, t)),), dtype=torch.uint8, device=dev)
        base = tables.data_ptr()
        hip.call("x3d_randaug_clips", base + starts_[0], base + starts_[2], base + starts_[3], base + starts_[1],
                 clips.ctypes.data, ops.ctypes.data, xform.ctypes.data, work.data_ptr(), work.numel(), scratch.data_ptr(),
                 n, int(t), int(rate), int(ops.shape[1]), int(fill[0]), int(fill[1]), int(fill[2]))
    return frames, tables, starts_[4:]


def make_train_batch_aug(videos, cfg, params_list=None, rng: np.random.Generator = None, dtype=torch.float32,
                         out: torch.Tensor = None, rate: int = None, randaug_list=None) -> torch.Tensor:
    """videos: decoded videos [F_i, H_i, W_i, 3] uint8 on the GPU (contiguous; any mix of extents).  Returns the batch
    [N, T, S, S, 3] with T = cfg.DATA.TEMP_DURATION, S = cfg.DATA.TRAIN_CROP_SIZE: one clip per video with the geometry,
    mirror, colour chain and erase box of its `aug.AugParams` (`params_list`; drawn with `aug.draw_aug_params` from `rng`
    when None), normalised with cfg.DATA.MEAN / STD.  One batched library call: one launch, two when a clip's contrast factor
    is not 1 (include/x3d_hip.h).  `rate` overrides cfg.DATA.FRAME_RATE.  The noise of AUG.RE_MODE "pixel" is keyed per
    clip: an element's value depends on (its clip's `seed`, the clip's index in the batch, the element's index) only.

    RandAugment: `randaug_list` (one tuple of aug.RandAugOp per clip; when None and AUG.AA_TYPE is set, drawn with
    `aug.draw_randaug` from `rng` after all the AugParams) runs first, on the uint8 frames the clips sample
    (x3d_randaug_clips, its tables in the same upload); x3d_train_clips_aug then reads each clip's result as a video of T
    frames with start = 0, rate = 1.  With randaug_list None and AA_TYPE "" the calls are exactly those described above."""
    from .aug import draw_aug_params, draw_randaug
    from .config import aug_settings, randaug_settings
    videos = list(videos)
    if not videos:
        raise ValueError("make_train_batch_aug: empty batch")
    _check_videos("make_train_batch_aug", videos)
    shapes = [tuple(int(d) for d in v.shape[:3]) for v in videos]
    if params_list is None:
        if rng is None:
            rng = np.random.default_rng()
        params_list = [draw_aug_params(cfg, f, h, w, rng) for f, h, w in shapes]
    if len(params_list) != len(videos):
        raise ValueError(f"{len(videos)} videos but {len(params_list)} parameter sets")
    if randaug_list is None:
        spec = randaug_settings(cfg)
        if spec is not None:
            if rng is None:
                rng = np.random.default_rng()
            randaug_list = [draw_randaug(spec, h, w, rng) for _, h, w in shapes]
    elif len(randaug_list) != len(videos):
        raise ValueError(f"{len(videos)} videos but {len(randaug_list)} RandAugment op tuples")
    n, dev = len(videos), videos[0].device
    t, s = int(cfg.DATA.TEMP_DURATION), int(cfg.DATA.TRAIN_CROP_SIZE)
    rate = int(cfg.DATA.FRAME_RATE if rate is None else rate)
    if out is None:
        out = torch.empty((n, t, s, s, 3), dtype=dtype, device=dev)
    elif tuple(out.shape) != (n, t, s, s, 3) or not out.is_cuda or not out.is_contiguous():
        raise ValueError(f"out must be a contiguous GPU tensor {(n, t, s, s, 3)}, got {tuple(out.shape)}")
    if randaug_list is not None:
        # the draws were made for the whole video (start, crop); the clip's frames are now frames 0..T-1 of the result
        geom, color = aug_tables([(t, h, w) for _, h, w in shapes], [p._replace(start=0) for p in params_list], cfg)
        frames, tables, (o_addrs, o_geom, o_color) = randaug_clips(
            videos, randaug_list, t, rate, [p.start for p in params_list], randaug_fill(cfg),
            extra=lambda fr: [np.array([v.data_ptr() for v in fr], np.int64), geom, color])
        rate = 1
    else:
        geom, color = aug_tables(shapes, params_list, cfg)
        addrs = np.array([v.data_ptr() for v in videos], np.int64)
        # one upload for the three tables: [addresses | geom | color]
        host = np.concatenate([addrs.view(np.uint8), geom.reshape(-1).view(np.uint8), color.reshape(-1).view(np.uint8)])
        tables = torch.from_numpy(host).to(dev)
        o_addrs, o_geom = 0, addrs.nbytes
        o_color = o_geom + geom.nbytes
    lib = hip.load()
    scratch = torch.empty((int(lib.x3d_train_clips_aug_scratch(n, t, s)),), dtype=torch.uint8, device=dev)
    mean = (hip._f * 3)(*[float(m) for m in cfg.DATA.MEAN])
    std = (hip._f * 3)(*[float(m) for m in cfg.DATA.STD])
    mode = hip.AUG_ERASE_PIXEL if aug_settings(cfg).re_mode == "pixel" else hip.AUG_ERASE_CONST
    hip.call("x3d_train_clips_aug", tables.data_ptr() + o_addrs, tables.data_ptr() + o_geom, tables.data_ptr() + o_color,
             geom.ctypes.data, color.ctypes.data, out.data_ptr(), scratch.data_ptr(), n, t, rate, s, mean, std, mode,
             hip.dtype_code(out.dtype))
    return out
