"""Eval-side view construction on the GPU: what the reference's eval input pipeline does to one
decoded video before `model(clips, training=False)` -- temporal looping sampler (transforms.py:48-65), short-side
resize to TEST_CROP_SIZE with the cast back to uint8 (:112-147), uniform crop (:149-190), normalisation
(utils.py:42-72) and the [crops][views] clip order the model's view averaging expects (dataloader.py:107-116,
model.py:123-127).  One HIP launch (`x3d_eval_views`); there is no CPU path.

Train-side clip construction (the device half of the training input pipeline -- decoding stays on the
host): `make_train_clip` / `make_train_batch` do what `TemporalTransforms` / `SpatialTransforms` do to one decoded
video in training mode (transforms.py:31-47, 112-147, 199-206, utils.py:42-72), one HIP launch per clip
(`x3d_train_clip`).  `make_train_batch_aug` builds the whole batch with the AUG.* augmentations (aug.py) in one call of
`x3d_train_clips_aug`."""
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


def make_train_batch_aug(videos, cfg, params_list=None, rng: np.random.Generator = None, dtype=torch.float32,
                         out: torch.Tensor = None, rate: int = None) -> torch.Tensor:
    """videos: decoded videos [F_i, H_i, W_i, 3] uint8 on the GPU (contiguous; any mix of extents).  Returns the batch
    [N, T, S, S, 3] with T = cfg.DATA.TEMP_DURATION, S = cfg.DATA.TRAIN_CROP_SIZE: one clip per video with the geometry,
    mirror, colour chain and erase box of its `aug.AugParams` (`params_list`; drawn with `aug.draw_aug_params` from `rng`
    when None), normalised with cfg.DATA.MEAN / STD.  One batched library call: one launch, two when a clip's contrast factor
    is not 1 (include/x3d_hip.h).  `rate` overrides cfg.DATA.FRAME_RATE.  The noise of AUG.RE_MODE "pixel" is keyed per
    clip: an element's value depends on (its clip's `seed`, the clip's index in the batch, the element's index) only."""
    from .aug import draw_aug_params
    from .config import aug_settings
    videos = list(videos)
    if not videos:
        raise ValueError("make_train_batch_aug: empty batch")
    for v in videos:
        if not v.is_cuda or v.dtype != torch.uint8 or not v.is_contiguous():
            raise hip.X3DHipError("make_train_batch_aug needs contiguous uint8 GPU tensors [F, H, W, 3] (no CPU fallback)")
        if v.dim() != 4 or v.shape[-1] != 3:
            raise ValueError(f"expected [F, H, W, 3], got {tuple(v.shape)}")
    shapes = [tuple(int(d) for d in v.shape[:3]) for v in videos]
    if params_list is None:
        if rng is None:
            rng = np.random.default_rng()
        params_list = [draw_aug_params(cfg, f, h, w, rng) for f, h, w in shapes]
    if len(params_list) != len(videos):
        raise ValueError(f"{len(videos)} videos but {len(params_list)} parameter sets")
    n, dev = len(videos), videos[0].device
    t, s = int(cfg.DATA.TEMP_DURATION), int(cfg.DATA.TRAIN_CROP_SIZE)
    if out is None:
        out = torch.empty((n, t, s, s, 3), dtype=dtype, device=dev)
    elif tuple(out.shape) != (n, t, s, s, 3) or not out.is_cuda or not out.is_contiguous():
        raise ValueError(f"out must be a contiguous GPU tensor {(n, t, s, s, 3)}, got {tuple(out.shape)}")
    geom, color = aug_tables(shapes, params_list, cfg)
    addrs = np.array([v.data_ptr() for v in videos], np.int64)
    # one upload for the three tables: [addresses | geom | color]
    host = np.concatenate([addrs.view(np.uint8), geom.reshape(-1).view(np.uint8), color.reshape(-1).view(np.uint8)])
    tables = torch.from_numpy(host).to(dev)
    o_geom = addrs.nbytes
    o_color = o_geom + geom.nbytes
    lib = hip.load()
    scratch = torch.empty((int(lib.x3d_train_clips_aug_scratch(n, t, s)),), dtype=torch.uint8, device=dev)
    mean = (hip._f * 3)(*[float(m) for m in cfg.DATA.MEAN])
    std = (hip._f * 3)(*[float(m) for m in cfg.DATA.STD])
    mode = hip.AUG_ERASE_PIXEL if aug_settings(cfg).re_mode == "pixel" else hip.AUG_ERASE_CONST
    hip.call("x3d_train_clips_aug", tables.data_ptr(), tables.data_ptr() + o_geom, tables.data_ptr() + o_color,
             geom.ctypes.data, color.ctypes.data, out.data_ptr(), scratch.data_ptr(), n, t,
             int(cfg.DATA.FRAME_RATE if rate is None else rate), s, mean, std, mode,
             hip.dtype_code(out.dtype))
    return out
