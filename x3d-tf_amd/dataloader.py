"""Host half of the input pipeline: the reference's ``dataloader.InputReader`` (reference
dataloader.py:11-197) and the record format of ``datasets/create_tfrecords.py`` (:48-141), without TensorFlow.

What the reference does                                             here
-----------------------------------------------------------------   ---------------------------------------------------
GZIP TFRecord files of tf.train.SequenceExample, one per video:     `read_tfrecords` (length | masked CRC32C | bytes |
  context video/num_frames, video/class/label (int64), feature        masked CRC32C, gzip stream), `parse_sequence_example`
  list `video` = one JPEG string per frame (create_tfrecords.py:      (protobuf wire format restated), `decode_jpeg` (PIL /
  48-82, dataloader.py:63-88: tf.image.decode_jpeg)                   libjpeg; tf.image.decode_jpeg's DCT method is [TF-3p])
text file of "<path> <label>" lines decoded with decord             `decode_video`: needs a `decoder` callable (decord is
  (dataloader.py:29-61), undecodable video -> zeros [100,240,144,3]    not installed here); the zeros replacement is kept
list_files(shuffle) -> interleave -> shuffle(16 * batch | 1024)     `InputReader.__call__`: the same stages as Python
  -> decode -> repeat (train) -> temporal + spatial transforms         generators, decode on a thread pool, the transforms on
  -> batch(drop_remainder) -> process_batch -> prefetch               the GPU (views.py: x3d_train_clip / x3d_eval_views),
  (dataloader.py:126-197)                                             batches prefetched by a background thread
`create_tfrecords.to_tf_example` / TFRecordWriter (GZIP, level 9)    `make_sequence_example`, `write_tfrecords`

The decoded video goes to the GPU as uint8 [F, H, W, 3]; everything after decoding is the device half (views.py).  The
order of a shuffled training stream is this module's own (seeded torch/NumPy generators): TF's is not reproducible [TF-3p].
"""
import glob
import gzip
import io
import queue
import struct
import threading
import warnings
from concurrent.futures import ThreadPoolExecutor
from typing import Callable, Dict, Iterable, Iterator, List, Optional, Sequence, Tuple, Union

import numpy as np
import torch

from .checkpoint import _get_varint, _parse_proto, _put_varint, crc32c, mask_crc

FAILED_VIDEO_SHAPE = (100, 240, 144, 3)   # dataloader.py:58-61: what an undecodable video is replaced with


# ------------------------------------------------------------------------------------------------
# TFRecord framing (tensorflow/core/lib/io/record_writer.cc) [TF-3p]:
#   uint64 length | uint32 masked_crc32c(length) | byte data[length] | uint32 masked_crc32c(data)
# ------------------------------------------------------------------------------------------------
def read_tfrecords(path: str, compression: str = "GZIP", verify: bool = True) -> Iterator[bytes]:
    """Yield the raw records of one TFRecord file (dataloader.py:150-153: compression_type="GZIP")."""
    opener = gzip.open if compression == "GZIP" else open
    with opener(path, "rb") as f:
        while True:
            head = f.read(12)
            if not head:
                return
            if len(head) < 12:
                raise ValueError(f"{path}: truncated record header")
            (length,), (lcrc,) = struct.unpack("<Q", head[:8]), struct.unpack("<I", head[8:])
            if verify and mask_crc(crc32c(head[:8])) != lcrc:
                raise ValueError(f"{path}: corrupted record length")
            data = f.read(length)
            tail = f.read(4)
            if len(data) < length or len(tail) < 4:
                raise ValueError(f"{path}: truncated record")
            if verify and mask_crc(crc32c(data)) != struct.unpack("<I", tail)[0]:
                raise ValueError(f"{path}: corrupted record data")
            yield data


def write_tfrecords(path: str, records: Iterable[bytes], compression: str = "GZIP", level: int = 9) -> int:
    """create_tfrecords.py:103-107: tf.io.TFRecordWriter(path, TFRecordOptions("GZIP", compression_level=9))."""
    opener = (lambda p: gzip.open(p, "wb", compresslevel=level)) if compression == "GZIP" else (lambda p: open(p, "wb"))
    n = 0
    with opener(path) as f:
        for rec in records:
            head = struct.pack("<Q", len(rec))
            f.write(head + struct.pack("<I", mask_crc(crc32c(head))) + rec + struct.pack("<I", mask_crc(crc32c(rec))))
            n += 1
    return n


# ------------------------------------------------------------------------------------------------
# tf.train.SequenceExample (tensorflow/core/example/{example,feature}.proto) [TF-3p]
#   SequenceExample { Features context = 1; FeatureLists feature_lists = 2; }
#   Features     { map<string, Feature> feature = 1; }          (map entry: key = 1, value = 2)
#   FeatureLists { map<string, FeatureList> feature_list = 1; }  FeatureList { repeated Feature feature = 1; }
#   Feature { oneof { BytesList bytes_list = 1; FloatList float_list = 2; Int64List int64_list = 3; } }
#   BytesList { repeated bytes value = 1; }   Int64List { repeated int64 value = 1 [packed]; }
# ------------------------------------------------------------------------------------------------
def _len(field: int, payload: bytes) -> bytes:
    return _put_varint((field << 3) | 2) + _put_varint(len(payload)) + payload


def _int64_feature(v: int) -> bytes:
    return _len(3, _len(1, _put_varint(v & 0xFFFFFFFFFFFFFFFF)))


def _int64_list_feature(vs: Sequence[int]) -> bytes:
    """Int64List of any length (packed; an empty list has no value field)"""
    packed = b"".join(_put_varint(int(v) & 0xFFFFFFFFFFFFFFFF) for v in vs)
    return _len(3, _len(1, packed) if vs else b"")


def _bytes_feature(b: bytes) -> bytes:
    return _len(1, _len(1, b))


def _map_entry(key: str, value: bytes) -> bytes:
    return _len(1, _len(1, key.encode()) + _len(2, value))


def encode_jpeg(frame_u8: np.ndarray, quality: int = 90) -> bytes:
    """create_tfrecords.py:64-65: tf.image.encode_jpeg(frame, format='rgb', quality=90, optimize_size=True)."""
    from PIL import Image
    buf = io.BytesIO()
    Image.fromarray(np.ascontiguousarray(frame_u8), "RGB").save(buf, format="JPEG", quality=quality, optimize=True)
    return buf.getvalue()


def decode_jpeg(data: bytes) -> np.ndarray:
    """dataloader.py:85: tf.image.decode_jpeg -> uint8 [H, W, 3]."""
    from PIL import Image
    with Image.open(io.BytesIO(data)) as im:
        return np.asarray(im.convert("RGB"), dtype=np.uint8)


def make_sequence_example(frames_u8: np.ndarray, class_id: Union[int, Sequence[int]], quality: int = 90,
                          encoded: Optional[List[bytes]] = None) -> bytes:
    """create_tfrecords.py:48-82 `to_tf_example`: frames [F, H, W, 3] uint8 + label -> serialized SequenceExample
    (`encoded`: already JPEG-encoded frames instead of `frames_u8`).  `class_id` may be a sequence of class ids (a
    multi-label video, any number of them): they are written as one int64 list under video/class/label."""
    jpegs = encoded if encoded is not None else [encode_jpeg(f, quality) for f in frames_u8]
    if isinstance(class_id, (int, np.integer)):
        label = _int64_feature(int(class_id))
    else:
        label = _int64_list_feature([int(c) for c in class_id])
    context = _map_entry("video/num_frames", _int64_feature(len(jpegs))) + _map_entry("video/class/label", label)
    flist = b"".join(_len(1, _bytes_feature(j)) for j in jpegs)
    return _len(1, context) + _len(2, _map_entry("video", flist))


def _int64_list(feature: bytes) -> List[int]:
    f = _parse_proto(feature)
    out: List[int] = []
    for lst in f.get(3, []):
        for v in _parse_proto(lst).get(1, []):
            if isinstance(v, (bytes, bytearray)):        # packed
                pos = 0
                while pos < len(v):
                    x, pos = _get_varint(v, pos)
                    out.append(x)
            else:
                out.append(v)
    return [x - (1 << 64) if x >= (1 << 63) else x for x in out]


def parse_sequence_example(buf: bytes) -> Tuple[List[bytes], int, int]:
    """dataloader.py:63-88 `parse_and_decode` up to the JPEG decode: -> (JPEG strings of the frames, num_frames, label);
    absent context features default to -1 as FixedLenFeature([], tf.int64, -1) does.  Of a multi-label record this is
    the first label (parse_sequence_example_labels returns them all)."""
    frames, nf, lb = parse_sequence_example_labels(buf)
    return frames, nf, (lb[0] if lb else -1)


def parse_sequence_example_labels(buf: bytes) -> Tuple[List[bytes], int, List[int]]:
    """parse_sequence_example with every label: -> (JPEG strings of the frames, num_frames, the video/class/label list,
    empty when absent)."""
    top = _parse_proto(buf)
    ctx: Dict[str, bytes] = {}
    for feats in top.get(1, []):
        for entry in _parse_proto(feats).get(1, []):
            e = _parse_proto(entry)
            ctx[e[1][0].decode()] = e[2][0]
    nf = _int64_list(ctx["video/num_frames"]) if "video/num_frames" in ctx else []
    lb = _int64_list(ctx["video/class/label"]) if "video/class/label" in ctx else []
    frames: List[bytes] = []
    for fl in top.get(2, []):
        for entry in _parse_proto(fl).get(1, []):
            e = _parse_proto(entry)
            if e[1][0].decode() != "video":
                continue
            for feat in _parse_proto(e[2][0]).get(1, []):
                for bl in _parse_proto(feat).get(1, []):
                    frames += _parse_proto(bl).get(1, [])
    return frames, (nf[0] if nf else -1), lb


def parse_label_list(field: str) -> List[int]:
    """The label field of a multi-label text line, "<l1>,<l2>,..." -> [l1, l2, ...] ("" -> [])."""
    return [int(x) for x in field.split(",") if x.strip()]


def multi_hot(label_lists: Sequence[Sequence[int]], num_classes: int, names: Optional[Sequence[str]] = None) -> torch.Tensor:
    """[len(label_lists), num_classes] fp32 multi-hot targets on the host; a class id outside [0, num_classes) raises
    ValueError naming its record (`names`)."""
    t = torch.zeros((len(label_lists), num_classes), dtype=torch.float32)
    for i, lbs in enumerate(label_lists):
        for c in lbs:
            if not 0 <= int(c) < num_classes:
                who = names[i] if names is not None else f"#{i}"
                raise ValueError(f"record {who}: class id {c} outside [0, {num_classes})")
            t[i, int(c)] = 1.0
    return t


def _named_records(path: str, records: Iterator[bytes]) -> Iterator[Tuple[str, bytes]]:
    """("<path>#<index in the file>", record) for every record of one file"""
    for i, r in enumerate(records):
        yield f"{path}#{i}", r


def _label_of(labels: List[int], all_labels: bool):
    """the label of a record: the first (-1 without one), or the whole list"""
    return list(labels) if all_labels else int(labels[0] if labels else -1)


# ------------------------------------------------------------------------------------------------
class InputReader:
    """reference dataloader.py:11-27.  `reader(file_pattern, batch_size)` iterates over (clips, labels) batches on the GPU:
    training [B, T, S, S, 3] / [B]; evaluation [B * views * crops, T, S, S, 3] / [B] (dataloader.py:90-116).

    Additional arguments (the reference gets them from TF's globals): `device`, `dtype` (the compute type clips are cast
    to under mixed precision, dataloader.py:111-113), `seed`, `decoder` (path -> uint8 [F, H, W, 3] array for the
    non-TFRecord path), `num_workers` (decode threads), `prefetch` (batches kept ready).

    `jpeg_decode` (TFRecords only): "host" (default) -- the workers decode every frame with `decode_jpeg`, as the
    reference does; "device" -- the workers only parse the records, and each batch decodes just the frames its clips read,
    all of them together on the GPU (`jpeg.decode_jpeg_batch`, bit-identical to `decode_jpeg`; frames outside the device
    decoder's scope go to `decode_jpeg`).  The random draws, their order and the batches are those of the host mode.  In
    device mode the batches are built on the reader's own stream and handed over with an event.

    Data parallelism (`rank`, `world`; default: the torchrun environment).  The reference feeds ONE dataset of global
    batches to MirroredStrategy, which splits each batch over the replicas (train.py:145-152, utils.py:160-167).  Here
    every process owns its reader, so the split is made at the source: `batch_size` stays the reference's GLOBAL batch
    (cfg.TRAIN.BATCH_SIZE), rank r keeps records r, r + world, ... of the interleaved record stream (disjoint shards that
    cover the dataset) and yields batch_size // world clips per step -- `Trainer.fit`'s DATASET_SIZE // BATCH_SIZE steps
    are then one pass over the data, and the lr schedule sees the reference's epochs.  The file order is drawn from a
    generator seeded by `seed` alone (identical on every rank, or the shards would overlap: with world > 1 an unset seed
    becomes 0); shuffle buffer and augmentation draws use (seed, rank).

    Multi-label mode (cfg.DATA.MULTI_LABEL): the second element of a batch is the targets [B, NUM_CLASSES] fp32
    multi-hot on the device instead of the labels [B] -- built on the host from every label of the record
    (`parse_sequence_example_labels`; text lines "<path> <l1>,<l2>,...") and copied with the batch.  A class id outside
    [0, NUM_CLASSES) raises ValueError naming the record (TFRecords: "<file>#<index in the file>").  The random draws and
    the batch order are those of the single-label mode.

    Augmentation (cfg.AUG.ENABLE, training): every clip's `aug.AugParams` are drawn with `aug.draw_aug_params` from a NumPy
    generator derived from (seed, rank), in record order, and the batch is built by one `views.make_train_batch_aug` call
    in both `jpeg_decode` modes (device decode still decodes only the T frames a clip reads); `last_params` holds the
    AugParams.  With AUG.AA_TYPE set on top, every clip's RandAugment ops are drawn with `aug.draw_randaug` from a further
    generator of their own (the existing draws and their order do not move) and handed to the same call; `last_randaug`
    holds them.  With AUG.ENABLE off nothing differs from the above: the same draws from the torch generator in the same
    order, one x3d_train_clip launch per clip."""

    _multi = False        # multi-label mode (set from cfg in __init__)

    def __init__(self, cfg, is_training: bool, use_tfrecord: bool, mixed_precision: bool = False, device=None,
                 dtype: torch.dtype = torch.float32, seed: Optional[int] = None, decoder: Optional[Callable] = None,
                 num_workers: int = 4, prefetch: int = 2, rank: Optional[int] = None, world: Optional[int] = None,
                 jpeg_decode: str = "host"):
        self._cfg = cfg
        self._is_training = bool(is_training)
        self._use_tfrecord = bool(use_tfrecord)
        self._mixed_prec = bool(mixed_precision)
        self._device = torch.device(device if device is not None else "cuda")
        self._dtype = dtype if mixed_precision else torch.float32
        if rank is None or world is None:
            from .dist import env_world
            env_rank, _, env_size = env_world()
            rank = env_rank if rank is None else rank
            world = env_size if world is None else world
        self._rank, self._world = int(rank), max(1, int(world))
        if not 0 <= self._rank < self._world:
            raise ValueError(f"rank {rank} outside [0, {world})")
        if self._world > 1 and seed is None:
            seed = 0
        self._rng_files = np.random.default_rng(seed)                       # the same stream on every rank
        self._rng = np.random.default_rng(seed if self._world == 1 else [int(seed), self._rank])
        self._gen = torch.Generator()
        self._gen.manual_seed(int(self._rng.integers(0, 2 ** 31)))
        self._decoder = decoder
        self._workers = max(1, int(num_workers))
        self._prefetch = max(1, int(prefetch))
        self.last_params: List[dict] = []      # the random draws of the clips of the last training batch (tests)
        if jpeg_decode not in ("host", "device"):
            raise ValueError(f"jpeg_decode must be 'host' or 'device', not {jpeg_decode!r}")
        if jpeg_decode == "device" and not self._use_tfrecord:
            raise ValueError("jpeg_decode='device' decodes the JPEG frames of TFRecords (use_tfrecord=True)")
        self._jpeg_decode = jpeg_decode
        from .config import aug_settings, multi_label
        self._multi = multi_label(cfg)
        # AUG.ENABLE (training): aug.AugParams per clip instead of draw_train_params, from a NumPy generator of their own -- a
        # child of the (seed, rank) generator's seed sequence, so neither the shuffle buffer's stream nor the torch
        # generator's changes -- and the batch built by one make_train_batch_aug call
        self._aug = self._is_training and aug_settings(cfg).enable
        self._rng_aug = np.random.default_rng(self._rng.bit_generator.seed_seq.spawn(1)[0]) if self._aug else None
        # AUG.AA_TYPE: every clip's RandAugment ops (aug.draw_randaug) from a further generator of their own -- the NEXT child of
        # the same seed sequence, spawned only when the policy is on, so the AugParams stream above does not move
        from .config import randaug_settings
        self._randaug = randaug_settings(cfg) if self._aug else None
        self._rng_ra = (np.random.default_rng(self._rng.bit_generator.seed_seq.spawn(1)[0])
                        if self._randaug is not None else None)
        self.last_randaug: List[tuple] = []    # the RandAugment draws of the last training batch ([] with AA_TYPE off)
        self._num_classes = int(cfg.NETWORK.NUM_CLASSES)

    # -- decode ------------------------------------------------------------------------------------
    def decode_video(self, line: str) -> Tuple[np.ndarray, Union[int, List[int]]]:
        """dataloader.py:29-61: "<path> <label>" -> (all frames uint8 [F, H, W, 3], label); an undecodable video becomes
        zeros [100, 240, 144, 3] with a warning, as in the reference.  Multi-label mode: "<path> <l1>,<l2>,..." -> the
        list of class ids."""
        parts = line.strip().split(" ")
        path = parts[0]
        if self._multi:
            label = parse_label_list(parts[1] if len(parts) > 1 else "")
        else:
            label = int(parts[1])
        try:
            if self._decoder is None:
                raise RuntimeError("no video decoder configured (the reference uses decord, which is not installed): "
                                   "pass InputReader(..., decoder=callable) or use TFRecords")
            video = np.ascontiguousarray(self._decoder(path), dtype=np.uint8)
            if video.ndim != 4 or video.shape[-1] != 3:
                raise ValueError(f"decoder returned shape {video.shape}")
        except Exception as e:   # noqa: BLE001 -- the reference catches everything here
            warnings.warn(f"Failed to decode video {path} ({e}). Replacing with zeros...")
            video = np.zeros(FAILED_VIDEO_SHAPE, np.uint8)
        return video, label

    def parse_and_decode(self, serialized_example: bytes,
                         all_labels: bool = False) -> Tuple[np.ndarray, Union[int, List[int]]]:
        """dataloader.py:63-88: SequenceExample -> (video uint8 [num_frames, H, W, 3], label); all_labels: the record's
        list of labels instead (multi-label mode)."""
        jpegs, num_frames, labels = parse_sequence_example_labels(serialized_example)
        n = num_frames if num_frames >= 0 else len(jpegs)
        return np.stack([decode_jpeg(j) for j in jpegs[:n]]), _label_of(labels, all_labels)

    def parse_frames(self, serialized_example: bytes,
                     all_labels: bool = False) -> Tuple[Tuple[List[bytes], int, int], Union[int, List[int]]]:
        """jpeg_decode="device": SequenceExample -> ((the num_frames JPEG strings, H, W), label), no pixel decoded.  The
        headers of all frames are read (one library call): a video whose frames differ in size fails as np.stack fails
        in the host mode, and a frame whose header does not parse is handed to `decode_jpeg`, which raises as it does
        there."""
        from .jpeg import parse_headers
        jpegs, num_frames, labels = parse_sequence_example_labels(serialized_example)
        n = num_frames if num_frames >= 0 else len(jpegs)
        jpegs = [bytes(j) for j in jpegs[:n]]
        if not jpegs:
            raise ValueError("need at least one array to stack")
        imgs, _ = parse_headers(jpegs)
        shapes = set()
        for i, im in enumerate(imgs[:len(jpegs)]):
            shapes.add(decode_jpeg(jpegs[i]).shape[:2] if im.status == 2 else (im.height, im.width))   # 2: X3D_JPEG_MALFORMED
        if len(shapes) > 1:
            raise ValueError("all input arrays must have the same shape")
        h, w = shapes.pop()
        return (jpegs, int(h), int(w)), _label_of(labels, all_labels)

    # -- stages ------------------------------------------------------------------------------------
    def _shuffle(self, it: Iterator, size: int) -> Iterator:
        """tf.data shuffle: a buffer of `size` elements, a uniformly drawn one leaves when the next arrives."""
        buf: List = []
        for x in it:
            if len(buf) < size:
                buf.append(x)
                continue
            i = int(self._rng.integers(0, size))
            yield buf[i]
            buf[i] = x
        while buf:
            i = int(self._rng.integers(0, len(buf)))
            yield buf.pop(i)

    def _records(self, file_pattern: str, batch_size: Optional[int]) -> Iterator:
        files = sorted(glob.glob(file_pattern))
        if not files:
            raise FileNotFoundError(f"no files match {file_pattern}")
        if self._use_tfrecord:
            if self._is_training:
                files = [files[i] for i in self._rng_files.permutation(len(files))]     # list_files(shuffle=True)
            its = [read_tfrecords(f) for f in files]
            if self._multi:      # records carry their name (for the class-id check of process_batch)
                its = [_named_records(f, it) for f, it in zip(files, its)]

            def interleave():                    # cycle over the open files, one record each (dataloader.py:149-155)
                live = list(its)
                while live:
                    for it in list(live):
                        try:
                            yield next(it)
                        except StopIteration:
                            live.remove(it)
            recs = self._shard(interleave(), batch_size)
            if self._is_training:
                recs = self._shuffle(recs, batch_size * 16 if batch_size else 1024)
            return recs
        lines = [ln for f in files for ln in open(f).read().splitlines() if ln.strip()]   # TextLineDataset(...).cache()
        if self._is_training:
            # .shuffle(DATASET_SIZE, reshuffle_each_iteration): a fresh permutation of the WHOLE list every pass, drawn from
            # the rank-independent generator BEFORE the split -- every rank sees every video over the epochs, as the
            # replicas of the reference's one shuffled dataset do (a per-rank shuffle of a fixed shard would not)
            lines = [lines[i] for i in self._rng_files.permutation(len(lines))]
        if self._multi:
            lines = [(ln.strip().split(" ")[0], ln) for ln in lines]
        return self._shard(iter(lines), batch_size)

    def _shard(self, it: Iterator, local_batch: Optional[int] = None) -> Iterator:
        """this rank's records of the (rank-independent) record stream, cut so that every rank gets the SAME number:
        training -- records r, r + world, ... of the complete groups of `world` records (tf.data's `shard`; the
        pass's last N % world records are dropped, so all ranks cross pass boundaries at the same step and keep drawing the
        same per-pass permutations); evaluation -- the stream is cut into GLOBAL batches of world * local_batch records,
        rank r takes records [r * b, (r + 1) * b) of each complete one and the trailing partial global batch is dropped:
        exactly the videos `batch(drop_remainder=True)` of the reference's single dataset evaluates."""
        if self._world == 1:
            return it
        group = self._world if self._is_training or not local_batch else self._world * local_batch
        per = group // self._world

        def gen():
            buf = []
            for x in it:
                buf.append(x)
                if len(buf) == group:
                    if self._is_training:
                        yield buf[self._rank]
                    else:
                        yield from buf[self._rank * per:(self._rank + 1) * per]
                    buf = []
        return gen()

    def local_batch(self, batch_size: Optional[int]) -> Optional[int]:
        """clips (videos in evaluation) per step on this rank for the reference's global `batch_size`"""
        if batch_size is None or self._world == 1:
            return batch_size
        if batch_size % self._world:
            raise ValueError(f"global batch {batch_size} is not divisible by {self._world} replicas")
        return batch_size // self._world

    def _decoded(self, recs_factory: Callable[[], Iterator]) -> Iterator[Tuple[np.ndarray, int]]:
        fn = self.decode_video
        if self._use_tfrecord:
            fn = self.parse_frames if self._jpeg_decode == "device" else self.parse_and_decode
        if self._multi:          # (name, record) -> (video, (name, labels))
            base = fn
            kw = dict(all_labels=True) if self._use_tfrecord else {}

            def fn(item):
                video, labels = base(item[1], **kw)
                return video, (item[0], labels)
        with ThreadPoolExecutor(self._workers) as ex:
            while True:
                pending: "queue.Queue" = queue.Queue()
                n = 0
                for rec in recs_factory():
                    pending.put(ex.submit(fn, rec))
                    n += 1
                    if pending.qsize() >= 2 * self._workers:
                        yield pending.get().result()
                while not pending.empty():
                    yield pending.get().result()
                if not self._is_training or n == 0:     # dataset.repeat() only in training (dataloader.py:171-172)
                    return

    def _clips(self, video: np.ndarray) -> torch.Tensor:
        from .views import draw_train_params, make_eval_views, make_train_clip
        v = torch.from_numpy(video).to(self._device, non_blocking=True)
        if self._aug:               # the batch is built in one call when it is complete (_aug_batch)
            from .aug import draw_aug_params
            f, h, w, _ = video.shape
            self._batch_params.append(draw_aug_params(self._cfg, f, h, w, self._rng_aug))
            if self._randaug is not None:
                from .aug import draw_randaug
                self._batch_randaug.append(draw_randaug(self._randaug, h, w, self._rng_ra))
            return v
        if self._is_training:
            f, h, w, _ = video.shape
            p = draw_train_params(f, h, w, self._cfg, self._gen)
            self._batch_params.append(p)
            return make_train_clip(v, self._cfg, params=p, dtype=self._dtype)[None]
        return make_eval_views(v, self._cfg, dtype=self._dtype)

    def process_batch(self, clips: List[torch.Tensor], labels: List[int],
                      batch: Optional[torch.Tensor] = None) -> Tuple[torch.Tensor, torch.Tensor]:
        """dataloader.py:90-116: [B, T, S, S, 3] in training, [B * views * crops, T, S, S, 3] otherwise.  Multi-label
        mode: `labels` holds (record name, class ids) pairs and become the multi-hot targets [B, NUM_CLASSES].
        `batch`: the finished clip tensor (AUG.ENABLE builds it in one call, `_aug_batch`); `clips` is then not read."""
        if batch is None:
            batch = torch.cat(clips, 0)
        if self._multi:
            names = [nm for nm, _ in labels]
            targets = multi_hot([lbs for _, lbs in labels], self._num_classes, names)
            return batch, targets.to(self._device, non_blocking=True)
        return batch, torch.tensor(labels, dtype=torch.int64, device=self._device)

    def _aug_batch(self, videos: List[torch.Tensor], params: List, rate: Optional[int] = None,
                   randaug: Optional[List] = None) -> torch.Tensor:
        """AUG.ENABLE: the batch [B, T, S, S, 3] from its uploaded videos, one make_train_batch_aug call (`randaug`: the
        clips' RandAugment ops when AUG.AA_TYPE is set)"""
        from .views import make_train_batch_aug
        if self._randaug is None:
            return make_train_batch_aug(videos, self._cfg, params_list=params, dtype=self._dtype, rate=rate)
        return make_train_batch_aug(videos, self._cfg, params_list=params, dtype=self._dtype, rate=rate, randaug_list=randaug)

    def _device_batch(self, items: List[Tuple[List[bytes], int, int]], labels: List[int]):
        """jpeg_decode="device": one batch from parsed records.  Training: the draws of every clip in the host mode's order,
        then only the T frames a clip reads -- (start + t * rate) mod F -- go into a compact [T, H, W, 3] video, which
        make_train_clip reads with start = 0, rate = 1 (the same frames: views.hip's index formula).  Evaluation: the
        frames x3d_eval_views reads, decoded into their slots of a full [F, H, W, 3] video (the others are never read).
        Every frame of the batch is decoded in one decode_jpeg_batch call."""
        from .jpeg import decode_jpeg_batch
        from .views import draw_train_params, make_eval_views, make_train_clip
        cfg = self._cfg
        t_len = int(cfg.DATA.TEMP_DURATION)
        frames: List[bytes] = []
        slots: List[torch.Tensor] = []
        videos: List[torch.Tensor] = []
        params: List[dict] = []
        randaug: List[tuple] = []
        for jpegs, h, w in items:
            f = len(jpegs)
            if self._is_training:
                if self._aug:
                    from .aug import draw_aug_params
                    p = draw_aug_params(cfg, f, h, w, self._rng_aug)
                    start = p.start
                    if self._randaug is not None:
                        from .aug import draw_randaug
                        randaug.append(draw_randaug(self._randaug, h, w, self._rng_ra))
                else:
                    p = draw_train_params(f, h, w, cfg, self._gen)
                    start = p["start"]
                params.append(p)
                v = torch.empty((t_len, h, w, 3), dtype=torch.uint8, device=self._device)
                rate = int(cfg.DATA.FRAME_RATE)
                for t in range(t_len):
                    frames.append(jpegs[(start + t * rate) % f])
                    slots.append(v[t])
            else:
                v = torch.empty((f, h, w, 3), dtype=torch.uint8, device=self._device)
                rate = f // t_len if f // t_len > 1 else 1                           # views.hip (transforms.py:51)
                views = int(cfg.TEST.NUM_TEMPORAL_VIEWS)
                for i in sorted({(k * rate) % f for k in range(views * t_len)}):
                    frames.append(jpegs[i])
                    slots.append(v[i])
            videos.append(v)
        decode_jpeg_batch(frames, self._device, out=slots, on_corrupt="host")
        if self._aug:
            batch = self._aug_batch(videos, [p._replace(start=0) for p in params], rate=1, randaug=randaug)
            return self.process_batch([], labels, batch=batch) + (params, randaug)
        if self._is_training:
            clips = [make_train_clip(v, cfg, params=dict(p, start=0), dtype=self._dtype, rate=1)[None]
                     for v, p in zip(videos, params)]
        else:
            clips = [make_eval_views(v, cfg, dtype=self._dtype) for v in videos]
        return self.process_batch(clips, labels) + (params, randaug)

    def _batches(self, file_pattern: str, batch_size: Optional[int]) -> Iterator[Tuple[torch.Tensor, torch.Tensor]]:
        if self._jpeg_decode == "device":
            items: List = []
            dlabels: List[int] = []
            for item, label in self._decoded(lambda: self._records(file_pattern, batch_size)):
                items.append(item)
                dlabels.append(label)
                if len(items) == (batch_size or 1):
                    yield self._device_batch(items, dlabels)
                    items, dlabels = [], []
            return
        clips: List[torch.Tensor] = []
        labels: List[int] = []
        self._batch_params: List[dict] = []
        self._batch_randaug: List[tuple] = []
        bs = batch_size or 1
        for video, label in self._decoded(lambda: self._records(file_pattern, batch_size)):
            clips.append(self._clips(video))
            labels.append(label)
            if len(clips) == bs:
                params, self._batch_params = self._batch_params, []
                randaug, self._batch_randaug = self._batch_randaug, []
                batch = self._aug_batch(clips, params, randaug=randaug) if self._aug else None
                yield self.process_batch(clips, labels, batch=batch) + (params, randaug)
                clips, labels = [], []
        # drop_remainder=True (dataloader.py:186): a trailing partial batch is not emitted

    def __call__(self, file_pattern: str, batch_size: Optional[int] = None) -> Iterator[Tuple[torch.Tensor, torch.Tensor]]:
        """dataloader.py:126-197.  Iterate to get batches; a background thread keeps `prefetch` of them ready.
        `batch_size` is the GLOBAL batch; with world > 1 this rank yields its batch_size // world share (class docstring)."""
        batch_size = self.local_batch(batch_size)
        yield from self._prefetched(lambda: self._batches(file_pattern, batch_size), 2)

    def _prefetched(self, batches: Callable[[], Iterator[tuple]], n_out: int) -> Iterator[tuple]:
        """The batches of `batches()` -- tuples (n_out items to yield..., params, randaug) -- made by a background thread that
        keeps `prefetch` of them ready; the first n_out items of each are yielded, `last_params` / `last_randaug` set from the
        other two.  Device mode: made on the reader's own stream and handed over with an event."""
        q: "queue.Queue" = queue.Queue(self._prefetch)
        stop = threading.Event()
        END = object()

        device_mode = self._jpeg_decode == "device" and self._device.type == "cuda"

        def work():
            try:
                if self._device.type == "cuda":
                    torch.cuda.set_device(self._device)
                if device_mode:       # the batches are made on the reader's own stream, handed over by an event
                    stream = torch.cuda.Stream(self._device)
                    torch.cuda.set_stream(stream)
                for b in batches():
                    if device_mode:
                        ev = torch.cuda.Event()
                        ev.record(stream)
                        b = b + (ev,)
                    elif self._device.type == "cuda":
                        torch.cuda.current_stream().synchronize()     # the consumer thread uses another stream context
                    while not stop.is_set():
                        try:
                            q.put(b, timeout=0.2)
                            break
                        except queue.Full:
                            continue
                    if stop.is_set():
                        return
                q.put(END)
            except BaseException as e:   # noqa: BLE001 -- re-raised in the consumer
                q.put(e)

        th = threading.Thread(target=work, daemon=True)
        th.start()
        try:
            while True:
                item = q.get()
                if item is END:
                    return
                if isinstance(item, BaseException):
                    raise item
                self.last_params = item[n_out]  # the draws of THIS batch (the producer thread runs `prefetch` batches ahead)
                self.last_randaug = item[n_out + 1]
                if device_mode:
                    consumer = torch.cuda.current_stream(self._device)
                    consumer.wait_event(item[n_out + 2])
                    for t in item[:n_out]:              # made on the reader's stream: not reused before the consumer is done
                        if torch.is_tensor(t) and t.is_cuda:
                            t.record_stream(consumer)
                yield item[:n_out]
        finally:
            stop.set()
