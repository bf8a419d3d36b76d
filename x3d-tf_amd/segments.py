"""The chunk table of the layer-wise optimizers (x3d_seg_sumsq / x3d_lars / x3d_adamw / x3d_lamb, include/x3d_hip.h).

A segment is one trainable tensor of the flat parameter buffer: (offset, length, l2 flag).  The kernels do not look a segment
up per element; they walk a table of chunks built once, here, on the host:

    chunks [nchunk][3] int32 = (segment, first element, count)   count <= CHUNK, inside one segment, first % 4 == 0
    segs   [nseg][3]   int32 = (first chunk, number of chunks, l2 flag)

Every element of every segment lies in exactly one chunk, the chunks of a segment are adjacent and ascending, and what lies
between segments (the padding that keeps tensor offsets 16-byte aligned) is in no chunk.  Plain numpy: no device needed."""
import collections

import numpy as np

Segment = collections.namedtuple("Segment", "name offset length l2")


def chunk_size() -> int:
    """X3D_SEG_CHUNK of the header: the most elements one wave takes in one turn."""
    from . import hip
    return hip.SEG_CHUNK


def build_chunk_table(segments, chunk=None):
    """(chunks [nchunk, 3] int32, segs [nseg, 3] int32) for `segments`: an iterable of (offset, length, l2) or Segment.

    ValueError for no segment, a length < 1, an offset that is negative or no multiple of 4 (the kernels move 16-byte vectors
    from a chunk's first element), segments that overlap or are not in ascending order, a chunk size that is not a positive
    multiple of 4, and a buffer of 2^31 elements or more (the tables index with int32)."""
    chunk = chunk_size() if chunk is None else int(chunk)
    if chunk < 4 or chunk % 4:
        raise ValueError(f"chunk must be a positive multiple of 4, not {chunk}")
    items = [(int(s.offset), int(s.length), bool(s.l2)) if isinstance(s, Segment) else (int(s[0]), int(s[1]), bool(s[2]))
             for s in segments]
    if not items:
        raise ValueError("no segments")
    chunks, segs, end = [], [], 0
    for t, (off, n, l2) in enumerate(items):
        if n < 1:
            raise ValueError(f"segment {t}: length must be >= 1, not {n}")
        if off < 0 or off % 4:
            raise ValueError(f"segment {t}: offset must be a non-negative multiple of 4 elements, not {off}")
        if off < end:
            raise ValueError(f"segment {t}: starts at {off}, inside or in front of the segment before it (ends at {end})")
        end = off + n
        if end >= 2 ** 31:
            raise ValueError(f"segment {t}: ends at {end}; the chunk table indexes with int32")
        first = len(chunks)
        chunks += [(t, at, min(chunk, end - at)) for at in range(off, end, chunk)]
        segs.append((first, len(chunks) - first, int(l2)))
    return np.asarray(chunks, dtype=np.int32).reshape(-1, 3), np.asarray(segs, dtype=np.int32).reshape(-1, 3)


class SegTable:
    """A chunk table on the host (`chunks`, `segs`: int32 numpy) and, after `.to(device)`, on the device (`d_chunks`,
    `d_segs`: the int32 tensors the kernels read).  `end` = one past the last element any chunk covers: every buffer handed to
    a launch with this table must hold at least that many elements."""

    def __init__(self, segments, chunk=None):
        self.segments = [s if isinstance(s, Segment) else Segment(str(i), int(s[0]), int(s[1]), bool(s[2]))
                         for i, s in enumerate(segments)]
        self.chunks, self.segs = build_chunk_table(self.segments, chunk)
        self.nchunk, self.nseg = len(self.chunks), len(self.segs)
        self.end = int((self.chunks[:, 1].astype(np.int64) + self.chunks[:, 2]).max())
        self.d_chunks = self.d_segs = None

    def to(self, device):
        import torch
        self.d_chunks = torch.from_numpy(self.chunks.copy()).to(device)
        self.d_segs = torch.from_numpy(self.segs.copy()).to(device)
        return self
