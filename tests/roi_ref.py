"""fp64 NumPy restatement of x3d_roi_pool_fwd / x3d_roi_pool_bwd (the rules are in include/x3d_hip.h, "K7r"): the temporal mean of
relu(s*x + t), aligned ROIAlign with border clamp, the spatial max over the R*R bins, and the backward through the max, the
bilinear weights, the mean over time and the ReLU.

Bilinear weights are separable, so a bin is a matrix over pixels: A[bin][h][w] = (sum over its sample rows of the row weights of h)
* (sum over its sample columns of the column weights of w) / (gh * gw).  tests/test_roi_head.py checks this against torch's
grid_sample, sample by sample."""
import math

import numpy as np


def box_geometry(box, filled, spatial_scale, H, W, R, sampling_ratio):
    """None for an empty slot (not filled, a non-finite coordinate, x2' <= x1' or y2' <= y1'), else (x1', y1', bin_w, bin_h, gh, gw)
    of the box scaled and clamped to the frame."""
    if not filled:
        return None
    b = np.asarray(box, dtype=np.float64)
    if not np.all(np.isfinite(b)):
        return None
    x1, y1, x2, y2 = (float(v) * float(spatial_scale) for v in b)
    x1, x2 = min(max(x1, 0.0), float(W)), min(max(x2, 0.0), float(W))
    y1, y2 = min(max(y1, 0.0), float(H)), min(max(y2, 0.0), float(H))
    if not (x2 > x1 and y2 > y1):
        return None
    bin_w, bin_h = (x2 - x1) / R, (y2 - y1) / R
    gw = int(sampling_ratio) if sampling_ratio > 0 else max(1, math.ceil(bin_w))
    gh = int(sampling_ratio) if sampling_ratio > 0 else max(1, math.ceil(bin_h))
    return x1, y1, bin_w, bin_h, gh, gw


def sample_coords(start, bin_size, g, R):
    """[R][g] sample coordinates along one axis, before the border clamp"""
    p = np.arange(R, dtype=np.float64)[:, None]
    i = np.arange(g, dtype=np.float64)[None, :]
    return start - 0.5 + p * bin_size + (i + 0.5) * bin_size / g


def axis_weights(start, bin_size, g, L, R):
    """A [R][L]: A[p][l] = sum over the g samples of bin p of the bilinear weight of pixel l (border clamp)"""
    a = np.zeros((R, L), dtype=np.float64)
    ys = sample_coords(start, bin_size, g, R)
    for p in range(R):
        for y in ys[p]:
            y = 0.0 if y <= 0.0 else float(y)
            lo = int(math.floor(y))
            if lo >= L - 1:
                lo = hi = L - 1
                y = float(L - 1)
            else:
                hi = lo + 1
            a[p, lo] += 1.0 - (y - lo)
            a[p, hi] += y - lo
    return a


def bin_matrix(geom, H, W, R):
    """[R*R][H*W] weights of one box, bins in row-major order"""
    x1, y1, bin_w, bin_h, gh, gw = geom
    ay = axis_weights(y1, bin_h, gh, H, R)
    ax = axis_weights(x1, bin_w, gw, W, R)
    return (ay[:, None, :, None] * ax[None, :, None, :]).reshape(R * R, H * W) / (gh * gw)


def temporal_map(x, ss):
    """[N][C][H*W] = mean_t relu(s*x + t) of x [N][C][T][H][W]"""
    x = np.asarray(x, dtype=np.float64)
    ss = np.asarray(ss, dtype=np.float64).reshape(-1, 2)
    z = ss[None, :, 0, None, None, None] * x + ss[None, :, 1, None, None, None]
    return np.maximum(z, 0.0).mean(axis=2).reshape(x.shape[0], x.shape[1], -1)


def forward(x, ss, boxes, num_boxes, R, sampling_ratio, spatial_scale):
    """(pooled [N*K][C], bins [N*K][C][R*R], argmax [N*K][C] uint8, valid [N*K] bool); an empty slot has all three zero"""
    x = np.asarray(x, dtype=np.float64)
    n_, c_, _, H, W = x.shape
    K = boxes.shape[1]
    m = temporal_map(x, ss)
    pooled = np.zeros((n_ * K, c_))
    bins = np.zeros((n_ * K, c_, R * R))
    argmax = np.zeros((n_ * K, c_), dtype=np.uint8)
    valid = np.zeros(n_ * K, dtype=bool)
    for n in range(n_):
        for k in range(K):
            geom = box_geometry(boxes[n, k], k < int(num_boxes[n]), spatial_scale, H, W, R, sampling_ratio)
            if geom is None:
                continue
            r = n * K + k
            valid[r] = True
            bins[r] = m[n] @ bin_matrix(geom, H, W, R).T
            argmax[r] = bins[r].argmax(axis=1)          # the first maximal bin
            pooled[r] = bins[r].max(axis=1)
    return pooled, bins, argmax, valid


def backward(dpooled, argmax, boxes, num_boxes, yraw, ss, R, sampling_ratio, spatial_scale):
    """(g [N][C][T][H][W] fp64, unrounded; z = s*yraw + t) for the given argmax (teacher forcing: the kernel's own)"""
    y = np.asarray(yraw, dtype=np.float64)
    n_, c_, T, H, W = y.shape
    K = boxes.shape[1]
    ss = np.asarray(ss, dtype=np.float64).reshape(-1, 2)
    z = ss[None, :, 0, None, None, None] * y + ss[None, :, 1, None, None, None]
    dm = np.zeros((n_, c_, H * W))
    dp = np.asarray(dpooled, dtype=np.float64)
    for n in range(n_):
        for k in range(K):
            geom = box_geometry(boxes[n, k], k < int(num_boxes[n]), spatial_scale, H, W, R, sampling_ratio)
            if geom is None:
                continue
            r = n * K + k
            a = bin_matrix(geom, H, W, R)
            dm[n] += dp[r][:, None] * a[np.asarray(argmax[r], dtype=np.int64)]
    g = dm.reshape(n_, c_, 1, H, W) / T * (z > 0)
    return g, z


BOX_KINDS = ("inside", "touching", "beyond", "subpixel", "zero_width", "nan")


def box_mix(n, k, height, width, seed, first_kind=0, grid=8.0):
    """boxes [n][k][4] float32 in pixels of a height x width clip, on the 1/8-pixel grid (so that a power-of-two spatial_scale
    keeps every coordinate, difference and bin count exact in fp32 and fp64 alike), cycling through BOX_KINDS from `first_kind`:
    inside the frame, touching its borders, reaching beyond it, narrower than a feature-map pixel, zero width, a NaN coordinate.
    grid = None: the coordinates as drawn, rounded to fp32 only (box_mix_offgrid)."""
    rng = np.random.default_rng(seed)
    if grid is None:
        q = lambda v: np.asarray(v, dtype=np.float64)
    else:
        q = lambda v: np.round(np.asarray(v, dtype=np.float64) * grid) / grid
    out = np.zeros((n, k, 4), dtype=np.float32)
    i = first_kind
    for a in range(n):
        for b in range(k):
            kind = BOX_KINDS[i % len(BOX_KINDS)]
            i += 1
            x1, x2 = np.sort(rng.uniform(0.05, 0.95, 2) * width)
            y1, y2 = np.sort(rng.uniform(0.05, 0.95, 2) * height)
            x2, y2 = max(x2, x1 + 1.0), max(y2, y1 + 1.0)
            if kind == "touching":
                x1, y1, x2, y2 = 0.0, 0.0, float(width), float(height)
            elif kind == "beyond":
                x1, y1, x2, y2 = x1 - width, y1 - 0.5 * height, x2 + 2.0 * width, y2 + height
            elif kind == "subpixel":
                x2, y2 = x1 + 0.375, y1 + 2.125
            elif kind == "zero_width":
                x2 = x1
            box = q([x1, y1, x2, y2])
            if kind == "nan":
                box[int(rng.integers(4))] = np.nan
            out[a, b] = box
    return out


def box_mix_offgrid(n, k, height, width, seed, first_kind=0):
    """box_mix without the grid: coordinates drawn uniformly and kept as fp32 rounds them, for a spatial_scale that is not a power
    of two.  Kernel and reference then see products and quotients that are inexact in fp64 -- the same ones, from the same fp32
    inputs in the same order.  A zero-width box keeps x2 == x1 exactly (the same fp32 value twice)."""
    return box_mix(n, k, height, width, seed, first_kind, grid=None)
