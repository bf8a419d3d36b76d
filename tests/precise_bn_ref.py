"""numpy fp64 restatement of precise BatchNorm (x3d_precise_bn_accum / x3d_precise_bn_final, include/x3d_hip.h): the sum over
the replicated copies of a statistics accumulator, the pooling over batches and ranks, and the final formula."""
import numpy as np


def replica_sum(stats, c, replicas, stride):
    """stats: the flat fp64 accumulator of one layer (`replicas` copies of [c][2], `stride` doubles apart) -> [c][2] totals
    (sum, sum of squares), the copies added in index order"""
    s = np.asarray(stats, dtype=np.float64).reshape(replicas, stride)[:, :2 * c].reshape(replicas, c, 2)
    return s.sum(axis=0)


def pool(batches):
    """batches: (sums [c][2], count) per batch and rank, in any order -> (pooled sums [c][2], pooled count)"""
    total, n = None, 0.0
    for sums, count in batches:
        sums = np.asarray(sums, dtype=np.float64)
        total = sums.copy() if total is None else total + sums
        n += float(count)
    return total, n


def final(sums, n):
    """pooled sums [c][2] over n elements per channel -> (mean [c], unbiased variance [c]) in fp64, unrounded"""
    sums = np.asarray(sums, dtype=np.float64)
    mean = sums[:, 0] / n
    var = np.maximum(sums[:, 1] / n - mean * mean, 0.0)
    unb = var * (n / (n - 1.0)) if n > 1 else var
    return mean, unb


def ulps(got, want64):
    """distance of the fp32 array `got` from the fp64 values `want64` in units of the fp32 spacing at each value's fp32
    rounding (0 where `got` is that rounding, 1 where it is a neighbour)"""
    w32 = np.asarray(want64, dtype=np.float64).astype(np.float32)
    return np.abs(np.asarray(got, dtype=np.float64) - w32.astype(np.float64)) / np.spacing(np.abs(w32)).astype(np.float64)
