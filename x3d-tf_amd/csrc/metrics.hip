// Keras training / validation metrics on the device (reference train.py:102-108, eval.py:48-66): the summed loss rows
// of SparseCategoricalCrossentropy and the hit counts of SparseCategoricalAccuracy ('acc') and
// SparseTopKCategoricalAccuracy(k) ('top_5_acc'), added into four fp64 counters that the host reads once per epoch.
//
// Per row n with label y and fp32 probabilities p_j (j in [0, M)):
//   valid   = 0 <= y < M                       (an out-of-range label is never used as an index)
//   finite  = every p_j of the row is finite
//   loss    = -log q_y + log sum_j q_j,  q = clamp((double)p, 1e-7, 1 - 1e-7) in fp64   (the x3d_softmax_xent /
//             evaluate.Metrics expression); NaN when !valid
//   top-k   = valid && finite && #{j : p_j > p_y} < k.  This is tf.math.in_top_k, which SparseTopKCategoricalAccuracy
//             calls (TensorFlow's CPU InTopK kernel [TF-3p]): ties at the k-th place count as hits, a row holding an inf
//             or a NaN is never a hit, and k >= M makes every valid finite row a hit.
//   top-1   = valid && finite && no p_j > p_y && no j < y with p_j == p_y: the FIRST-index argmax equals y (numpy's
//             argmax).  SparseCategoricalAccuracy compares argmax with y and TensorFlow does not define which index of
//             a tie its argmax returns; this is the rule the tests pin.
//
// The rows are few (<= 64 per rank in training, a few hundred view-averaged videos per validation batch) and M = 400:
// one workgroup.  Each wave owns rows n = wave, wave + 16, ...; its lanes stride over the classes, the comparisons are
// counted with ballots (wave-uniform, exact) and the fp64 sum of q by a butterfly over the lanes.  Per-wave partials go
// through LDS and thread 0 adds them in wave order, then does the one read-add-write of `acc`: no floating-point
// atomics, so the same inputs give bit-identical counters, and successive launches add up in stream order.
#include "common.h"

#define METRICS_THREADS 1024
#define METRICS_WAVES (METRICS_THREADS / WAVE)
#define METRICS_VEC 8

__device__ __forceinline__ double clamp_q(float p) {
  const double q = (double)p;
  return q < 1e-7 ? 1e-7 : (q > 1.0 - 1e-7 ? 1.0 - 1e-7 : q);   // NaN stays NaN (numpy clip, torch clamp)
}

// L = int (int32 labels) | long long (int64): a branch-free label load, so the next row's can stay in flight
template <typename L>
__global__ __launch_bounds__(METRICS_THREADS) void topk_metrics_kernel(const float* __restrict__ probs,
                                                                       const L* __restrict__ labels, double* acc, int N,
                                                                       int M, int k) {
  __shared__ double part_loss[METRICS_WAVES];
  __shared__ int part_hits[METRICS_WAVES][2];
  const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
  double loss = 0.0;   // wave-uniform from here on
  int top1 = 0, topk = 0;
  // The loop is latency-bound (a few rows per wave, nothing else in flight): the next row's label is loaded with this
  // row's p_y, and a row is read in chunks of METRICS_VEC values per lane whose loads are issued together -- at M = 400
  // two round trips per row (label + p_y, then the row) instead of one per 64 classes: 26.5 -> 18.6 us at 64 x 400
  // (rocprofv3, MI355X).  Loading the row without waiting for p_y (taking p_y from the registers) is the next step.
  long long y = wid < N ? (long long)labels[wid] : 0;
  for (int n = wid; n < N; n += METRICS_WAVES) {
    const long long y_next = (long long)labels[min(n + METRICS_WAVES, N - 1)];   // unconditional: no wait at a join
    const bool valid = y >= 0 && y < M;
    const float* row = probs + (long long)n * M;
    const float py_ld = row[valid ? y : 0];
    const float py = valid ? py_ld : 0.f;
    double sq = 0.0;
    int above = 0, tie_before = 0;
    unsigned long long nonfinite = 0;
    for (int j0 = 0; j0 < M; j0 += METRICS_VEC * WAVE) {
      float p[METRICS_VEC];
#pragma unroll
      for (int v = 0; v < METRICS_VEC; v++) {
        const int j = j0 + v * WAVE + lane;
        p[v] = j < M ? row[j] : 0.f;
      }
#pragma unroll
      for (int v = 0; v < METRICS_VEC; v++) {
        const int j = j0 + v * WAVE + lane;
        const bool in = j < M;
        if (in) sq += clamp_q(p[v]);
        above += __popcll(__ballot(in && p[v] > py));
        tie_before += __popcll(__ballot(in && j < y && p[v] == py));
        nonfinite |= __ballot(in && !isfinite(p[v]));
      }
    }
    sq = wave_sum_d(sq);
    const bool hit_ok = valid && nonfinite == 0;
    top1 += (hit_ok && above == 0 && tie_before == 0) ? 1 : 0;
    topk += (hit_ok && above < k) ? 1 : 0;
    loss += valid ? -log(clamp_q(py)) + log(sq) : __builtin_nan("");
    y = y_next;
  }
  if (lane == 0) {
    part_loss[wid] = loss;
    part_hits[wid][0] = top1;
    part_hits[wid][1] = topk;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    double l = 0.0;
    long long h1 = 0, hk = 0;
    for (int w = 0; w < METRICS_WAVES; w++) {
      l += part_loss[w];
      h1 += part_hits[w][0];
      hk += part_hits[w][1];
    }
    acc[0] += l;
    acc[1] += (double)h1;
    acc[2] += (double)hk;
    acc[3] += (double)N;
  }
}

extern "C" int x3d_topk_metrics(const float* probs, const void* labels, int label_bytes, double* acc, int N, int M,
                                int k, void* stream) {
  X3D_REQUIRE(label_bytes == 4 || label_bytes == 8, "topk_metrics: label_bytes %d (int32 = 4 or int64 = 8)", label_bytes);
  X3D_REQUIRE(N >= 0 && M > 0 && k >= 1, "topk_metrics: bad sizes N=%d M=%d k=%d", N, M, k);
  X3D_REQUIRE((long long)N * M < (1LL << 31), "topk_metrics: N*M = %lld >= 2^31", (long long)N * M);
  if (N == 0) return X3D_OK;
  X3D_REQUIRE(probs && labels && acc, "topk_metrics: null pointer");
  if (label_bytes == 8)
    hipLaunchKernelGGL(topk_metrics_kernel<long long>, dim3(1), dim3(METRICS_THREADS), 0, (hipStream_t)stream, probs,
                       (const long long*)labels, acc, N, M, k);
  else
    hipLaunchKernelGGL(topk_metrics_kernel<int>, dim3(1), dim3(METRICS_THREADS), 0, (hipStream_t)stream, probs,
                       (const int*)labels, acc, N, M, k);
  X3D_LAUNCH_CHECK("topk_metrics");
  return X3D_OK;
}

// ------------------------------------------------------------------------------------------------
// Per-class hit counts (mean per-class accuracy): counts[y] += 1 for every row with a label in [0, M), hits[y] += 1 where the
// row is a top-1 hit by the rule above (first-index argmax, every p_j finite).  One wave per row, the comparisons counted with
// ballots; lane 0 adds into the int64 counters with integer atomics, so the counters do not depend on the order of the rows.
// ------------------------------------------------------------------------------------------------
#define HITS_THREADS 256
#define HITS_WAVES (HITS_THREADS / WAVE)

template <typename L>
__global__ __launch_bounds__(HITS_THREADS) void class_hits_kernel(const float* __restrict__ probs, const L* __restrict__ labels,
                                                                  unsigned long long* hits, unsigned long long* counts, int N,
                                                                  int M) {
  const int lane = threadIdx.x & 63;
  const int n = blockIdx.x * HITS_WAVES + (threadIdx.x >> 6);     // wave-uniform
  if (n >= N) return;
  const long long y = (long long)labels[n];
  if (y < 0 || y >= M) return;                                    // counted nowhere, never used as an index
  const float* row = probs + (long long)n * M;
  const float py = row[y];
  int above = 0, tie_before = 0;
  unsigned long long nonfinite = 0;
  for (int j0 = 0; j0 < M; j0 += WAVE) {
    const int j = j0 + lane;
    const bool in = j < M;
    const float p = in ? row[j] : 0.f;
    above += __popcll(__ballot(in && p > py));
    tie_before += __popcll(__ballot(in && j < y && p == py));
    nonfinite |= __ballot(in && !isfinite(p));
  }
  if (lane == 0) {
    atomicAdd(counts + y, 1ULL);
    if (nonfinite == 0 && above == 0 && tie_before == 0) atomicAdd(hits + y, 1ULL);
  }
}

extern "C" int x3d_class_hits(const float* probs, const void* labels, int label_bytes, long long* hits, long long* counts, int N,
                              int M, void* stream) {
  X3D_REQUIRE(label_bytes == 4 || label_bytes == 8, "class_hits: label_bytes %d (int32 = 4 or int64 = 8)", label_bytes);
  X3D_REQUIRE(N >= 0 && M > 0, "class_hits: bad sizes N=%d M=%d", N, M);
  X3D_REQUIRE((long long)N * M < (1LL << 31), "class_hits: N*M = %lld >= 2^31", (long long)N * M);
  if (N == 0) return X3D_OK;
  X3D_REQUIRE(probs && labels && hits && counts, "class_hits: null pointer");
  X3D_REQUIRE(((uintptr_t)hits | (uintptr_t)counts) % 8 == 0, "class_hits: hits / counts must be 8-byte aligned");
  const dim3 grid((N + HITS_WAVES - 1) / HITS_WAVES), block(HITS_THREADS);
  if (label_bytes == 8)
    hipLaunchKernelGGL(class_hits_kernel<long long>, grid, block, 0, (hipStream_t)stream, probs, (const long long*)labels,
                       (unsigned long long*)hits, (unsigned long long*)counts, N, M);
  else
    hipLaunchKernelGGL(class_hits_kernel<int>, grid, block, 0, (hipStream_t)stream, probs, (const int*)labels,
                       (unsigned long long*)hits, (unsigned long long*)counts, N, M);
  X3D_LAUNCH_CHECK("class_hits");
  return X3D_OK;
}
