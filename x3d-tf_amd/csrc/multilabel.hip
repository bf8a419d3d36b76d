// Multi-label evaluation (DATA.MULTI_LABEL, Charades-style training): the element-wise max over the views of a video and
// per-class average precision over a whole evaluation set.  The exact rules are in include/x3d_hip.h.  (The sigmoid / binary
// cross-entropy head: loss.hip.)
#include "common.h"

// ------------------------------------------------------------------------------------------------
// out[v][m] = max over `views` consecutive rows; a NaN in any view makes the output NaN (torch.amax)
// ------------------------------------------------------------------------------------------------
__global__ void view_max_kernel(const float* __restrict__ probs, float* out, int views, int M) {
  const int v = blockIdx.y;
  const int m = blockIdx.x * blockDim.x + threadIdx.x;
  if (m >= M) return;
  float acc = probs[(long long)v * views * M + m];
  for (int i = 1; i < views; i++) {
    const float x = probs[((long long)v * views + i) * M + m];
    if (x > acc || x != x) acc = x;        // once acc is NaN, x > acc is false: it stays NaN
  }
  out[(long long)v * M + m] = acc;
}

extern "C" int x3d_view_max(const float* probs, float* out, int videos, int views, int M, void* stream) {
  X3D_REQUIRE(probs && out && videos > 0 && views > 0 && M > 0, "view_max: bad args");
  hipLaunchKernelGGL(view_max_kernel, dim3(ceil_div(M, 128), videos), dim3(128), 0, (hipStream_t)stream, probs, out,
                     views, M);
  X3D_LAUNCH_CHECK("view_max");
  return X3D_OK;
}

// ------------------------------------------------------------------------------------------------
// Per-class average precision (sklearn.metrics.average_precision_score).  One workgroup per class c:
//   1. read the column once: count the positives (target >= 0.5) into P, note any NaN score, put the positives' scores
//      (-0 made +0) into LDS -- in arrival order (an LDS integer counter); the sort below makes the order irrelevant
//   2. bitonic sort of the positives, padded with +inf to a power of two
//   3. for rank chunks [lo, hi) of AP_HIST ranks: read the column again, for every element find ub = #{positives <= s_j}
//      by binary search and add 1 to hist[ub - 1 - lo] (ranks below the chunk are dropped, ranks above it are one
//      counter); a block suffix sum then gives D_r = #{j : s_j >= u_r} for the chunk's ranks, and a lower-bound search
//      TP_r = P - #{positives < u_r}.  sum_r TP_r / D_r in fp64, per thread over its own contiguous ranks, then over
//      the threads in a fixed order: the same inputs give bit-identical results.
//   ap[c] = sum / P.  Every count is an integer (LDS integer atomics only).
// LDS: AP_MAX_POS keys (128 KiB) + AP_HIST counters (28 KiB) + a few hundred bytes: one workgroup per CU.  A column with
// more than AP_MAX_POS positives is refused in-kernel (npos[c] = -P, ap[c] = NaN); it can only occur when N > AP_MAX_POS,
// which the host checks (ops.multilabel_ap).
// ------------------------------------------------------------------------------------------------
#define AP_THREADS 1024
#define AP_WAVES (AP_THREADS / WAVE)
#define AP_MAX_POS X3D_AP_MAX_POSITIVES
#define AP_HIST 7168
#define AP_SEG ((AP_HIST + AP_THREADS - 1) / AP_THREADS)

__device__ __forceinline__ float canon0(float s) { return s == 0.f ? 0.f : s; }   // -0 -> +0 (one threshold)

// #{k < P : keys[k] <= v}, keys ascending
__device__ __forceinline__ int upper_bound_lds(const float* keys, int P, float v) {
  int lo = 0, hi = P;
  while (lo < hi) {
    const int mid = (lo + hi) >> 1;
    if (keys[mid] <= v) lo = mid + 1; else hi = mid;
  }
  return lo;
}

// #{k < P : keys[k] < v}
__device__ __forceinline__ int lower_bound_lds(const float* keys, int P, float v) {
  int lo = 0, hi = P;
  while (lo < hi) {
    const int mid = (lo + hi) >> 1;
    if (keys[mid] < v) lo = mid + 1; else hi = mid;
  }
  return lo;
}

__global__ __launch_bounds__(AP_THREADS) void multilabel_ap_kernel(const float* __restrict__ scores,
                                                                    const float* __restrict__ targets, int N, int M,
                                                                    double* ap, int* npos) {
  __shared__ float keys[AP_MAX_POS];
  __shared__ int hist[AP_HIST];
  __shared__ int wave_int[AP_WAVES];
  __shared__ double wave_d[AP_WAVES];
  __shared__ int s_count, s_nan;
  const int c = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
  if (tid == 0) { s_count = 0; s_nan = 0; }
  __syncthreads();

  // 1. positives into LDS
  int nan_local = 0;
  for (int j = tid; j < N; j += AP_THREADS) {
    const long long i = (long long)j * M + c;
    const float s = scores[i];
    const float y = targets[i];
    nan_local |= (s != s);
    if (y >= 0.5f) {
      const int k = atomicAdd(&s_count, 1);
      if (k < AP_MAX_POS) keys[k] = canon0(s);
    }
  }
  if (__any(nan_local) && lane == 0) atomicOr(&s_nan, 1);
  __syncthreads();
  const int P = s_count;
  if (P == 0 || P > AP_MAX_POS || s_nan) {
    if (tid == 0) {
      ap[c] = __builtin_nan("");
      npos[c] = P > AP_MAX_POS ? -P : P;
    }
    return;
  }

  // 2. bitonic sort of keys[0, P2), P2 = next power of two >= P
  int P2 = 1;
  while (P2 < P) P2 <<= 1;
  for (int k = P + tid; k < P2; k += AP_THREADS) keys[k] = INFINITY;
  __syncthreads();
  for (int size = 2; size <= P2; size <<= 1) {
    for (int stride = size >> 1; stride > 0; stride >>= 1) {
      for (int k = tid; k < P2; k += AP_THREADS) {
        const int partner = k ^ stride;
        if (partner > k) {
          const float a = keys[k], b = keys[partner];
          const bool up = (k & size) == 0;
          if ((a > b) == up) { keys[k] = b; keys[partner] = a; }
        }
      }
      __syncthreads();
    }
  }

  // 3. rank chunks
  double total = 0.0;   // thread 0's running sum, chunks in ascending order
  for (int lo = 0; lo < P; lo += AP_HIST) {
    const int hi = min(P, lo + AP_HIST), L = hi - lo;
    for (int k = tid; k < L; k += AP_THREADS) hist[k] = 0;
    __syncthreads();
    int above = 0;   // elements with ub - 1 >= hi
    for (int j = tid; j < N; j += AP_THREADS) {
      const float s = canon0(scores[(long long)j * M + c]);
      const int r = upper_bound_lds(keys, P, s) - 1;   // highest rank with u_r <= s (-1: below every positive)
      if (r >= hi) above++;
      else if (r >= lo) atomicAdd(&hist[r - lo], 1);
    }
    // block sum of `above` (wave ballot-free integer reduction)
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) above += __shfl_xor(above, o, 64);
    if (lane == 0) wave_int[wid] = above;
    __syncthreads();
    int above_all = 0;
    for (int w = 0; w < AP_WAVES; w++) above_all += wave_int[w];
    // suffix sums over the chunk: thread t owns hist[t*AP_SEG, (t+1)*AP_SEG)
    const int k0 = tid * AP_SEG;
    int seg = 0;
#pragma unroll
    for (int e = 0; e < AP_SEG; e++) seg += (k0 + e < L) ? hist[k0 + e] : 0;
    // suffix of the segment sums of the lanes at or after this one (within the wave)
    int suf = seg;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
      const int v = __shfl_down(suf, o, 64);
      if (lane + o < 64) suf += v;
    }
    __syncthreads();   // wave_int is reused
    if (lane == 0) wave_int[wid] = suf;   // the wave's total
    __syncthreads();
    int later = above_all;   // everything in segments after this thread's
    for (int w = wid + 1; w < AP_WAVES; w++) later += wave_int[w];
    later += suf - seg;
    double part = 0.0;
    int run = later;
    for (int e = AP_SEG - 1; e >= 0; e--) {   // descending ranks: D_r = hist[r..] + later
      const int k = k0 + e;
      if (k >= L) continue;
      run += hist[k];
      const int r = lo + k;
      const int tp = P - lower_bound_lds(keys, P, keys[r]);
      part += (double)tp / (double)run;
    }
    part = wave_sum_d(part);
    if (lane == 0) wave_d[wid] = part;
    __syncthreads();
    if (tid == 0)
      for (int w = 0; w < AP_WAVES; w++) total += wave_d[w];
    __syncthreads();   // hist / wave_int / wave_d are rewritten by the next chunk
  }
  if (tid == 0) {
    ap[c] = total / (double)P;
    npos[c] = P;
  }
}

extern "C" int x3d_multilabel_ap(const float* scores, const float* targets, int N, int M, double* ap, int* npos,
                                 void* stream) {
  X3D_REQUIRE(N > 0 && M > 0, "multilabel_ap: bad sizes N=%d M=%d", N, M);
  X3D_REQUIRE((long long)N * M < (1LL << 31), "multilabel_ap: N*M = %lld >= 2^31", (long long)N * M);
  X3D_REQUIRE(scores && targets && ap && npos, "multilabel_ap: null pointer");
  hipLaunchKernelGGL(multilabel_ap_kernel, dim3(M), dim3(AP_THREADS), 0, (hipStream_t)stream, scores, targets, N, M,
                     ap, npos);
  X3D_LAUNCH_CHECK("multilabel_ap");
  return X3D_OK;
}
