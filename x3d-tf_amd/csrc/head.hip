// Classification head on pooled vectors (reference model.py:95-111,119-127; the losses, train.py:104: loss.hip) and the
// loss-scaling / L2-loss helpers of the train step (the optimizer itself: solver.hip).  All fp32; sizes are [N <= a few hundred] x [432..2048] x [400].
#include "common.h"

// y[n][m] = act(sum_k xm[n][k]*w[m][k] + b[m]), xm = x * (mask ? mask*mask_scale : 1).
// One wave per DENSE_MT output features and DENSE_NT samples: lanes split K, coalesced on w[m][:] and x[n][:].
// The x rows are the traffic (every feature block re-reads them from L2: M/MT * N * K floats), so a wave keeps
// MT features: with one feature per wave fc2 (2048 -> 400, 64 samples) moved 210 MB through L1 in 105 us.
#define DENSE_NT 8
#define DENSE_MT 4
__global__ __launch_bounds__(64) void dense_fwd_kernel(const float* __restrict__ x, const float* __restrict__ mask,
                                                       float mask_scale, const float* __restrict__ w,
                                                       const float* __restrict__ b, float* y, int act, int N, int K,
                                                       int M) {
  const int m0 = blockIdx.x * DENSE_MT, n0 = blockIdx.y * DENSE_NT, lane = threadIdx.x;
  float acc[DENSE_MT][DENSE_NT];
#pragma unroll
  for (int j = 0; j < DENSE_MT; j++)
#pragma unroll
    for (int i = 0; i < DENSE_NT; i++) acc[j][i] = 0.f;
  // rows past M / N are clamped (computed twice, never stored): every load of the loop is unconditional, so the
  // MT + NT (+ NT mask) loads of an iteration are in flight together instead of one branch at a time
  const float* wr[DENSE_MT];
  const float* xr[DENSE_NT];
  const float* mr[DENSE_NT];
#pragma unroll
  for (int j = 0; j < DENSE_MT; j++) wr[j] = w + (long long)min(m0 + j, M - 1) * K;
#pragma unroll
  for (int i = 0; i < DENSE_NT; i++) {
    xr[i] = x + (long long)min(n0 + i, N - 1) * K;
    mr[i] = mask ? mask + (long long)min(n0 + i, N - 1) * K : nullptr;
  }
  if (mask) {
#pragma unroll 2
    for (int k = lane; k < K; k += 64) {
      float wv[DENSE_MT], xv[DENSE_NT], mv[DENSE_NT];
#pragma unroll
      for (int j = 0; j < DENSE_MT; j++) wv[j] = wr[j][k];
#pragma unroll
      for (int i = 0; i < DENSE_NT; i++) { xv[i] = xr[i][k]; mv[i] = mr[i][k]; }
#pragma unroll
      for (int i = 0; i < DENSE_NT; i++) xv[i] *= mv[i] * mask_scale;
#pragma unroll
      for (int j = 0; j < DENSE_MT; j++)
#pragma unroll
        for (int i = 0; i < DENSE_NT; i++) acc[j][i] += wv[j] * xv[i];
    }
  } else {
#pragma unroll 2
    for (int k = lane; k < K; k += 64) {
      float wv[DENSE_MT], xv[DENSE_NT];
#pragma unroll
      for (int j = 0; j < DENSE_MT; j++) wv[j] = wr[j][k];
#pragma unroll
      for (int i = 0; i < DENSE_NT; i++) xv[i] = xr[i][k];
#pragma unroll
      for (int j = 0; j < DENSE_MT; j++)
#pragma unroll
        for (int i = 0; i < DENSE_NT; i++) acc[j][i] += wv[j] * xv[i];
    }
  }
#pragma unroll
  for (int j = 0; j < DENSE_MT; j++)
#pragma unroll
    for (int i = 0; i < DENSE_NT; i++) {
      const float s = wave_sum(acc[j][i]);
      const int n = n0 + i, m = m0 + j;
      if (lane == 0 && n < N && m < M) {
        float v = s + (b ? b[m] : 0.f);
        if (act == X3D_ACT_RELU) v = fmaxf(v, 0.f);
        y[(long long)n * M + m] = v;
      }
    }
}

// dx[n][k] = (sum_m dz[n][m]*w[m][k]) * (mask ? mask*scale : 1); dz = dy*[y>0] for ReLU.
// A workgroup owns 64 inputs k (the lanes) and DENSE_BN samples; its four waves split M (the long, latency-bound
// loop: 2048 features for fc1) and meet in LDS.  w[m][k] is read once per DENSE_BN samples.
#define DENSE_BN 4
__global__ __launch_bounds__(256) void dense_bwd_dx_kernel(const float* __restrict__ dy, const float* __restrict__ y,
                                                           int act, const float* __restrict__ mask, float mask_scale,
                                                           const float* __restrict__ w, float* dx, int N, int K, int M) {
  extern __shared__ float dz[];  // [DENSE_BN][M], then the partial sums [4 waves][DENSE_BN][64]
  const int n0 = blockIdx.y * DENSE_BN;
  for (int i = threadIdx.x; i < DENSE_BN * M; i += 256) {
    const int nn = i / M, m = i - nn * M, n = n0 + nn;
    float d = 0.f;
    if (n < N) {
      d = dy[(long long)n * M + m];
      if (act == X3D_ACT_RELU && !(y[(long long)n * M + m] > 0.f)) d = 0.f;
    }
    dz[i] = d;
  }
  __syncthreads();
  const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
  const int k = blockIdx.x * 64 + lane;
  const int kc = k < K ? k : K - 1;   // clamped: every lane loads, only k < K is stored
  float acc[DENSE_BN];
#pragma unroll
  for (int i = 0; i < DENSE_BN; i++) acc[i] = 0.f;
  // batches of 16 loads issued together (written out: left to the unroller, every load was followed by vmcnt(0))
  constexpr int DXB = 16;
  int m = wid;
  for (; m + 4 * (DXB - 1) < M; m += 4 * DXB) {
    float wv[DXB];
#pragma unroll
    for (int j = 0; j < DXB; j++) wv[j] = w[(long long)(m + 4 * j) * K + kc];
#pragma unroll
    for (int j = 0; j < DXB; j++)
#pragma unroll
      for (int i = 0; i < DENSE_BN; i++) acc[i] += dz[i * M + m + 4 * j] * wv[j];   // dz: LDS broadcast reads
  }
  for (; m < M; m += 4) {
    const float wv = w[(long long)m * K + kc];
#pragma unroll
    for (int i = 0; i < DENSE_BN; i++) acc[i] += dz[i * M + m] * wv;
  }
  __syncthreads();   // everyone is done with dz
#pragma unroll
  for (int i = 0; i < DENSE_BN; i++) dz[(wid * DENSE_BN + i) * 64 + lane] = acc[i];
  __syncthreads();
  if (wid == 0 && k < K) {
#pragma unroll
    for (int i = 0; i < DENSE_BN; i++) {
      const int n = n0 + i;
      if (n < N) {
        float v = dz[i * 64 + lane] + dz[(DENSE_BN + i) * 64 + lane] + dz[(2 * DENSE_BN + i) * 64 + lane] +
                  dz[(3 * DENSE_BN + i) * 64 + lane];
        if (mask) v *= mask[(long long)n * K + k] * mask_scale;
        dx[(long long)n * K + k] = v;
      }
    }
  }
}

// dw[m][k] += sum_n dz[n][m]*xm[n][k] ; db[m] += sum_n dz[n][m].
// A workgroup owns 256 inputs k and DENSE_BM features: xm[n][k] is read once per DENSE_BM features.
#define DENSE_BM 8
__global__ __launch_bounds__(256) void dense_bwd_dw_kernel(const float* __restrict__ dy, const float* __restrict__ y,
                                                           int act, const float* __restrict__ x,
                                                           const float* __restrict__ mask, float mask_scale, float* dw,
                                                           float* db, int N, int K, int M) {
  extern __shared__ float dzs[];   // [N rounded up to 8][DENSE_BM]: dz of this workgroup's features, ReLU mask applied, 0 past N
  const int m0 = blockIdx.y * DENSE_BM;
  const int Np = (N + 7) & ~7;
  for (int i = threadIdx.x; i < Np * DENSE_BM; i += 256) {
    const int n = i / DENSE_BM, m = m0 + (i - n * DENSE_BM);
    float d = 0.f;
    if (m < M && n < N) {
      d = dy[(long long)n * M + m];
      if (act == X3D_ACT_RELU && !(y[(long long)n * M + m] > 0.f)) d = 0.f;
    }
    dzs[i] = d;
  }
  __syncthreads();
  const int k = blockIdx.x * 256 + threadIdx.x;
  const int kc = k < K ? k : K - 1;   // clamped: every lane loads (unconditional, 8 samples in flight), only k < K is stored
  float acc[DENSE_BM], accb[DENSE_BM];
#pragma unroll
  for (int j = 0; j < DENSE_BM; j++) { acc[j] = 0.f; accb[j] = 0.f; }
  // samples in batches of 8 with the loads written out first (left to the unroller, the masked variant waited for
  // every load separately); rows past N are clamped and weighted by dz = 0
  constexpr int DWB = 8;
  for (int nb = 0; nb < N; nb += DWB) {
    float xv[DWB], mv[DWB];
#pragma unroll
    for (int u = 0; u < DWB; u++) xv[u] = x[(long long)min(nb + u, N - 1) * K + kc];
    if (mask) {
#pragma unroll
      for (int u = 0; u < DWB; u++) mv[u] = mask[(long long)min(nb + u, N - 1) * K + kc];
#pragma unroll
      for (int u = 0; u < DWB; u++) xv[u] *= mv[u] * mask_scale;
    }
#pragma unroll
    for (int u = 0; u < DWB; u++) {
      const f32x4 d0 = *(const f32x4*)&dzs[(nb + u) * DENSE_BM], d1 = *(const f32x4*)&dzs[(nb + u) * DENSE_BM + 4];   // LDS broadcast
#pragma unroll
      for (int j = 0; j < 4; j++) {
        accb[j] += d0[j]; acc[j] += d0[j] * xv[u];
        accb[4 + j] += d1[j]; acc[4 + j] += d1[j] * xv[u];
      }
    }
  }
#pragma unroll
  for (int j = 0; j < DENSE_BM; j++) {
    const int m = m0 + j;
    if (m < M) {
      if (k < K) dw[(long long)m * K + k] += acc[j];
      if (db && blockIdx.x == 0 && threadIdx.x == 0) db[m] += accb[j];
    }
  }
}

extern "C" int x3d_dense_fwd(const float* x, const float* mask, float mask_scale, const float* w, const float* b,
                             float* y, int act, int N, int K, int M, void* stream) {
  X3D_REQUIRE(x && w && y && N > 0 && K > 0 && M > 0, "dense_fwd: bad args");
  X3D_REQUIRE(act == X3D_ACT_NONE || act == X3D_ACT_RELU, "dense_fwd: act must be none/relu");
  hipLaunchKernelGGL(dense_fwd_kernel, dim3(ceil_div(M, DENSE_MT), ceil_div(N, DENSE_NT)), dim3(64), 0, (hipStream_t)stream,
                     x, mask, mask_scale, w, b, y, act, N, K, M);
  X3D_LAUNCH_CHECK("dense_fwd");
  return X3D_OK;
}

extern "C" int x3d_dense_bwd(const float* dy, const float* y, int act, const float* x, const float* mask,
                             float mask_scale, const float* w, float* dx, float* dw, float* db, int N, int K, int M,
                             void* stream) {
  X3D_REQUIRE(dy && x && w && dw && N > 0 && K > 0 && M > 0, "dense_bwd: bad args");
  X3D_REQUIRE(act == X3D_ACT_NONE || (act == X3D_ACT_RELU && y), "dense_bwd: relu needs y");
  const size_t dz_bytes = (size_t)DENSE_BN * (M > 256 ? M : 256) * sizeof(float);   // >= the [4][DENSE_BN][64] partial sums
  X3D_REQUIRE(dz_bytes <= 64 * 1024, "dense_bwd: M too large");
  // (both limits before the first launch: a refused call leaves dx untouched as well)
  const size_t dzs_bytes = (size_t)((N + 7) & ~7) * DENSE_BM * sizeof(float);
  X3D_REQUIRE(dzs_bytes <= 64 * 1024, "dense_bwd: N too large");
  hipStream_t st = (hipStream_t)stream;
  if (dx) {
    hipLaunchKernelGGL(dense_bwd_dx_kernel, dim3(ceil_div(K, 64), ceil_div(N, DENSE_BN)), dim3(256), dz_bytes, st, dy, y, act,
                       mask, mask_scale, w, dx, N, K, M);
    X3D_LAUNCH_CHECK("dense_bwd_dx");
  }
  hipLaunchKernelGGL(dense_bwd_dw_kernel, dim3(ceil_div(K, 256), ceil_div(M, DENSE_BM)), dim3(256), dzs_bytes, st, dy, y, act, x, mask, mask_scale, dw, db, N, K, M);
  X3D_LAUNCH_CHECK("dense_bwd_dw");
  return X3D_OK;
}

__global__ void view_mean_kernel(const float* __restrict__ probs, float* out, int views, int M) {
  const int v = blockIdx.y;
  const int m = blockIdx.x * blockDim.x + threadIdx.x;
  if (m >= M) return;
  float acc = 0.f;
  for (int i = 0; i < views; i++) acc += probs[((long long)v * views + i) * M + m];
  out[(long long)v * M + m] = acc / (float)views;
}

extern "C" int x3d_view_mean(const float* probs, float* out, int videos, int views, int M, void* stream) {
  X3D_REQUIRE(probs && out && videos > 0 && views > 0 && M > 0, "view_mean: bad args");
  hipLaunchKernelGGL(view_mean_kernel, dim3(ceil_div(M, 128), videos), dim3(128), 0, (hipStream_t)stream, probs, out,
                     views, M);
  X3D_LAUNCH_CHECK("view_mean");
  return X3D_OK;
}

// (SGD-Nesterov and Adam, with their clipping / EMA forms: solver.hip)

// ------------------------------------------------------------------------------------------------
// LossScaleOptimizer support (train.py:99-100, Keras mixed_float16): are all gradients finite?  *flag (device int,
// set to 1 by the caller) is cleared when any of the n values is inf / nan.
// ------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void all_finite_kernel(const float* __restrict__ g, long long n, int* flag) {
  bool bad = false;
  for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < n; i += (long long)gridDim.x * 256) {
    const unsigned u = __float_as_uint(g[i]);
    bad |= (u & 0x7f800000u) == 0x7f800000u;     // exponent all ones: inf or nan
  }
  if (__any(bad) && (threadIdx.x & 63) == 0) atomicAnd(flag, 0);
}

extern "C" int x3d_all_finite(const float* g, long long n, int* flag, void* stream) {
  X3D_REQUIRE(g && flag && n > 0, "all_finite: bad args");
  long long blocks = ceil_div_ll(n, 256 * 8);
  if (blocks > 2048) blocks = 2048;
  hipLaunchKernelGGL(all_finite_kernel, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, g, n, flag);
  X3D_LAUNCH_CHECK("all_finite");
  return X3D_OK;
}

__global__ __launch_bounds__(256) void l2_sumsq_kernel(const float* __restrict__ w,
                                                       const unsigned char* __restrict__ l2, double* out, long long n) {
  __shared__ float scratch[4];
  float red[1] = {0.f};
  for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < n; i += (long long)gridDim.x * 256)
    if (!l2 || l2[i]) red[0] += w[i] * w[i];
  block_sum<1>(red, scratch);
  if (threadIdx.x == 0) atomic_add_d(out, (double)red[0]);
}

extern "C" int x3d_l2_sumsq(const float* w, const unsigned char* l2_mask, double* out, long long n, void* stream) {
  X3D_REQUIRE(w && out && n > 0, "l2_sumsq: bad args");
  long long blocks = ceil_div_ll(n, 256 * 8);
  if (blocks > 1024) blocks = 1024;
  hipLaunchKernelGGL(l2_sumsq_kernel, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, w, l2_mask, out, n);
  X3D_LAUNCH_CHECK("l2_sumsq");
  return X3D_OK;
}
