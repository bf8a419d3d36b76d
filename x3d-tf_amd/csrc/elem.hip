// BatchNorm bookkeeping and the bandwidth-bound elementwise / reduction kernels around the convs:
// BN finalize (train / eval / backward), residual tail (Add+ReLU) forward and backward, ReLU+BN
// backward reduce (stem, conv5 after global pooling), pool5, NTHWC<->NCTHW at the module boundary.
#include "common.h"
#include <type_traits>

// ------------------------------------------------------------------------------------------------
// BN finalize kernels: one thread per channel (C <= a few hundred)
// ------------------------------------------------------------------------------------------------
// One lane per (channel, copy): 32 lanes load the 32 copies of a channel in ONE round trip and add them with an xor
// butterfly (1, 2, 4, 8, 16); a 64-thread block finalizes two channels.  (One thread per channel summing the copies
// itself is four dependent round trips: 84 such launches sit between producers and consumers in every train step.)
static_assert(STATS_R == 32, "bn_finalize_kernel maps one half-wave to the copies of a channel");
__global__ __launch_bounds__(64) void bn_finalize_kernel(const x3d_bn_fold f, int C) {
  const int c = blockIdx.x * 2 + (threadIdx.x >> 5), r = threadIdx.x & 31;
  const int cc = c < C ? c : C - 1;
  const long long rs = stats_stride(C);
  double s1 = f.stats[r * rs + cc * 2], s2 = f.stats[r * rs + cc * 2 + 1];
  const float ga = f.gamma[cc], be = f.beta[cc];
#pragma unroll
  for (int o = 1; o < 32; o <<= 1) {
    s1 += __shfl_xor(s1, o, 64);
    s2 += __shfl_xor(s2, o, 64);
  }
  float sc, sh;
  bn_coefs(f, cc, s1, s2, ga, be, r == 0 && c < C, sc, sh);
}

__global__ void bn_bwd_finalize_kernel(const double* __restrict__ sums, double count,
                                       const float* __restrict__ mi, const float* __restrict__ gamma,
                                       float* coef, float* dgamma, float* dbeta, int C) {
  const int c = blockIdx.x * blockDim.x + threadIdx.x;
  if (c >= C) return;
  float A, B, Cc;
  double dga, dbe;
  bn_bwd_coefs_signed(sums, count, mi, gamma, c, A, B, Cc, dga, dbe);     // (common.h: the one definition; count < 0: frozen statistics)
  coef[c * 4] = A;
  coef[c * 4 + 1] = B;
  coef[c * 4 + 2] = Cc;
  coef[c * 4 + 3] = 0.f;
  dgamma[c] += (float)dga;
  dbeta[c] += (float)dbe;
}

extern "C" int x3d_stats_replicas(void) { return STATS_R; }
extern "C" long long x3d_stats_stride(int C) { return stats_stride(C); }

extern "C" int x3d_bn_finalize(const double* stats, double count, const float* gamma, const float* beta,
                               float* moving_mean, float* moving_var, float eps, float momentum,
                               int update_moving, float* scale_shift, float* mean_invstd, int C,
                               void* stream) {
  X3D_REQUIRE(stats && gamma && beta && scale_shift && mean_invstd && C > 0 && count > 0, "bn_finalize: bad args");
  X3D_REQUIRE(!update_moving || (moving_mean && moving_var), "bn_finalize: moving stats required");
  x3d_bn_fold f;
  f.stats = stats; f.count = count; f.gamma = gamma; f.beta = beta; f.moving_mean = moving_mean; f.moving_var = moving_var;
  f.eps = eps; f.momentum = momentum; f.update_moving = update_moving; f.scale_shift = scale_shift; f.mean_invstd = mean_invstd;
  hipLaunchKernelGGL(bn_finalize_kernel, dim3(ceil_div(C, 2)), dim3(64), 0, (hipStream_t)stream, f, C);
  X3D_LAUNCH_CHECK("bn_finalize");
  return X3D_OK;
}

__global__ __launch_bounds__(64) void bn_eval_coef_batched_kernel(const x3d_bn_eval_item* __restrict__ items, float eps) {
  const x3d_bn_eval_item it = items[blockIdx.x];
  for (int c = threadIdx.x; c < it.C; c += 64) {
    const float invstd = 1.0f / sqrtf(it.moving_var[c] + eps);
    const float sc = it.gamma[c] * invstd;
    it.scale_shift[c * 2] = sc;
    it.scale_shift[c * 2 + 1] = it.beta[c] - it.moving_mean[c] * sc;
    it.mean_invstd[c * 2] = it.moving_mean[c];
    it.mean_invstd[c * 2 + 1] = invstd;
  }
}

extern "C" int x3d_bn_eval_coef_batched(const x3d_bn_eval_item* items, int n_items, float eps, void* stream) {
  X3D_REQUIRE(items && n_items > 0, "bn_eval_coef_batched: no items");
  hipLaunchKernelGGL(bn_eval_coef_batched_kernel, dim3(n_items), dim3(64), 0, (hipStream_t)stream, items, eps);
  X3D_LAUNCH_CHECK("bn_eval_coef_batched");
  return X3D_OK;
}

extern "C" int x3d_bn_bwd_finalize(const double* sums, double count, const float* mean_invstd,
                                   const float* gamma, float* coef, float* dgamma, float* dbeta, int C,
                                   void* stream) {
  X3D_REQUIRE(sums && mean_invstd && gamma && coef && dgamma && dbeta && C > 0 && count != 0, "bn_bwd_finalize: bad args");      // (count < 0: frozen statistics)
  hipLaunchKernelGGL(bn_bwd_finalize_kernel, dim3(ceil_div(C, 64)), dim3(64), 0, (hipStream_t)stream, sums, count,
                     mean_invstd, gamma, coef, dgamma, dbeta, C);
  X3D_LAUNCH_CHECK("bn_bwd_finalize");
  return X3D_OK;
}

// ------------------------------------------------------------------------------------------------
// plane-wise elementwise kernels.  grid = (chunks over P, N*C): the channel is uniform per block.
// Each thread handles VEC contiguous elements per iteration.
// ------------------------------------------------------------------------------------------------
#define ELEM_BLOCK 256
#define ELEM_ITERS 4

static inline dim3 elem_grid(long long P, int vec, int NC) {
  return dim3((unsigned)ceil_div_ll(P, (long long)ELEM_BLOCK * vec * ELEM_ITERS), (unsigned)NC);
}

// The launch ladder of this file, once: fn(ElemType<T>, integral_constant<int, VEC>) for the storage type of `dtype` and
// vec = norm_vec() of the result of pick_vec: the full 16-byte vector (4 fp32 / 8 16-bit elements), or scalars
template <typename T> struct ElemType { typedef T type; };
template <int VEC> using ElemVec = std::integral_constant<int, VEC>;
static inline int norm_vec(int dtype, int vec) {
  const int full = dtype == X3D_F32 ? 4 : 8;
  return vec >= full ? full : 1;
}
template <typename F>
static inline void elem_dispatch(int dtype, int vec, F&& fn) {
  const bool full = vec > 1;
  if (dtype == X3D_F32) {
    if (full) fn(ElemType<float>(), ElemVec<4>()); else fn(ElemType<float>(), ElemVec<1>());
  } else if (dtype == X3D_F16) {
    if (full) fn(ElemType<f16>(), ElemVec<8>()); else fn(ElemType<f16>(), ElemVec<1>());
  } else {
    if (full) fn(ElemType<bf16>(), ElemVec<8>()); else fn(ElemType<bf16>(), ElemVec<1>());
  }
}
#define ELEM_T(t) typename decltype(t)::type

// Residual tail (Add + ReLU).  One forward body, one general and one small-plane backward body for the plain tail, the tail
// with the BatchNorm finalize folded in (FOLD) and the tail with stochastic depth (DP: keep[n] scales the branch).
// The chunk of one workgroup, ELEM_ITERS vectors per thread.  DP: y = relu(k * (sc*craw + tc) + (sr*sh + tr)); !KEPT (k == 0):
// y = relu(sr*sh + tr), craw not loaded.  KEPT is a template argument so that the uniform branch on keep[n] stands in front of
// the loop, one loop per side.  (The pointers are the kernel's __restrict__ arguments; repeating the qualifier on these inlined
// functions costs up to 4 VGPRs in the backward.)
template <typename T, int VEC, bool DP, bool KEPT>
__device__ __forceinline__ void tail_fwd_chunk(const T* craw, const T* sh, T* y, long long base, long long P, float sc, float tc,
                                               float sr, float tr, float k) {
  long long p = ((long long)blockIdx.x * ELEM_ITERS * ELEM_BLOCK + threadIdx.x) * VEC;
#pragma unroll
  for (int it = 0; it < ELEM_ITERS; it++, p += (long long)ELEM_BLOCK * VEC) {
    if (p < P) {
      float a[VEC], b[VEC], o[VEC];
      if (KEPT) VecIO<T, VEC>::load(craw + base + p, a);
      if (DP || sh) VecIO<T, VEC>::load(sh + base + p, b);   // (DP: the entry point requires the shortcut)
      if (!KEPT) {
#pragma unroll
        for (int e = 0; e < VEC; e++) o[e] = fmaxf(sr * b[e] + tr, 0.f);
      } else if (DP) {
#pragma unroll
        for (int e = 0; e < VEC; e++) o[e] = fmaxf(k * (sc * a[e] + tc) + (sr * b[e] + tr), 0.f);
      } else if (sh) {
#pragma unroll
        for (int e = 0; e < VEC; e++) o[e] = fmaxf(sc * a[e] + tc + (sr * b[e] + tr), 0.f);
      } else {  // plain BN + ReLU (stem output)
#pragma unroll
        for (int e = 0; e < VEC; e++) o[e] = fmaxf(sc * a[e] + tc, 0.f);
      }
      VecIO<T, VEC>::store(y + base + p, o);
    }
  }
}

// FOLD: the BatchNorm finalize of bn_c / bn_r runs here (x3d_bn_fold); the first workgroup of each channel of
// sample 0 publishes the coefficients and updates the moving statistics
// DP: keep[n] is uniform per workgroup in the (n, c) grid, read through a scalar load, and so is the branch on it
struct TailFold { x3d_bn_fold c, r; int has_r; };
template <typename T, int VEC, bool FOLD, bool DP>
__global__ __launch_bounds__(ELEM_BLOCK) void tail_fwd_kernel(const T* __restrict__ craw,
                                                             const float* __restrict__ ssc,
                                                             const T* __restrict__ sh,
                                                             const float* __restrict__ ssr,
                                                             const float* __restrict__ keep, T* __restrict__ y,
                                                             int C, long long P, const TailFold fold) {
  static_assert(!(FOLD && DP), "the plan never folds a drop-path tail");
  const int nc = blockIdx.y, c = nc % C;
  float sc, tc, sr = 1.f, tr = 0.f;
  if constexpr (FOLD) {
    const bool writer = (nc < C) && blockIdx.x == 0 && threadIdx.x == 0;
    bn_fold_channel(fold.c, c, writer, sc, tc, C);
    if (fold.has_r) bn_fold_channel(fold.r, c, writer, sr, tr, C);
  } else {
    sc = ssc[c * 2]; tc = ssc[c * 2 + 1];
    if (ssr) { sr = ssr[c * 2]; tr = ssr[c * 2 + 1]; }
  }
  const long long base = (long long)nc * P;
  if constexpr (DP) {
    const float k = keep[nc / C];
    if (k == 0.f) tail_fwd_chunk<T, VEC, true, false>(craw, sh, y, base, P, sc, tc, sr, tr, k);
    else tail_fwd_chunk<T, VEC, true, true>(craw, sh, y, base, P, sc, tc, sr, tr, k);
  } else {
    tail_fwd_chunk<T, VEC, false, true>(craw, sh, y, base, P, sc, tc, sr, tr, 1.f);
  }
}

// Tail backward: g = dy*[y>0] in place; gb = the gradient of the branch: g itself, or with DP round(keep[n]*g), stored to
// gbr; sums_c += (sum gb, sum gb*craw); sums_r += (sum g, sum g*rraw).
// One element into the partial sums of its thread: red = (sum gb, sum gb*craw, sum g*rraw[, sum g: DP, where gb is not g]).
// !KEPT (a dropped sample of the general kernel): gb = 0, cr is not read and nothing is added for the branch
template <typename T, bool DP, bool KEPT>
__device__ __forceinline__ float tail_bwd_term(float g, float k, const float& cr, const float& rr, bool has_r,
                                               float (&red)[DP ? 4 : 3]) {
  float gb = 0.f;
  if constexpr (KEPT) {
    gb = g;
    if constexpr (DP) gb = round_to<T>(k * g);
    red[0] += gb;
    red[1] += gb * cr;
  }
  if (has_r) {
    if constexpr (DP) red[3] += g;
    red[2] += g * rr;
  }
  return gb;
}
// ... the chunk of one workgroup of the general kernel
template <typename T, int VEC, bool DP, bool KEPT>
__device__ __forceinline__ void tail_bwd_chunk(T* dyg, T* gbr, const T* y, const T* craw, const T* rraw, long long base,
                                               long long P, float k, float (&red)[DP ? 4 : 3]) {
  long long p = ((long long)blockIdx.x * ELEM_ITERS * ELEM_BLOCK + threadIdx.x) * VEC;
#pragma unroll
  for (int it = 0; it < ELEM_ITERS; it++, p += (long long)ELEM_BLOCK * VEC) {
    if (p < P) {
      float d[VEC], yy[VEC], cr[VEC], rr[VEC], g[VEC], gb[VEC];
      VecIO<T, VEC>::load(dyg + base + p, d);
      VecIO<T, VEC>::load(y + base + p, yy);
      if (KEPT) VecIO<T, VEC>::load(craw + base + p, cr);
      if (rraw) VecIO<T, VEC>::load(rraw + base + p, rr);
#pragma unroll
      for (int e = 0; e < VEC; e++) {
        g[e] = yy[e] > 0.f ? d[e] : 0.f;
        gb[e] = tail_bwd_term<T, DP, KEPT>(g[e], k, cr[e], rr[e], rraw != nullptr, red);
      }
      VecIO<T, VEC>::store(dyg + base + p, g);
      if constexpr (DP) VecIO<T, VEC>::store(gbr + base + p, gb);
    }
  }
}
// ... and the sums of a workgroup into the fp64 accumulators (any_kept false: a dropped workgroup adds nothing to sums_c)
template <bool DP>
__device__ __forceinline__ void tail_bwd_flush(const float (&red)[DP ? 4 : 3], bool any_kept, bool has_r, double* sums_c,
                                               double* sums_r, int c) {
  if (any_kept) {
    atomic_add_d(&sums_c[c * 2], (double)red[0]);
    atomic_add_d(&sums_c[c * 2 + 1], (double)red[1]);
  }
  if (has_r) {
    atomic_add_d(&sums_r[c * 2], (double)red[DP ? 3 : 0]);
    atomic_add_d(&sums_r[c * 2 + 1], (double)red[2]);
  }
}

// DP: keep[n] and the branch on it are uniform per workgroup, as in the forward
template <typename T, int VEC, bool DP>
__global__ __launch_bounds__(ELEM_BLOCK) void tail_bwd_kernel(T* __restrict__ dyg, T* __restrict__ gbr, const T* __restrict__ y,
                                                             const T* __restrict__ craw, const T* __restrict__ rraw,
                                                             const float* __restrict__ keep, double* sums_c,
                                                             double* sums_r, int C, long long P) {
  constexpr int NR = DP ? 4 : 3;
  __shared__ float scratch[NR * (ELEM_BLOCK / 64)];
  const int nc = blockIdx.y, c = nc % C;
  const long long base = (long long)nc * P;
  float red[NR] = {};
  bool kept = true;
  if constexpr (DP) {
    const float k = keep[nc / C];
    kept = k != 0.f;
    if (kept) tail_bwd_chunk<T, VEC, true, true>(dyg, gbr, y, craw, rraw, base, P, k, red);
    else tail_bwd_chunk<T, VEC, true, false>(dyg, gbr, y, craw, rraw, base, P, k, red);
  } else {
    tail_bwd_chunk<T, VEC, false, true>(dyg, gbr, y, craw, rraw, base, P, 1.f, red);
  }
  block_sum<NR>(red, scratch);
  if (threadIdx.x == 0) tail_bwd_flush<DP>(red, kept, rraw != nullptr, sums_c, sums_r, c);
}

// ... small planes (P / VEC < 256: the 7 x 7 stage): one workgroup takes NB samples of ONE channel -- with a workgroup per (n, c)
// 98 of 256 threads had a vector and N workgroups per channel met in the fp64 atomics (192 ch x 64 clips of 16x7x7: 28 us for
// 77 MB).  grid = (C, ceil(N / NB)); the flat index runs over (sample in the group, vector of the plane).
// DP: keep belongs to the sample, so here it is per lane: a dropped sample's lanes skip the craw load and, with craw = 0 and
// gb = round(0 * g), add exact zeros to sums_c.
template <typename T, int VEC, bool DP>
__global__ __launch_bounds__(ELEM_BLOCK) void tail_bwd_small_kernel(T* __restrict__ dyg, T* __restrict__ gbr, const T* __restrict__ y,
                                                                   const T* __restrict__ craw, const T* __restrict__ rraw,
                                                                   const float* __restrict__ keep, double* sums_c,
                                                                   double* sums_r, int N, int C, int P, int NB) {
  constexpr int NR = DP ? 4 : 3;
  __shared__ float scratch[NR * (ELEM_BLOCK / 64)];
  const int c = blockIdx.x, n0 = blockIdx.y * NB;
  const int nb = min(NB, N - n0);
  const int vpp = P / VEC, total = nb * vpp;
  float red[NR] = {};
  for (int i0 = threadIdx.x; i0 < total; i0 += 2 * ELEM_BLOCK) {
    // two vectors per thread and round, their loads issued together
    float d[2][VEC], yy[2][VEC], cr[2][VEC], rr[2][VEC], k[2];
    long long off[2];
    bool ok[2];
#pragma unroll
    for (int u = 0; u < 2; u++) {
      const int i = i0 + u * ELEM_BLOCK;
      ok[u] = i < total;
      const int nl = ok[u] ? i / vpp : 0, pv = ok[u] ? i - nl * vpp : 0;
      off[u] = ((long long)(n0 + nl) * C + c) * P + (long long)pv * VEC;
      k[u] = 1.f;
      if constexpr (DP) {
        k[u] = ok[u] ? keep[n0 + nl] : 0.f;
#pragma unroll
        for (int e = 0; e < VEC; e++) cr[u][e] = 0.f;
      }
      if (ok[u]) {
        VecIO<T, VEC>::load(dyg + off[u], d[u]);
        VecIO<T, VEC>::load(y + off[u], yy[u]);
        if (!DP || k[u] != 0.f) VecIO<T, VEC>::load(craw + off[u], cr[u]);
        if (rraw) VecIO<T, VEC>::load(rraw + off[u], rr[u]);
      }
    }
#pragma unroll
    for (int u = 0; u < 2; u++) {
      if (!ok[u]) continue;
      float g[VEC], gb[VEC];
#pragma unroll
      for (int e = 0; e < VEC; e++) {
        g[e] = yy[u][e] > 0.f ? d[u][e] : 0.f;
        gb[e] = tail_bwd_term<T, DP, true>(g[e], k[u], cr[u][e], rr[u][e], rraw != nullptr, red);
      }
      VecIO<T, VEC>::store(dyg + off[u], g);
      if constexpr (DP) VecIO<T, VEC>::store(gbr + off[u], gb);
    }
  }
  block_sum<NR>(red, scratch);
  if (threadIdx.x == 0) tail_bwd_flush<DP>(red, true, rraw != nullptr, sums_c, sums_r, c);
}

// z = s*yraw + t ; g = (dy ? dy : dpool[n][c]/P) * [z > 0]; sums += (sum g, sum g*yraw)
template <typename T, int VEC>
__global__ __launch_bounds__(ELEM_BLOCK) void relu_bn_bwd_reduce_kernel(const T* __restrict__ dy,
                                                                       const float* __restrict__ dpool,
                                                                       const T* __restrict__ yraw,
                                                                       const float* __restrict__ ss, T* g,
                                                                       double* sums, int C, long long P) {
  __shared__ float scratch[2 * (ELEM_BLOCK / 64)];
  const int nc = blockIdx.y, c = nc % C;
  const float s = ss[c * 2], t = ss[c * 2 + 1];
  const float dp = dpool ? dpool[nc] / (float)P : 0.f;
  const long long base = (long long)nc * P;
  float red[2] = {0.f, 0.f};
  long long p = ((long long)blockIdx.x * ELEM_ITERS * ELEM_BLOCK + threadIdx.x) * VEC;
#pragma unroll
  for (int it = 0; it < ELEM_ITERS; it++, p += (long long)ELEM_BLOCK * VEC) {
    if (p < P) {
      float d[VEC], yr[VEC], o[VEC];
      VecIO<T, VEC>::load(yraw + base + p, yr);
      if (dy) {
        VecIO<T, VEC>::load(dy + base + p, d);
      } else {
#pragma unroll
        for (int e = 0; e < VEC; e++) d[e] = dp;
      }
#pragma unroll
      for (int e = 0; e < VEC; e++) {
        o[e] = (s * yr[e] + t > 0.f) ? d[e] : 0.f;
        const float gr = round_to<T>(o[e]);
        red[0] += gr;
        red[1] += gr * yr[e];
      }
      if (g) VecIO<T, VEC>::store(g + base + p, o);   // g == NULL: reduce only (the consumer applies the mask itself)
    }
  }
  block_sum<2>(red, scratch);
  if (threadIdx.x == 0) {
    atomic_add_d(&sums[c * 2], (double)red[0]);
    atomic_add_d(&sums[c * 2 + 1], (double)red[1]);
  }
}

// pooled[n][c] = mean_p relu(s*x + t): one block per (n, c)
template <typename T, int VEC>
__global__ __launch_bounds__(ELEM_BLOCK) void pool_fwd_kernel(const T* __restrict__ x,
                                                             const float* __restrict__ ss, float* pooled,
                                                             int C, long long P) {
  __shared__ float scratch[ELEM_BLOCK / 64];
  const int nc = blockIdx.x, c = nc % C;
  const float s = ss[c * 2], t = ss[c * 2 + 1];
  const long long base = (long long)nc * P;
  float red[1] = {0.f};
  for (long long p = (long long)threadIdx.x * VEC; p < P; p += (long long)ELEM_BLOCK * VEC) {
    float v[VEC];
    VecIO<T, VEC>::load(x + base + p, v);
#pragma unroll
    for (int e = 0; e < VEC; e++) red[0] += fmaxf(s * v[e] + t, 0.f);
  }
  block_sum<1>(red, scratch);
  if (threadIdx.x == 0) pooled[nc] = red[0] / (float)P;
}

template <bool FOLD, bool DP>
static void tail_fwd_launch(const void* c_raw, const float* c_scale_shift, const void* shortcut, const float* r_scale_shift,
                            const float* keep, void* y, int N, int C, long long P, int dtype, const TailFold& fold, void* stream) {
  const int eb = dtype == X3D_F32 ? 4 : 2;
  const int vec = norm_vec(dtype, pick_vec(eb, P, c_raw, shortcut, y));
  elem_dispatch(dtype, vec, [&](auto t, auto v) {
    typedef ELEM_T(t) T;
    hipLaunchKernelGGL((tail_fwd_kernel<T, decltype(v)::value, FOLD, DP>), elem_grid(P, vec, N * C), dim3(ELEM_BLOCK), 0,
                       (hipStream_t)stream, (const T*)c_raw, c_scale_shift, (const T*)shortcut, r_scale_shift, keep, (T*)y, C, P, fold);
  });
}

extern "C" int x3d_tail_fwd(const void* c_raw, const float* c_scale_shift, const void* shortcut,
                            const float* r_scale_shift, void* y, int N, int C, long long P, int dtype,
                            void* stream) {
  X3D_REQUIRE(c_raw && c_scale_shift && y && N > 0 && C > 0 && P > 0, "tail_fwd: bad args");
  X3D_REQUIRE(x3d_dtype_ok(dtype), "tail_fwd: bad dtype");
  TailFold nofold;
  memset(&nofold, 0, sizeof(nofold));
  tail_fwd_launch<false, false>(c_raw, c_scale_shift, shortcut, r_scale_shift, nullptr, y, N, C, P, dtype, nofold, stream);
  X3D_LAUNCH_CHECK("tail_fwd");
  return X3D_OK;
}

extern "C" int x3d_tail_fwd_bn(const void* c_raw, const x3d_bn_fold* c_bn, const void* shortcut, const x3d_bn_fold* r_bn,
                               void* y, int N, int C, long long P, int dtype, void* stream) {
  X3D_REQUIRE(c_raw && y && N > 0 && C > 0 && P > 0, "tail_fwd_bn: bad args");
  X3D_REQUIRE(bn_fold_valid(c_bn), "tail_fwd_bn: incomplete x3d_bn_fold for bn_c");
  X3D_REQUIRE(!r_bn || (shortcut && bn_fold_valid(r_bn)), "tail_fwd_bn: incomplete x3d_bn_fold for bn_r");
  X3D_REQUIRE(x3d_dtype_ok(dtype), "tail_fwd_bn: bad dtype");
  TailFold fold;
  memset(&fold, 0, sizeof(fold));
  fold.c = *c_bn;
  if (r_bn) { fold.r = *r_bn; fold.has_r = 1; }
  tail_fwd_launch<true, false>(c_raw, nullptr, shortcut, nullptr, nullptr, y, N, C, P, dtype, fold, stream);
  X3D_LAUNCH_CHECK("tail_fwd_bn");
  return X3D_OK;
}

extern "C" int x3d_tail_fwd_dp(const void* c_raw, const float* c_scale_shift, const void* shortcut, const float* r_scale_shift,
                               const float* keep, void* y, int N, int C, long long P, int dtype, void* stream) {
  X3D_REQUIRE(c_raw && c_scale_shift && y && keep && N > 0 && C > 0 && P > 0, "tail_fwd_dp: bad args");
  X3D_REQUIRE(shortcut, "tail_fwd_dp: shortcut required (the stem's BatchNorm + ReLU has no branch to drop)");
  X3D_REQUIRE(x3d_dtype_ok(dtype), "tail_fwd_dp: bad dtype");
  TailFold nofold;
  memset(&nofold, 0, sizeof(nofold));
  tail_fwd_launch<false, true>(c_raw, c_scale_shift, shortcut, r_scale_shift, keep, y, N, C, P, dtype, nofold, stream);
  X3D_LAUNCH_CHECK("tail_fwd_dp");
  return X3D_OK;
}

// small planes in 16-bit storage: the number of samples of one channel a workgroup of tail_bwd_small_kernel takes
// (0: the plane is not small, the general kernel takes it)
static inline int tail_small_nb(int dtype, int vec, int N, long long P) {
  if (dtype == X3D_F32 || vec != 8 || P / 8 >= ELEM_BLOCK) return 0;
  int nb = (int)(4 * ELEM_BLOCK / (P / 8));
  if (nb > N) nb = N;
  if (nb > 16) nb = 16;
  return nb;
}

// nb: tail_small_nb(), or 0 for the general kernel whatever the plane
template <bool DP>
static void tail_bwd_launch(void* dy_g, void* g_branch, const void* y, const void* c_raw, const void* r_raw, const float* keep,
                            double* sums_c, double* sums_r, int N, int C, long long P, int dtype, int vec, int nb, void* stream) {
  elem_dispatch(dtype, vec, [&](auto t, auto v) {
    typedef ELEM_T(t) T;
    constexpr int VEC = decltype(v)::value;
    if constexpr (VEC == 8) {
      if (nb > 0) {
        hipLaunchKernelGGL((tail_bwd_small_kernel<T, 8, DP>), dim3((unsigned)C, (unsigned)ceil_div(N, nb)), dim3(ELEM_BLOCK), 0,
                           (hipStream_t)stream, (T*)dy_g, (T*)g_branch, (const T*)y, (const T*)c_raw, (const T*)r_raw, keep, sums_c,
                           sums_r, N, C, (int)P, nb);
        return;
      }
    }
    hipLaunchKernelGGL((tail_bwd_kernel<T, VEC, DP>), elem_grid(P, vec, N * C), dim3(ELEM_BLOCK), 0, (hipStream_t)stream, (T*)dy_g,
                       (T*)g_branch, (const T*)y, (const T*)c_raw, (const T*)r_raw, keep, sums_c, sums_r, C, P);
  });
}

extern "C" int x3d_tail_bwd(void* dy_g, const void* y, const void* c_raw, const void* r_raw, double* sums_c,
                            double* sums_r, int N, int C, long long P, int dtype, void* stream) {
  X3D_REQUIRE(dy_g && y && c_raw && sums_c && N > 0 && C > 0 && P > 0, "tail_bwd: bad args");
  X3D_REQUIRE(!r_raw || sums_r, "tail_bwd: sums_r required with r_raw");
  X3D_REQUIRE(x3d_dtype_ok(dtype), "tail_bwd: bad dtype");
  const int eb = dtype == X3D_F32 ? 4 : 2;
  const int vec = norm_vec(dtype, pick_vec(eb, P, dy_g, y, c_raw, r_raw));
  // (X3D_TAIL_SMALL=0: A/B hook of the small-plane kernel)
  const int nb = x3d_env_int("X3D_TAIL_SMALL", 1) != 0 ? tail_small_nb(dtype, vec, N, P) : 0;
  tail_bwd_launch<false>(dy_g, nullptr, y, c_raw, r_raw, nullptr, sums_c, sums_r, N, C, P, dtype, vec, nb, stream);
  X3D_LAUNCH_CHECK("tail_bwd");
  return X3D_OK;
}

extern "C" int x3d_tail_bwd_dp(void* dy_g, void* g_branch, const void* y, const void* c_raw, const void* r_raw, const float* keep,
                               double* sums_c, double* sums_r, int N, int C, long long P, int dtype, void* stream) {
  X3D_REQUIRE(dy_g && g_branch && y && c_raw && keep && sums_c && N > 0 && C > 0 && P > 0, "tail_bwd_dp: bad args");
  X3D_REQUIRE(dy_g != g_branch, "tail_bwd_dp: g_branch must not alias dy_g");
  X3D_REQUIRE(!r_raw || sums_r, "tail_bwd_dp: sums_r required with r_raw");
  X3D_REQUIRE(x3d_dtype_ok(dtype), "tail_bwd_dp: bad dtype");
  const int eb = dtype == X3D_F32 ? 4 : 2;
  int vec = pick_vec(eb, P, dy_g, y, c_raw, r_raw);
  const int vec_g = pick_vec(eb, P, g_branch);      // (g_branch may be the one misaligned pointer)
  vec = norm_vec(dtype, vec < vec_g ? vec : vec_g);
  tail_bwd_launch<true>(dy_g, g_branch, y, c_raw, r_raw, keep, sums_c, sums_r, N, C, P, dtype, vec, tail_small_nb(dtype, vec, N, P),
                        stream);
  X3D_LAUNCH_CHECK("tail_bwd_dp");
  return X3D_OK;
}

extern "C" int x3d_relu_bn_bwd_reduce(const void* dy, const float* dpool, const void* yraw,
                                      const float* scale_shift, void* g, double* sums, int N, int C,
                                      long long P, int dtype, void* stream) {
  X3D_REQUIRE((dy != nullptr) != (dpool != nullptr), "relu_bn_bwd_reduce: exactly one of dy / dpool");
  X3D_REQUIRE(yraw && scale_shift && sums && N > 0 && C > 0 && P > 0, "relu_bn_bwd_reduce: bad args");
  X3D_REQUIRE(x3d_dtype_ok(dtype), "relu_bn_bwd_reduce: bad dtype");
  const int eb = dtype == X3D_F32 ? 4 : 2;
  const int vec = norm_vec(dtype, pick_vec(eb, P, dy, yraw, g));
  elem_dispatch(dtype, vec, [&](auto t, auto v) {
    typedef ELEM_T(t) T;
    hipLaunchKernelGGL((relu_bn_bwd_reduce_kernel<T, decltype(v)::value>), elem_grid(P, vec, N * C), dim3(ELEM_BLOCK), 0,
                       (hipStream_t)stream, (const T*)dy, dpool, (const T*)yraw, scale_shift, (T*)g, sums, C, P);
  });
  X3D_LAUNCH_CHECK("relu_bn_bwd_reduce");
  return X3D_OK;
}

extern "C" int x3d_pool_fwd(const void* x_raw, const float* scale_shift, float* pooled, int N, int C,
                            long long P, int dtype, void* stream) {
  X3D_REQUIRE(x_raw && scale_shift && pooled && N > 0 && C > 0 && P > 0, "pool_fwd: bad args");
  X3D_REQUIRE(x3d_dtype_ok(dtype), "pool_fwd: bad dtype");
  const int eb = dtype == X3D_F32 ? 4 : 2;
  const int vec = norm_vec(dtype, pick_vec(eb, P, x_raw));
  elem_dispatch(dtype, vec, [&](auto t, auto v) {
    typedef ELEM_T(t) T;
    hipLaunchKernelGGL((pool_fwd_kernel<T, decltype(v)::value>), dim3((unsigned)(N * C)), dim3(ELEM_BLOCK), 0, (hipStream_t)stream,
                       (const T*)x_raw, scale_shift, pooled, C, P);
  });
  X3D_LAUNCH_CHECK("pool_fwd");
  return X3D_OK;
}

// ------------------------------------------------------------------------------------------------
// module boundary: NTHWC (reference) -> NCTHW (internal).  C is tiny (3), P is huge: one thread per
// point reads C contiguous values and writes C planes (coalesced along P).
// ------------------------------------------------------------------------------------------------
template <typename TS, typename TD>
__global__ void nthwc_to_ncthw_kernel(const TS* __restrict__ src, TD* __restrict__ dst, int C, long long P) {
  const int n = blockIdx.y;
  const long long p = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (p >= P) return;
  const TS* s = src + ((long long)n * P + p) * C;
  for (int c = 0; c < C; c++) dst[((long long)n * C + c) * P + p] = from_f<TD>(to_f<TS>(s[c]));
}

// C = 3, P % 8 == 0, 16-byte aligned tensors (the clips of every X3D configuration): a thread takes 8 points -- 24
// contiguous source values as three vector loads -- and writes one 8-point vector per channel plane.  The one-point form
// above moves 2-byte pieces and is instruction bound (190 us for 64 clips of 16 x 224 x 224 against ~40 us of HBM time).
template <typename TS, typename TD>
__global__ __launch_bounds__(256) void nthwc_to_ncthw_c3_kernel(const TS* __restrict__ src, TD* __restrict__ dst, long long P8) {
  const int n = blockIdx.y;
  const long long q = (long long)blockIdx.x * blockDim.x + threadIdx.x;   // group of 8 points
  if (q >= P8) return;
  float v[3][8];
  const TS* s = src + ((long long)n * P8 + q) * 24;
#pragma unroll
  for (int k = 0; k < 3; k++) VecIO<TS, 8>::load(s + 8 * k, v[k]);
#pragma unroll
  for (int c = 0; c < 3; c++) {
    float o[8];
#pragma unroll
    for (int j = 0; j < 8; j++) o[j] = v[(3 * j + c) >> 3][(3 * j + c) & 7];
    VecIO<TD, 8>::store(dst + ((long long)n * 3 + c) * (P8 * 8) + q * 8, o);
  }
}
template <typename TS, typename TD>
static bool nthwc_c3_fast(const void* src, void* dst, int N, int C, long long P, hipStream_t st) {
  if (C != 3 || (P & 7) || ((uintptr_t)src & 15) || ((uintptr_t)dst & 15)) return false;
  const long long P8 = P >> 3;
  dim3 grid((unsigned)ceil_div_ll(P8, 256), (unsigned)N);
  hipLaunchKernelGGL((nthwc_to_ncthw_c3_kernel<TS, TD>), grid, dim3(256), 0, st, (const TS*)src, (TD*)dst, P8);
  return true;
}

extern "C" int x3d_nthwc_to_ncthw(const void* src, int src_dtype, void* dst, int dst_dtype, int N, int C,
                                  long long P, void* stream) {
  X3D_REQUIRE(src && dst && N > 0 && C > 0 && P > 0, "nthwc_to_ncthw: bad args");
  dim3 grid((unsigned)ceil_div_ll(P, 256), (unsigned)N);
  hipStream_t st = (hipStream_t)stream;
  if (src_dtype == X3D_F32 && dst_dtype == X3D_F32)
    { if (!nthwc_c3_fast<float, float>(src, dst, N, C, P, st))
      hipLaunchKernelGGL((nthwc_to_ncthw_kernel<float, float>), grid, dim3(256), 0, st, (const float*)src, (float*)dst, C, P); }
  else if (src_dtype == X3D_F32 && dst_dtype == X3D_BF16)
    { if (!nthwc_c3_fast<float, bf16>(src, dst, N, C, P, st))
      hipLaunchKernelGGL((nthwc_to_ncthw_kernel<float, bf16>), grid, dim3(256), 0, st, (const float*)src, (bf16*)dst, C, P); }
  else if (src_dtype == X3D_BF16 && dst_dtype == X3D_BF16)
    { if (!nthwc_c3_fast<bf16, bf16>(src, dst, N, C, P, st))
      hipLaunchKernelGGL((nthwc_to_ncthw_kernel<bf16, bf16>), grid, dim3(256), 0, st, (const bf16*)src, (bf16*)dst, C, P); }
  else if (src_dtype == X3D_BF16 && dst_dtype == X3D_F32)
    { if (!nthwc_c3_fast<bf16, float>(src, dst, N, C, P, st))
      hipLaunchKernelGGL((nthwc_to_ncthw_kernel<bf16, float>), grid, dim3(256), 0, st, (const bf16*)src, (float*)dst, C, P); }
  else if (src_dtype == X3D_F32 && dst_dtype == X3D_F16)
    { if (!nthwc_c3_fast<float, f16>(src, dst, N, C, P, st))
      hipLaunchKernelGGL((nthwc_to_ncthw_kernel<float, f16>), grid, dim3(256), 0, st, (const float*)src, (f16*)dst, C, P); }
  else if (src_dtype == X3D_F16 && dst_dtype == X3D_F16)
    { if (!nthwc_c3_fast<f16, f16>(src, dst, N, C, P, st))
      hipLaunchKernelGGL((nthwc_to_ncthw_kernel<f16, f16>), grid, dim3(256), 0, st, (const f16*)src, (f16*)dst, C, P); }
  else if (src_dtype == X3D_F16 && dst_dtype == X3D_F32)
    { if (!nthwc_c3_fast<f16, float>(src, dst, N, C, P, st))
      hipLaunchKernelGGL((nthwc_to_ncthw_kernel<f16, float>), grid, dim3(256), 0, st, (const f16*)src, (float*)dst, C, P); }
  else {
    x3d_set_error("nthwc_to_ncthw: bad dtype");
    return X3D_ERR_INVALID;
  }
  X3D_LAUNCH_CHECK("nthwc_to_ncthw");
  return X3D_OK;
}


// ------------------------------------------------------------------------------------------------------------------------
// Even-pixel copy of a block input: dst[plane][ho][wo] = src[plane][2 ho][2 wo], Ho = ceil(H / 2), Wo = ceil(W / 2) -- the pixels
// a stride-(1,2,2) 'valid' 1x1x1 shortcut conv samples (reference model.py:360-367).  Round 6: with this compact tensor the
// shortcut conv's forward, data gradient and weight gradient are plain dense launches (16-byte coalesced rows) instead of the
// strided gathers, whose rows of 7 / 14 outputs took one output per 4-byte load (96 -> 192 @14^2: 68 us for 29 MB).
// One thread = VEC consecutive outputs of an output row: 2 * VEC input elements in one aligned load (VEC = 8 / 4 / 2), or
// element loads (odd widths).
// ------------------------------------------------------------------------------------------------------------------------
template <typename T, int VEC>
__global__ __launch_bounds__(256) void subsample2_kernel(const T* __restrict__ src, T* __restrict__ dst, int H, int W, int Ho, int Wo,
                                                         long long rows /* planes * Ho */) {
  const int vpr = (Wo + VEC - 1) / VEC;                       // vectors per output row (VEC > 1: Wo % VEC == 0, host check)
  const long long v = (long long)blockIdx.x * 256 + threadIdx.x;
  if (v >= rows * vpr) return;
  const long long row = v / vpr;
  const int wo0 = (int)(v - row * vpr) * VEC;
  const long long plane = row / Ho;
  const int ho = (int)(row - plane * Ho);
  const T* s = src + (plane * H + 2 * ho) * (long long)W + 2 * wo0;
  T* d = dst + row * Wo + wo0;
  if constexpr (VEC == 1) {
    d[0] = s[0];
  } else {
    typedef __attribute__((ext_vector_type(2 * VEC))) T in_t;
    typedef __attribute__((ext_vector_type(VEC))) T out_t;
    const in_t a = *(const in_t*)s;
    out_t o;
#pragma unroll
    for (int e = 0; e < VEC; e++) o[e] = a[2 * e];
    *(out_t*)d = o;
  }
}

template <typename T>
static void subsample2_launch(const void* src, void* dst, long long planes, int H, int W, hipStream_t st) {
  const int Ho = (H + 1) / 2, Wo = (W + 1) / 2;
  const long long rows = planes * Ho;
  int vec = 1;
  // 2 * vec input elements per load: rows of whole loads (W % (2 vec) == 0), both tensors aligned for their vector
  for (int v = 16 / (int)sizeof(T); v >= 2; v >>= 1)
    if ((W % (2 * v)) == 0 && ((uintptr_t)src % (2 * v * sizeof(T))) == 0 && ((uintptr_t)dst % (v * sizeof(T))) == 0) { vec = v; break; }
  const long long nv = rows * ((Wo + vec - 1) / vec);
  const unsigned grid = (unsigned)ceil_div_ll(nv, 256);
#define SS2(V) hipLaunchKernelGGL((subsample2_kernel<T, V>), dim3(grid), dim3(256), 0, st, (const T*)src, (T*)dst, H, W, Ho, Wo, rows)
  switch (vec) {
    case 8: if constexpr (sizeof(T) == 2) { SS2(8); } break;
    case 4: SS2(4); break;
    case 2: SS2(2); break;
    default: SS2(1); break;
  }
#undef SS2
}

extern "C" int x3d_subsample2(const void* src, void* dst, long long planes, int H, int W, int dtype, void* stream) {
  X3D_REQUIRE(src && dst && planes > 0 && H > 0 && W > 0, "subsample2: bad args");
  X3D_REQUIRE(x3d_dtype_ok(dtype), "subsample2: bad dtype");
  X3D_REQUIRE(ceil_div_ll(planes * ((H + 1) / 2) * ((W + 1) / 2), 256) < (1ll << 31), "subsample2: grid too large");
  hipStream_t st = (hipStream_t)stream;
  if (dtype == X3D_F32) subsample2_launch<float>(src, dst, planes, H, W, st);
  else subsample2_launch<unsigned short>(src, dst, planes, H, W, st);      // (a copy: the 16-bit types move as bits)
  X3D_LAUNCH_CHECK("subsample2");
  return X3D_OK;
}
