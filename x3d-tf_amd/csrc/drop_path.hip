// Stochastic depth (drop-path) of the bottleneck branch, per sample (include/x3d_hip.h K9d): the keep table drawn on the device
// from a counter-based generator, and the residual tail forward / backward that apply it.  The tail kernels keep the forms of
// elem.hip's x3d_tail_fwd / x3d_tail_bwd (grid = (chunks over P, N*C), 8-wide 16-bit / 4-wide fp32 vectors or scalars, the
// small-plane backward with several samples of one channel per workgroup); what is new is keep[n] -- uniform per workgroup in
// the (n, c) grid, read through a scalar load -- and the uniform branch on it that leaves a dropped sample's c_raw unread.
#include "common.h"

// ------------------------------------------------------------------------------------------------
// Philox4x32-10 (Salmon et al., "Parallel random numbers: as easy as 1, 2, 3", SC'11): counter (c0, c1, c2, c3), key (k0, k1).
// A device function of its own so that other draws (the head dropout) can move onto it.
// ------------------------------------------------------------------------------------------------
struct Philox4 { uint32_t v[4]; };
__host__ __device__ __forceinline__ Philox4 philox4x32_10(uint32_t c0, uint32_t c1, uint32_t c2, uint32_t c3, uint32_t k0,
                                                          uint32_t k1) {
  const uint32_t M0 = 0xD2511F53u, M1 = 0xCD9E8D57u;
#pragma unroll
  for (int r = 0; r < 10; r++) {
    const uint64_t p0 = (uint64_t)M0 * c0, p1 = (uint64_t)M1 * c2;
    const uint32_t n0 = (uint32_t)(p1 >> 32) ^ c1 ^ k0, n2 = (uint32_t)(p0 >> 32) ^ c3 ^ k1;
    c1 = (uint32_t)p1; c3 = (uint32_t)p0; c0 = n0; c2 = n2;
    k0 += 0x9E3779B9u; k1 += 0xBB67AE85u;
  }
  Philox4 o;
  o.v[0] = c0; o.v[1] = c1; o.v[2] = c2; o.v[3] = c3;
  return o;
}
// uniform in [0, 1) on a 2^-24 grid: exact in fp32
__host__ __device__ __forceinline__ float philox_u24(uint32_t w) { return (float)(w >> 8) * 5.9604644775390625e-8f; }

#define DRAW_BLOCK 256
// ONE workgroup, and only its thread 0 touches `state`: it reads seed and step, hands them to the others through LDS and
// stores step + 1 -- nothing else reads or writes the step, so there is no race to order
__global__ __launch_bounds__(DRAW_BLOCK) void drop_path_draw_kernel(float* __restrict__ keep, const float* __restrict__ rates,
                                                                    uint32_t* state, int L, int N) {
  __shared__ uint32_t st[4];
  if (threadIdx.x == 0) {
#pragma unroll
    for (int i = 0; i < 4; i++) st[i] = state[i];
    const uint64_t next = (((uint64_t)st[3] << 32) | st[2]) + 1ull;
    state[2] = (uint32_t)next;
    state[3] = (uint32_t)(next >> 32);
  }
  __syncthreads();
  const uint32_t k0 = st[0], k1 = st[1], s_lo = st[2], s_hi = st[3];
  const int total = L * N;
  for (int i = threadIdx.x; i < total; i += DRAW_BLOCK) {
    const int l = i / N, n = i - l * N;
    const float rate = rates[l];
    const float u = philox_u24(philox4x32_10(s_lo, s_hi, (uint32_t)l, (uint32_t)n, k0, k1).v[0]);
    keep[i] = u >= rate ? 1.0f / (1.0f - rate) : 0.f;
  }
}

extern "C" int x3d_drop_path_draw(float* keep, const float* rates, void* state, int L, int N, void* stream) {
  X3D_REQUIRE(keep && rates && state && L > 0 && N > 0, "drop_path_draw: bad args");
  X3D_REQUIRE((long long)L * N <= 65536, "drop_path_draw: table of %d x %d entries (one workgroup draws at most 65536)", L, N);
  hipLaunchKernelGGL(drop_path_draw_kernel, dim3(1), dim3(DRAW_BLOCK), 0, (hipStream_t)stream, keep, rates, (uint32_t*)state, L, N);
  X3D_LAUNCH_CHECK("drop_path_draw");
  return X3D_OK;
}

// ------------------------------------------------------------------------------------------------
// tail forward / backward.  grid = (chunks over P, N*C); each thread handles VEC contiguous elements per iteration.
// ------------------------------------------------------------------------------------------------
#define DP_BLOCK 256
#define DP_ITERS 4

static inline dim3 dp_grid(long long P, int vec, int NC) {
  return dim3((unsigned)ceil_div_ll(P, (long long)DP_BLOCK * vec * DP_ITERS), (unsigned)NC);
}
static inline int dp_norm_vec(int dtype, int vec) {
  const int full = dtype == X3D_F32 ? 4 : 8;
  return vec >= full ? full : 1;
}

// y = relu(keep[n] * (sc*craw + tc) + (sr*sh + tr)); keep[n] == 0: y = relu(sr*sh + tr), craw not loaded
template <typename T, int VEC>
__global__ __launch_bounds__(DP_BLOCK) void tail_fwd_dp_kernel(const T* __restrict__ craw, const float* __restrict__ ssc,
                                                               const T* __restrict__ sh, const float* __restrict__ ssr,
                                                               const float* __restrict__ keep, T* __restrict__ y, int C,
                                                               long long P) {
  const int nc = blockIdx.y, n = nc / C, c = nc - n * C;
  const float k = keep[n];
  const float sc = ssc[c * 2], tc = ssc[c * 2 + 1];
  float sr = 1.f, tr = 0.f;
  if (ssr) { sr = ssr[c * 2]; tr = ssr[c * 2 + 1]; }
  const long long base = (long long)nc * P;
  long long p = ((long long)blockIdx.x * DP_ITERS * DP_BLOCK + threadIdx.x) * VEC;
  if (k == 0.f) {
#pragma unroll
    for (int it = 0; it < DP_ITERS; it++, p += (long long)DP_BLOCK * VEC) {
      if (p < P) {
        float b[VEC], o[VEC];
        VecIO<T, VEC>::load(sh + base + p, b);
#pragma unroll
        for (int e = 0; e < VEC; e++) o[e] = fmaxf(sr * b[e] + tr, 0.f);
        VecIO<T, VEC>::store(y + base + p, o);
      }
    }
  } else {
#pragma unroll
    for (int it = 0; it < DP_ITERS; it++, p += (long long)DP_BLOCK * VEC) {
      if (p < P) {
        float a[VEC], b[VEC], o[VEC];
        VecIO<T, VEC>::load(craw + base + p, a);
        VecIO<T, VEC>::load(sh + base + p, b);
#pragma unroll
        for (int e = 0; e < VEC; e++) o[e] = fmaxf(k * (sc * a[e] + tc) + (sr * b[e] + tr), 0.f);
        VecIO<T, VEC>::store(y + base + p, o);
      }
    }
  }
}

// red: (sum g, sum gb, sum gb*craw, sum g*rraw) of one workgroup -> the fp64 accumulators
__device__ __forceinline__ void tail_bwd_dp_flush(const float (&red)[4], bool any_kept, bool has_r, double* sums_c, double* sums_r,
                                                  int c) {
  if (any_kept) {
    atomic_add_d(&sums_c[c * 2], (double)red[1]);
    atomic_add_d(&sums_c[c * 2 + 1], (double)red[2]);
  }
  if (has_r) {
    atomic_add_d(&sums_r[c * 2], (double)red[0]);
    atomic_add_d(&sums_r[c * 2 + 1], (double)red[3]);
  }
}

// g = dy*[y>0] in place; gb = round(keep[n]*g) into gbr; sums_c += (sum gb, sum gb*craw); sums_r += (sum g, sum g*rraw)
template <typename T, int VEC>
__global__ __launch_bounds__(DP_BLOCK) void tail_bwd_dp_kernel(T* __restrict__ dyg, T* __restrict__ gbr, const T* __restrict__ y,
                                                               const T* __restrict__ craw, const T* __restrict__ rraw,
                                                               const float* __restrict__ keep, double* sums_c, double* sums_r,
                                                               int C, long long P) {
  __shared__ float scratch[4 * (DP_BLOCK / 64)];
  const int nc = blockIdx.y, n = nc / C, c = nc - n * C;
  const float k = keep[n];
  const long long base = (long long)nc * P;
  float red[4] = {0.f, 0.f, 0.f, 0.f};
  long long p = ((long long)blockIdx.x * DP_ITERS * DP_BLOCK + threadIdx.x) * VEC;
  if (k == 0.f) {
#pragma unroll
    for (int it = 0; it < DP_ITERS; it++, p += (long long)DP_BLOCK * VEC) {
      if (p < P) {
        float d[VEC], yy[VEC], rr[VEC], g[VEC], z[VEC];
        VecIO<T, VEC>::load(dyg + base + p, d);
        VecIO<T, VEC>::load(y + base + p, yy);
        if (rraw) VecIO<T, VEC>::load(rraw + base + p, rr);
#pragma unroll
        for (int e = 0; e < VEC; e++) {
          g[e] = yy[e] > 0.f ? d[e] : 0.f;
          z[e] = 0.f;
          if (rraw) { red[0] += g[e]; red[3] += g[e] * rr[e]; }
        }
        VecIO<T, VEC>::store(dyg + base + p, g);
        VecIO<T, VEC>::store(gbr + base + p, z);
      }
    }
  } else {
#pragma unroll
    for (int it = 0; it < DP_ITERS; it++, p += (long long)DP_BLOCK * VEC) {
      if (p < P) {
        float d[VEC], yy[VEC], cr[VEC], rr[VEC], g[VEC], gb[VEC];
        VecIO<T, VEC>::load(dyg + base + p, d);
        VecIO<T, VEC>::load(y + base + p, yy);
        VecIO<T, VEC>::load(craw + base + p, cr);
        if (rraw) VecIO<T, VEC>::load(rraw + base + p, rr);
#pragma unroll
        for (int e = 0; e < VEC; e++) {
          g[e] = yy[e] > 0.f ? d[e] : 0.f;
          gb[e] = round_to<T>(k * g[e]);
          red[1] += gb[e];
          red[2] += gb[e] * cr[e];
          if (rraw) { red[0] += g[e]; red[3] += g[e] * rr[e]; }
        }
        VecIO<T, VEC>::store(dyg + base + p, g);
        VecIO<T, VEC>::store(gbr + base + p, gb);
      }
    }
  }
  block_sum<4>(red, scratch);
  if (threadIdx.x == 0) tail_bwd_dp_flush(red, k != 0.f, rraw != nullptr, sums_c, sums_r, c);
}

// ... small planes (P / VEC < 256: the 7 x 7 stage), as elem.hip's tail_bwd_small_kernel: one workgroup takes NB samples of
// ONE channel, grid = (C, ceil(N / NB)), the flat index runs over (sample in the group, vector of the plane).  keep belongs to
// the sample, so here it is per lane: a dropped sample's lanes skip the c_raw load and add nothing to sums_c.
template <typename T, int VEC>
__global__ __launch_bounds__(DP_BLOCK) void tail_bwd_dp_small_kernel(T* __restrict__ dyg, T* __restrict__ gbr, const T* __restrict__ y,
                                                                     const T* __restrict__ craw, const T* __restrict__ rraw,
                                                                     const float* __restrict__ keep, double* sums_c,
                                                                     double* sums_r, int N, int C, int P, int NB) {
  __shared__ float scratch[4 * (DP_BLOCK / 64)];
  const int c = blockIdx.x, n0 = blockIdx.y * NB;
  const int nb = min(NB, N - n0);
  const int vpp = P / VEC, total = nb * vpp;
  float red[4] = {0.f, 0.f, 0.f, 0.f};
  for (int i0 = threadIdx.x; i0 < total; i0 += 2 * DP_BLOCK) {
    // two vectors per thread and round, their loads issued together
    float d[2][VEC], yy[2][VEC], cr[2][VEC], rr[2][VEC], k[2];
    long long off[2];
    bool ok[2];
#pragma unroll
    for (int u = 0; u < 2; u++) {
      const int i = i0 + u * DP_BLOCK;
      ok[u] = i < total;
      const int nl = ok[u] ? i / vpp : 0, pv = ok[u] ? i - nl * vpp : 0;
      off[u] = ((long long)(n0 + nl) * C + c) * P + (long long)pv * VEC;
      k[u] = ok[u] ? keep[n0 + nl] : 0.f;
#pragma unroll
      for (int e = 0; e < VEC; e++) cr[u][e] = 0.f;
      if (ok[u]) {
        VecIO<T, VEC>::load(dyg + off[u], d[u]);
        VecIO<T, VEC>::load(y + off[u], yy[u]);
        if (k[u] != 0.f) VecIO<T, VEC>::load(craw + off[u], cr[u]);
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
        gb[e] = round_to<T>(k[u] * g[e]);
        red[1] += gb[e];
        red[2] += gb[e] * cr[u][e];
        if (rraw) { red[0] += g[e]; red[3] += g[e] * rr[u][e]; }
      }
      VecIO<T, VEC>::store(dyg + off[u], g);
      VecIO<T, VEC>::store(gbr + off[u], gb);
    }
  }
  block_sum<4>(red, scratch);
  // (a group of dropped samples only adds exact zeros to sums_c)
  if (threadIdx.x == 0) tail_bwd_dp_flush(red, true, rraw != nullptr, sums_c, sums_r, c);
}

extern "C" int x3d_tail_fwd_dp(const void* c_raw, const float* c_scale_shift, const void* shortcut, const float* r_scale_shift,
                               const float* keep, void* y, int N, int C, long long P, int dtype, void* stream) {
  X3D_REQUIRE(c_raw && c_scale_shift && y && keep && N > 0 && C > 0 && P > 0, "tail_fwd_dp: bad args");
  X3D_REQUIRE(shortcut, "tail_fwd_dp: shortcut required (the stem's BatchNorm + ReLU has no branch to drop)");
  X3D_REQUIRE(x3d_dtype_ok(dtype), "tail_fwd_dp: bad dtype");
  const int eb = dtype == X3D_F32 ? 4 : 2;
  const int vec = dp_norm_vec(dtype, pick_vec(eb, P, c_raw, shortcut, y));
  hipStream_t st = (hipStream_t)stream;
  dim3 grid = dp_grid(P, vec, N * C);
#define ARGS(T) (const T*)c_raw, c_scale_shift, (const T*)shortcut, r_scale_shift, keep, (T*)y, C, P
  if (dtype == X3D_F32) {
    if (vec == 4) hipLaunchKernelGGL((tail_fwd_dp_kernel<float, 4>), grid, dim3(DP_BLOCK), 0, st, ARGS(float));
    else hipLaunchKernelGGL((tail_fwd_dp_kernel<float, 1>), grid, dim3(DP_BLOCK), 0, st, ARGS(float));
  } else if (dtype == X3D_F16) {
    if (vec == 8) hipLaunchKernelGGL((tail_fwd_dp_kernel<f16, 8>), grid, dim3(DP_BLOCK), 0, st, ARGS(f16));
    else hipLaunchKernelGGL((tail_fwd_dp_kernel<f16, 1>), grid, dim3(DP_BLOCK), 0, st, ARGS(f16));
  } else {
    if (vec == 8) hipLaunchKernelGGL((tail_fwd_dp_kernel<bf16, 8>), grid, dim3(DP_BLOCK), 0, st, ARGS(bf16));
    else hipLaunchKernelGGL((tail_fwd_dp_kernel<bf16, 1>), grid, dim3(DP_BLOCK), 0, st, ARGS(bf16));
  }
#undef ARGS
  X3D_LAUNCH_CHECK("tail_fwd_dp");
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
  const int vec_g = pick_vec(eb, P, g_branch);
  vec = dp_norm_vec(dtype, vec < vec_g ? vec : vec_g);
  hipStream_t st = (hipStream_t)stream;
  dim3 grid = dp_grid(P, vec, N * C);
  // small planes in 16-bit storage: NB samples of one channel per workgroup
  if (dtype != X3D_F32 && vec == 8 && P / 8 < DP_BLOCK) {
    int nb = (int)(4 * DP_BLOCK / (P / 8));
    if (nb > N) nb = N;
    if (nb > 16) nb = 16;
    const dim3 g2((unsigned)C, (unsigned)ceil_div(N, nb));
    if (dtype == X3D_F16)
      hipLaunchKernelGGL((tail_bwd_dp_small_kernel<f16, 8>), g2, dim3(DP_BLOCK), 0, st, (f16*)dy_g, (f16*)g_branch, (const f16*)y,
                         (const f16*)c_raw, (const f16*)r_raw, keep, sums_c, sums_r, N, C, (int)P, nb);
    else
      hipLaunchKernelGGL((tail_bwd_dp_small_kernel<bf16, 8>), g2, dim3(DP_BLOCK), 0, st, (bf16*)dy_g, (bf16*)g_branch, (const bf16*)y,
                         (const bf16*)c_raw, (const bf16*)r_raw, keep, sums_c, sums_r, N, C, (int)P, nb);
    X3D_LAUNCH_CHECK("tail_bwd_dp");
    return X3D_OK;
  }
#define ARGS(T) (T*)dy_g, (T*)g_branch, (const T*)y, (const T*)c_raw, (const T*)r_raw, keep, sums_c, sums_r, C, P
  if (dtype == X3D_F32) {
    if (vec == 4) hipLaunchKernelGGL((tail_bwd_dp_kernel<float, 4>), grid, dim3(DP_BLOCK), 0, st, ARGS(float));
    else hipLaunchKernelGGL((tail_bwd_dp_kernel<float, 1>), grid, dim3(DP_BLOCK), 0, st, ARGS(float));
  } else if (dtype == X3D_F16) {
    if (vec == 8) hipLaunchKernelGGL((tail_bwd_dp_kernel<f16, 8>), grid, dim3(DP_BLOCK), 0, st, ARGS(f16));
    else hipLaunchKernelGGL((tail_bwd_dp_kernel<f16, 1>), grid, dim3(DP_BLOCK), 0, st, ARGS(f16));
  } else {
    if (vec == 8) hipLaunchKernelGGL((tail_bwd_dp_kernel<bf16, 8>), grid, dim3(DP_BLOCK), 0, st, ARGS(bf16));
    else hipLaunchKernelGGL((tail_bwd_dp_kernel<bf16, 1>), grid, dim3(DP_BLOCK), 0, st, ARGS(bf16));
  }
#undef ARGS
  X3D_LAUNCH_CHECK("tail_bwd_dp");
  return X3D_OK;
}
