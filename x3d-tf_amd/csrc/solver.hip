// The solver step on the flat fp32 buffers: SGD-Nesterov / Adam (+ L2), and around them global-norm gradient clipping,
// gradient accumulation and an exponential moving average of the weights -- without a host round trip.
//
//   x3d_grad_sumsq          sum of squares of the gradient in fp64 + the number of non-finite entries: one pass over g into
//                           per-workgroup partials, one tiny launch that adds them in a fixed order.  No floating-point
//                           atomics anywhere in this file: the same inputs give the same bits on every run.
//   x3d_sgd_nesterov(_ex)   the update.  _ex reads the clip coefficient (and whether to skip the step) from the two doubles
//   x3d_adam(_ex)           x3d_grad_sumsq left in device memory and writes the weight EMA in the same pass.
//   x3d_ema_update          the same EMA rule for buffers the optimizer does not own (BatchNorm moving statistics)
//   x3d_grad_accum          acc = g / acc += g
//
// Shape.  Plain streaming kernels: a thread moves 16 bytes per array and iteration, the grid is capped at SOLVER_MAX_BLOCKS
// workgroups and strides over the rest.  The vector kernels need every array 16-byte aligned (the l2 mask 4-byte); the n % 4
// elements at the end are further one-element work items of the same grid-stride walk.  Any other pointer takes the one-element
// instantiation of the same kernel.  The plain entry points keep their one-element-per-thread launch: their results and
// their speed are what they were.
//
// The update arithmetic exists once: sgd_nesterov_step / adam_step below, called by the old and the new kernels.
#include "common.h"

#define SOLVER_BLOCK 256
#define SOLVER_MAX_BLOCKS 1024          // = the largest partial count of x3d_grad_sumsq
#define SOLVER_UNROLL 4                 // vectors a workgroup's thread takes before the grid is made larger

// ------------------------------------------------------------------------------------------------
// K12  the one definition of the update arithmetic
// ------------------------------------------------------------------------------------------------
// Every rounding is written out (no contraction left to the compiler): which products fuse into an FMA otherwise depends on
// the code around the call, and the plain kernels, the _ex kernels and their one-element paths must agree to the bit.  The
// choice of fusions is the one the plain kernels have always had.
//
// g' = g*gscale + 2*wd*w (where l2) ; v = mom*v - lr*g' ; w = w + mom*v - lr*g'
__device__ __forceinline__ void sgd_nesterov_step(float& w, float& v, float g, bool l2, float lr, float mom, float wd,
                                                  float gscale) {
#pragma clang fp contract(off)
  float gi = g * gscale;
  const float wi = w;
  if (l2) gi = __builtin_fmaf(wd + wd, wi, gi);
  const float step = lr * gi;
  const float vi = __builtin_fmaf(mom, v, -step);
  v = vi;
  w = __builtin_fmaf(-lr, gi, __builtin_fmaf(mom, vi, wi));
}

// Adam (tf.optimizers.Adam(learning_rate), the reference's other optimizer branch, train.py:93-95; Keras defaults
// beta_1 = 0.9, beta_2 = 0.999, epsilon = 1e-7, no amsgrad):  g' as above
//   m = b1*m + (1-b1)*g' ; v = b2*v + (1-b2)*g'^2 ; w -= lr_t * m / (sqrt(v) + eps), lr_t = lr*sqrt(1-b2^t)/(1-b1^t)  [TF-3p]
__device__ __forceinline__ void adam_step(float& w, float& m, float& v, float g, bool l2, float lr_t, float b1, float b2,
                                          float eps, float wd, float gscale) {
#pragma clang fp contract(off)
  float gi = g * gscale;
  const float wi = w;
  if (l2) gi = __builtin_fmaf(wd + wd, wi, gi);
  const float mi = __builtin_fmaf(1.f - b1, gi, b1 * m);
  const float vi = __builtin_fmaf(gi, (1.f - b2) * gi, b2 * v);
  m = mi;
  v = vi;
  w = wi - (lr_t * mi) / (sqrtf(vi) + eps);
}

// ema = d*ema + (1-d)*w, evaluated as ema + (1-d)*(w - ema): w == ema is a fixed point for every d
__device__ __forceinline__ float ema_step(float e, float w, float omd) { return __builtin_fmaf(omd, w - e, e); }

// norm = the out[2] of x3d_grad_sumsq.  false: a non-finite gradient, the launch writes nothing.  Else c = the factor the
// raw gradient is multiplied by: grad_scale * min(1, max_norm / (||g|| * grad_scale + 1e-6)), torch's clip_grad_norm_ rule
// on the unscaled gradient; fp64, rounded once (no clipping: exactly grad_scale).
__device__ __forceinline__ bool solver_coef(const double* __restrict__ norm, float gscale, float max_norm, float& c) {
  c = gscale;
  if (!norm) return true;
  if (norm[1] != 0.0) return false;
  const double total = sqrt(norm[0]) * (double)gscale;
  c = (float)((double)gscale * fmin(1.0, (double)max_norm / (total + 1e-6)));
  return true;
}

static inline double adam_lr_t(float lr, float beta1, float beta2, long long step) {
  return (double)lr * sqrt(1.0 - pow((double)beta2, (double)step)) / (1.0 - pow((double)beta1, (double)step));
}

// ------------------------------------------------------------------------------------------------
// the plain entry points: one element per thread, as they always were
// ------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void sgd_nesterov_kernel(float* __restrict__ w, float* __restrict__ v,
                                                           const float* __restrict__ g,
                                                           const unsigned char* __restrict__ l2, float lr, float mom,
                                                           float wd, float gscale, long long n) {
  const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  float wi = w[i], vi = v[i];
  sgd_nesterov_step(wi, vi, g[i], l2 && l2[i], lr, mom, wd, gscale);
  v[i] = vi;
  w[i] = wi;
}

extern "C" int x3d_sgd_nesterov(float* w, float* v, const float* g, const unsigned char* l2_mask, float lr,
                                float momentum, float weight_decay, float grad_scale, long long n, void* stream) {
  X3D_REQUIRE(w && v && g && n > 0, "sgd_nesterov: bad args");
  hipLaunchKernelGGL(sgd_nesterov_kernel, dim3((unsigned)ceil_div_ll(n, 256)), dim3(256), 0, (hipStream_t)stream, w,
                     v, g, l2_mask, lr, momentum, weight_decay, grad_scale, n);
  X3D_LAUNCH_CHECK("sgd_nesterov");
  return X3D_OK;
}

__global__ __launch_bounds__(256) void adam_kernel(float* __restrict__ w, float* __restrict__ m, float* __restrict__ v,
                                                   const float* __restrict__ g, const unsigned char* __restrict__ l2,
                                                   float lr_t, float b1, float b2, float eps, float wd, float gscale,
                                                   long long n) {
  const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  float wi = w[i], mi = m[i], vi = v[i];
  adam_step(wi, mi, vi, g[i], l2 && l2[i], lr_t, b1, b2, eps, wd, gscale);
  m[i] = mi;
  v[i] = vi;
  w[i] = wi;
}

extern "C" int x3d_adam(float* w, float* m, float* v, const float* g, const unsigned char* l2_mask, float lr, float beta1,
                        float beta2, float eps, float weight_decay, float grad_scale, long long step, long long n,
                        void* stream) {
  X3D_REQUIRE(w && m && v && g && n > 0 && step >= 1, "adam: bad args (step counts from 1)");
  hipLaunchKernelGGL(adam_kernel, dim3((unsigned)ceil_div_ll(n, 256)), dim3(256), 0, (hipStream_t)stream, w, m, v, g,
                     l2_mask, (float)adam_lr_t(lr, beta1, beta2, step), beta1, beta2, eps, weight_decay, grad_scale, n);
  X3D_LAUNCH_CHECK("adam");
  return X3D_OK;
}

// ------------------------------------------------------------------------------------------------
// streaming helpers of the new kernels
// ------------------------------------------------------------------------------------------------
// Work items of a launch over n elements in vectors of VEC: the n / VEC whole vectors, then the n % VEC last elements as
// items of one element each.  item -> (first element, count); every item is inside [0, n).
template <int VEC>
__device__ __forceinline__ void solver_item(long long item, long long n, long long& first, int& count) {
  const long long nv = n / VEC;
  if (item < nv) { first = item * VEC; count = VEC; }
  else { first = nv * VEC + (item - nv); count = 1; }
}
static inline long long solver_items(long long n, int vec) { return n / vec + n % vec; }
static inline unsigned solver_grid(long long items) {
  long long b = ceil_div_ll(items, (long long)SOLVER_BLOCK * SOLVER_UNROLL);
  if (b > SOLVER_MAX_BLOCKS) b = SOLVER_MAX_BLOCKS;
  return (unsigned)(b < 1 ? 1 : b);
}
// 4 when every array given is 16-byte aligned and the mask (if any) 4-byte aligned, else 1
static inline int solver_vec(const void* mask, const void* p0, const void* p1 = nullptr, const void* p2 = nullptr,
                             const void* p3 = nullptr, const void* p4 = nullptr) {
  const void* ps[5] = {p0, p1, p2, p3, p4};
  for (const void* p : ps)
    if (p && ((uintptr_t)p & 15)) return 1;
  if (mask && ((uintptr_t)mask & 3)) return 1;
  return 4;
}

template <int VEC> __device__ __forceinline__ void load_mask(const unsigned char* l2, long long i, bool (&o)[VEC]) {
  if (!l2) {
#pragma unroll
    for (int e = 0; e < VEC; e++) o[e] = false;
  } else if constexpr (VEC == 4) {
    const unsigned u = *(const unsigned*)(l2 + i);
#pragma unroll
    for (int e = 0; e < 4; e++) o[e] = ((u >> (8 * e)) & 0xffu) != 0;
  } else {
    o[0] = l2[i] != 0;
  }
}

// ------------------------------------------------------------------------------------------------
// x3d_grad_sumsq
// ------------------------------------------------------------------------------------------------
static inline long long sumsq_parts(long long n) { return n > 0 ? (long long)solver_grid(solver_items(n, 4)) : 0; }

__device__ __forceinline__ void sumsq_add(float x, double& s, unsigned& bad) {
  const bool fin = (__float_as_uint(x) & 0x7f800000u) != 0x7f800000u;   // exponent all ones: inf or nan
  const double d = fin ? (double)x : 0.0;
  s += d * d;                                                            // the square in fp64: 1e-30 and 1e18 are fine
  bad += fin ? 0u : 1u;
}

// scratch [2][parts]: partial sums, then partial counts.  Every workgroup writes its slot (zero when it had no item).
template <int VEC>
__global__ __launch_bounds__(SOLVER_BLOCK) void grad_sumsq_kernel(const float* __restrict__ g, long long n,
                                                                  double* __restrict__ scratch) {
  __shared__ double sh_s[SOLVER_BLOCK / 64];
  __shared__ unsigned sh_b[SOLVER_BLOCK / 64];
  const long long items = n / VEC + n % VEC;
  double s = 0.0;
  unsigned bad = 0;
  for (long long it = (long long)blockIdx.x * SOLVER_BLOCK + threadIdx.x; it < items; it += (long long)gridDim.x * SOLVER_BLOCK) {
    long long i;
    int cnt;
    solver_item<VEC>(it, n, i, cnt);
    if (cnt == VEC) {
      float x[VEC];
      VecIO<float, VEC>::load(g + i, x);
#pragma unroll
      for (int e = 0; e < VEC; e++) sumsq_add(x[e], s, bad);
    } else {
      sumsq_add(g[i], s, bad);
    }
  }
  // lanes by xor butterfly, then the waves in ascending order: a fixed tree
  s = wave_sum_d(s);
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) bad += __shfl_xor(bad, o, 64);
  const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
  if (lane == 0) { sh_s[wid] = s; sh_b[wid] = bad; }
  __syncthreads();
  if (threadIdx.x == 0) {
    double t = 0.0;
    unsigned b = 0;
    for (int k = 0; k < SOLVER_BLOCK / 64; k++) { t += sh_s[k]; b += sh_b[k]; }
    scratch[blockIdx.x] = t;
    scratch[gridDim.x + blockIdx.x] = (double)b;
  }
}

// one wave: lane l adds partials [l*per, (l+1)*per) in ascending order, lane 0 then adds the 64 lane sums in ascending order
__global__ __launch_bounds__(64) void grad_sumsq_final_kernel(const double* __restrict__ scratch, int parts,
                                                              double* __restrict__ out) {
  __shared__ double sh[2][64];
  const int per = (parts + 63) / 64, lo = threadIdx.x * per, hi = min(lo + per, parts);
  double s = 0.0, b = 0.0;
  for (int k = lo; k < hi; k++) { s += scratch[k]; b += scratch[parts + k]; }
  sh[0][threadIdx.x] = s;
  sh[1][threadIdx.x] = b;
  __syncthreads();
  if (threadIdx.x == 0) {
    s = 0.0; b = 0.0;
    for (int l = 0; l < 64; l++) { s += sh[0][l]; b += sh[1][l]; }
    out[0] = s;
    out[1] = b;
  }
}

extern "C" long long x3d_grad_sumsq_scratch(long long n) { return 2 * sumsq_parts(n); }

extern "C" int x3d_grad_sumsq(const float* g, long long n, double* scratch, double* out, void* stream) {
  X3D_REQUIRE(g && scratch && out && n > 0, "grad_sumsq: bad args");
  X3D_REQUIRE(((uintptr_t)scratch & 7) == 0 && ((uintptr_t)out & 7) == 0 && ((uintptr_t)g & 3) == 0, "grad_sumsq: misaligned pointer");
  const unsigned parts = (unsigned)sumsq_parts(n);      // the grid: a function of n alone, whatever path the pointer takes
  hipStream_t st = (hipStream_t)stream;
  if (solver_vec(nullptr, g) == 4)
    hipLaunchKernelGGL((grad_sumsq_kernel<4>), dim3(parts), dim3(SOLVER_BLOCK), 0, st, g, n, scratch);
  else
    hipLaunchKernelGGL((grad_sumsq_kernel<1>), dim3(parts), dim3(SOLVER_BLOCK), 0, st, g, n, scratch);
  hipLaunchKernelGGL(grad_sumsq_final_kernel, dim3(1), dim3(64), 0, st, (const double*)scratch, (int)parts, out);
  X3D_LAUNCH_CHECK("grad_sumsq");
  return X3D_OK;
}

// ------------------------------------------------------------------------------------------------
// x3d_sgd_nesterov_ex / x3d_adam_ex
// ------------------------------------------------------------------------------------------------
template <int VEC>
__global__ __launch_bounds__(SOLVER_BLOCK) void sgd_nesterov_ex_kernel(float* __restrict__ w, float* __restrict__ v,
                                                                       const float* __restrict__ g,
                                                                       const unsigned char* __restrict__ l2, float lr, float mom,
                                                                       float wd, float gscale, const double* __restrict__ norm,
                                                                       float max_norm, float* __restrict__ ema, float omd,
                                                                       long long n) {
  float c;
  if (!solver_coef(norm, gscale, max_norm, c)) return;
  const long long items = n / VEC + n % VEC;
  for (long long it = (long long)blockIdx.x * SOLVER_BLOCK + threadIdx.x; it < items; it += (long long)gridDim.x * SOLVER_BLOCK) {
    long long i;
    int cnt;
    solver_item<VEC>(it, n, i, cnt);
    if (cnt == VEC) {
      float wi[VEC], vi[VEC], gi[VEC], ei[VEC];
      bool m[VEC];
      VecIO<float, VEC>::load(w + i, wi);
      VecIO<float, VEC>::load(v + i, vi);
      VecIO<float, VEC>::load(g + i, gi);
      load_mask<VEC>(l2, i, m);
      if (ema) VecIO<float, VEC>::load(ema + i, ei);
#pragma unroll
      for (int e = 0; e < VEC; e++) sgd_nesterov_step(wi[e], vi[e], gi[e], m[e], lr, mom, wd, c);
      VecIO<float, VEC>::store(v + i, vi);
      VecIO<float, VEC>::store(w + i, wi);
      if (ema) {
#pragma unroll
        for (int e = 0; e < VEC; e++) ei[e] = ema_step(ei[e], wi[e], omd);
        VecIO<float, VEC>::store(ema + i, ei);
      }
    } else {
      float wi = w[i], vi = v[i];
      sgd_nesterov_step(wi, vi, g[i], l2 && l2[i], lr, mom, wd, c);
      v[i] = vi;
      w[i] = wi;
      if (ema) ema[i] = ema_step(ema[i], wi, omd);
    }
  }
}

template <int VEC>
__global__ __launch_bounds__(SOLVER_BLOCK) void adam_ex_kernel(float* __restrict__ w, float* __restrict__ m, float* __restrict__ v,
                                                               const float* __restrict__ g, const unsigned char* __restrict__ l2,
                                                               float lr_t, float b1, float b2, float eps, float wd, float gscale,
                                                               const double* __restrict__ norm, float max_norm,
                                                               float* __restrict__ ema, float omd, long long n) {
  float c;
  if (!solver_coef(norm, gscale, max_norm, c)) return;
  const long long items = n / VEC + n % VEC;
  for (long long it = (long long)blockIdx.x * SOLVER_BLOCK + threadIdx.x; it < items; it += (long long)gridDim.x * SOLVER_BLOCK) {
    long long i;
    int cnt;
    solver_item<VEC>(it, n, i, cnt);
    if (cnt == VEC) {
      float wi[VEC], mi[VEC], vi[VEC], gi[VEC], ei[VEC];
      bool k[VEC];
      VecIO<float, VEC>::load(w + i, wi);
      VecIO<float, VEC>::load(m + i, mi);
      VecIO<float, VEC>::load(v + i, vi);
      VecIO<float, VEC>::load(g + i, gi);
      load_mask<VEC>(l2, i, k);
      if (ema) VecIO<float, VEC>::load(ema + i, ei);
#pragma unroll
      for (int e = 0; e < VEC; e++) adam_step(wi[e], mi[e], vi[e], gi[e], k[e], lr_t, b1, b2, eps, wd, c);
      VecIO<float, VEC>::store(m + i, mi);
      VecIO<float, VEC>::store(v + i, vi);
      VecIO<float, VEC>::store(w + i, wi);
      if (ema) {
#pragma unroll
        for (int e = 0; e < VEC; e++) ei[e] = ema_step(ei[e], wi[e], omd);
        VecIO<float, VEC>::store(ema + i, ei);
      }
    } else {
      float wi = w[i], mi = m[i], vi = v[i];
      adam_step(wi, mi, vi, g[i], l2 && l2[i], lr_t, b1, b2, eps, wd, c);
      m[i] = mi;
      v[i] = vi;
      w[i] = wi;
      if (ema) ema[i] = ema_step(ema[i], wi, omd);
    }
  }
}

// what the two _ex entry points and x3d_ema_update refuse alike
#define SOLVER_REQUIRE_EXTRAS(name)                                                                                           \
  X3D_REQUIRE(!norm || (max_norm > 0.f && max_norm <= 3.0e38f), name ": max_norm must be positive and finite with norm");     \
  X3D_REQUIRE(!norm || ((uintptr_t)norm & 7) == 0, name ": misaligned norm");                                                 \
  X3D_REQUIRE(!ema || (ema_decay >= 0.f && ema_decay < 1.f), name ": ema_decay must lie in [0, 1)")

extern "C" int x3d_sgd_nesterov_ex(float* w, float* v, const float* g, const unsigned char* l2_mask, float lr, float momentum,
                                   float weight_decay, float grad_scale, const double* norm, float max_norm, float* ema,
                                   float ema_decay, long long n, void* stream) {
  X3D_REQUIRE(w && v && g && n > 0, "sgd_nesterov_ex: bad args");
  X3D_REQUIRE((((uintptr_t)w | (uintptr_t)v | (uintptr_t)g | (uintptr_t)ema) & 3) == 0, "sgd_nesterov_ex: misaligned pointer");
  SOLVER_REQUIRE_EXTRAS("sgd_nesterov_ex");
  const int vec = solver_vec(l2_mask, w, v, g, ema);
  const dim3 grid(solver_grid(solver_items(n, vec)));
  const float nm = norm ? max_norm : 0.f, omd = ema ? 1.f - ema_decay : 0.f;
#define ARGS w, v, g, l2_mask, lr, momentum, weight_decay, grad_scale, norm, nm, ema, omd, n
  if (vec == 4) hipLaunchKernelGGL((sgd_nesterov_ex_kernel<4>), grid, dim3(SOLVER_BLOCK), 0, (hipStream_t)stream, ARGS);
  else hipLaunchKernelGGL((sgd_nesterov_ex_kernel<1>), grid, dim3(SOLVER_BLOCK), 0, (hipStream_t)stream, ARGS);
#undef ARGS
  X3D_LAUNCH_CHECK("sgd_nesterov_ex");
  return X3D_OK;
}

extern "C" int x3d_adam_ex(float* w, float* m, float* v, const float* g, const unsigned char* l2_mask, float lr, float beta1,
                           float beta2, float eps, float weight_decay, float grad_scale, long long step, const double* norm,
                           float max_norm, float* ema, float ema_decay, long long n, void* stream) {
  X3D_REQUIRE(w && m && v && g && n > 0 && step >= 1, "adam_ex: bad args (step counts from 1)");
  X3D_REQUIRE((((uintptr_t)w | (uintptr_t)m | (uintptr_t)v | (uintptr_t)g | (uintptr_t)ema) & 3) == 0, "adam_ex: misaligned pointer");
  SOLVER_REQUIRE_EXTRAS("adam_ex");
  const int vec = solver_vec(l2_mask, w, m, v, g, ema);
  const dim3 grid(solver_grid(solver_items(n, vec)));
  const float nm = norm ? max_norm : 0.f, omd = ema ? 1.f - ema_decay : 0.f;
  const float lr_t = (float)adam_lr_t(lr, beta1, beta2, step);
#define ARGS w, m, v, g, l2_mask, lr_t, beta1, beta2, eps, weight_decay, grad_scale, norm, nm, ema, omd, n
  if (vec == 4) hipLaunchKernelGGL((adam_ex_kernel<4>), grid, dim3(SOLVER_BLOCK), 0, (hipStream_t)stream, ARGS);
  else hipLaunchKernelGGL((adam_ex_kernel<1>), grid, dim3(SOLVER_BLOCK), 0, (hipStream_t)stream, ARGS);
#undef ARGS
  X3D_LAUNCH_CHECK("adam_ex");
  return X3D_OK;
}

// ------------------------------------------------------------------------------------------------
// x3d_ema_update / x3d_grad_accum
// ------------------------------------------------------------------------------------------------
template <int VEC>
__global__ __launch_bounds__(SOLVER_BLOCK) void ema_update_kernel(float* __restrict__ ema, const float* __restrict__ w, float omd,
                                                                  const double* __restrict__ norm, long long n) {
  if (norm && norm[1] != 0.0) return;
  const long long items = n / VEC + n % VEC;
  for (long long it = (long long)blockIdx.x * SOLVER_BLOCK + threadIdx.x; it < items; it += (long long)gridDim.x * SOLVER_BLOCK) {
    long long i;
    int cnt;
    solver_item<VEC>(it, n, i, cnt);
    if (cnt == VEC) {
      float ei[VEC], wi[VEC];
      VecIO<float, VEC>::load(ema + i, ei);
      VecIO<float, VEC>::load(w + i, wi);
#pragma unroll
      for (int e = 0; e < VEC; e++) ei[e] = ema_step(ei[e], wi[e], omd);
      VecIO<float, VEC>::store(ema + i, ei);
    } else {
      ema[i] = ema_step(ema[i], w[i], omd);
    }
  }
}

extern "C" int x3d_ema_update(float* ema, const float* w, float decay, const double* norm, long long n, void* stream) {
  X3D_REQUIRE(ema && w && n > 0, "ema_update: bad args");
  X3D_REQUIRE((((uintptr_t)ema | (uintptr_t)w) & 3) == 0 && ((uintptr_t)norm & 7) == 0, "ema_update: misaligned pointer");
  X3D_REQUIRE(decay >= 0.f && decay < 1.f, "ema_update: decay must lie in [0, 1)");
  const int vec = solver_vec(nullptr, ema, w);
  const dim3 grid(solver_grid(solver_items(n, vec)));
  if (vec == 4) hipLaunchKernelGGL((ema_update_kernel<4>), grid, dim3(SOLVER_BLOCK), 0, (hipStream_t)stream, ema, w, 1.f - decay, norm, n);
  else hipLaunchKernelGGL((ema_update_kernel<1>), grid, dim3(SOLVER_BLOCK), 0, (hipStream_t)stream, ema, w, 1.f - decay, norm, n);
  X3D_LAUNCH_CHECK("ema_update");
  return X3D_OK;
}

// acc and g may be the same array (acc = 2 g): no __restrict__; an element is read and written by one thread
template <int VEC, bool FIRST>
__global__ __launch_bounds__(SOLVER_BLOCK) void grad_accum_kernel(float* acc, const float* g, long long n) {
  const long long items = n / VEC + n % VEC;
  for (long long it = (long long)blockIdx.x * SOLVER_BLOCK + threadIdx.x; it < items; it += (long long)gridDim.x * SOLVER_BLOCK) {
    long long i;
    int cnt;
    solver_item<VEC>(it, n, i, cnt);
    if (cnt == VEC) {
      float a[VEC], b[VEC];
      VecIO<float, VEC>::load(g + i, b);
      if constexpr (!FIRST) {
        VecIO<float, VEC>::load(acc + i, a);
#pragma unroll
        for (int e = 0; e < VEC; e++) b[e] = a[e] + b[e];
      }
      VecIO<float, VEC>::store(acc + i, b);
    } else {
      acc[i] = FIRST ? g[i] : acc[i] + g[i];
    }
  }
}

extern "C" int x3d_grad_accum(float* acc, const float* g, long long n, int first, void* stream) {
  X3D_REQUIRE(acc && g && n > 0, "grad_accum: bad args");
  X3D_REQUIRE((((uintptr_t)acc | (uintptr_t)g) & 3) == 0, "grad_accum: misaligned pointer");
  const int vec = solver_vec(nullptr, acc, g);
  const dim3 grid(solver_grid(solver_items(n, vec)));
  hipStream_t st = (hipStream_t)stream;
  if (vec == 4) {
    if (first) hipLaunchKernelGGL((grad_accum_kernel<4, true>), grid, dim3(SOLVER_BLOCK), 0, st, acc, g, n);
    else hipLaunchKernelGGL((grad_accum_kernel<4, false>), grid, dim3(SOLVER_BLOCK), 0, st, acc, g, n);
  } else {
    if (first) hipLaunchKernelGGL((grad_accum_kernel<1, true>), grid, dim3(SOLVER_BLOCK), 0, st, acc, g, n);
    else hipLaunchKernelGGL((grad_accum_kernel<1, false>), grid, dim3(SOLVER_BLOCK), 0, st, acc, g, n);
  }
  X3D_LAUNCH_CHECK("grad_accum");
  return X3D_OK;
}
