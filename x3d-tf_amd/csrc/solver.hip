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
//   x3d_seg_sumsq           per-tensor sums of squares and the layer-wise optimizers built on them (LARS, AdamW, LAMB): a chunk
//   x3d_lars / _adamw / _lamb   table instead of one flat range, a fixed number of launches (at the end of this file)
//   x3d_seg_grad_sumsq      fine-tuning (frozen tensors, per-tensor learning rates): the chunk table holds the tuned tensors only,
//   x3d_*_pt                the gradient reduction and all five rules walk it, and the learning rate of a chunk is lr *
//                           lr_scale[segment].  The same kernels: the learning rate is a policy (LrOne / LrSeg) they are
//                           instantiated with
//   x3d_unscale_sumsq       the fp16 loss scaler on the device: the two gradient reductions with g * (1 / scale) written back in
//   x3d_seg_unscale_sumsq   the same pass (the same walks, instantiated with SumsqUnscale), the scale applied to dlogits, and
//   x3d_loss_scale_apply / _update   Keras' DynamicLossScale on eight doubles of device memory (at the end of this file)
//
// Every streaming kernel is ONE BODY handed to one of two walkers.  A body is a generic lambda body(N, at): it loads N
// elements at `at` (vec_load), applies the rule to each (solver_each) and stores N elements (vec_store); N is a
// std::integral_constant, so the vector and the one-element form of a kernel are two instantiations of the same text and
// agree to the bit by construction.
//   solver_for_items<VEC>   the flat walk: a thread moves 16 bytes per array and iteration, the grid is capped at
//                           SOLVER_MAX_BLOCKS workgroups and strides over the rest.  VEC = 4 needs every array 16-byte aligned
//                           (the l2 mask 4-byte); the n % 4 elements at the end are further work items of the same walk, with
//                           N = 1.  Any other pointer takes VEC = 1.
//   seg_for_items           the walk over one chunk of the chunk table by one wave (the layer-wise kernels; the loop over the
//                           chunks stays in the kernel: SEG_FOR_CHUNKS): lane l takes the vectors l, l + 64, ..., lanes 0..2
//                           then the count % 4 last elements with N = 1.
// The EMA written in the same pass is EmaPass in every kernel that takes an `ema` pointer; solver_launch picks the
// instantiation on the host.  The plain entry points keep their one-element-per-thread kernels: their results and their
// speed are what they were.
//
// The update arithmetic exists once: sgd_nesterov_step / adam_step below, called by the old and the new kernels; the layer-wise
// rules (lars_step, adamw_step, lamb_moments / lamb_u) are built on them.
#include "common.h"
#include <type_traits>

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

// the flat walk: the items of this thread's grid-stride turns, each handed to body(N, first element) with N = VEC or 1
template <int VEC, class Body> __device__ __forceinline__ void solver_for_items(long long n, Body&& body) {
  const long long items = n / VEC + n % VEC;
  for (long long it = (long long)blockIdx.x * SOLVER_BLOCK + threadIdx.x; it < items; it += (long long)gridDim.x * SOLVER_BLOCK) {
    long long i;
    int cnt;
    solver_item<VEC>(it, n, i, cnt);
    if (cnt == VEC) body(std::integral_constant<int, VEC>{}, i);
    else body(std::integral_constant<int, 1>{}, i);
  }
}

// f(e) for the N elements of an item: what a body writes instead of a loop over e.  N = 1 is a plain call -- behind a one-trip
// loop the compiler stops sharing code between the vector and the one-element path of a walk (grad_sumsq_kernel<4>: three more
// VALU instructions per vector item in a kernel that is bound by them).
template <int N, class F> __device__ __forceinline__ void solver_each(F&& f) {
  if constexpr (N == 1) f(0);
  else {
#pragma unroll
    for (int e = 0; e < N; e++) f(e);
  }
}

// N floats at p.  AL: one access (16 bytes for N = 4); else the same floats one by one, for a p that is only 4-byte aligned
template <int N, bool AL = true> __device__ __forceinline__ void vec_load(const float* p, float (&o)[N]) {
  if constexpr (AL || N == 1) VecIO<float, N>::load(p, o);
  else {
    solver_each<N>([&](int e) { o[e] = p[e]; });
  }
}
template <int N, bool AL = true> __device__ __forceinline__ void vec_store(float* p, const float (&o)[N]) {
  if constexpr (AL || N == 1) VecIO<float, N>::store(p, o);
  else {
    solver_each<N>([&](int e) { p[e] = o[e]; });
  }
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

// The EMA written in the same pass, in two halves: load() goes out with the kernel's other loads (one memory round trip per
// item, not two), apply() takes the w the kernel has just computed.  The caller puts both behind `if (ema)`: the same answer
// in every lane.
template <int N, bool AL = true> struct EmaPass {
  float e[N];
  __device__ __forceinline__ void load(const float* p) { vec_load<N, AL>(p, e); }
  __device__ __forceinline__ void apply(float* p, const float (&w)[N], float omd) {
#pragma unroll
    for (int k = 0; k < N; k++) e[k] = ema_step(e[k], w[k], omd);
    vec_store<N, AL>(p, e);
  }
};

// One launch of a streaming kernel: the instantiation `yes` or `no` of it, SOLVER_BLOCK threads.
template <class... P, class... A>
static inline void solver_launch(bool pick, void (*yes)(P...), void (*no)(P...), unsigned grid, void* stream, A... args) {
  void (*kernel)(P...) = pick ? yes : no;
  hipLaunchKernelGGL(kernel, dim3(grid), dim3(SOLVER_BLOCK), 0, (hipStream_t)stream, static_cast<P>(args)...);
}
// what the kernels get of max_norm and ema_decay: 0 where the pointer they belong to is null
struct SolverExtras {
  float nm, omd;
  SolverExtras(const double* norm, float max_norm, const float* ema, float ema_decay)
      : nm(norm ? max_norm : 0.f), omd(ema ? 1.f - ema_decay : 0.f) {}
};

// ------------------------------------------------------------------------------------------------
// x3d_grad_sumsq
// ------------------------------------------------------------------------------------------------
static inline long long sumsq_parts(long long n) { return n > 0 ? (long long)solver_grid(solver_items(n, 4)) : 0; }

__device__ __forceinline__ void sumsq_add(float x, double& s, unsigned& bad) {
  const bool fin = (__float_as_uint(x) & 0x7f800000u) != 0x7f800000u;   // exponent all ones: inf or nan
  const double d = fin ? (double)x : 0.0;
  // the square in fp64: 1e-30 and 1e18 are fine.  The FMA is the fusion the compiler always made of s += d * d, spelled out:
  // with it the two paths of the flat walk end in the same instruction and share it, as they did when they were written apart
  s = __builtin_fma(d, d, s);
  bad += fin ? 0u : 1u;
}

// What the sum-of-squares walks (flat and chunk table) do to an element before they add it.  SumsqKeep: nothing, g is read-only
// (x3d_grad_sumsq / x3d_seg_grad_sumsq).  SumsqUnscale: g = g * inv, ONE fp32 product, written back in the same pass; the sum
// and the count are those of the product (x3d_unscale_sumsq / x3d_seg_unscale_sumsq; inv a power of two: exact, so the sum is
// the plain walk's times inv^2 to the bit).  inf and nan stay what they are under a finite positive inv.
struct SumsqKeep {
  static constexpr bool writes = false;
  using ptr = const float*;
  __device__ __forceinline__ float at(float x) const { return x; }
};
struct SumsqUnscale {
  static constexpr bool writes = true;
  using ptr = float*;
  float inv;
  __device__ __forceinline__ float at(float x) const { return x * inv; }
};

// scratch [2][parts]: partial sums, then partial counts.  Every workgroup writes its slot (zero when it had no item).
template <int VEC, class OP>
__device__ __forceinline__ void grad_sumsq_walk(typename OP::ptr __restrict__ g, long long n, double* __restrict__ scratch, OP op) {
  __shared__ double sh_s[SOLVER_BLOCK / 64];
  __shared__ unsigned sh_b[SOLVER_BLOCK / 64];
  double s = 0.0;
  unsigned bad = 0;
  solver_for_items<VEC>(n, [&](auto nc, long long i) {
    constexpr int N = decltype(nc)::value;
    float x[N];
    vec_load<N>(g + i, x);
    solver_each<N>([&](int e) {
      x[e] = op.at(x[e]);
      sumsq_add(x[e], s, bad);
    });
    if constexpr (OP::writes) vec_store<N>(g + i, x);
  });
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

template <int VEC>
__global__ __launch_bounds__(SOLVER_BLOCK) void grad_sumsq_kernel(const float* __restrict__ g, long long n,
                                                                  double* __restrict__ scratch) {
  grad_sumsq_walk<VEC>(g, n, scratch, SumsqKeep{});
}

// state: the X3D_LOSS_SCALE_STATE doubles of the loss scaler (further down); slot 1 = 1 / scale
template <int VEC>
__global__ __launch_bounds__(SOLVER_BLOCK) void unscale_sumsq_kernel(float* __restrict__ g, long long n,
                                                                     const double* __restrict__ state,
                                                                     double* __restrict__ scratch) {
  grad_sumsq_walk<VEC>(g, n, scratch, SumsqUnscale{(float)state[1]});
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
  solver_launch(solver_vec(nullptr, g) == 4, grad_sumsq_kernel<4>, grad_sumsq_kernel<1>, parts, stream, g, n, scratch);
  hipLaunchKernelGGL(grad_sumsq_final_kernel, dim3(1), dim3(64), 0, (hipStream_t)stream, (const double*)scratch, (int)parts, out);
  X3D_LAUNCH_CHECK("grad_sumsq");
  return X3D_OK;
}

// x3d_grad_sumsq's grid, partial layout and final launch; the walk multiplies by state[1] and writes g back
extern "C" int x3d_unscale_sumsq(float* g, long long n, const double* state, double* scratch, double* out, void* stream) {
  X3D_REQUIRE(g && state && scratch && out && n > 0, "unscale_sumsq: bad args");
  X3D_REQUIRE((((uintptr_t)state | (uintptr_t)scratch | (uintptr_t)out) & 7) == 0 && ((uintptr_t)g & 3) == 0,
              "unscale_sumsq: misaligned pointer");
  const unsigned parts = (unsigned)sumsq_parts(n);
  solver_launch(solver_vec(nullptr, g) == 4, unscale_sumsq_kernel<4>, unscale_sumsq_kernel<1>, parts, stream, g, n, state, scratch);
  hipLaunchKernelGGL(grad_sumsq_final_kernel, dim3(1), dim3(64), 0, (hipStream_t)stream, (const double*)scratch, (int)parts, out);
  X3D_LAUNCH_CHECK("unscale_sumsq");
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
  solver_for_items<VEC>(n, [&](auto nc, long long i) {
    constexpr int N = decltype(nc)::value;
    float wi[N], vi[N], gi[N];
    bool k[N];
    vec_load<N>(w + i, wi);
    vec_load<N>(v + i, vi);
    vec_load<N>(g + i, gi);
    load_mask<N>(l2, i, k);
    EmaPass<N> ea;
    if (ema) ea.load(ema + i);
    solver_each<N>([&](int e) { sgd_nesterov_step(wi[e], vi[e], gi[e], k[e], lr, mom, wd, c); });
    vec_store<N>(v + i, vi);
    vec_store<N>(w + i, wi);
    if (ema) ea.apply(ema + i, wi, omd);
  });
}

template <int VEC>
__global__ __launch_bounds__(SOLVER_BLOCK) void adam_ex_kernel(float* __restrict__ w, float* __restrict__ m, float* __restrict__ v,
                                                               const float* __restrict__ g, const unsigned char* __restrict__ l2,
                                                               float lr_t, float b1, float b2, float eps, float wd, float gscale,
                                                               const double* __restrict__ norm, float max_norm,
                                                               float* __restrict__ ema, float omd, long long n) {
  float c;
  if (!solver_coef(norm, gscale, max_norm, c)) return;
  solver_for_items<VEC>(n, [&](auto nc, long long i) {
    constexpr int N = decltype(nc)::value;
    float wi[N], mi[N], vi[N], gi[N];
    bool k[N];
    vec_load<N>(w + i, wi);
    vec_load<N>(m + i, mi);
    vec_load<N>(v + i, vi);
    vec_load<N>(g + i, gi);
    load_mask<N>(l2, i, k);
    EmaPass<N> ea;
    if (ema) ea.load(ema + i);
    solver_each<N>([&](int e) { adam_step(wi[e], mi[e], vi[e], gi[e], k[e], lr_t, b1, b2, eps, wd, c); });
    vec_store<N>(m + i, mi);
    vec_store<N>(v + i, vi);
    vec_store<N>(w + i, wi);
    if (ema) ea.apply(ema + i, wi, omd);
  });
}

// what the two _ex entry points and x3d_ema_update refuse alike
#define SOLVER_REQUIRE_EXTRAS(name)                                                                                           \
  X3D_REQUIRE(!norm || (max_norm > 0.f && max_norm <= 3.0e38f), "%s: max_norm must be positive and finite with norm", name);  \
  X3D_REQUIRE(!norm || ((uintptr_t)norm & 7) == 0, "%s: misaligned norm", name);                                              \
  X3D_REQUIRE(!ema || (ema_decay >= 0.f && ema_decay < 1.f), "%s: ema_decay must lie in [0, 1)", name)

extern "C" int x3d_sgd_nesterov_ex(float* w, float* v, const float* g, const unsigned char* l2_mask, float lr, float momentum,
                                   float weight_decay, float grad_scale, const double* norm, float max_norm, float* ema,
                                   float ema_decay, long long n, void* stream) {
  X3D_REQUIRE(w && v && g && n > 0, "sgd_nesterov_ex: bad args");
  X3D_REQUIRE((((uintptr_t)w | (uintptr_t)v | (uintptr_t)g | (uintptr_t)ema) & 3) == 0, "sgd_nesterov_ex: misaligned pointer");
  SOLVER_REQUIRE_EXTRAS("sgd_nesterov_ex");
  const int vec = solver_vec(l2_mask, w, v, g, ema);
  const SolverExtras x(norm, max_norm, ema, ema_decay);
  solver_launch(vec == 4, sgd_nesterov_ex_kernel<4>, sgd_nesterov_ex_kernel<1>, solver_grid(solver_items(n, vec)), stream, w, v,
                g, l2_mask, lr, momentum, weight_decay, grad_scale, norm, x.nm, ema, x.omd, n);
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
  const SolverExtras x(norm, max_norm, ema, ema_decay);
  solver_launch(vec == 4, adam_ex_kernel<4>, adam_ex_kernel<1>, solver_grid(solver_items(n, vec)), stream, w, m, v, g, l2_mask,
                (float)adam_lr_t(lr, beta1, beta2, step), beta1, beta2, eps, weight_decay, grad_scale, norm, x.nm, ema, x.omd, n);
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
  solver_for_items<VEC>(n, [&](auto nc, long long i) {
    constexpr int N = decltype(nc)::value;
    float wi[N];
    EmaPass<N> ea;
    ea.load(ema + i);
    vec_load<N>(w + i, wi);
    ea.apply(ema + i, wi, omd);
  });
}

extern "C" int x3d_ema_update(float* ema, const float* w, float decay, const double* norm, long long n, void* stream) {
  X3D_REQUIRE(ema && w && n > 0, "ema_update: bad args");
  X3D_REQUIRE((((uintptr_t)ema | (uintptr_t)w) & 3) == 0 && ((uintptr_t)norm & 7) == 0, "ema_update: misaligned pointer");
  X3D_REQUIRE(decay >= 0.f && decay < 1.f, "ema_update: decay must lie in [0, 1)");
  const int vec = solver_vec(nullptr, ema, w);
  solver_launch(vec == 4, ema_update_kernel<4>, ema_update_kernel<1>, solver_grid(solver_items(n, vec)), stream, ema, w,
                1.f - decay, norm, n);
  X3D_LAUNCH_CHECK("ema_update");
  return X3D_OK;
}

// acc and g may be the same array (acc = 2 g): no __restrict__; an element is read and written by one thread
template <int VEC, bool FIRST>
__global__ __launch_bounds__(SOLVER_BLOCK) void grad_accum_kernel(float* acc, const float* g, long long n) {
  solver_for_items<VEC>(n, [&](auto nc, long long i) {
    constexpr int N = decltype(nc)::value;
    float a[N], b[N];
    vec_load<N>(g + i, b);
    if constexpr (!FIRST) {
      vec_load<N>(acc + i, a);
      solver_each<N>([&](int e) { b[e] = a[e] + b[e]; });
    }
    vec_store<N>(acc + i, b);
  });
}

extern "C" int x3d_grad_accum(float* acc, const float* g, long long n, int first, void* stream) {
  X3D_REQUIRE(acc && g && n > 0, "grad_accum: bad args");
  X3D_REQUIRE((((uintptr_t)acc | (uintptr_t)g) & 3) == 0, "grad_accum: misaligned pointer");
  const int vec = solver_vec(nullptr, acc, g);
  solver_launch(vec == 4, first ? grad_accum_kernel<4, true> : grad_accum_kernel<4, false>,
                first ? grad_accum_kernel<1, true> : grad_accum_kernel<1, false>, solver_grid(solver_items(n, vec)), stream, acc,
                g, n);
  X3D_LAUNCH_CHECK("grad_accum");
  return X3D_OK;
}

// ------------------------------------------------------------------------------------------------
// layer-wise optimizers: x3d_seg_sumsq / x3d_lars / x3d_adamw / x3d_lamb
// ------------------------------------------------------------------------------------------------
// Driven by the chunk table (include/x3d_hip.h): chunks [nchunk][3] = (segment, first element, count), segs [nseg][3] =
// (first chunk, chunks, l2).  ONE WAVE takes one chunk, the waves of the grid stride over the table: no workgroup barrier, no
// LDS, a tensor of 24 floats costs one wave and not a workgroup.  Lane l takes the vectors l, l + 64, ... of the chunk (16
// bytes each; SEG_CHUNK = 1024 elements = 4 per lane, all in flight), lanes 0..2 then the count % 4 last elements.  The
// element -> lane map and the order a lane adds in do not depend on the alignment path (AL = false loads the same four floats
// one by one), so the sums have the same bits on both.  Padding is in no chunk: it is never touched.
#define SEG_CHUNK X3D_SEG_CHUNK
#define SEG_WAVES (SOLVER_BLOCK / 64)
static_assert(SEG_CHUNK % 4 == 0, "a chunk is whole vectors unless its segment ends");

static inline unsigned seg_grid(int nchunk) {
  long long b = ceil_div_ll(nchunk, SEG_WAVES);
  if (b > SOLVER_MAX_BLOCKS) b = SOLVER_MAX_BLOCKS;
  return (unsigned)(b < 1 ? 1 : b);
}
static inline bool seg_aligned(const void* p0, const void* p1 = nullptr, const void* p2 = nullptr, const void* p3 = nullptr,
                               const void* p4 = nullptr) {
  return solver_vec(nullptr, p0, p1, p2, p3, p4) == 4;
}

// the chunk of this wave's turn `ch` (wave-uniform: kept in scalar registers)
__device__ __forceinline__ void seg_chunk(const int* __restrict__ chunks, int ch, int& seg, int& first, int& cnt) {
  seg = __builtin_amdgcn_readfirstlane(chunks[3 * ch]);
  first = __builtin_amdgcn_readfirstlane(chunks[3 * ch + 1]);
  cnt = __builtin_amdgcn_readfirstlane(chunks[3 * ch + 2]);
}
#define SEG_FOR_CHUNKS(ch)                                                                                           \
  const int lane = threadIdx.x & 63;                                                                                 \
  for (int ch = blockIdx.x * SEG_WAVES + (threadIdx.x >> 6); ch < nchunk; ch += gridDim.x * SEG_WAVES)

// the walk of one wave over one chunk [first, first + cnt): body(N, element) with N = 4 for the vectors, then N = 1 for the
// cnt % 4 last elements
template <class Body> __device__ __forceinline__ void seg_for_items(int first, int cnt, int lane, Body&& body) {
  const int nv = cnt >> 2, rem = cnt & 3;
  for (int i = lane; i < nv; i += 64) body(std::integral_constant<int, 4>{}, first + 4 * i);
  if (lane < rem) body(std::integral_constant<int, 1>{}, first + 4 * nv + lane);
}

__device__ __forceinline__ void sq_add(float x, double& s) {
  const double d = (double)x;
  s += d * d;
}

// ---- the one definition of the per-element arithmetic (contraction off: every rounding is written out) ----
// LARS: g' = q (c g + [l2] 2 wd w), then the Nesterov step of x3d_sgd_nesterov on g' (q = 1: that step's bits)
__device__ __forceinline__ void lars_step(float& w, float& v, float g, bool l2, float q, float lr, float mom, float wd, float c) {
#pragma clang fp contract(off)
  float gi = g * c;
  if (l2) gi = __builtin_fmaf(wd + wd, w, gi);
  gi = gi * q;
  sgd_nesterov_step(w, v, gi, false, lr, mom, 0.f, 1.f);
}
// AdamW: adam_step without the coupled L2 term, then the decoupled decay of the weight the step started from (ld = lr * decay)
__device__ __forceinline__ void adamw_step(float& w, float& m, float& v, float g, bool l2, float lr_t, float b1, float b2,
                                           float eps, float ld, float c) {
#pragma clang fp contract(off)
  const float w0 = w;
  adam_step(w, m, v, g, false, lr_t, b1, b2, eps, 0.f, c);
  if (l2 && ld > 0.f) w = __builtin_fmaf(-ld, w0, w);
}
// LAMB: the moments as adam_step forms them (L2 off), and u = r m / (sqrt(v) + eps) + [l2] decay w
__device__ __forceinline__ void lamb_moments(float& m, float& v, float g, float b1, float b2, float c) {
#pragma clang fp contract(off)
  const float gi = g * c;
  const float mi = __builtin_fmaf(1.f - b1, gi, b1 * m);
  const float vi = __builtin_fmaf(gi, (1.f - b2) * gi, b2 * v);
  m = mi;
  v = vi;
}
__device__ __forceinline__ float lamb_u(float w, float m, float v, bool l2, float r, float eps, float decay) {
#pragma clang fp contract(off)
  float u = (r * m) / (sqrtf(v) + eps);
  if (l2) u = __builtin_fmaf(decay, w, u);
  return u;
}
__device__ __forceinline__ float lamb_apply(float w, float u, float lq) { return __builtin_fmaf(-lq, u, w); }

// ---- the learning rate of a segment: what the kernels below are instantiated with (wave-uniform, read once per chunk) ----
// LrOne: the one value of the launch -- x3d_lars / x3d_adamw / x3d_lamb, whose kernels are what they were.
// LrSeg: lr_t = lr * lr_scale[t], one fp32 product (lr_scale NULL: lr itself) -- the _pt entry points.  A tensor's update at
// (lr, lr_scale[t]) then has the bits of the plain update at fl32(lr * lr_scale[t]).
__device__ __forceinline__ float seg_uniform(const float* __restrict__ p, int seg) {
  return __builtin_bit_cast(float, __builtin_amdgcn_readfirstlane(__builtin_bit_cast(int, p[seg])));
}
struct LrOne {
  float lr;
  __device__ __forceinline__ float at(int) const { return lr; }
};
struct LrSeg {
  float lr;
  const float* s;
  __device__ __forceinline__ float at(int seg) const {
#pragma clang fp contract(off)
    return s ? lr * seg_uniform(s, seg) : lr;
  }
};
// Adam's two uses of it: the bias-corrected lr_t and AdamW's ld = lr * decay.  AdamLrOne: both formed on the host, as ever.
// AdamLrSeg: the host's expressions on the device -- (float)((double)lr_t * num / den) with num = sqrt(1 - b2^step), den = 1 -
// b1^step from the host (adam_lr_t's order of operations; an fp64 quotient is correctly rounded on both sides) and lr_t * decay.
struct AdamLrOne {
  float lr_t, ld;
  __device__ __forceinline__ void at(int, float& lt, float& d) const { lt = lr_t; d = ld; }
};
struct AdamLrSeg {
  LrSeg lr;
  double num, den;
  float decay;
  __device__ __forceinline__ void at(int seg, float& lt, float& d) const {
#pragma clang fp contract(off)
    const float l = lr.at(seg);
    lt = (float)((double)l * num / den);
    d = l * decay;
  }
};
static inline AdamLrSeg adam_lr_seg(float lr, const float* lr_scale, float beta1, float beta2, long long step, float decay) {
  return AdamLrSeg{LrSeg{lr, lr_scale}, sqrt(1.0 - pow((double)beta2, (double)step)), 1.0 - pow((double)beta1, (double)step), decay};
}

// ---- partial sums: partials[ch] (and partials[nchunk + ch]) of chunk ch ----
// FINITE (x3d_seg_grad_sumsq): x3d_grad_sumsq's rule -- a non-finite entry adds nothing to the sum and one to the chunk's count
// OP: SumsqKeep, or SumsqUnscale (x3d_seg_unscale_sumsq): the elements of the chunks are rewritten, nothing outside them is touched
template <bool AL, bool FINITE, class OP>
__device__ __forceinline__ void seg_sumsq_walk(typename OP::ptr __restrict__ a, const int* __restrict__ chunks, int nchunk,
                                               double* __restrict__ partials, OP op) {
  SEG_FOR_CHUNKS(ch) {
    int seg, first, cnt;
    seg_chunk(chunks, ch, seg, first, cnt);
    double s = 0.0;
    unsigned bad = 0;
    seg_for_items(first, cnt, lane, [&](auto nc, int at) {
      constexpr int N = decltype(nc)::value;
      float x[N];
      vec_load<N, AL>(a + at, x);
      solver_each<N>([&](int e) {
        x[e] = op.at(x[e]);
        if constexpr (FINITE) sumsq_add(x[e], s, bad);
        else sq_add(x[e], s);
      });
      if constexpr (OP::writes) vec_store<N, AL>(a + at, x);
    });
    s = wave_sum_d(s);
    if constexpr (FINITE) {
#pragma unroll
      for (int o = 32; o > 0; o >>= 1) bad += __shfl_xor(bad, o, 64);
    }
    if (lane == 0) {
      partials[ch] = s;
      if constexpr (FINITE) partials[nchunk + ch] = (double)bad;
    }
  }
}

template <bool AL, bool FINITE>
__global__ __launch_bounds__(SOLVER_BLOCK) void seg_sumsq_kernel(const float* __restrict__ a, const int* __restrict__ chunks,
                                                                 int nchunk, double* __restrict__ partials) {
  seg_sumsq_walk<AL, FINITE>(a, chunks, nchunk, partials, SumsqKeep{});
}

template <bool AL>
__global__ __launch_bounds__(SOLVER_BLOCK) void seg_unscale_sumsq_kernel(float* __restrict__ g, const int* __restrict__ chunks,
                                                                         int nchunk, const double* __restrict__ state,
                                                                         double* __restrict__ partials) {
  seg_sumsq_walk<AL, true>(g, chunks, nchunk, partials, SumsqUnscale{(float)state[1]});
}

template <bool AL>
__global__ __launch_bounds__(SOLVER_BLOCK) void lars_sums_kernel(const float* __restrict__ w, const float* __restrict__ g,
                                                                 const int* __restrict__ chunks, int nchunk,
                                                                 const double* __restrict__ norm, double* __restrict__ partials) {
  if (norm && norm[1] != 0.0) return;
  SEG_FOR_CHUNKS(ch) {
    int seg, first, cnt;
    seg_chunk(chunks, ch, seg, first, cnt);
    double sw = 0.0, sg = 0.0;
    seg_for_items(first, cnt, lane, [&](auto nc, int at) {
      constexpr int N = decltype(nc)::value;
      float x[N], y[N];
      vec_load<N, AL>(w + at, x);
      vec_load<N, AL>(g + at, y);
      solver_each<N>([&](int e) { sq_add(x[e], sw); sq_add(y[e], sg); });
    });
    sw = wave_sum_d(sw);
    sg = wave_sum_d(sg);
    if (lane == 0) { partials[ch] = sw; partials[nchunk + ch] = sg; }
  }
}

// LAMB's first pass: m, v are updated and stored; partial sums of w (not yet updated) and of u
template <bool AL>
__global__ __launch_bounds__(SOLVER_BLOCK) void lamb_moments_kernel(const float* __restrict__ w, float* __restrict__ m,
                                                                    float* __restrict__ v, const float* __restrict__ g,
                                                                    const int* __restrict__ chunks, int nchunk,
                                                                    const int* __restrict__ segs, float r, float b1, float b2,
                                                                    float eps, float decay, float gscale,
                                                                    const double* __restrict__ norm, float max_norm,
                                                                    double* __restrict__ partials) {
  float c;
  if (!solver_coef(norm, gscale, max_norm, c)) return;
  SEG_FOR_CHUNKS(ch) {
    int seg, first, cnt;
    seg_chunk(chunks, ch, seg, first, cnt);
    const bool l2 = __builtin_amdgcn_readfirstlane(segs[3 * seg + 2]) != 0;
    double sw = 0.0, su = 0.0;
    seg_for_items(first, cnt, lane, [&](auto nc, int at) {
      constexpr int N = decltype(nc)::value;
      float wi[N], mi[N], vi[N], gi[N];
      vec_load<N, AL>(w + at, wi);
      vec_load<N, AL>(m + at, mi);
      vec_load<N, AL>(v + at, vi);
      vec_load<N, AL>(g + at, gi);
      solver_each<N>([&](int e) {
        lamb_moments(mi[e], vi[e], gi[e], b1, b2, c);
        sq_add(wi[e], sw);
        sq_add(lamb_u(wi[e], mi[e], vi[e], l2, r, eps, decay), su);
      });
      vec_store<N, AL>(m + at, mi);
      vec_store<N, AL>(v + at, vi);
    });
    sw = wave_sum_d(sw);
    su = wave_sum_d(su);
    if (lane == 0) { partials[ch] = sw; partials[nchunk + ch] = su; }
  }
}

// ---- per segment: one wave adds the segment's partials -- lane l those of chunks l, l + 64, ... in ascending order, the
// lanes by the butterfly -- and lane 0 writes the sum (SEG_SUM) or q (SEG_LARS / SEG_LAMB: fp64, rounded once) ----
enum { SEG_SUM = 0, SEG_LARS = 1, SEG_LAMB = 2 };
template <int MODE, class LR>
__global__ __launch_bounds__(SOLVER_BLOCK) void seg_final_kernel(const double* __restrict__ partials, int nchunk,
                                                                 const int* __restrict__ segs, int nseg, LR lrp, float wd,
                                                                 float gscale, float eta, float eps, int clip,
                                                                 const double* __restrict__ norm, float max_norm,
                                                                 double* __restrict__ out, float* __restrict__ q) {
  float c = gscale;
  if constexpr (MODE != SEG_SUM) {
    if (!solver_coef(norm, gscale, max_norm, c)) return;
  }
  const int lane = threadIdx.x & 63;
  const int seg = blockIdx.x * SEG_WAVES + (threadIdx.x >> 6);
  if (seg >= nseg) return;
  const int c0 = segs[3 * seg], nc = segs[3 * seg + 1];
  const bool l2 = segs[3 * seg + 2] != 0;
  double s0 = 0.0, s1 = 0.0;
  for (int k = lane; k < nc; k += 64) {
    s0 += partials[c0 + k];
    if constexpr (MODE != SEG_SUM) s1 += partials[nchunk + c0 + k];
  }
  s0 = wave_sum_d(s0);
  if constexpr (MODE != SEG_SUM) s1 = wave_sum_d(s1);
  if (lane != 0) return;
  if constexpr (MODE == SEG_SUM) {
    out[seg] = s0;
  } else {
    double t = 1.0;
    if (l2 && s0 > 0.0 && s1 > 0.0) {
      const double nw = sqrt(s0), nx = sqrt(s1);
      if constexpr (MODE == SEG_LARS) {
        t = (double)eta * nw / ((double)c * nx + 2.0 * (double)wd * nw + (double)eps);
        if (clip) t = fmin(t / (double)lrp.at(seg), 1.0);
      } else {
        t = nw / nx;
      }
    }
    q[seg] = (float)t;
  }
}
// its launch: one wave per segment
template <int MODE, class LR, class... A>
static inline void seg_final_launch(int nseg, void* stream, const double* partials, int nchunk, const int* segs, LR lrp, A... args) {
  hipLaunchKernelGGL((seg_final_kernel<MODE, LR>), dim3((unsigned)ceil_div_ll(nseg, SEG_WAVES)), dim3(SOLVER_BLOCK), 0,
                     (hipStream_t)stream, partials, nchunk, segs, nseg, lrp, args...);
}

// ---- apply passes ----
// LARS = false (x3d_sgd_pt): no q, the plain sgd_nesterov_step on the chunk -- x3d_sgd_nesterov_ex's rule on this walker
template <bool AL, class LR, bool LARS>
__global__ __launch_bounds__(SOLVER_BLOCK) void lars_apply_kernel(float* __restrict__ w, float* __restrict__ v,
                                                                  const float* __restrict__ g, const int* __restrict__ chunks,
                                                                  int nchunk, const int* __restrict__ segs,
                                                                  const float* __restrict__ q, LR lrp, float mom, float wd,
                                                                  float gscale, const double* __restrict__ norm, float max_norm,
                                                                  float* __restrict__ ema, float omd) {
  float c;
  if (!solver_coef(norm, gscale, max_norm, c)) return;
  SEG_FOR_CHUNKS(ch) {
    int seg, first, cnt;
    seg_chunk(chunks, ch, seg, first, cnt);
    const bool l2 = __builtin_amdgcn_readfirstlane(segs[3 * seg + 2]) != 0;
    float qt = 1.f;
    if constexpr (LARS) qt = seg_uniform(q, seg);
    const float lr = lrp.at(seg);
    seg_for_items(first, cnt, lane, [&](auto nc, int at) {
      constexpr int N = decltype(nc)::value;
      float wi[N], vi[N], gi[N];
      vec_load<N, AL>(w + at, wi);
      vec_load<N, AL>(v + at, vi);
      vec_load<N, AL>(g + at, gi);
      EmaPass<N, AL> ea;
      if (ema) ea.load(ema + at);
      solver_each<N>([&](int e) {
        if constexpr (LARS) lars_step(wi[e], vi[e], gi[e], l2, qt, lr, mom, wd, c);
        else sgd_nesterov_step(wi[e], vi[e], gi[e], l2, lr, mom, wd, c);
      });
      vec_store<N, AL>(v + at, vi);
      vec_store<N, AL>(w + at, wi);
      if (ema) ea.apply(ema + at, wi, omd);
    });
  }
}

// DECOUPLED = false (x3d_adam_pt): adam_step with the coupled L2 term (wd) -- x3d_adam_ex's rule on this walker
template <bool AL, class LR, bool DECOUPLED>
__global__ __launch_bounds__(SOLVER_BLOCK) void adamw_kernel(float* __restrict__ w, float* __restrict__ m, float* __restrict__ v,
                                                             const float* __restrict__ g, const int* __restrict__ chunks,
                                                             int nchunk, const int* __restrict__ segs, LR lrp, float b1,
                                                             float b2, float eps, float wd, float gscale,
                                                             const double* __restrict__ norm, float max_norm,
                                                             float* __restrict__ ema, float omd) {
  float c;
  if (!solver_coef(norm, gscale, max_norm, c)) return;
  SEG_FOR_CHUNKS(ch) {
    int seg, first, cnt;
    seg_chunk(chunks, ch, seg, first, cnt);
    const bool l2 = __builtin_amdgcn_readfirstlane(segs[3 * seg + 2]) != 0;
    float lr_t, ld;
    lrp.at(seg, lr_t, ld);
    seg_for_items(first, cnt, lane, [&](auto nc, int at) {
      constexpr int N = decltype(nc)::value;
      float wi[N], mi[N], vi[N], gi[N];
      vec_load<N, AL>(w + at, wi);
      vec_load<N, AL>(m + at, mi);
      vec_load<N, AL>(v + at, vi);
      vec_load<N, AL>(g + at, gi);
      EmaPass<N, AL> ea;
      if (ema) ea.load(ema + at);
      solver_each<N>([&](int e) {
        if constexpr (DECOUPLED) adamw_step(wi[e], mi[e], vi[e], gi[e], l2, lr_t, b1, b2, eps, ld, c);
        else adam_step(wi[e], mi[e], vi[e], gi[e], l2, lr_t, b1, b2, eps, wd, c);
      });
      vec_store<N, AL>(m + at, mi);
      vec_store<N, AL>(v + at, vi);
      vec_store<N, AL>(w + at, wi);
      if (ema) ea.apply(ema + at, wi, omd);
    });
  }
}

template <bool AL, class LR>
__global__ __launch_bounds__(SOLVER_BLOCK) void lamb_apply_kernel(float* __restrict__ w, const float* __restrict__ m,
                                                                  const float* __restrict__ v, const int* __restrict__ chunks,
                                                                  int nchunk, const int* __restrict__ segs,
                                                                  const float* __restrict__ q, LR lrp, float r, float eps,
                                                                  float decay, const double* __restrict__ norm,
                                                                  float* __restrict__ ema, float omd) {
  if (norm && norm[1] != 0.0) return;
  SEG_FOR_CHUNKS(ch) {
    int seg, first, cnt;
    seg_chunk(chunks, ch, seg, first, cnt);
    const bool l2 = __builtin_amdgcn_readfirstlane(segs[3 * seg + 2]) != 0;
    const float qt = seg_uniform(q, seg);
    const float lq = lrp.at(seg) * qt;
    seg_for_items(first, cnt, lane, [&](auto nc, int at) {
      constexpr int N = decltype(nc)::value;
      float wi[N], mi[N], vi[N];
      vec_load<N, AL>(w + at, wi);
      vec_load<N, AL>(m + at, mi);
      vec_load<N, AL>(v + at, vi);
      EmaPass<N, AL> ea;
      if (ema) ea.load(ema + at);
      solver_each<N>([&](int e) { wi[e] = lamb_apply(wi[e], lamb_u(wi[e], mi[e], vi[e], l2, r, eps, decay), lq); });
      vec_store<N, AL>(w + at, wi);
      if (ema) ea.apply(ema + at, wi, omd);
    });
  }
}

// ---- entry points ----
// Each rule has ONE host function, a template over the learning-rate policy; the plain entry point hands it LrOne and the _pt
// entry point LrSeg.  What an entry point refuses is written once that way, under the caller's name.
#define SEG_REQUIRE_TABLE(name)                                                                                               \
  X3D_REQUIRE(chunks && segs && nchunk > 0 && nseg > 0 && nseg <= nchunk, "%s: bad chunk table (null, or nseg / nchunk <= 0)", name); \
  X3D_REQUIRE((((uintptr_t)chunks | (uintptr_t)segs) & 3) == 0, "%s: misaligned table", name)
#define SEG_REQUIRE_LR_SCALE(name) X3D_REQUIRE(((uintptr_t)lr_scale & 3) == 0, "%s: misaligned lr_scale", name)
static inline bool seg_finite_ge0(float x) { return x >= 0.f && x <= 3.0e38f; }

template <bool FINITE>
static int seg_sumsq_run(const char* name, const float* a, const int* chunks, int nchunk, const int* segs, int nseg,
                         double* partials, double* out, void* stream) {
  X3D_REQUIRE(a && partials && out, "%s: bad args", name);
  SEG_REQUIRE_TABLE(name);
  X3D_REQUIRE(((uintptr_t)a & 3) == 0 && (((uintptr_t)partials | (uintptr_t)out) & 7) == 0, "%s: misaligned pointer", name);
  solver_launch(seg_aligned(a), seg_sumsq_kernel<true, FINITE>, seg_sumsq_kernel<false, FINITE>, seg_grid(nchunk), stream, a,
                chunks, nchunk, partials);
  if constexpr (FINITE)     // all chunks in ascending order, sums and counts: x3d_grad_sumsq's final launch on nchunk partials
    hipLaunchKernelGGL(grad_sumsq_final_kernel, dim3(1), dim3(64), 0, (hipStream_t)stream, (const double*)partials, nchunk, out);
  else
    seg_final_launch<SEG_SUM>(nseg, stream, (const double*)partials, nchunk, segs, LrOne{0.f}, 0.f, 1.f, 0.f, 0.f, 0,
                              (const double*)nullptr, 0.f, out, (float*)nullptr);
  X3D_LAUNCH_CHECK(name);
  return X3D_OK;
}

extern "C" int x3d_seg_sumsq(const float* a, const int* chunks, int nchunk, const int* segs, int nseg, double* partials,
                             double* out, void* stream) {
  return seg_sumsq_run<false>("seg_sumsq", a, chunks, nchunk, segs, nseg, partials, out, stream);
}

extern "C" int x3d_seg_grad_sumsq(const float* g, const int* chunks, int nchunk, const int* segs, int nseg, double* partials,
                                  double* out, void* stream) {
  return seg_sumsq_run<true>("seg_grad_sumsq", g, chunks, nchunk, segs, nseg, partials, out, stream);
}

// x3d_lars / x3d_lars_pt (LARS = true: sums, q, apply) and x3d_sgd_pt (LARS = false: the apply pass alone; partials, q unused)
template <bool LARS, class LR>
static int lars_run(const char* name, float* w, float* v, const float* g, const int* chunks, int nchunk, const int* segs, int nseg,
                    LR lrp, float momentum, float weight_decay, float grad_scale, float trust_coef, float eps, int clip,
                    const double* norm, float max_norm, float* ema, float ema_decay, double* partials, float* q, void* stream) {
  X3D_REQUIRE(w && v && g && (!LARS || (partials && q)), "%s: bad args", name);
  SEG_REQUIRE_TABLE(name);
  X3D_REQUIRE((((uintptr_t)w | (uintptr_t)v | (uintptr_t)g | (uintptr_t)ema | (uintptr_t)q) & 3) == 0 &&
              ((uintptr_t)partials & 7) == 0, "%s: misaligned pointer", name);
  if constexpr (LARS) {
    X3D_REQUIRE(trust_coef > 0.f && trust_coef <= 3.0e38f, "%s: trust_coef must be positive and finite", name);
    X3D_REQUIRE(seg_finite_ge0(eps) && seg_finite_ge0(weight_decay), "%s: eps and weight_decay must be >= 0 and finite", name);
    X3D_REQUIRE(!clip || lrp.lr > 0.f, "%s: clip needs lr > 0", name);
  }
  SOLVER_REQUIRE_EXTRAS(name);
  const unsigned grid = seg_grid(nchunk);
  const SolverExtras x(norm, max_norm, ema, ema_decay);
  const bool al = seg_aligned(w, v, g, ema);
  if constexpr (LARS) {
    solver_launch(al, lars_sums_kernel<true>, lars_sums_kernel<false>, grid, stream, w, g, chunks, nchunk, norm, partials);
    seg_final_launch<SEG_LARS>(nseg, stream, (const double*)partials, nchunk, segs, lrp, weight_decay, grad_scale, trust_coef,
                               eps, clip, norm, x.nm, (double*)nullptr, q);
  }
  solver_launch(al, lars_apply_kernel<true, LR, LARS>, lars_apply_kernel<false, LR, LARS>, grid, stream, w, v, g, chunks, nchunk,
                segs, q, lrp, momentum, weight_decay, grad_scale, norm, x.nm, ema, x.omd);
  X3D_LAUNCH_CHECK(name);
  return X3D_OK;
}

extern "C" int x3d_lars(float* w, float* v, const float* g, const int* chunks, int nchunk, const int* segs, int nseg, float lr,
                        float momentum, float weight_decay, float grad_scale, float trust_coef, float eps, int clip,
                        const double* norm, float max_norm, float* ema, float ema_decay, double* partials, float* q,
                        void* stream) {
  return lars_run<true>("lars", w, v, g, chunks, nchunk, segs, nseg, LrOne{lr}, momentum, weight_decay, grad_scale, trust_coef,
                        eps, clip, norm, max_norm, ema, ema_decay, partials, q, stream);
}

extern "C" int x3d_lars_pt(float* w, float* v, const float* g, const int* chunks, int nchunk, const int* segs, int nseg,
                           const float* lr_scale, float lr, float momentum, float weight_decay, float grad_scale,
                           float trust_coef, float eps, int clip, const double* norm, float max_norm, float* ema,
                           float ema_decay, double* partials, float* q, void* stream) {
  SEG_REQUIRE_LR_SCALE("lars_pt");
  return lars_run<true>("lars_pt", w, v, g, chunks, nchunk, segs, nseg, LrSeg{lr, lr_scale}, momentum, weight_decay, grad_scale,
                        trust_coef, eps, clip, norm, max_norm, ema, ema_decay, partials, q, stream);
}

extern "C" int x3d_sgd_pt(float* w, float* v, const float* g, const int* chunks, int nchunk, const int* segs, int nseg,
                          const float* lr_scale, float lr, float momentum, float weight_decay, float grad_scale,
                          const double* norm, float max_norm, float* ema, float ema_decay, void* stream) {
  SEG_REQUIRE_LR_SCALE("sgd_pt");
  return lars_run<false>("sgd_pt", w, v, g, chunks, nchunk, segs, nseg, LrSeg{lr, lr_scale}, momentum, weight_decay, grad_scale,
                         0.f, 0.f, 0, norm, max_norm, ema, ema_decay, (double*)nullptr, (float*)nullptr, stream);
}

// x3d_adamw / x3d_adamw_pt (DECOUPLED = true; weight_decay unused) and x3d_adam_pt (false: the coupled L2 term weight_decay)
template <bool DECOUPLED, class LR>
static int adamw_run(const char* name, float* w, float* m, float* v, const float* g, const int* chunks, int nchunk,
                     const int* segs, int nseg, LR lrp, float beta1, float beta2, float eps, float decay, float weight_decay,
                     float grad_scale, long long step, const double* norm, float max_norm, float* ema, float ema_decay,
                     void* stream) {
  X3D_REQUIRE(w && m && v && g && step >= 1, "%s: bad args (step counts from 1)", name);
  SEG_REQUIRE_TABLE(name);
  X3D_REQUIRE((((uintptr_t)w | (uintptr_t)m | (uintptr_t)v | (uintptr_t)g | (uintptr_t)ema) & 3) == 0, "%s: misaligned pointer", name);
  X3D_REQUIRE(seg_finite_ge0(decay), "%s: decay must be >= 0 and finite", name);
  SOLVER_REQUIRE_EXTRAS(name);
  const SolverExtras x(norm, max_norm, ema, ema_decay);
  solver_launch(seg_aligned(w, m, v, g, ema), adamw_kernel<true, LR, DECOUPLED>, adamw_kernel<false, LR, DECOUPLED>,
                seg_grid(nchunk), stream, w, m, v, g, chunks, nchunk, segs, lrp, beta1, beta2, eps, weight_decay, grad_scale, norm,
                x.nm, ema, x.omd);
  X3D_LAUNCH_CHECK(name);
  return X3D_OK;
}

extern "C" int x3d_adamw(float* w, float* m, float* v, const float* g, const int* chunks, int nchunk, const int* segs, int nseg,
                         float lr, float beta1, float beta2, float eps, float decay, float grad_scale, long long step,
                         const double* norm, float max_norm, float* ema, float ema_decay, void* stream) {
  return adamw_run<true>("adamw", w, m, v, g, chunks, nchunk, segs, nseg,
                         AdamLrOne{(float)adam_lr_t(lr, beta1, beta2, step > 0 ? step : 1), lr * decay}, beta1, beta2, eps, decay,
                         0.f, grad_scale, step, norm, max_norm, ema, ema_decay, stream);
}

extern "C" int x3d_adamw_pt(float* w, float* m, float* v, const float* g, const int* chunks, int nchunk, const int* segs,
                            int nseg, const float* lr_scale, float lr, float beta1, float beta2, float eps, float decay,
                            float grad_scale, long long step, const double* norm, float max_norm, float* ema, float ema_decay,
                            void* stream) {
  SEG_REQUIRE_LR_SCALE("adamw_pt");
  return adamw_run<true>("adamw_pt", w, m, v, g, chunks, nchunk, segs, nseg,
                         adam_lr_seg(lr, lr_scale, beta1, beta2, step > 0 ? step : 1, decay), beta1, beta2, eps, decay, 0.f,
                         grad_scale, step, norm, max_norm, ema, ema_decay, stream);
}

extern "C" int x3d_adam_pt(float* w, float* m, float* v, const float* g, const int* chunks, int nchunk, const int* segs, int nseg,
                           const float* lr_scale, float lr, float beta1, float beta2, float eps, float weight_decay,
                           float grad_scale, long long step, const double* norm, float max_norm, float* ema, float ema_decay,
                           void* stream) {
  SEG_REQUIRE_LR_SCALE("adam_pt");
  return adamw_run<false>("adam_pt", w, m, v, g, chunks, nchunk, segs, nseg,
                          adam_lr_seg(lr, lr_scale, beta1, beta2, step > 0 ? step : 1, 0.f), beta1, beta2, eps, 0.f, weight_decay,
                          grad_scale, step, norm, max_norm, ema, ema_decay, stream);
}

template <class LR>
static int lamb_run(const char* name, float* w, float* m, float* v, const float* g, const int* chunks, int nchunk, const int* segs,
                    int nseg, LR lrp, float beta1, float beta2, float eps, float decay, float grad_scale, long long step,
                    const double* norm, float max_norm, float* ema, float ema_decay, double* partials, float* q, void* stream) {
  X3D_REQUIRE(w && m && v && g && partials && q && step >= 1, "%s: bad args (step counts from 1)", name);
  SEG_REQUIRE_TABLE(name);
  X3D_REQUIRE((((uintptr_t)w | (uintptr_t)m | (uintptr_t)v | (uintptr_t)g | (uintptr_t)ema | (uintptr_t)q) & 3) == 0 &&
              ((uintptr_t)partials & 7) == 0, "%s: misaligned pointer", name);
  X3D_REQUIRE(eps > 0.f && eps <= 3.0e38f, "%s: eps must be positive and finite", name);
  X3D_REQUIRE(seg_finite_ge0(decay), "%s: decay must be >= 0 and finite", name);
  SOLVER_REQUIRE_EXTRAS(name);
  const unsigned grid = seg_grid(nchunk);
  const SolverExtras x(norm, max_norm, ema, ema_decay);
  const float r = (float)adam_lr_t(1.f, beta1, beta2, step);
  const bool al = seg_aligned(w, m, v, g, ema);
  solver_launch(al, lamb_moments_kernel<true>, lamb_moments_kernel<false>, grid, stream, w, m, v, g, chunks, nchunk, segs, r,
                beta1, beta2, eps, decay, grad_scale, norm, x.nm, partials);
  seg_final_launch<SEG_LAMB>(nseg, stream, (const double*)partials, nchunk, segs, LrOne{0.f}, 0.f, grad_scale, 0.f, 0.f, 0, norm,
                             x.nm, (double*)nullptr, q);
  solver_launch(al, lamb_apply_kernel<true, LR>, lamb_apply_kernel<false, LR>, grid, stream, w, m, v, chunks, nchunk, segs, q,
                lrp, r, eps, decay, norm, ema, x.omd);
  X3D_LAUNCH_CHECK(name);
  return X3D_OK;
}

extern "C" int x3d_lamb(float* w, float* m, float* v, const float* g, const int* chunks, int nchunk, const int* segs, int nseg,
                        float lr, float beta1, float beta2, float eps, float decay, float grad_scale, long long step,
                        const double* norm, float max_norm, float* ema, float ema_decay, double* partials, float* q,
                        void* stream) {
  return lamb_run("lamb", w, m, v, g, chunks, nchunk, segs, nseg, LrOne{lr}, beta1, beta2, eps, decay, grad_scale, step, norm,
                  max_norm, ema, ema_decay, partials, q, stream);
}

extern "C" int x3d_lamb_pt(float* w, float* m, float* v, const float* g, const int* chunks, int nchunk, const int* segs, int nseg,
                           const float* lr_scale, float lr, float beta1, float beta2, float eps, float decay, float grad_scale,
                           long long step, const double* norm, float max_norm, float* ema, float ema_decay, double* partials,
                           float* q, void* stream) {
  SEG_REQUIRE_LR_SCALE("lamb_pt");
  return lamb_run("lamb_pt", w, m, v, g, chunks, nchunk, segs, nseg, LrSeg{lr, lr_scale}, beta1, beta2, eps, decay, grad_scale,
                  step, norm, max_norm, ema, ema_decay, partials, q, stream);
}

// ------------------------------------------------------------------------------------------------
// the fp16 loss scaler on the device: x3d_loss_scale_apply / x3d_seg_unscale_sumsq / x3d_loss_scale_update
// (x3d_unscale_sumsq stands beside x3d_grad_sumsq above)
// ------------------------------------------------------------------------------------------------
// state = X3D_LOSS_SCALE_STATE doubles (include/x3d_hip.h): scale S, 1 / S, consecutive finite steps, skipped steps, applied
// steps, 1.0 after a skipped update, two zeros.  S is a power of two, so every product with it or with 1 / S is exact.
enum { LS_SCALE = 0, LS_INV = 1, LS_GOOD = 2, LS_SKIPPED = 3, LS_APPLIED = 4, LS_LAST_SKIPPED = 5 };

template <int VEC>
__global__ __launch_bounds__(SOLVER_BLOCK) void loss_scale_apply_kernel(float* __restrict__ x, long long n,
                                                                        const double* __restrict__ state) {
  const float s = (float)state[LS_SCALE];
  solver_for_items<VEC>(n, [&](auto nc, long long i) {
    constexpr int N = decltype(nc)::value;
    float v[N];
    vec_load<N>(x + i, v);
    solver_each<N>([&](int e) { v[e] = v[e] * s; });
    vec_store<N>(x + i, v);
  });
}

extern "C" int x3d_loss_scale_apply(float* x, long long n, const double* state, void* stream) {
  X3D_REQUIRE(x && state && n > 0, "loss_scale_apply: bad args");
  X3D_REQUIRE(((uintptr_t)x & 3) == 0 && ((uintptr_t)state & 7) == 0, "loss_scale_apply: misaligned pointer");
  const int vec = solver_vec(nullptr, x);
  solver_launch(vec == 4, loss_scale_apply_kernel<4>, loss_scale_apply_kernel<1>, solver_grid(solver_items(n, vec)), stream, x, n,
                state);
  X3D_LAUNCH_CHECK("loss_scale_apply");
  return X3D_OK;
}

extern "C" int x3d_seg_unscale_sumsq(float* g, const int* chunks, int nchunk, const int* segs, int nseg, const double* state,
                                     double* partials, double* out, void* stream) {
  X3D_REQUIRE(g && state && partials && out, "seg_unscale_sumsq: bad args");
  SEG_REQUIRE_TABLE("seg_unscale_sumsq");
  X3D_REQUIRE(((uintptr_t)g & 3) == 0 && (((uintptr_t)state | (uintptr_t)partials | (uintptr_t)out) & 7) == 0,
              "seg_unscale_sumsq: misaligned pointer");
  solver_launch(seg_aligned(g), seg_unscale_sumsq_kernel<true>, seg_unscale_sumsq_kernel<false>, seg_grid(nchunk), stream, g,
                chunks, nchunk, state, partials);
  // x3d_seg_grad_sumsq's reduction: all chunks in ascending order, sums and counts
  hipLaunchKernelGGL(grad_sumsq_final_kernel, dim3(1), dim3(64), 0, (hipStream_t)stream, (const double*)partials, nchunk, out);
  X3D_LAUNCH_CHECK("seg_unscale_sumsq");
  return X3D_OK;
}

// Keras' DynamicLossScale on the state, from the norm block the update launches of the same step have read.  One workgroup of
// one wave, one lane of it: eight doubles.
__global__ __launch_bounds__(64) void loss_scale_update_kernel(double* __restrict__ state, const double* __restrict__ norm,
                                                               long long growth_steps) {
  if (threadIdx.x != 0) return;
  double s = state[LS_SCALE], good = state[LS_GOOD];
  if (norm[1] != 0.0) {
    s = fmax(s * 0.5, 1.0);
    good = 0.0;
    state[LS_SKIPPED] = state[LS_SKIPPED] + 1.0;
    state[LS_LAST_SKIPPED] = 1.0;
  } else {
    state[LS_APPLIED] = state[LS_APPLIED] + 1.0;
    good += 1.0;
    state[LS_LAST_SKIPPED] = 0.0;
    const float twice = (float)(2.0 * s);
    if (good >= (double)growth_steps && (__float_as_uint(twice) & 0x7f800000u) != 0x7f800000u) {
      s = 2.0 * s;
      good = 0.0;
    }
  }
  state[LS_SCALE] = s;
  state[LS_INV] = 1.0 / s;
  state[LS_GOOD] = good;
}

extern "C" int x3d_loss_scale_update(double* state, const double* norm, long long growth_steps, void* stream) {
  X3D_REQUIRE(state && norm && growth_steps >= 1, "loss_scale_update: bad args (growth_steps counts from 1)");
  X3D_REQUIRE((((uintptr_t)state | (uintptr_t)norm) & 7) == 0, "loss_scale_update: misaligned pointer");
  hipLaunchKernelGGL(loss_scale_update_kernel, dim3(1), dim3(64), 0, (hipStream_t)stream, state, norm, growth_steps);
  X3D_LAUNCH_CHECK("loss_scale_update");
  return X3D_OK;
}
