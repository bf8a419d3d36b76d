// The training losses of the head, all seven entry points: softmax cross-entropy on labels (x3d_softmax_xent) and on dense target
// rows (x3d_softmax_xent_soft: label smoothing, mixup / CutMix), sigmoid / binary cross-entropy (x3d_sigmoid_bce: DATA.MULTI_LABEL),
// the knowledge-distillation forms of the three (x3d_softmax_xent_kd, x3d_sigmoid_bce_kd: DISTILL.*), and the weighted / focal
// form of each head (x3d_softmax_xent_w, x3d_sigmoid_bce_w: LOSS.*, sample weights).  The exact rules are in
// include/x3d_hip.h.  One 256-thread workgroup per row, sums in a fixed order, no atomics.
//
// Every term is written once, as a device function, and the kernels are compositions of them:
//   softmax_row           row maximum, sum of exp -> (mx, inv)
//   clip_p, in_range      q = clip(p, 1e-7, 1 - 1e-7) and [1e-7 <= p <= 1 - 1e-7]
//   hard_terms<SOFT>      stores probs; the row's sums, inner, q_y, the hard loss, the unusable-row flag.  SOFT = false: labels,
//                         SOFT = true: dense target rows
//   hard_grad<SOFT>       scale * p * (dL/dp - inner) for one element
//   hard_row<SOFT>        the stores of a row without a KD term: the two plain kernels and alpha == 0 of the KD kernel
//   void_row              NaN loss row, zero gradient
//   sigmoid_d, softplus_d, bce_term_d, block_sum_d, block_max_d      the fp64 pieces of the sigmoid head and of the KD terms
//   sigmoid_bce_row       the plain sigmoid row: sigmoid_bce_kernel and alpha == 0 of its KD kernel
// A distillation kernel with alpha == 0 takes a uniform branch into hard_row / sigmoid_bce_row -- the statements the plain kernel
// runs -- so its results are bit-identical to the plain kernel's and the teacher is never read.
//   clip_d, in_range_d, focal_d, softmax_kd_row, bce_w_term_d, bce_w_grad_d      the fp64 pieces of the two _w kernels
// A _w entry point with nothing set launches the distillation kernel of its head, so it inherits those bits.
#include "common.h"

#define LOSS_THREADS 256
#define LOSS_WAVES (LOSS_THREADS / WAVE)

// ------------------------------------------------------------------------------------------------
// softmax + Keras cross-entropy on probabilities.                                                    [TF-3p]
//   p = softmax(z);  q = clip(p, 1e-7, 1-1e-7)
//   labels        L = -log q_y + log sum_j q_j;                      dL/dp_j = [p_j in range] * (-[j==y]/q_y + 1/sum q)
//   dense rows y  S = sum_j y_j;  L = sum_j y_j * (-log q_j) + S * log sum_k q_k;
//                                                                     dL/dp_j = [p_j in range] * (-y_j / q_j + S / sum q)
//   dz = p * (dL/dp - inner),  inner = sum_k p_k dL/dp_k.  A one-hot row y gives the expressions of the label form.
// ------------------------------------------------------------------------------------------------
struct SoftmaxRow { float mx, inv; };

// scratch: >= LOSS_WAVES floats, bc: >= 1 float; both are free again on return
__device__ __forceinline__ SoftmaxRow softmax_row(const float* __restrict__ z, int M, float* scratch, float* bc) {
  const int tid = threadIdx.x;
  float mx = -INFINITY;
  for (int j = tid; j < M; j += LOSS_THREADS) mx = fmaxf(mx, z[j]);
  for (int o = 32; o > 0; o >>= 1) mx = fmaxf(mx, __shfl_xor(mx, o, 64));
  if ((tid & 63) == 0) scratch[tid >> 6] = mx;
  __syncthreads();
  mx = fmaxf(fmaxf(scratch[0], scratch[1]), fmaxf(scratch[2], scratch[3]));
  __syncthreads();
  float red[1] = {0.f};
  for (int j = tid; j < M; j += LOSS_THREADS) red[0] += expf(z[j] - mx);
  block_sum<1>(red, scratch);
  if (tid == 0) bc[0] = red[0];
  __syncthreads();
  const float inv = 1.f / bc[0];
  __syncthreads();
  return {mx, inv};
}

__device__ __forceinline__ float softmax_p(const float* __restrict__ z, int j, SoftmaxRow r) { return expf(z[j] - r.mx) * r.inv; }
__device__ __forceinline__ float clip_p(float p) { return fminf(fmaxf(p, 1e-7f), 1.f - 1e-7f); }
__device__ __forceinline__ bool in_range(float p) { return p >= 1e-7f && p <= 1.f - 1e-7f; }

struct HardTerms {
  float sumq, S, inner, qy, loss;
  const float* y;   // SOFT: the row of targets
  int label;        // !SOFT
  bool bad;         // label outside [0, M) (TF raises InvalidArgument; never used as an index) / a NaN target (x3d_mix_targets
                    // writes one for such a label)
};

// Stores the row of probs and fills `h`.  false (uniformly) when there is nothing to compare with -- labels / targets null:
// probs only.  scratch: 4 * NV floats, bc: NV floats, NV = 6 (SOFT) or 2.
template <bool SOFT>
__device__ __forceinline__ bool hard_terms(const float* __restrict__ z, SoftmaxRow r, const int* __restrict__ labels,
                                           const float* __restrict__ targets, float* probs, int n, int M, float* scratch,
                                           float* bc, HardTerms& h) {
  const int tid = threadIdx.x;
  h.S = 0.f; h.qy = 1.f; h.y = nullptr; h.label = -1;
  if (SOFT) {
    const float* y = h.y = targets ? targets + (long long)n * M : nullptr;
    // sum q, sum_k p_k*[in range], S, sum y*(-log q), sum [in range]*y*p/q, #NaN targets
    float r6[6] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
    for (int j = tid; j < M; j += LOSS_THREADS) {
      const float p = softmax_p(z, j, r);
      probs[(long long)n * M + j] = p;
      if (!y) continue;
      const float q = clip_p(p);
      const bool in = in_range(p);
      const float yj = y[j];
      r6[0] += q;
      r6[1] += in ? p : 0.f;
      if (yj != yj) { r6[5] += 1.f; continue; }
      r6[2] += yj;
      r6[3] += yj * -logf(q);
      r6[4] += in ? yj * p / q : 0.f;
    }
    if (!y) return false;
    block_sum<6>(r6, scratch);
    if (tid == 0) {
#pragma unroll
      for (int i = 0; i < 6; i++) bc[i] = r6[i];
    }
    __syncthreads();
    h.sumq = bc[0]; h.S = bc[2];
    h.bad = bc[5] > 0.f;
    h.loss = bc[3] + h.S * logf(h.sumq);
    // inner = S * sum_p_in / sumq - sum_k [in range] * y_k * p_k / q_k
    h.inner = h.S * bc[1] / h.sumq - bc[4];
  } else {
    h.label = labels ? labels[n] : -1;
    float r2[2] = {0.f, 0.f};  // sum q, sum_k p_k*[in range]
    for (int j = tid; j < M; j += LOSS_THREADS) {
      const float p = softmax_p(z, j, r);
      probs[(long long)n * M + j] = p;
      r2[0] += clip_p(p);
      r2[1] += in_range(p) ? p : 0.f;
    }
    if (!labels) return false;
    block_sum<2>(r2, scratch);
    if (tid == 0) { bc[0] = r2[0]; bc[1] = r2[1]; }
    __syncthreads();
    h.sumq = bc[0];
    h.bad = h.label < 0 || h.label >= M;
    h.loss = 0.f; h.inner = 0.f;
    if (!h.bad) {
      const float py = softmax_p(z, h.label, r);
      h.qy = clip_p(py);
      h.loss = -logf(h.qy) + logf(h.sumq);
      // inner = sum_p_in / sumq - [y in range] * p_y / q_y
      h.inner = bc[1] / h.sumq - (in_range(py) ? py / h.qy : 0.f);
    }
  }
  return true;
}

// d hard / dz_j times `scale`, in exactly this association: scale = 1 is the unscaled gradient to the bit
template <bool SOFT>
__device__ __forceinline__ float hard_grad(const HardTerms& h, float p, int j, float scale) {
  const bool in = in_range(p);
  float dldp;
  if (SOFT) {
    dldp = in ? h.S / h.sumq - h.y[j] / clip_p(p) : 0.f;
  } else {
    dldp = in ? 1.f / h.sumq : 0.f;
    if (j == h.label && in) dldp -= 1.f / h.qy;
  }
  return scale * p * (dldp - h.inner);
}

// an unusable sample: the loss row is NaN (so the step's loss is visibly non-finite) and the sample contributes no gradient
__device__ __forceinline__ void void_row(float* loss_rows, float* dlogits, int n, int M) {
  if (threadIdx.x == 0 && loss_rows) loss_rows[n] = __builtin_nanf("");
  if (dlogits)
    for (int j = threadIdx.x; j < M; j += LOSS_THREADS) dlogits[(long long)n * M + j] = 0.f;
}

template <bool SOFT>
__device__ __forceinline__ void hard_row(const float* __restrict__ z, SoftmaxRow r, const HardTerms& h, float* loss_rows,
                                         float* dlogits, float grad_scale, int n, int M) {
  if (h.bad) return void_row(loss_rows, dlogits, n, M);
  if (threadIdx.x == 0 && loss_rows) loss_rows[n] = h.loss;
  if (dlogits)
    for (int j = threadIdx.x; j < M; j += LOSS_THREADS)
      dlogits[(long long)n * M + j] = hard_grad<SOFT>(h, softmax_p(z, j, r), j, grad_scale);
}

__global__ __launch_bounds__(LOSS_THREADS) void softmax_xent_kernel(const float* __restrict__ logits,
                                                                    const int* __restrict__ labels, float* probs,
                                                                    float* loss_rows, float* dlogits, float grad_scale, int M) {
  __shared__ float scratch[8];
  __shared__ float bc[2];
  const int n = blockIdx.x;
  const float* z = logits + (long long)n * M;
  const SoftmaxRow r = softmax_row(z, M, scratch, bc);
  HardTerms h;
  if (!hard_terms<false>(z, r, labels, nullptr, probs, n, M, scratch, bc, h)) return;
  hard_row<false>(z, r, h, loss_rows, dlogits, grad_scale, n, M);
}

__global__ __launch_bounds__(LOSS_THREADS) void softmax_xent_soft_kernel(const float* __restrict__ logits,
                                                                         const float* __restrict__ targets, float* probs,
                                                                         float* loss_rows, float* dlogits, float grad_scale,
                                                                         int M) {
  __shared__ float scratch[24];
  __shared__ float bc[6];
  const int n = blockIdx.x;
  const float* z = logits + (long long)n * M;
  const SoftmaxRow r = softmax_row(z, M, scratch, bc);
  HardTerms h;
  if (!hard_terms<true>(z, r, nullptr, targets, probs, n, M, scratch, bc, h)) return;
  hard_row<true>(z, r, h, loss_rows, dlogits, grad_scale, n, M);
}

// ------------------------------------------------------------------------------------------------
// fp64 pieces of the sigmoid head and of the KD terms
// ------------------------------------------------------------------------------------------------
__device__ __forceinline__ double sigmoid_d(double z) {
  // exp of a non-positive argument only: no overflow for any finite z, 0 / 1 at the far ends
  if (z >= 0.0) return 1.0 / (1.0 + exp(-z));
  const double e = exp(z);
  return e / (1.0 + e);
}

__device__ __forceinline__ double softplus_d(double x) { return (x > 0.0 ? x : 0.0) + log1p(exp(-fabs(x))); }

// max(z, 0) - z*y + log1p(exp(-|z|)); max(z, 0) written as a select: NaN must not become 0 (the -z*y and log1p terms carry it anyway)
__device__ __forceinline__ double bce_term_d(double z, double y) { return (z > 0.0 ? z : 0.0) - z * y + log1p(exp(-fabs(z))); }

__device__ __forceinline__ bool nonfinite(float x) { return (__float_as_uint(x) & 0x7f800000u) == 0x7f800000u; }

// block-wide sum / max of one double per thread, returned to every thread; the waves' parts are added in wave order
__device__ __forceinline__ double block_sum_d(double v, double* part) {
  v = wave_sum_d(v);
  __syncthreads();   // `part` may still be read from the previous reduction
  if ((threadIdx.x & 63) == 0) part[threadIdx.x >> 6] = v;
  __syncthreads();
  double s = 0.0;
#pragma unroll
  for (int w = 0; w < LOSS_WAVES; w++) s += part[w];
  return s;
}

__device__ __forceinline__ double block_max_d(double v, double* part) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v = fmax(v, __shfl_xor(v, o, 64));
  __syncthreads();
  if ((threadIdx.x & 63) == 0) part[threadIdx.x >> 6] = v;
  __syncthreads();
  double s = part[0];
#pragma unroll
  for (int w = 1; w < LOSS_WAVES; w++) s = fmax(s, part[w]);
  return s;
}

// ------------------------------------------------------------------------------------------------
// sigmoid + Keras BinaryCrossentropy on the logits of Dense(activation="sigmoid") (TF 2.x evaluates it in the logits
// form [TF-3p]).  The element terms and the row sum in fp64:
//   p = sigmoid(z);  loss_row = mean_j ( max(z,0) - z*y + log1p(exp(-|z|)) );  dz = grad_scale * (p - y) / M
// ------------------------------------------------------------------------------------------------
__device__ __forceinline__ void sigmoid_bce_row(const float* __restrict__ logits, const float* __restrict__ targets,
                                                float* probs, float* loss_rows, float* dlogits, float grad_scale, int n, int M,
                                                double* part) {
  const long long row = (long long)n * M;
  const double gs = (double)grad_scale / (double)M;
  double acc = 0.0;
  for (int j = threadIdx.x; j < M; j += LOSS_THREADS) {
    const double z = (double)logits[row + j];
    const double p = sigmoid_d(z);      // NaN in, NaN out
    probs[row + j] = (float)p;
    if (!targets) continue;
    const double y = (double)targets[row + j];
    acc += bce_term_d(z, y);
    if (dlogits) dlogits[row + j] = (float)(gs * (p - y));
  }
  if (!targets || !loss_rows) return;
  const double s = block_sum_d(acc, part);
  if (threadIdx.x == 0) loss_rows[n] = (float)(s / (double)M);
}

__global__ __launch_bounds__(LOSS_THREADS) void sigmoid_bce_kernel(const float* __restrict__ logits,
                                                                   const float* __restrict__ targets, float* probs,
                                                                   float* loss_rows, float* dlogits, float grad_scale, int M) {
  __shared__ double part[LOSS_WAVES];
  sigmoid_bce_row(logits, targets, probs, loss_rows, dlogits, grad_scale, blockIdx.x, M, part);
}

// ------------------------------------------------------------------------------------------------
// Knowledge distillation: a second term against a teacher's logits at a temperature T (Hinton et al.).  With z the student's
// logits, t the teacher's, u = z / T, v = t / T and a = alpha:
//   softmax head   kd = T^2 * sum_j p_t,j * (log p_t,j - log p_s,j),  log p = x - lse(x), p_t = exp(log p_t);  d kd / dz = T * (p_s - p_t)
//   sigmoid head   kd = T^2 * mean_j [ (softplus(u_j) - s(v_j) u_j) - (softplus(v_j) - s(v_j) v_j) ];      d kd / dz_j = T * (s(u_j) - s(v_j)) / M
//   loss_rows = (1 - a) * hard + a * kd,  dlogits = grad_scale * ((1 - a) * d hard + a * d kd)
// The KD term is fp64 throughout -- it is a difference of log-probabilities that nearly cancel when the student is close to the
// teacher, and at 64 x 400 the launch is a few microseconds either way.  A non-finite teacher logit makes the row unusable.
// ------------------------------------------------------------------------------------------------
template <bool SOFT>
__global__ __launch_bounds__(LOSS_THREADS) void softmax_xent_kd_kernel(const float* __restrict__ logits,
                                                                       const float* __restrict__ teacher,
                                                                       const int* __restrict__ labels,
                                                                       const float* __restrict__ targets, float* probs,
                                                                       float* loss_rows, float* kd_rows, float* dlogits,
                                                                       float grad_scale, float alpha, float temperature, int M) {
  __shared__ float scratch[24];
  __shared__ float bc[6];
  __shared__ double part[LOSS_WAVES];
  const int n = blockIdx.x, tid = threadIdx.x;
  const float* z = logits + (long long)n * M;
  const SoftmaxRow r = softmax_row(z, M, scratch, bc);
  HardTerms h;
  if (!hard_terms<SOFT>(z, r, labels, targets, probs, n, M, scratch, bc, h)) return;
  if (alpha == 0.f) {
    if (tid == 0 && kd_rows) kd_rows[n] = 0.f;
    return hard_row<SOFT>(z, r, h, loss_rows, dlogits, grad_scale, n, M);
  }

  // ---- KD term, in log space ----
  const float* t = teacher + (long long)n * M;
  const double T = (double)temperature;
  double mv = -INFINITY, bad = 0.0;
  for (int j = tid; j < M; j += LOSS_THREADS) {
    const float tj = t[j];
    if (nonfinite(tj)) bad = 1.0;
    else mv = fmax(mv, (double)tj / T);
  }
  const bool kd_bad = block_max_d(bad, part) > 0.0;
  mv = block_max_d(mv, part);
  const double mu = (double)r.mx / T;       // T > 0: the maximum of z / T
  double su = 0.0, sv = 0.0;
  if (!kd_bad)
    for (int j = tid; j < M; j += LOSS_THREADS) {
      su += exp((double)z[j] / T - mu);
      sv += exp((double)t[j] / T - mv);
    }
  const double lse_u = mu + log(block_sum_d(su, part));
  const double lse_v = mv + log(block_sum_d(sv, part));
  double acc = 0.0;
  if (!kd_bad)
    for (int j = tid; j < M; j += LOSS_THREADS) {
      const double lps = (double)z[j] / T - lse_u, lpt = (double)t[j] / T - lse_v;
      acc += exp(lpt) * (lpt - lps);      // a teacher probability that underflows: 0 * finite = 0
    }
  const double kd = kd_bad ? (double)__builtin_nanf("") : T * T * block_sum_d(acc, part);
  if (tid == 0 && kd_rows) kd_rows[n] = (float)kd;
  if (h.bad || kd_bad) return void_row(loss_rows, dlogits, n, M);
  const double a = (double)alpha, b = 1.0 - (double)alpha;
  if (tid == 0 && loss_rows) loss_rows[n] = (float)(b * (double)h.loss + a * kd);
  if (dlogits) {
    for (int j = tid; j < M; j += LOSS_THREADS) {
      const float gh = hard_grad<SOFT>(h, softmax_p(z, j, r), j, 1.f);
      const double ps = exp((double)z[j] / T - lse_u), pt = exp((double)t[j] / T - lse_v);
      dlogits[(long long)n * M + j] = (float)((double)grad_scale * (b * (double)gh + a * T * (ps - pt)));
    }
  }
}

// sigmoid head: the hard term of sigmoid_bce_row, the Bernoulli KL per class against sigmoid(t / T)
__global__ __launch_bounds__(LOSS_THREADS) void sigmoid_bce_kd_kernel(const float* __restrict__ logits,
                                                                      const float* __restrict__ teacher,
                                                                      const float* __restrict__ targets, float* probs,
                                                                      float* loss_rows, float* kd_rows, float* dlogits,
                                                                      float grad_scale, float alpha, float temperature, int M) {
  __shared__ double part[LOSS_WAVES];
  const int n = blockIdx.x, tid = threadIdx.x;
  if (alpha == 0.f) {
    if (tid == 0 && kd_rows) kd_rows[n] = 0.f;
    return sigmoid_bce_row(logits, targets, probs, loss_rows, dlogits, grad_scale, n, M, part);
  }
  const long long row = (long long)n * M;
  const double gs = (double)grad_scale / (double)M;
  const double T = (double)temperature;
  double acc = 0.0, kacc = 0.0, bad = 0.0;
  for (int j = tid; j < M; j += LOSS_THREADS) {
    const double z = (double)logits[row + j];
    probs[row + j] = (float)sigmoid_d(z);
    acc += bce_term_d(z, (double)targets[row + j]);
    const float tj = teacher[row + j];
    if (nonfinite(tj)) { bad = 1.0; continue; }
    const double u = z / T, v = (double)tj / T, sv = sigmoid_d(v);
    kacc += (softplus_d(u) - sv * u) - (softplus_d(v) - sv * v);
  }
  const bool kd_bad = block_max_d(bad, part) > 0.0;
  const double hard = block_sum_d(acc, part) / (double)M;
  const double kd = kd_bad ? (double)__builtin_nanf("") : T * T * block_sum_d(kacc, part) / (double)M;
  const double a = (double)alpha, b = 1.0 - (double)alpha;
  if (tid == 0) {
    if (kd_rows) kd_rows[n] = (float)kd;
    if (loss_rows) loss_rows[n] = (float)(b * hard + a * kd);     // (NaN with a non-finite teacher logit)
  }
  if (kd_bad) return void_row(nullptr, dlogits, n, M);
  if (!dlogits) return;
  for (int j = tid; j < M; j += LOSS_THREADS) {
    const double z = (double)logits[row + j], y = (double)targets[row + j];
    const double su = sigmoid_d(z / T), sv = sigmoid_d((double)teacher[row + j] / T);
    dlogits[row + j] = (float)(gs * (b * (sigmoid_d(z) - y) + a * T * (su - sv)));
  }
}

// ------------------------------------------------------------------------------------------------
// Class-imbalance losses (LOSS.*): class weights c_j, a positive weight w+_j (sigmoid head), a sample weight r_n and focal
// factors on the hard term; the formulas are in include/x3d_hip.h.  With nothing set the host launches the kernels above, so
// these two only ever run with a modifier.  p, mx and inv come from the fp32 softmax_row / softmax_p (probs has the plain
// kernel's bits); everything behind them is fp64, stored as fp32, like the KD term.
// ------------------------------------------------------------------------------------------------
__device__ __forceinline__ bool bad_row_weight(float w) { return !(w >= 0.f) || nonfinite(w); }   // NaN, negative, inf
__device__ __forceinline__ double clip_d(float p) { return fmin(fmax((double)p, 1e-7), 1.0 - 1e-7); }
__device__ __forceinline__ bool in_range_d(float p) { return (double)p >= 1e-7 && (double)p <= 1.0 - 1e-7; }
__device__ __forceinline__ double pow_g(double x, double g) { return g == 0.0 ? 1.0 : pow(x, g); }   // x >= 0; x^0 = 1 also at x = 0

// f(x) = (1 - x)^g * (-log x) and f'(x) for x in (0, 1].  x = 1 (one class): f = 0 and f' = 0 -- its limit for g >= 1, and the
// element is outside the clip range there, so its gradient is masked anyway: 0, not inf * 0
struct Focal { double f, df; };
__device__ __forceinline__ Focal focal_d(double x, double g) {
  const double om = 1.0 - x;
  if (om <= 0.0) return {0.0, 0.0};
  const double L = -log(x), pw = pow_g(om, g);
  return {pw * L, -(g == 0.0 ? 0.0 : g * pw / om * L) - pw / x};
}

// the KD term of a softmax row in log space (the arithmetic of softmax_xent_kd_kernel); kd is NaN with a non-finite teacher logit
struct KdRow { double lse_u, lse_v, kd; bool bad; };
__device__ __forceinline__ KdRow softmax_kd_row(const float* __restrict__ z, const float* __restrict__ t, SoftmaxRow r, double T,
                                                int M, double* part) {
  const int tid = threadIdx.x;
  double mv = -INFINITY, bad = 0.0;
  for (int j = tid; j < M; j += LOSS_THREADS) {
    const float tj = t[j];
    if (nonfinite(tj)) bad = 1.0;
    else mv = fmax(mv, (double)tj / T);
  }
  KdRow k;
  k.bad = block_max_d(bad, part) > 0.0;
  mv = block_max_d(mv, part);
  const double mu = (double)r.mx / T;
  double su = 0.0, sv = 0.0;
  if (!k.bad)
    for (int j = tid; j < M; j += LOSS_THREADS) {
      su += exp((double)z[j] / T - mu);
      sv += exp((double)t[j] / T - mv);
    }
  k.lse_u = mu + log(block_sum_d(su, part));
  k.lse_v = mv + log(block_sum_d(sv, part));
  double acc = 0.0;
  if (!k.bad)
    for (int j = tid; j < M; j += LOSS_THREADS) {
      const double lps = (double)z[j] / T - k.lse_u, lpt = (double)t[j] / T - k.lse_v;
      acc += exp(lpt) * (lpt - lps);
    }
  const double s = block_sum_d(acc, part);
  k.kd = k.bad ? (double)__builtin_nanf("") : T * T * s;
  return k;
}

// hard = r * sum_j c_j y_j f(q_j / sum q);  loss_rows = (1 - a) * hard + a * r * kd.  SOFT = false: y is the one-hot row of labels[n]
template <bool SOFT>
__global__ __launch_bounds__(LOSS_THREADS) void softmax_xent_w_kernel(
    const float* __restrict__ logits, const float* __restrict__ teacher, const int* __restrict__ labels,
    const float* __restrict__ targets, const float* __restrict__ class_w, const float* __restrict__ row_w, float* probs,
    float* loss_rows, float* kd_rows, float* dlogits, float grad_scale, float gamma, float alpha, float temperature, int M) {
  __shared__ float scratch[8];
  __shared__ float bc[2];
  __shared__ double part[LOSS_WAVES];
  const int n = blockIdx.x, tid = threadIdx.x;
  const long long row = (long long)n * M;
  const float* z = logits + row;
  const SoftmaxRow r = softmax_row(z, M, scratch, bc);
  const float* y = SOFT ? targets + row : nullptr;
  const int label = SOFT ? -1 : labels[n];
  const float rwf = row_w ? row_w[n] : 1.f;
  const double rw = (double)rwf, g = (double)gamma;

  // sum q, sum_k p_k * [in range], NaN targets
  double sq = 0.0, spin = 0.0, nb = 0.0;
  for (int j = tid; j < M; j += LOSS_THREADS) {
    const float p = softmax_p(z, j, r);
    probs[row + j] = p;
    sq += clip_d(p);
    spin += in_range_d(p) ? (double)p : 0.0;
    if (SOFT && y[j] != y[j]) nb = 1.0;
  }
  const double sumq = block_sum_d(sq, part), sum_p_in = block_sum_d(spin, part);
  const bool bad = block_max_d(nb, part) > 0.0 || (!SOFT && (label < 0 || label >= M)) || bad_row_weight(rwf);

  const bool kd_on = alpha != 0.f;             // uniform; alpha == 0 never reads the teacher
  const double T = (double)temperature, a = (double)alpha, b = 1.0 - (double)alpha;
  const float* t = kd_on ? teacher + row : nullptr;
  KdRow k = {0.0, 0.0, 0.0, false};
  if (kd_on) k = softmax_kd_row(z, t, r, T, M, part);
  if (tid == 0 && kd_rows) kd_rows[n] = (float)k.kd;
  if (bad || k.bad) return void_row(loss_rows, dlogits, n, M);

  // hard term; B = sum_j a_j f'(x_j) x_j; sum_k [in range] p_k a_k f'(x_k)      (x = q / sum q, a_j = r c_j y_j)
  double hl = 0.0, Bs = 0.0, C1 = 0.0;
  for (int j = tid; j < M; j += LOSS_THREADS) {
    const double yj = SOFT ? (double)y[j] : (j == label ? 1.0 : 0.0);
    const double aj = rw * (class_w ? (double)class_w[j] : 1.0) * yj;
    if (aj == 0.0) continue;
    const float p = softmax_p(z, j, r);
    const double x = clip_d(p) / sumq;
    const Focal F = focal_d(x, g);
    hl += aj * F.f;
    Bs += aj * F.df * x;
    C1 += in_range_d(p) ? (double)p * aj * F.df : 0.0;
  }
  hl = block_sum_d(hl, part);
  Bs = block_sum_d(Bs, part);
  C1 = block_sum_d(C1, part);
  if (tid == 0 && loss_rows) loss_rows[n] = (float)(kd_on ? b * hl + a * rw * k.kd : hl);
  if (!dlogits) return;
  const double inner = (C1 - Bs * sum_p_in) / sumq;      // sum_k p_k dL/dp_k
  const double gs = (double)grad_scale;
  for (int j = tid; j < M; j += LOSS_THREADS) {
    const float p = softmax_p(z, j, r);
    const double yj = SOFT ? (double)y[j] : (j == label ? 1.0 : 0.0);
    const double aj = rw * (class_w ? (double)class_w[j] : 1.0) * yj;
    double dldp = 0.0;
    if (in_range_d(p)) dldp = ((aj == 0.0 ? 0.0 : aj * focal_d(clip_d(p) / sumq, g).df) - Bs) / sumq;
    const double dh = (double)p * (dldp - inner);
    double d = dh;
    if (kd_on) {
      const double ps = exp((double)z[j] / T - k.lse_u), pt = exp((double)t[j] / T - k.lse_v);
      d = b * dh + a * rw * T * (ps - pt);
    }
    dlogits[row + j] = (float)(gs * d);
  }
}

// hard = r * mean_j c_j [ y w+ (1 - s)^g+ softplus(-z) + (1 - y) s^g- softplus(z) ], s = sigmoid(z);  the derivative in closed form:
//   d/dz (1 - s)^g softplus(-z) = -(1 - s)^g (g s softplus(-z) + (1 - s)),   d/dz s^g softplus(z) = s^g (g (1 - s) softplus(z) + s)
__device__ __forceinline__ double bce_w_term_d(double z, double y, double c, double wp, double gp, double gn) {
  const double s = sigmoid_d(z), oms = sigmoid_d(-z);
  return c * (y * wp * pow_g(oms, gp) * softplus_d(-z) + (1.0 - y) * pow_g(s, gn) * softplus_d(z));
}

__device__ __forceinline__ double bce_w_grad_d(double z, double y, double c, double wp, double gp, double gn) {
  const double s = sigmoid_d(z), oms = sigmoid_d(-z);
  return c * ((1.0 - y) * pow_g(s, gn) * (gn * oms * softplus_d(z) + s) - y * wp * pow_g(oms, gp) * (gp * s * softplus_d(-z) + oms));
}

__global__ __launch_bounds__(LOSS_THREADS) void sigmoid_bce_w_kernel(
    const float* __restrict__ logits, const float* __restrict__ teacher, const float* __restrict__ targets,
    const float* __restrict__ class_w, const float* __restrict__ pos_w, const float* __restrict__ row_w, float* probs,
    float* loss_rows, float* kd_rows, float* dlogits, float grad_scale, float gamma_pos, float gamma_neg, float alpha,
    float temperature, int M) {
  __shared__ double part[LOSS_WAVES];
  const int n = blockIdx.x, tid = threadIdx.x;
  const long long row = (long long)n * M;
  const float rwf = row_w ? row_w[n] : 1.f;
  const double rw = (double)rwf, gp = (double)gamma_pos, gn = (double)gamma_neg;
  const bool kd_on = alpha != 0.f;             // uniform; alpha == 0 never reads the teacher
  const double T = (double)temperature, a = (double)alpha, b = 1.0 - (double)alpha;
  double acc = 0.0, kacc = 0.0, nb = 0.0, tb = 0.0;
  for (int j = tid; j < M; j += LOSS_THREADS) {
    const double z = (double)logits[row + j];
    probs[row + j] = (float)sigmoid_d(z);
    const double y = (double)targets[row + j];
    if (y != y) nb = 1.0;
    else acc += bce_w_term_d(z, y, class_w ? (double)class_w[j] : 1.0, pos_w ? (double)pos_w[j] : 1.0, gp, gn);
    if (!kd_on) continue;
    const float tj = teacher[row + j];
    if (nonfinite(tj)) { tb = 1.0; continue; }
    const double u = z / T, v = (double)tj / T, sv = sigmoid_d(v);
    kacc += (softplus_d(u) - sv * u) - (softplus_d(v) - sv * v);
  }
  const bool bad = block_max_d(nb, part) > 0.0 || bad_row_weight(rwf);
  const bool kd_bad = block_max_d(tb, part) > 0.0;
  const double hard = rw * block_sum_d(acc, part) / (double)M;
  const double ks = block_sum_d(kacc, part);
  const double kd = kd_bad ? (double)__builtin_nanf("") : T * T * ks / (double)M;
  if (tid == 0 && kd_rows) kd_rows[n] = (float)kd;     // (alpha == 0: 0)
  if (bad || kd_bad) return void_row(loss_rows, dlogits, n, M);
  if (tid == 0 && loss_rows) loss_rows[n] = (float)(kd_on ? b * hard + a * rw * kd : hard);
  if (!dlogits) return;
  const double gs = (double)grad_scale * rw / (double)M;
  for (int j = tid; j < M; j += LOSS_THREADS) {
    const double z = (double)logits[row + j];
    double d = bce_w_grad_d(z, (double)targets[row + j], class_w ? (double)class_w[j] : 1.0, pos_w ? (double)pos_w[j] : 1.0, gp, gn);
    if (kd_on) d = b * d + a * T * (sigmoid_d(z / T) - sigmoid_d((double)teacher[row + j] / T));
    dlogits[row + j] = (float)(gs * d);
  }
}

// ------------------------------------------------------------------------------------------------
// host side
// ------------------------------------------------------------------------------------------------
extern "C" int x3d_softmax_xent(const float* logits, const int* labels, float* probs, float* loss_rows,
                                float* dlogits, float grad_scale, int N, int M, void* stream) {
  X3D_REQUIRE(logits && probs && N > 0 && M > 0, "softmax_xent: bad args");
  X3D_REQUIRE(labels || (!loss_rows && !dlogits), "softmax_xent: loss/grad need labels");
  hipLaunchKernelGGL(softmax_xent_kernel, dim3(N), dim3(LOSS_THREADS), 0, (hipStream_t)stream, logits, labels, probs,
                     loss_rows, dlogits, grad_scale, M);
  X3D_LAUNCH_CHECK("softmax_xent");
  return X3D_OK;
}

extern "C" int x3d_softmax_xent_soft(const float* logits, const float* targets, float* probs, float* loss_rows,
                                     float* dlogits, float grad_scale, int N, int M, void* stream) {
  X3D_REQUIRE(logits && probs && N > 0 && M > 0, "softmax_xent_soft: bad args (N=%d M=%d)", N, M);
  X3D_REQUIRE(targets || (!loss_rows && !dlogits), "softmax_xent_soft: loss/grad need targets");
  X3D_REQUIRE((long long)N * M < (1LL << 31), "softmax_xent_soft: N*M = %lld >= 2^31", (long long)N * M);
  hipLaunchKernelGGL(softmax_xent_soft_kernel, dim3(N), dim3(LOSS_THREADS), 0, (hipStream_t)stream, logits, targets, probs,
                     loss_rows, dlogits, grad_scale, M);
  X3D_LAUNCH_CHECK("softmax_xent_soft");
  return X3D_OK;
}

extern "C" int x3d_sigmoid_bce(const float* logits, const float* targets, float* probs, float* loss_rows,
                               float* dlogits, float grad_scale, int N, int M, void* stream) {
  X3D_REQUIRE(logits && probs && N > 0 && M > 0, "sigmoid_bce: bad args (N=%d M=%d)", N, M);
  X3D_REQUIRE(targets || (!loss_rows && !dlogits), "sigmoid_bce: loss/grad need targets");
  X3D_REQUIRE((long long)N * M < (1LL << 31), "sigmoid_bce: N*M = %lld >= 2^31", (long long)N * M);
  hipLaunchKernelGGL(sigmoid_bce_kernel, dim3(N), dim3(LOSS_THREADS), 0, (hipStream_t)stream, logits, targets, probs,
                     loss_rows, dlogits, grad_scale, M);
  X3D_LAUNCH_CHECK("sigmoid_bce");
  return X3D_OK;
}

// do the byte ranges [a, a + na) and [b, b + nb) share a byte?  (a null pointer overlaps nothing)
static bool kd_overlap(const void* a, size_t na, const void* b, size_t nb) {
  if (!a || !b) return false;
  const uintptr_t x = (uintptr_t)a, y = (uintptr_t)b;
  return x < y + nb && y < x + na;
}

// the checks both distillation entry points share; `in` / `in_name`: a matrix input that must not alias an output
#define KD_COMMON_CHECKS(fn)                                                                                               \
  X3D_REQUIRE(logits, fn ": logits is null");                                                                              \
  X3D_REQUIRE(probs, fn ": probs is null");                                                                                \
  X3D_REQUIRE(N > 0 && M > 0, fn ": bad sizes N=%d M=%d", N, M);                                                           \
  X3D_REQUIRE((long long)N * M < (1LL << 31), fn ": N*M = %lld >= 2^31", (long long)N * M);                                \
  X3D_REQUIRE(alpha >= 0.f && alpha <= 1.f, fn ": alpha = %g outside [0, 1]", (double)alpha);                              \
  X3D_REQUIRE(temperature > 0.f && temperature <= 3.402823466e+38f, fn ": temperature = %g is not finite and > 0",         \
              (double)temperature);                                                                                        \
  X3D_REQUIRE(alpha == 0.f || teacher_logits, fn ": teacher_logits is null with alpha = %g > 0", (double)alpha)

#define KD_ALIAS_CHECK(fn, in, in_name)                                                                                    \
  X3D_REQUIRE(!kd_overlap(in, mat, probs, mat) && !kd_overlap(in, mat, dlogits, mat) &&                                    \
                  !kd_overlap(in, mat, loss_rows, vec) && !kd_overlap(in, mat, kd_rows, vec),                              \
              fn ": " in_name " overlaps an output")

extern "C" int x3d_softmax_xent_kd(const float* logits, const float* teacher_logits, const int* labels, const float* targets,
                                   float* probs, float* loss_rows, float* kd_rows, float* dlogits, float grad_scale,
                                   float alpha, float temperature, int N, int M, void* stream) {
  KD_COMMON_CHECKS("softmax_xent_kd");
  X3D_REQUIRE((labels != nullptr) != (targets != nullptr), "softmax_xent_kd: exactly one of labels / targets must be given (%s)",
              labels ? "both are" : "neither is");
  const size_t mat = (size_t)N * M * sizeof(float), vec = (size_t)N * sizeof(float);
  KD_ALIAS_CHECK("softmax_xent_kd", teacher_logits, "teacher_logits");
  KD_ALIAS_CHECK("softmax_xent_kd", targets, "targets");
  if (targets)
    hipLaunchKernelGGL(softmax_xent_kd_kernel<true>, dim3(N), dim3(LOSS_THREADS), 0, (hipStream_t)stream, logits, teacher_logits,
                       labels, targets, probs, loss_rows, kd_rows, dlogits, grad_scale, alpha, temperature, M);
  else
    hipLaunchKernelGGL(softmax_xent_kd_kernel<false>, dim3(N), dim3(LOSS_THREADS), 0, (hipStream_t)stream, logits, teacher_logits,
                       labels, targets, probs, loss_rows, kd_rows, dlogits, grad_scale, alpha, temperature, M);
  X3D_LAUNCH_CHECK("softmax_xent_kd");
  return X3D_OK;
}

extern "C" int x3d_sigmoid_bce_kd(const float* logits, const float* teacher_logits, const float* targets, float* probs,
                                  float* loss_rows, float* kd_rows, float* dlogits, float grad_scale, float alpha,
                                  float temperature, int N, int M, void* stream) {
  KD_COMMON_CHECKS("sigmoid_bce_kd");
  X3D_REQUIRE(targets, "sigmoid_bce_kd: targets is null");
  const size_t mat = (size_t)N * M * sizeof(float), vec = (size_t)N * sizeof(float);
  KD_ALIAS_CHECK("sigmoid_bce_kd", teacher_logits, "teacher_logits");
  KD_ALIAS_CHECK("sigmoid_bce_kd", targets, "targets");
  hipLaunchKernelGGL(sigmoid_bce_kd_kernel, dim3(N), dim3(LOSS_THREADS), 0, (hipStream_t)stream, logits, teacher_logits, targets,
                     probs, loss_rows, kd_rows, dlogits, grad_scale, alpha, temperature, M);
  X3D_LAUNCH_CHECK("sigmoid_bce_kd");
  return X3D_OK;
}

// a weight table / vector (`n` floats) that must not alias an output
#define W_ALIAS_CHECK(fn, in, n, in_name)                                                                                  \
  X3D_REQUIRE(!kd_overlap(in, (size_t)(n) * sizeof(float), probs, mat) && !kd_overlap(in, (size_t)(n) * sizeof(float), dlogits, mat) && \
                  !kd_overlap(in, (size_t)(n) * sizeof(float), loss_rows, vec) &&                                          \
                  !kd_overlap(in, (size_t)(n) * sizeof(float), kd_rows, vec),                                              \
              fn ": " in_name " overlaps an output")

#define W_GAMMA_CHECK(fn, g, g_name) \
  X3D_REQUIRE(g >= 0.f && g <= 8.f, fn ": " g_name " = %g outside [0, 8]", (double)g)

// Nothing set (no table, no row weights, every gamma 0): the launch of x3d_softmax_xent_kd / x3d_sigmoid_bce_kd itself, whose
// alpha == 0 branch in turn runs the plain kernels' statements -- the bits of the five entry points above by construction.
extern "C" int x3d_softmax_xent_w(const float* logits, const float* teacher_logits, const int* labels, const float* targets,
                                  const float* class_w, const float* row_w, float* probs, float* loss_rows, float* kd_rows,
                                  float* dlogits, float grad_scale, float gamma, float alpha, float temperature, int N, int M,
                                  void* stream) {
  KD_COMMON_CHECKS("softmax_xent_w");
  W_GAMMA_CHECK("softmax_xent_w", gamma, "gamma");
  X3D_REQUIRE((labels != nullptr) != (targets != nullptr), "softmax_xent_w: exactly one of labels / targets must be given (%s)",
              labels ? "both are" : "neither is");
  const size_t mat = (size_t)N * M * sizeof(float), vec = (size_t)N * sizeof(float);
  KD_ALIAS_CHECK("softmax_xent_w", teacher_logits, "teacher_logits");
  KD_ALIAS_CHECK("softmax_xent_w", targets, "targets");
  W_ALIAS_CHECK("softmax_xent_w", class_w, M, "class_w");
  W_ALIAS_CHECK("softmax_xent_w", row_w, N, "row_w");
  const dim3 grid(N), block(LOSS_THREADS);
  hipStream_t s = (hipStream_t)stream;
  if (!class_w && !row_w && gamma == 0.f) {
    if (targets)
      hipLaunchKernelGGL(softmax_xent_kd_kernel<true>, grid, block, 0, s, logits, teacher_logits, labels, targets, probs,
                         loss_rows, kd_rows, dlogits, grad_scale, alpha, temperature, M);
    else
      hipLaunchKernelGGL(softmax_xent_kd_kernel<false>, grid, block, 0, s, logits, teacher_logits, labels, targets, probs,
                         loss_rows, kd_rows, dlogits, grad_scale, alpha, temperature, M);
  } else if (targets) {
    hipLaunchKernelGGL(softmax_xent_w_kernel<true>, grid, block, 0, s, logits, teacher_logits, labels, targets, class_w, row_w,
                       probs, loss_rows, kd_rows, dlogits, grad_scale, gamma, alpha, temperature, M);
  } else {
    hipLaunchKernelGGL(softmax_xent_w_kernel<false>, grid, block, 0, s, logits, teacher_logits, labels, targets, class_w, row_w,
                       probs, loss_rows, kd_rows, dlogits, grad_scale, gamma, alpha, temperature, M);
  }
  X3D_LAUNCH_CHECK("softmax_xent_w");
  return X3D_OK;
}

extern "C" int x3d_sigmoid_bce_w(const float* logits, const float* teacher_logits, const float* targets, const float* class_w,
                                 const float* pos_w, const float* row_w, float* probs, float* loss_rows, float* kd_rows,
                                 float* dlogits, float grad_scale, float gamma_pos, float gamma_neg, float alpha,
                                 float temperature, int N, int M, void* stream) {
  KD_COMMON_CHECKS("sigmoid_bce_w");
  W_GAMMA_CHECK("sigmoid_bce_w", gamma_pos, "gamma_pos");
  W_GAMMA_CHECK("sigmoid_bce_w", gamma_neg, "gamma_neg");
  X3D_REQUIRE(targets, "sigmoid_bce_w: targets is null");
  const size_t mat = (size_t)N * M * sizeof(float), vec = (size_t)N * sizeof(float);
  KD_ALIAS_CHECK("sigmoid_bce_w", teacher_logits, "teacher_logits");
  KD_ALIAS_CHECK("sigmoid_bce_w", targets, "targets");
  W_ALIAS_CHECK("sigmoid_bce_w", class_w, M, "class_w");
  W_ALIAS_CHECK("sigmoid_bce_w", pos_w, M, "pos_w");
  W_ALIAS_CHECK("sigmoid_bce_w", row_w, N, "row_w");
  if (!class_w && !pos_w && !row_w && gamma_pos == 0.f && gamma_neg == 0.f)
    hipLaunchKernelGGL(sigmoid_bce_kd_kernel, dim3(N), dim3(LOSS_THREADS), 0, (hipStream_t)stream, logits, teacher_logits,
                       targets, probs, loss_rows, kd_rows, dlogits, grad_scale, alpha, temperature, M);
  else
    hipLaunchKernelGGL(sigmoid_bce_w_kernel, dim3(N), dim3(LOSS_THREADS), 0, (hipStream_t)stream, logits, teacher_logits,
                       targets, class_w, pos_w, row_w, probs, loss_rows, kd_rows, dlogits, grad_scale, gamma_pos, gamma_neg,
                       alpha, temperature, M);
  X3D_LAUNCH_CHECK("sigmoid_bce_w");
  return X3D_OK;
}
