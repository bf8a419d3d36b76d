// Knowledge distillation (DISTILL.* of the config): the three training losses with a second term against a teacher's logits
// at a temperature T (Hinton et al.).  The exact rules are in include/x3d_hip.h.  With z the student's logits, t the teacher's,
// u = z / T, v = t / T and a = alpha:
//   softmax head   kd = T^2 * sum_j p_t,j * (log p_t,j - log p_s,j),  log p = x - lse(x), p_t = exp(log p_t);  d kd / dz = T * (p_s - p_t)
//   sigmoid head   kd = T^2 * mean_j [ (softplus(u_j) - s(v_j) u_j) - (softplus(v_j) - s(v_j) v_j) ];      d kd / dz_j = T * (s(u_j) - s(v_j)) / M
//   loss_rows = (1 - a) * hard + a * kd,  dlogits = grad_scale * ((1 - a) * d hard + a * d kd)
// The hard term and `probs` are the statements of softmax_xent_kernel / softmax_xent_soft_kernel (head.hip) and
// sigmoid_bce_kernel (multilabel.hip), repeated here expression for expression: a == 0 is a uniform branch that ends in exactly
// their stores, so the results are bit-identical to theirs and the teacher is never read.  The KD term is fp64 throughout -- it
// is a difference of log-probabilities that nearly cancel when the student is close to the teacher, and at 64 x 400 the launch
// is a few microseconds either way.  One 256-thread workgroup per row, sums in a fixed order, no atomics.
#include "common.h"

#define KD_THREADS 256
#define KD_WAVES (KD_THREADS / WAVE)

__device__ __forceinline__ double kd_sigmoid_d(double z) {   // as sigmoid_d of multilabel.hip: exp of a non-positive argument only
  if (z >= 0.0) return 1.0 / (1.0 + exp(-z));
  const double e = exp(z);
  return e / (1.0 + e);
}

__device__ __forceinline__ double kd_softplus_d(double x) { return (x > 0.0 ? x : 0.0) + log1p(exp(-fabs(x))); }

__device__ __forceinline__ bool kd_nonfinite(float x) { return (__float_as_uint(x) & 0x7f800000u) == 0x7f800000u; }

// block-wide sum / max of one double per thread, returned to every thread; the waves' parts are added in wave order
__device__ __forceinline__ double kd_block_sum_d(double v, double* part) {
  v = wave_sum_d(v);
  __syncthreads();   // `part` may still be read from the previous reduction
  if ((threadIdx.x & 63) == 0) part[threadIdx.x >> 6] = v;
  __syncthreads();
  double s = 0.0;
#pragma unroll
  for (int w = 0; w < KD_WAVES; w++) s += part[w];
  return s;
}

__device__ __forceinline__ double kd_block_max_d(double v, double* part) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v = fmax(v, __shfl_xor(v, o, 64));
  __syncthreads();
  if ((threadIdx.x & 63) == 0) part[threadIdx.x >> 6] = v;
  __syncthreads();
  double s = part[0];
#pragma unroll
  for (int w = 1; w < KD_WAVES; w++) s = fmax(s, part[w]);
  return s;
}

// ------------------------------------------------------------------------------------------------
// softmax head.  SOFT = false: the hard term of softmax_xent_kernel on `labels`; SOFT = true: that of
// softmax_xent_soft_kernel on the dense rows in `targets`.
// ------------------------------------------------------------------------------------------------
template <bool SOFT>
__global__ __launch_bounds__(KD_THREADS) void softmax_xent_kd_kernel(const float* __restrict__ logits,
                                                                     const float* __restrict__ teacher,
                                                                     const int* __restrict__ labels,
                                                                     const float* __restrict__ targets, float* probs,
                                                                     float* loss_rows, float* kd_rows, float* dlogits,
                                                                     float grad_scale, float alpha, float temperature, int M) {
  __shared__ float scratch[24];
  __shared__ float bc[6];
  __shared__ double part[KD_WAVES];
  const int n = blockIdx.x, tid = threadIdx.x;
  const float* z = logits + (long long)n * M;
  float mx = -INFINITY;
  for (int j = tid; j < M; j += 256) mx = fmaxf(mx, z[j]);
  for (int o = 32; o > 0; o >>= 1) mx = fmaxf(mx, __shfl_xor(mx, o, 64));
  if ((tid & 63) == 0) scratch[tid >> 6] = mx;
  __syncthreads();
  mx = fmaxf(fmaxf(scratch[0], scratch[1]), fmaxf(scratch[2], scratch[3]));
  __syncthreads();
  float red[1] = {0.f};
  for (int j = tid; j < M; j += 256) red[0] += expf(z[j] - mx);
  block_sum<1>(red, scratch);
  if (tid == 0) bc[0] = red[0];
  __syncthreads();
  const float inv = 1.f / bc[0];
  __syncthreads();
  // ---- hard term: the sums of the sibling kernel, then hard_bad / hard_loss / the per-element gradient further down ----
  const float* y = SOFT ? targets + (long long)n * M : nullptr;
  const int label = SOFT ? -1 : labels[n];
  float sumq, sum_p_in, S = 0.f, inner, py = 0.f, qy = 1.f, hard_loss;
  bool hard_bad;
  if (SOFT) {
    // sum q, sum_k p_k*[in range], S, sum y*(-log q), sum [in range]*y*p/q, #NaN targets
    float r6[6] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
    for (int j = tid; j < M; j += 256) {
      const float p = expf(z[j] - mx) * inv;
      probs[(long long)n * M + j] = p;
      const float q = fminf(fmaxf(p, 1e-7f), 1.f - 1e-7f);
      const bool in = (p >= 1e-7f && p <= 1.f - 1e-7f);
      const float yj = y[j];
      r6[0] += q;
      r6[1] += in ? p : 0.f;
      if (yj != yj) { r6[5] += 1.f; continue; }
      r6[2] += yj;
      r6[3] += yj * -logf(q);
      r6[4] += in ? yj * p / q : 0.f;
    }
    block_sum<6>(r6, scratch);
    if (tid == 0) {
#pragma unroll
      for (int i = 0; i < 6; i++) bc[i] = r6[i];
    }
    __syncthreads();
    sumq = bc[0]; sum_p_in = bc[1]; S = bc[2];
    hard_bad = bc[5] > 0.f;
    hard_loss = bc[3] + S * logf(sumq);
    // inner = sum_k p_k * dL/dp_k = S * sum_p_in / sumq - sum_k [in range] * y_k * p_k / q_k
    inner = S * sum_p_in / sumq - bc[4];
  } else {
    float r2[2] = {0.f, 0.f};  // sum q, sum_k p_k*[in range]  (for the dz formula)
    for (int j = tid; j < M; j += 256) {
      const float p = expf(z[j] - mx) * inv;
      probs[(long long)n * M + j] = p;
      const float q = fminf(fmaxf(p, 1e-7f), 1.f - 1e-7f);
      r2[0] += q;
      r2[1] += (p >= 1e-7f && p <= 1.f - 1e-7f) ? p : 0.f;
    }
    block_sum<2>(r2, scratch);
    if (tid == 0) { bc[0] = r2[0]; bc[1] = r2[1]; }
    __syncthreads();
    sumq = bc[0]; sum_p_in = bc[1];
    hard_bad = label < 0 || label >= M;   // never used as an index
    hard_loss = 0.f; inner = 0.f;
    if (!hard_bad) {
      py = expf(z[label] - mx) * inv;
      qy = fminf(fmaxf(py, 1e-7f), 1.f - 1e-7f);
      const bool y_in = (py >= 1e-7f && py <= 1.f - 1e-7f);
      hard_loss = -logf(qy) + logf(sumq);
      // inner = sum_k p_k * dL/dp_k = sum_p_in / sumq - [y in range] * p_y / q_y
      inner = sum_p_in / sumq - (y_in ? py / qy : 0.f);
    }
  }

  if (alpha == 0.f) {
    // ---- no distillation: the stores of the sibling kernel, the teacher is not read ----
    if (tid == 0 && kd_rows) kd_rows[n] = 0.f;
    if (hard_bad) {
      if (tid == 0 && loss_rows) loss_rows[n] = __builtin_nanf("");
      if (dlogits)
        for (int j = tid; j < M; j += 256) dlogits[(long long)n * M + j] = 0.f;
      return;
    }
    if (tid == 0 && loss_rows) loss_rows[n] = hard_loss;
    if (dlogits) {
      for (int j = tid; j < M; j += 256) {
        const float p = expf(z[j] - mx) * inv;
        const bool in = (p >= 1e-7f && p <= 1.f - 1e-7f);
        if (SOFT) {
          const float q = fminf(fmaxf(p, 1e-7f), 1.f - 1e-7f);
          const float dldp = in ? S / sumq - y[j] / q : 0.f;
          dlogits[(long long)n * M + j] = grad_scale * p * (dldp - inner);
        } else {
          float dldp = in ? 1.f / sumq : 0.f;
          if (j == label && in) dldp -= 1.f / qy;
          dlogits[(long long)n * M + j] = grad_scale * p * (dldp - inner);
        }
      }
    }
    return;
  }

  // ---- KD term, fp64, in log space ----
  const float* t = teacher + (long long)n * M;
  const double T = (double)temperature;
  double mv = -INFINITY, bad = 0.0;
  for (int j = tid; j < M; j += 256) {
    const float tj = t[j];
    if (kd_nonfinite(tj)) bad = 1.0;
    else mv = fmax(mv, (double)tj / T);
  }
  const bool kd_bad = kd_block_max_d(bad, part) > 0.0;
  mv = kd_block_max_d(mv, part);
  const double mu = (double)mx / T;       // T > 0: the maximum of z / T
  double su = 0.0, sv = 0.0;
  if (!kd_bad)
    for (int j = tid; j < M; j += 256) {
      su += exp((double)z[j] / T - mu);
      sv += exp((double)t[j] / T - mv);
    }
  const double lse_u = mu + log(kd_block_sum_d(su, part));
  const double lse_v = mv + log(kd_block_sum_d(sv, part));
  double acc = 0.0;
  if (!kd_bad)
    for (int j = tid; j < M; j += 256) {
      const double lps = (double)z[j] / T - lse_u, lpt = (double)t[j] / T - lse_v;
      acc += exp(lpt) * (lpt - lps);      // a teacher probability that underflows: 0 * finite = 0
    }
  const double kd = kd_bad ? (double)__builtin_nanf("") : T * T * kd_block_sum_d(acc, part);
  if (tid == 0 && kd_rows) kd_rows[n] = (float)kd;
  if (hard_bad || kd_bad) {
    // an unusable sample (label outside [0, M), NaN target, non-finite teacher logit): NaN loss row, no gradient
    if (tid == 0 && loss_rows) loss_rows[n] = __builtin_nanf("");
    if (dlogits)
      for (int j = tid; j < M; j += 256) dlogits[(long long)n * M + j] = 0.f;
    return;
  }
  const double a = (double)alpha, b = 1.0 - (double)alpha;
  if (tid == 0 && loss_rows) loss_rows[n] = (float)(b * (double)hard_loss + a * kd);
  if (dlogits) {
    for (int j = tid; j < M; j += 256) {
      const float p = expf(z[j] - mx) * inv;
      const bool in = (p >= 1e-7f && p <= 1.f - 1e-7f);
      float gh;   // d hard / dz_j, as above without grad_scale
      if (SOFT) {
        const float q = fminf(fmaxf(p, 1e-7f), 1.f - 1e-7f);
        const float dldp = in ? S / sumq - y[j] / q : 0.f;
        gh = p * (dldp - inner);
      } else {
        float dldp = in ? 1.f / sumq : 0.f;
        if (j == label && in) dldp -= 1.f / qy;
        gh = p * (dldp - inner);
      }
      const double ps = exp((double)z[j] / T - lse_u), pt = exp((double)t[j] / T - lse_v);
      dlogits[(long long)n * M + j] = (float)((double)grad_scale * (b * (double)gh + a * T * (ps - pt)));
    }
  }
}

// ------------------------------------------------------------------------------------------------
// sigmoid head: the hard term of sigmoid_bce_kernel, the Bernoulli KL per class against sigmoid(t / T)
// ------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(KD_THREADS) void sigmoid_bce_kd_kernel(const float* __restrict__ logits,
                                                                    const float* __restrict__ teacher,
                                                                    const float* __restrict__ targets, float* probs,
                                                                    float* loss_rows, float* kd_rows, float* dlogits,
                                                                    float grad_scale, float alpha, float temperature, int M) {
  __shared__ double part[KD_WAVES];
  const int n = blockIdx.x, tid = threadIdx.x;
  const long long row = (long long)n * M;
  const double gs = (double)grad_scale / (double)M;
  if (alpha == 0.f) {
    // ---- no distillation: sigmoid_bce_kernel, the teacher is not read ----
    double acc = 0.0;
    for (int j = tid; j < M; j += KD_THREADS) {
      const double z = (double)logits[row + j];
      const double p = kd_sigmoid_d(z);      // NaN in, NaN out
      probs[row + j] = (float)p;
      const double y = (double)targets[row + j];
      // max(z, 0) written as a select: NaN must not become 0 (the -z*y and log1p terms carry it anyway)
      acc += (z > 0.0 ? z : 0.0) - z * y + log1p(exp(-fabs(z)));
      if (dlogits) dlogits[row + j] = (float)(gs * (p - y));
    }
    if (tid == 0 && kd_rows) kd_rows[n] = 0.f;
    if (!loss_rows) return;
    acc = wave_sum_d(acc);
    if ((tid & 63) == 0) part[tid >> 6] = acc;
    __syncthreads();
    if (tid == 0) {
      double s = 0.0;
      for (int w = 0; w < KD_WAVES; w++) s += part[w];
      loss_rows[n] = (float)(s / (double)M);
    }
    return;
  }
  const double T = (double)temperature;
  double acc = 0.0, kacc = 0.0, bad = 0.0;
  for (int j = tid; j < M; j += KD_THREADS) {
    const double z = (double)logits[row + j];
    const double p = kd_sigmoid_d(z);
    probs[row + j] = (float)p;
    const double y = (double)targets[row + j];
    acc += (z > 0.0 ? z : 0.0) - z * y + log1p(exp(-fabs(z)));
    const float tj = teacher[row + j];
    if (kd_nonfinite(tj)) { bad = 1.0; continue; }
    const double u = z / T, v = (double)tj / T, sv = kd_sigmoid_d(v);
    kacc += (kd_softplus_d(u) - sv * u) - (kd_softplus_d(v) - sv * v);
  }
  const bool kd_bad = kd_block_max_d(bad, part) > 0.0;
  const double hard = kd_block_sum_d(acc, part) / (double)M;
  const double kd = kd_bad ? (double)__builtin_nanf("") : T * T * kd_block_sum_d(kacc, part) / (double)M;
  const double a = (double)alpha, b = 1.0 - (double)alpha;
  if (tid == 0) {
    if (kd_rows) kd_rows[n] = (float)kd;
    if (loss_rows) loss_rows[n] = (float)(b * hard + a * kd);     // (NaN with a non-finite teacher logit)
  }
  if (!dlogits) return;
  for (int j = tid; j < M; j += KD_THREADS) {
    if (kd_bad) { dlogits[row + j] = 0.f; continue; }
    const double z = (double)logits[row + j], y = (double)targets[row + j];
    const double p = kd_sigmoid_d(z);
    const double su = kd_sigmoid_d(z / T), sv = kd_sigmoid_d((double)teacher[row + j] / T);
    dlogits[row + j] = (float)(gs * (b * (p - y) + a * T * (su - sv)));
  }
}

// do the byte ranges [a, a + na) and [b, b + nb) share a byte?  (a null pointer overlaps nothing)
static bool kd_overlap(const void* a, size_t na, const void* b, size_t nb) {
  if (!a || !b) return false;
  const uintptr_t x = (uintptr_t)a, y = (uintptr_t)b;
  return x < y + nb && y < x + na;
}

// the checks both entry points share; `in` / `in_name`: a matrix input that must not alias an output
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
    hipLaunchKernelGGL(softmax_xent_kd_kernel<true>, dim3(N), dim3(KD_THREADS), 0, (hipStream_t)stream, logits, teacher_logits,
                       labels, targets, probs, loss_rows, kd_rows, dlogits, grad_scale, alpha, temperature, M);
  else
    hipLaunchKernelGGL(softmax_xent_kd_kernel<false>, dim3(N), dim3(KD_THREADS), 0, (hipStream_t)stream, logits, teacher_logits,
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
  hipLaunchKernelGGL(sigmoid_bce_kd_kernel, dim3(N), dim3(KD_THREADS), 0, (hipStream_t)stream, logits, teacher_logits, targets,
                     probs, loss_rows, kd_rows, dlogits, grad_scale, alpha, temperature, M);
  X3D_LAUNCH_CHECK("sigmoid_bce_kd");
  return X3D_OK;
}
