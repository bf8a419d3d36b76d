// Frame-mAP for action detection (AVA): the matching of a validation batch's proposals against the annotated boxes and the
// PASCAL VOC average precision over a whole evaluation set.  The exact rules are in include/x3d_hip.h.  (The row-wise
// multi-label AP of the classification models: multilabel.hip.)
#include "common.h"

#define FM_THREADS 256
#define FM_WAVES (FM_THREADS / WAVE)
#define FM_MAX_BOXES 64          // K and G: one lane per detection, one ballot bit per ground-truth box

// the ROI head's "treated as empty" rule, negated (a slot index below the count is checked by the caller)
__device__ __forceinline__ bool fm_box_ok(const float* b) {
  return isfinite(b[0]) && isfinite(b[1]) && isfinite(b[2]) && isfinite(b[3]) && b[2] > b[0] && b[3] > b[1];
}

// IoU in IEEE double, every operation rounded on its own: hipcc would otherwise contract iw * ih and the two areas into the
// subtractions that follow.  The division is the correctly rounded one (no fast-math flag in the build).
__device__ __forceinline__ double fm_iou(const float* a, const float* b) {
#pragma clang fp contract(off)
  const double ax1 = a[0], ay1 = a[1], ax2 = a[2], ay2 = a[3], bx1 = b[0], by1 = b[1], bx2 = b[2], by2 = b[3];
  const double dw = (ax2 < bx2 ? ax2 : bx2) - (ax1 > bx1 ? ax1 : bx1);
  const double dh = (ay2 < by2 ? ay2 : by2) - (ay1 > by1 ? ay1 : by1);
  const double iw = dw > 0.0 ? dw : 0.0, ih = dh > 0.0 ? dh : 0.0;
  const double inter = iw * ih;
  const double ua = (ax2 - ax1) * (ay2 - ay1);
  const double ub = (bx2 - bx1) * (by2 - by1);
  const double uni = ua + ub - inter;
  return inter / uni;
}

// ------------------------------------------------------------------------------------------------
// One workgroup per image.  The K x G IoU table does not depend on the class: it is computed once into LDS, [g][k] so that
// the lanes of a wave (lane k = detection k) read consecutive doubles.  Then one wave per class, striding over C:
//   gm    = ballot of "box g is valid and carries c"                    (ngt[c] += popcount, one integer atomic)
//   g*(k) = arg-max over the set bits of gm, ascending, strict >        (the lowest g among equals)
//   cand  = valid, score not NaN, iou(k, g*) >= threshold
//   tp    = cand and no candidate j with g*(j) == g*(k) that comes before k in (score descending, slot ascending) order
// -- a detection is a true positive iff it is the FIRST candidate for its box, so there is no sort and no serial greedy
// pass: one K-step loop over lane broadcasts.
// LDS: 64 * 64 doubles (32 KiB) + the two box tiles (2 KiB).
// ------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(FM_THREADS) void frame_match_kernel(const float* __restrict__ scores,
                                                                  const float* __restrict__ boxes,
                                                                  const int* __restrict__ num_boxes,
                                                                  const float* __restrict__ gt_boxes,
                                                                  const unsigned char* __restrict__ gt_labels,
                                                                  const int* __restrict__ num_gt, int K, int G, int C,
                                                                  double thr, unsigned char* tp, float* det_scores, int* ngt) {
  __shared__ double iou[FM_MAX_BOXES * FM_MAX_BOXES];
  __shared__ float dbox[FM_MAX_BOXES][4], gbox[FM_MAX_BOXES][4];
  __shared__ unsigned long long s_valid[2];
  const int i = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;

  if (wid < 2) {   // wave 0: the proposals, wave 1: the ground-truth boxes
    const int n = wid == 0 ? K : G;
    const float* src = (wid == 0 ? boxes : gt_boxes) + ((long long)i * n + lane) * 4;
    float(*dst)[4] = wid == 0 ? dbox : gbox;
    const int filled = wid == 0 ? num_boxes[i] : num_gt[i];
    bool ok = false;
    if (lane < n) {
      float b[4];
#pragma unroll
      for (int e = 0; e < 4; e++) { b[e] = src[e]; dst[lane][e] = b[e]; }
      ok = lane < filled && fm_box_ok(b);
    }
    const unsigned long long mask = __ballot(ok);
    if (lane == 0) s_valid[wid] = mask;
  }
  __syncthreads();
  const unsigned long long dmask = s_valid[0], gmask = s_valid[1];
  for (int p = tid; p < G * K; p += FM_THREADS) {
    const int g = p / K, k = p - g * K;
    iou[p] = ((dmask >> k) & 1) && ((gmask >> g) & 1) ? fm_iou(dbox[k], gbox[g]) : 0.0;
  }
  __syncthreads();

  const bool valid = lane < K && ((dmask >> lane) & 1);
  const long long row = (long long)i * K + lane;
  for (int c = wid; c < C; c += FM_WAVES) {
    bool carries = false;
    if (lane < G && ((gmask >> lane) & 1)) carries = gt_labels[((long long)i * G + lane) * C + c] != 0;
    const unsigned long long gm = __ballot(carries);
    if (lane == 0 && gm) atomicAdd(&ngt[c], __popcll(gm));
    float s = -INFINITY;                 // what an empty or invalid slot holds is never read
    if (valid) s = scores[row * C + c];
    double best = -1.0;
    int bi = -1;
    for (unsigned long long m = gm; m; m &= m - 1) {   // gm is wave-uniform: no divergence
      const int g = __builtin_ctzll(m);
      if (lane < K) {
        const double v = iou[g * K + lane];
        if (v > best) { best = v; bi = g; }
      }
    }
    const bool cand = valid && s == s && bi >= 0 && best >= thr;
    const unsigned long long cm = __ballot(cand);
    bool first = cand;
    if (cm) {
      for (int j = 0; j < K; j++) {
        const float sj = __shfl(s, j, 64);
        const int bj = __shfl(bi, j, 64);
        if (((cm >> j) & 1) && bj == bi && (sj > s || (sj == s && j < lane))) first = false;
      }
    }
    if (lane < K) {
      tp[row * C + c] = first ? 1 : 0;
      det_scores[row * C + c] = s;
    }
  }
}

extern "C" int x3d_frame_match(const float* scores, const float* boxes, const int* num_boxes, const float* gt_boxes,
                               const unsigned char* gt_labels, const int* num_gt, int I, int K, int G, int C,
                               double iou_threshold, unsigned char* tp, float* det_scores, int* ngt, void* stream) {
  X3D_REQUIRE(scores, "frame_match: scores is null");
  X3D_REQUIRE(boxes, "frame_match: boxes is null");
  X3D_REQUIRE(num_boxes, "frame_match: num_boxes is null");
  X3D_REQUIRE(gt_boxes, "frame_match: gt_boxes is null");
  X3D_REQUIRE(gt_labels, "frame_match: gt_labels is null");
  X3D_REQUIRE(num_gt, "frame_match: num_gt is null");
  X3D_REQUIRE(tp, "frame_match: tp is null");
  X3D_REQUIRE(det_scores, "frame_match: det_scores is null");
  X3D_REQUIRE(ngt, "frame_match: ngt is null");
  X3D_REQUIRE(I >= 1, "frame_match: I = %d must be >= 1", I);
  X3D_REQUIRE(K >= 1 && K <= FM_MAX_BOXES, "frame_match: K = %d must be in 1..%d", K, FM_MAX_BOXES);
  X3D_REQUIRE(G >= 1 && G <= FM_MAX_BOXES, "frame_match: G = %d must be in 1..%d", G, FM_MAX_BOXES);
  X3D_REQUIRE(C >= 1, "frame_match: C = %d must be >= 1", C);
  X3D_REQUIRE((long long)I * K * C < (1LL << 31), "frame_match: I*K*C = %lld >= 2^31", (long long)I * K * C);
  X3D_REQUIRE(iou_threshold > 0.0 && iou_threshold <= 1.0, "frame_match: iou_threshold = %g must be in (0, 1]",
              iou_threshold);   // (false for NaN)
  hipLaunchKernelGGL(frame_match_kernel, dim3(I), dim3(FM_THREADS), 0, (hipStream_t)stream, scores, boxes, num_boxes,
                     gt_boxes, gt_labels, num_gt, K, G, C, iou_threshold, tp, det_scores, ngt);
  X3D_LAUNCH_CHECK("frame_match");
  return X3D_OK;
}

// ------------------------------------------------------------------------------------------------
// VOC average precision.  One workgroup of 1024 threads per class; thread t owns the sorted positions [t*L, (t+1)*L),
// L = ceil(N / 1024).  The true-positive flags are streamed from memory through `order` -- nothing per row is kept in LDS,
// so there is no cap on rows or true positives per class:
//   pass 1  the true positives of the run, block exclusive scan: every true positive knows its t
//   pass 2  the run's largest prec_t = t / pos_t, block suffix max: what lies behind the run
//   pass 3  the run backwards, carrying the running maximum: sum of env_t in double
// The thread sums are added in a fixed order (xor butterfly in the wave, then the 16 waves in order).
// ------------------------------------------------------------------------------------------------
#define FA_THREADS 1024
#define FA_WAVES (FA_THREADS / WAVE)

__device__ __forceinline__ int fa_flag(const unsigned char* __restrict__ tp, const long long* __restrict__ order, long long p,
                                       int N, int C, int c) {
  const unsigned long long r = (unsigned long long)order[p * C + c];
  return r < (unsigned long long)N ? (tp[r * C + c] != 0) : 0;   // an index outside the set is never followed
}

__global__ __launch_bounds__(FA_THREADS) void frame_ap_kernel(const unsigned char* __restrict__ tp,
                                                               const float* __restrict__ det_scores,
                                                               const long long* __restrict__ order,
                                                               const int* __restrict__ ngt, int N, int C, double* ap,
                                                               int* ntp) {
  __shared__ int wave_cnt[FA_WAVES];
  __shared__ double wave_d[FA_WAVES];
  const int c = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
  const long long L = ((long long)N + FA_THREADS - 1) / FA_THREADS;
  const long long lo = min((long long)N, tid * L), hi = min((long long)N, lo + L);

  // pass 1
  int cnt = 0;
#pragma unroll 4
  for (long long p = lo; p < hi; p++) cnt += fa_flag(tp, order, p, N, C, c);
  int inc = cnt;
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) {
    const int v = __shfl_up(inc, o, 64);
    if (lane >= o) inc += v;
  }
  if (lane == 63) wave_cnt[wid] = inc;
  __syncthreads();
  int base = inc - cnt, P = 0;
  for (int w = 0; w < FA_WAVES; w++) {
    if (w < wid) base += wave_cnt[w];
    P += wave_cnt[w];
  }

  // pass 2
  double rmax = 0.0;
  int t = base;
#pragma unroll 4
  for (long long p = lo; p < hi; p++) {
    if (fa_flag(tp, order, p, N, C, c)) {
      ++t;
      rmax = fmax(rmax, (double)t / (double)(p + 1));
    }
  }
  double suf = rmax;   // max over this lane and the lanes after it
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) {
    const double v = __shfl_down(suf, o, 64);
    if (lane + o < 64) suf = fmax(suf, v);
  }
  const double next = __shfl_down(suf, 1, 64);
  double behind = lane < 63 ? next : 0.0;
  if (lane == 0) wave_d[wid] = suf;
  __syncthreads();
  for (int w = wid + 1; w < FA_WAVES; w++) behind = fmax(behind, wave_d[w]);

  // pass 3 (t = base + cnt: the run's last true positive)
  double sum = 0.0, env = behind;
#pragma unroll 4
  for (long long p = hi - 1; p >= lo; p--) {
    if (fa_flag(tp, order, p, N, C, c)) {
      env = fmax(env, (double)t / (double)(p + 1));
      sum += env;
      --t;
    }
  }
  sum = wave_sum_d(sum);
  __syncthreads();   // wave_d is reused
  if (lane == 0) wave_d[wid] = sum;
  __syncthreads();
  if (tid == 0) {
    double total = 0.0;
    for (int w = 0; w < FA_WAVES; w++) total += wave_d[w];
    const int g = ngt[c];
    // a descending sort puts NaN first: one look at the class's first row
    const unsigned long long r0 = (unsigned long long)order[c];
    const bool has_nan = r0 < (unsigned long long)N && det_scores[r0 * C + c] != det_scores[r0 * C + c];
    ap[c] = (g <= 0 || has_nan) ? __builtin_nan("") : total / (double)g;
    ntp[c] = P;
  }
}

extern "C" int x3d_frame_ap(const unsigned char* tp, const float* det_scores, const long long* order, const int* ngt, int N,
                            int C, double* ap, int* ntp, void* stream) {
  X3D_REQUIRE(tp, "frame_ap: tp is null");
  X3D_REQUIRE(det_scores, "frame_ap: det_scores is null");
  X3D_REQUIRE(order, "frame_ap: order is null");
  X3D_REQUIRE(ngt, "frame_ap: ngt is null");
  X3D_REQUIRE(ap, "frame_ap: ap is null");
  X3D_REQUIRE(ntp, "frame_ap: ntp is null");
  X3D_REQUIRE(N >= 1, "frame_ap: N = %d must be >= 1", N);
  X3D_REQUIRE(C >= 1, "frame_ap: C = %d must be >= 1", C);
  X3D_REQUIRE((long long)N * C < (1LL << 31), "frame_ap: N*C = %lld >= 2^31", (long long)N * C);
  hipLaunchKernelGGL(frame_ap_kernel, dim3(C), dim3(FA_THREADS), 0, (hipStream_t)stream, tp, det_scores, order, ngt, N, C,
                     ap, ntp);
  X3D_LAUNCH_CHECK("frame_ap");
  return X3D_OK;
}
