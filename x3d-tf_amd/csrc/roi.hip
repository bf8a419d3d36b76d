// ROI head for action detection on conv5's output (include/x3d_hip.h, "K7r"): temporal mean of relu(bn5(conv5)), ROIAlign
// (aligned, border clamp) and a spatial max per box, forward and backward.  The two launches take the places of x3d_pool_fwd and
// of x3d_relu_bn_bwd_reduce in its dpool form and keep their contracts: pooled rows in, g5 and the BatchNorm-backward sums out.
//
// One workgroup per (n, c) plane, as pool_fwd_kernel: the plane is streamed once with VecIO, the per-pixel work is done by the
// thread that owns the pixel (so every sum has one fixed order and no LDS atomics exist), the per-box work by one wave per box.
// The box geometry -- the same for every channel -- is worked out in fp64: a sample coordinate near 32 carries 2^-19 of fp32
// rounding per operation, more than the whole fp32 budget of a bin of few samples, and ceil(roi / R) must not depend on the last
// bit of a quotient.  It is a dozen fp64 operations per sample row / column next to the four fp32 products of every sample.
#include "common.h"
#include <type_traits>

#define ROI_BLOCK 256
#define ROI_WAVES (ROI_BLOCK / 64)
#define ROI_MAX_HW 1024                           // a thread owns at most ROI_PIX pixels
#define ROI_PIX (ROI_MAX_HW / ROI_BLOCK)
#define ROI_STAGE 8192                            // floats of the forward's staging chunk: 8 time slices of the largest plane

struct RoiBox {
  bool valid;
  double x1, y1, bin_w, bin_h;
  int gh, gw;
};

// slot k of sample n: scaled by spatial_scale, clamped to the frame; empty slots, empty boxes and non-finite coordinates are invalid
__device__ __forceinline__ RoiBox roi_box(const float* __restrict__ b, bool filled, float spatial_scale, int H, int W, int R,
                                          int sampling_ratio) {
  RoiBox o;
  o.valid = false;
  o.x1 = o.y1 = o.bin_w = o.bin_h = 0.0;
  o.gh = o.gw = 1;
  if (!filled) return o;
  const float bx1 = b[0], by1 = b[1], bx2 = b[2], by2 = b[3];
  if (!(isfinite(bx1) && isfinite(by1) && isfinite(bx2) && isfinite(by2))) return o;
  const double sc = (double)spatial_scale;
  const double x1 = fmin(fmax((double)bx1 * sc, 0.0), (double)W), x2 = fmin(fmax((double)bx2 * sc, 0.0), (double)W);
  const double y1 = fmin(fmax((double)by1 * sc, 0.0), (double)H), y2 = fmin(fmax((double)by2 * sc, 0.0), (double)H);
  if (!(x2 > x1 && y2 > y1)) return o;
  o.valid = true;
  o.x1 = x1;
  o.y1 = y1;
  o.bin_w = (x2 - x1) / (double)R;
  o.bin_h = (y2 - y1) / (double)R;
  // (0 < roi <= W, H <= 1024: the counts are in [1, 1024])
  o.gw = sampling_ratio > 0 ? sampling_ratio : max(1, (int)ceil(o.bin_w));
  o.gh = sampling_ratio > 0 ? sampling_ratio : max(1, (int)ceil(o.bin_h));
  return o;
}

// sample i of g in bin p along an axis of L pixels: the two pixels it reads and their bilinear weights.  Border clamp; lo and hi are
// inside [0, L-1] whatever the coordinate is
__device__ __forceinline__ void roi_axis(double start, double bin, int p, int i, int g, int L, int& lo, int& hi, float& w_lo,
                                         float& w_hi) {
  double y = start - 0.5 + (double)p * bin + ((double)i + 0.5) * bin / (double)g;
  if (!(y > 0.0)) y = 0.0;
  lo = (int)y;
  if (lo >= L - 1) {
    lo = hi = L - 1;
    y = (double)(L - 1);
  } else {
    hi = lo + 1;
  }
  w_hi = (float)(y - (double)lo);     // weight of pixel hi
  w_lo = 1.f - w_hi;
}

// mean of the gh x gw bilinear samples of bin (ph, pw) of the fp32 map m [H][W]
__device__ __forceinline__ float roi_bin_mean(const float* m, const RoiBox& bx, int ph, int pw, int H, int W) {
  float acc = 0.f;
  for (int iy = 0; iy < bx.gh; iy++) {
    int yl, yh;
    float wyl, wyh;
    roi_axis(bx.y1, bx.bin_h, ph, iy, bx.gh, H, yl, yh, wyl, wyh);
    const float* r0 = m + yl * W;
    const float* r1 = m + yh * W;
    for (int ix = 0; ix < bx.gw; ix++) {
      int xl, xh;
      float wxl, wxh;
      roi_axis(bx.x1, bx.bin_w, pw, ix, bx.gw, W, xl, xh, wxl, wxh);
      acc += wyl * wxl * r0[xl] + wyl * wxh * r0[xh] + wyh * wxl * r1[xl] + wyh * wxh * r1[xh];
    }
  }
  return acc / (float)(bx.gh * bx.gw);
}

// (value, bin) of the first maximal bin among the lanes of a wave: the larger value wins, the lower bin on a tie
__device__ __forceinline__ void wave_first_max(float& v, int& b) {
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) {
    const float ov = __shfl_xor(v, o, 64);
    const int ob = __shfl_xor(b, o, 64);
    if (ov > v || (ov == v && ob < b)) { v = ov; b = ob; }
  }
}

template <typename T, int VEC>
__global__ __launch_bounds__(ROI_BLOCK) void roi_pool_fwd_kernel(const T* __restrict__ x, const float* __restrict__ ss,
                                                                 const float* __restrict__ boxes, const int* __restrict__ num_boxes,
                                                                 float* pooled, unsigned char* argmax, int C, int Tn, int H, int W,
                                                                 int K, int R, int sampling_ratio, float spatial_scale, int tc) {
  extern __shared__ float lds[];                 // map [H*W rounded up to 4] | stage [min(tc, T) * H*W]
  const int HW = H * W;
  float* map = lds;
  float* stage = lds + ((HW + 3) & ~3);
  const int nc = blockIdx.x, n = nc / C, c = nc - n * C;
  const int nb = min(max(num_boxes[n], 0), K);
  const long long row0 = (long long)n * K;
  if (nb == 0) {                                 // a sample without boxes: its plane is not read
    for (int k = threadIdx.x; k < K; k += ROI_BLOCK) {
      pooled[(row0 + k) * C + c] = 0.f;
      if (argmax) argmax[(row0 + k) * C + c] = 0;
    }
    return;
  }
  const float s = ss[c * 2], t = ss[c * 2 + 1];
  const T* xp = x + (long long)nc * Tn * HW;
  float acc[ROI_PIX];
#pragma unroll
  for (int j = 0; j < ROI_PIX; j++) acc[j] = 0.f;
  for (int t0 = 0; t0 < Tn; t0 += tc) {
    const int cnt = min(tc, Tn - t0), elems = cnt * HW;       // elems % VEC == 0 (the launcher's choice of tc)
    const T* xc = xp + (long long)t0 * HW;
    for (int i = threadIdx.x * VEC; i < elems; i += ROI_BLOCK * VEC) {
      float v[VEC];
      VecIO<T, VEC>::load(xc + i, v);
#pragma unroll
      for (int e = 0; e < VEC; e++) stage[i + e] = fmaxf(s * v[e] + t, 0.f);
    }
    __syncthreads();
#pragma unroll
    for (int j = 0; j < ROI_PIX; j++) {
      const int hw = threadIdx.x + j * ROI_BLOCK;
      if (hw < HW)
        for (int tt = 0; tt < cnt; tt++) acc[j] += stage[tt * HW + hw];      // time in order: one fixed sum per pixel
    }
    __syncthreads();
  }
#pragma unroll
  for (int j = 0; j < ROI_PIX; j++) {
    const int hw = threadIdx.x + j * ROI_BLOCK;
    if (hw < HW) map[hw] = acc[j] / (float)Tn;
  }
  __syncthreads();
  // one wave per box, its lanes over the R*R bins
  const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
  for (int k = wid; k < K; k += ROI_WAVES) {
    const RoiBox bx = roi_box(boxes + (row0 + k) * 4, k < nb, spatial_scale, H, W, R, sampling_ratio);
    float best = -INFINITY;
    int arg = 0x7fffffff;
    if (bx.valid) {
      for (int b = lane; b < R * R; b += 64) {
        const int ph = b / R;
        const float v = roi_bin_mean(map, bx, ph, b - ph * R, H, W);
        if (v > best) { best = v; arg = b; }                  // ascending b: the first maximal bin of the lane
      }
      wave_first_max(best, arg);
      if (arg == 0x7fffffff) { best = NAN; arg = 0; }         // every bin NaN: the input was
    } else {
      best = 0.f;
      arg = 0;
    }
    if (lane == 0) {
      pooled[(row0 + k) * C + c] = best;
      if (argmax) argmax[(row0 + k) * C + c] = (unsigned char)arg;
    }
  }
}

template <typename T, int VEC>
__global__ __launch_bounds__(ROI_BLOCK) void roi_pool_bwd_kernel(const float* __restrict__ dpooled,
                                                                 const unsigned char* __restrict__ argmax,
                                                                 const float* __restrict__ boxes, const int* __restrict__ num_boxes,
                                                                 const T* __restrict__ yraw, const float* __restrict__ ss, T* g,
                                                                 double* sums, int C, int Tn, int H, int W, int K, int R,
                                                                 int sampling_ratio, float spatial_scale) {
  extern __shared__ float lds[];                 // dm [H*W rounded up to 4] | wts [ROI_WAVES][H + W] | coef [ROI_WAVES] | scratch [2 * ROI_WAVES]
  const int HW = H * W;
  float* dm = lds;
  float* wts = lds + ((HW + 3) & ~3);
  float* coef = wts + ROI_WAVES * (H + W);
  float* scratch = coef + ROI_WAVES;
  const int nc = blockIdx.x, n = nc / C, c = nc - n * C;
  const int nb = min(max(num_boxes[n], 0), K);
  const long long row0 = (long long)n * K;
  const int P = Tn * HW;                         // (the launcher refuses planes past 2^31 elements)
  T* gp = g + (long long)nc * P;
  if (nb == 0) {                                 // no boxes: g = 0, nothing to add to the sums, yraw is not read
    float z[VEC];
#pragma unroll
    for (int e = 0; e < VEC; e++) z[e] = 0.f;
    for (int p = threadIdx.x * VEC; p < P; p += ROI_BLOCK * VEC) VecIO<T, VEC>::store(gp + p, z);
    return;
  }
  const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
  // dM / T of the pixels this thread owns: the boxes in order, four at a time -- wave w writes the row and column weight sums of box
  // k0 + w (the bilinear weights are separable: sum over the bin's samples of wy * wx = (sum wy) * (sum wx)), then every thread
  // adds the four boxes to its pixels in order
  float acc[ROI_PIX];
#pragma unroll
  for (int j = 0; j < ROI_PIX; j++) acc[j] = 0.f;
  for (int k0 = 0; k0 < nb; k0 += ROI_WAVES) {
    const int k = k0 + wid;
    const RoiBox bx = roi_box(boxes + (row0 + min(k, K - 1)) * 4, k < nb, spatial_scale, H, W, R, sampling_ratio);
    const int a = bx.valid ? argmax[(row0 + k) * C + c] : 0;
    const bool use = bx.valid && a < R * R;
    if (use) {
      const int ph = a / R, pw = a - ph * R;
      float* wy = wts + wid * (H + W);
      for (int i = lane; i < H + W; i += 64) {
        const bool row = i < H;
        const int px = row ? i : i - H, cnt = row ? bx.gh : bx.gw;
        float wsum = 0.f;
        for (int q = 0; q < cnt; q++) {
          int lo, hi;
          float wl, wh;
          if (row) roi_axis(bx.y1, bx.bin_h, ph, q, bx.gh, H, lo, hi, wl, wh);
          else roi_axis(bx.x1, bx.bin_w, pw, q, bx.gw, W, lo, hi, wl, wh);
          if (lo == px) wsum += wl;
          if (hi == px) wsum += wh;
        }
        wy[i] = wsum;
      }
    }
    // (the mean over time is folded in: one division, as relu_bn_bwd_reduce_kernel's dpool / P, which this is for a full-frame box)
    if (lane == 0) coef[wid] = use ? dpooled[(row0 + k) * C + c] / (float)((long long)bx.gh * bx.gw * Tn) : 0.f;
    __syncthreads();
#pragma unroll
    for (int j = 0; j < ROI_PIX; j++) {
      const int hw = threadIdx.x + j * ROI_BLOCK;
      if (hw < HW) {
        const int h = hw / W, w = hw - h * W;
        for (int q = 0; q < ROI_WAVES; q++) {
          const float cf = coef[q];
          if (cf != 0.f) acc[j] += cf * (wts[q * (H + W) + h] * wts[q * (H + W) + H + w]);   // (0: an unused slot, its weights unset)
        }
      }
    }
    __syncthreads();
  }
#pragma unroll
  for (int j = 0; j < ROI_PIX; j++) {
    const int hw = threadIdx.x + j * ROI_BLOCK;
    if (hw < HW) dm[hw] = acc[j];
  }
  __syncthreads();
  // the one pass over yraw of relu_bn_bwd_reduce_kernel
  const float s = ss[c * 2], t = ss[c * 2 + 1];
  const T* yp = yraw + (long long)nc * P;
  float red[2] = {0.f, 0.f};
  for (int p = threadIdx.x * VEC; p < P; p += ROI_BLOCK * VEC) {
    float yr[VEC], o[VEC];
    VecIO<T, VEC>::load(yp + p, yr);
    int hw = p % HW;
#pragma unroll
    for (int e = 0; e < VEC; e++) {
      o[e] = (s * yr[e] + t > 0.f) ? dm[hw] : 0.f;
      const float gr = round_to<T>(o[e]);
      red[0] += gr;
      red[1] += gr * yr[e];
      if (++hw == HW) hw = 0;
    }
    VecIO<T, VEC>::store(gp + p, o);
  }
  block_sum<2>(red, scratch);
  if (threadIdx.x == 0) {
    atomic_add_d(&sums[c * 2], (double)red[0]);
    atomic_add_d(&sums[c * 2 + 1], (double)red[1]);
  }
}

// the limits both entry points share; every one is checked before any launch
#define ROI_REQUIRE_SHAPE(name)                                                                                            \
  do {                                                                                                                     \
    X3D_REQUIRE(N > 0 && C > 0 && T > 0 && H > 0 && W > 0, name ": bad args (N, C, T, H, W must be positive)");           \
    X3D_REQUIRE((long long)H * W <= ROI_MAX_HW, name ": H*W = %lld, at most %d", (long long)H * W, ROI_MAX_HW);            \
    X3D_REQUIRE(R >= 1 && R <= 15, name ": R = %d, must be in 1..15", R);                                                  \
    X3D_REQUIRE(K >= 1 && K <= 64, name ": K = %d, must be in 1..64", K);                                                  \
    X3D_REQUIRE((long long)N * K <= 2048, name ": N*K = %lld, at most 2048 rows", (long long)N * K);                       \
    X3D_REQUIRE(sampling_ratio >= 0, name ": sampling_ratio = %d, must be >= 0", sampling_ratio);                          \
    X3D_REQUIRE(spatial_scale > 0.f && spatial_scale <= 3.0e38f, name ": spatial_scale must be positive and finite");      \
    X3D_REQUIRE((long long)N * C <= 0x7fffffffLL && (long long)T * H * W < 0x7fff0000LL, name ": N*C or T*H*W too large");                                               \
    X3D_REQUIRE(x3d_dtype_ok(dtype), name ": bad dtype");                                                                  \
  } while (0)

// fn(T(), integral_constant<VEC>) for the storage type and the full 16-byte vector or scalars
template <typename F>
static inline void roi_dispatch(int dtype, bool full, F&& fn) {
  if (dtype == X3D_F32) {
    if (full) fn(float(), std::integral_constant<int, 4>()); else fn(float(), std::integral_constant<int, 1>());
  } else if (dtype == X3D_F16) {
    if (full) fn(f16(), std::integral_constant<int, 8>()); else fn(f16(), std::integral_constant<int, 1>());
  } else {
    if (full) fn(bf16(), std::integral_constant<int, 8>()); else fn(bf16(), std::integral_constant<int, 1>());
  }
}

static inline int roi_gcd(int a, int b) { return b ? roi_gcd(b, a % b) : a; }

extern "C" int x3d_roi_pool_fwd(const void* x_raw, const float* scale_shift, const float* boxes, const int* num_boxes,
                                float* pooled, unsigned char* argmax, int N, int C, int T, int H, int W, int K, int R,
                                int sampling_ratio, float spatial_scale, int dtype, void* stream) {
  X3D_REQUIRE(x_raw && scale_shift && boxes && num_boxes && pooled, "roi_pool_fwd: bad args (NULL pointer)");
  ROI_REQUIRE_SHAPE("roi_pool_fwd");
  const int HW = H * W, full = dtype == X3D_F32 ? 4 : 8;
  const bool vec = pick_vec(dtype == X3D_F32 ? 4 : 2, (long long)T * HW, x_raw) >= full;
  // time slices per staging chunk: a multiple of q, so that every chunk starts and ends on a vector (q <= 8 slices always fit)
  const int q = vec ? full / roi_gcd(HW, full) : 1;
  int tc = ROI_STAGE / HW / q * q;
  if (tc < q) tc = q;
  if (tc > T) tc = T;
  const size_t lds = (size_t)(((HW + 3) & ~3) + tc * HW) * sizeof(float);
  roi_dispatch(dtype, vec, [&](auto t, auto v) {
    typedef decltype(t) TT;
    hipLaunchKernelGGL((roi_pool_fwd_kernel<TT, decltype(v)::value>), dim3((unsigned)(N * C)), dim3(ROI_BLOCK), lds, (hipStream_t)stream,
                       (const TT*)x_raw, scale_shift, boxes, num_boxes, pooled, argmax, C, T, H, W, K, R, sampling_ratio,
                       spatial_scale, tc);
  });
  X3D_LAUNCH_CHECK("roi_pool_fwd");
  return X3D_OK;
}

extern "C" int x3d_roi_pool_bwd(const float* dpooled, const unsigned char* argmax, const float* boxes, const int* num_boxes,
                                const void* yraw, const float* scale_shift, void* g, double* sums, int N, int C, int T, int H,
                                int W, int K, int R, int sampling_ratio, float spatial_scale, int dtype, void* stream) {
  X3D_REQUIRE(dpooled && argmax && boxes && num_boxes && yraw && scale_shift && g && sums, "roi_pool_bwd: bad args (NULL pointer)");
  ROI_REQUIRE_SHAPE("roi_pool_bwd");
  const int HW = H * W, full = dtype == X3D_F32 ? 4 : 8;
  const bool vec = pick_vec(dtype == X3D_F32 ? 4 : 2, (long long)T * HW, yraw, g) >= full;
  const size_t lds = (size_t)(((HW + 3) & ~3) + ROI_WAVES * (H + W) + ROI_WAVES + 2 * ROI_WAVES) * sizeof(float);
  roi_dispatch(dtype, vec, [&](auto t, auto v) {
    typedef decltype(t) TT;
    hipLaunchKernelGGL((roi_pool_bwd_kernel<TT, decltype(v)::value>), dim3((unsigned)(N * C)), dim3(ROI_BLOCK), lds, (hipStream_t)stream,
                       dpooled, argmax, boxes, num_boxes, (const TT*)yraw, scale_shift, (TT*)g, sums, C, T, H, W, K, R,
                       sampling_ratio, spatial_scale);
  });
  X3D_LAUNCH_CHECK("roi_pool_bwd");
  return X3D_OK;
}
