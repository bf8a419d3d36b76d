// x3d_train_clips_aug: the batched training augmentation (AUG.* of the config, x3d_tf_amd/aug.py).  N decoded videos of
// different extents -> the clip batch [N][T][size][size][3], geometry ("jitter": x3d_train_clip's arithmetic, bit for bit;
// "rrc": a random-resized crop), mirror, folded colour chain, normalisation and random erasing in one pass over the output.
// The exact rules are in include/x3d_hip.h.
//
// Shape.  A gather (4 taps x 3 bytes per pixel; neighbouring outputs share taps, so most of them should come from the caches --
// expected from the access pattern, not measured) and a streaming write
// (headline batch: 64 x 16 x 224 x 224 x 3 bf16 = 308 MB).  blockIdx.y is the clip, so every per-clip parameter is read
// from the tables at a workgroup-uniform address and lives in scalar registers.  A thread owns AUG_PX = 8 CONSECUTIVE output
// pixels of the clip (linear index over [T][size][size]; the output is contiguous, so a run may cross a row end): 24
// elements, written as three (16-bit storage) or six (fp32) aligned 16-byte stores when the clip base is 16-byte aligned,
// by element otherwise and in a clip's last, partial run.
// The mean pass (contrast) walks the same pixels with the same geometry function, so the m it hands to the apply pass is
// the mean of exactly the values that pass sees.
#include "common.h"

#define AUG_THREADS 256
#define AUG_PX 8
#define AUG_PARTS X3D_AUG_MEAN_PARTS

struct AugArgs {
  const long long* videos;
  const int* geom;
  const float* color;
  void* out;
  double* scratch;
  int T, rate, size;
  int erase_mode, use_mean, vec;
  float mean[3], std[3];
};

// A video's address comes out of a table, so the compiler cannot tell its address space and would use flat loads; it is
// global memory.
typedef const __attribute__((address_space(1))) unsigned char* aug_gptr;

// the per-clip row of the geometry table, in scalar registers
struct AugClip {
  aug_gptr video;
  int F, H, W, start, mode, nh, nw, y0, x0, bh, bw, flip, ey0, ey1, ex0, ex1;
  unsigned seed_lo, seed_hi;
  float sy, sx;
};

__device__ __forceinline__ AugClip aug_clip(const AugArgs& a, int n) {
#pragma clang fp contract(off)
  const int* g = a.geom + (long long)n * X3D_AUG_GEOM_COLS;
  AugClip c;
  c.video = (aug_gptr)(uintptr_t)a.videos[n];
  // max(., 1): no-ops for the rows the host wrapper accepted; they keep a device row that is not the validated host row from
  // dividing by zero or clamping a tap to -1 (scalar instructions, once per workgroup)
  c.F = max(g[X3D_AUG_G_F], 1); c.H = max(g[X3D_AUG_G_H], 1); c.W = max(g[X3D_AUG_G_W], 1); c.start = g[X3D_AUG_G_START];
  c.mode = g[X3D_AUG_G_MODE]; c.nh = max(g[X3D_AUG_G_NH], 1); c.nw = max(g[X3D_AUG_G_NW], 1);
  c.y0 = g[X3D_AUG_G_Y0]; c.x0 = g[X3D_AUG_G_X0]; c.bh = max(g[X3D_AUG_G_BH], 1); c.bw = max(g[X3D_AUG_G_BW], 1);
  c.flip = g[X3D_AUG_G_FLIP];
  c.ey0 = g[X3D_AUG_G_EY0]; c.ey1 = g[X3D_AUG_G_EY1]; c.ex0 = g[X3D_AUG_G_EX0]; c.ex1 = g[X3D_AUG_G_EX1];
  c.seed_lo = (unsigned)g[X3D_AUG_G_SEED_LO]; c.seed_hi = (unsigned)g[X3D_AUG_G_SEED_HI];
  if (c.mode == X3D_AUG_CROP_JITTER) { c.sy = (float)c.H / (float)c.nh; c.sx = (float)c.W / (float)c.nw; }   // views.hip
  else { c.sy = (float)c.bh / (float)a.size; c.sx = (float)c.bw / (float)a.size; }
  return c;
}

// frame t of the clip = (start + t * rate) mod F of the video (32-bit: the host wrapper checks T * rate + F < 2^31); the
// result is below F whatever `start` holds
__device__ __forceinline__ aug_gptr aug_frame(const AugArgs& a, const AugClip& c, int t) {
  const unsigned frame = ((unsigned)c.start + (unsigned)t * (unsigned)a.rate) % (unsigned)c.F;
  return c.video + (long long)frame * c.H * c.W * 3;
}

// the geometric output at (y, x) of the clip's frame `fr`: three values on the 0-255 scale.  Every tap index is clamped to
// the frame (a no-op for the rows the host wrapper accepts).
__device__ __forceinline__ void aug_geom_px(const AugArgs& a, const AugClip& c, const aug_gptr fr, int y, int x, float (&px)[3]) {
#pragma clang fp contract(off)   // as eval_views_kernel: separate roundings, the uint8 truncation makes 1 ulp visible
  const int xs = c.flip ? a.size - 1 - x : x;
  if (c.mode == X3D_AUG_CROP_JITTER) {
    const int ry = y + c.y0, rx = xs + c.x0;
    if (c.nh == c.H && c.nw == c.W) {
      const long long o = ((long long)min(ry, c.H - 1) * c.W + min(rx, c.W - 1)) * 3;
#pragma unroll
      for (int k = 0; k < 3; k++) px[k] = (float)fr[o + k];
      return;
    }
    const float fy = ((float)ry + 0.5f) * c.sy - 0.5f;
    const float fx = ((float)rx + 0.5f) * c.sx - 0.5f;
    const float fyf = floorf(fy), fxf = floorf(fx);
    const int y0 = min(max((int)fyf, 0), c.H - 1), y1 = max(min((int)ceilf(fy), c.H - 1), 0);
    const int x0 = min(max((int)fxf, 0), c.W - 1), x1 = max(min((int)ceilf(fx), c.W - 1), 0);
    const float ly = fy - fyf, lx = fx - fxf;
    const long long otl = ((long long)y0 * c.W + x0) * 3, otr = ((long long)y0 * c.W + x1) * 3;
    const long long obl = ((long long)y1 * c.W + x0) * 3, obr = ((long long)y1 * c.W + x1) * 3;
#pragma unroll
    for (int k = 0; k < 3; k++) {
      const float tl = (float)fr[otl + k], tr = (float)fr[otr + k];
      const float bl = (float)fr[obl + k], br = (float)fr[obr + k];
      const float top = tl + (tr - tl) * lx;
      const float bot = bl + (br - bl) * lx;
      const float val = top + (bot - top) * ly;
      px[k] = (float)(unsigned char)(int)val;    // cast back to uint8: truncation (values are inside [0, 255])
    }
    return;
  }
  // random-resized crop: source coordinate inside the box, clamped below at 0; the second tap clamped to the box
  const float fy = fmaxf(((float)y + 0.5f) * c.sy - 0.5f, 0.f);
  const float fx = fmaxf(((float)xs + 0.5f) * c.sx - 0.5f, 0.f);
  const int iy0 = min((int)fy, c.bh - 1), ix0 = min((int)fx, c.bw - 1);
  const int iy1 = min(iy0 + 1, c.bh - 1), ix1 = min(ix0 + 1, c.bw - 1);
  const float ly = fminf(fy - (float)iy0, 1.f), lx = fminf(fx - (float)ix0, 1.f);
  const int ya = min(max(c.y0 + iy0, 0), c.H - 1), yb = min(max(c.y0 + iy1, 0), c.H - 1);
  const int xa = min(max(c.x0 + ix0, 0), c.W - 1), xb = min(max(c.x0 + ix1, 0), c.W - 1);
  const long long otl = ((long long)ya * c.W + xa) * 3, otr = ((long long)ya * c.W + xb) * 3;
  const long long obl = ((long long)yb * c.W + xa) * 3, obr = ((long long)yb * c.W + xb) * 3;
#pragma unroll
  for (int k = 0; k < 3; k++) {
    const float tl = (float)fr[otl + k], tr = (float)fr[otr + k];
    const float bl = (float)fr[obl + k], br = (float)fr[obr + k];
    const float top = tl + (tr - tl) * lx;
    const float bot = bl + (br - bl) * lx;
    px[k] = top + (bot - top) * ly;
  }
}

// three N(0, 1) values of pixel `pix` of clip `clip` (philox4x32_10 of common.h, key: the clip's own seed): Box-Muller on uniforms (w >> 8) + 1) * 2^-24 in (0, 1] (exact in fp32)
__device__ __forceinline__ void aug_noise3(const AugClip& c, int clip, long long pix, float (&z)[3]) {
  const Philox4 w = philox4x32_10((uint32_t)pix, (uint32_t)((unsigned long long)pix >> 32), (uint32_t)clip, 0u, c.seed_lo, c.seed_hi);
  const uint32_t (&r)[4] = w.v;
  const float u0 = (float)((r[0] >> 8) + 1u) * 5.9604644775390625e-8f, u1 = (float)((r[1] >> 8) + 1u) * 5.9604644775390625e-8f;
  const float u2 = (float)((r[2] >> 8) + 1u) * 5.9604644775390625e-8f, u3 = (float)((r[3] >> 8) + 1u) * 5.9604644775390625e-8f;
  // hardware log2 / sin / cos (v_log_f32, v_sin_f32, v_cos_f32: the angle in revolutions, absolute error ~1e-6): plenty for
  // noise, and small enough to sit in the unrolled pixel loop eight times
  const float ra = sqrtf(-1.3862943611198906f * __builtin_amdgcn_logf(u0));    // -2 ln u = -2 ln 2 * log2 u
  const float rb = sqrtf(-1.3862943611198906f * __builtin_amdgcn_logf(u2));
  z[0] = ra * __builtin_amdgcn_cosf(u1);
  z[1] = ra * __builtin_amdgcn_sinf(u1);
  z[2] = rb * __builtin_amdgcn_cosf(u3);
}

// ------------------------------------------------------------------------------------------------
// mean pass: grid (AUG_PARTS, N).  Workgroup (p, n) sums the gray of pixels [p * per, (p + 1) * per) of clip n -- fp32 gray per
// pixel, fp64 sums: per thread in pixel order, then the xor butterfly of wave_sum_d, then the waves in ascending order -- and
// writes scratch[n][p].  A fixed order throughout; nothing is added into memory.
// ------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(AUG_THREADS) void aug_mean_kernel(const AugArgs a) {
#pragma clang fp contract(off)
  const int n = blockIdx.y, part = blockIdx.x;
  if (a.color[(long long)n * X3D_AUG_COLOR_COLS + X3D_AUG_C_K] == 0.f) return;    // uniform: the clip does not use m
  const AugClip c = aug_clip(a, n);
  const long long total = (long long)a.T * a.size * a.size;
  const long long per = (total + AUG_PARTS - 1) / AUG_PARTS;
  const long long lo = part * per, hi = min(lo + per, total);
  double acc = 0.0;
  for (long long i = lo + threadIdx.x; i < hi; i += AUG_THREADS) {
    const int x = (int)(i % a.size);
    const long long r = i / a.size;
    const int y = (int)(r % a.size), t = (int)(r / a.size);
    float px[3];
    aug_geom_px(a, c, aug_frame(a, c, t), y, x, px);
    acc += (double)(0.299f * px[0] + 0.587f * px[1] + 0.114f * px[2]);
  }
  acc = wave_sum_d(acc);
  __shared__ double red[AUG_THREADS / WAVE];
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = acc;
  __syncthreads();
  if (threadIdx.x == 0) {
    double s = 0.0;
    for (int w = 0; w < AUG_THREADS / WAVE; w++) s += red[w];
    a.scratch[(long long)n * AUG_PARTS + part] = s;
  }
}

// ------------------------------------------------------------------------------------------------
// apply pass: grid (ceil(T * size * size / (AUG_THREADS * AUG_PX)), N)
// ------------------------------------------------------------------------------------------------
template <typename T>
__global__ __launch_bounds__(AUG_THREADS) void aug_apply_kernel(const AugArgs a) {
#pragma clang fp contract(off)
  const int n = blockIdx.y;
  const AugClip c = aug_clip(a, n);
  const float* col = a.color + (long long)n * X3D_AUG_COLOR_COLS;
  float M[9];
#pragma unroll
  for (int k = 0; k < 9; k++) M[k] = col[k];
  const float K = col[X3D_AUG_C_K];
  const long long total = (long long)a.T * a.size * a.size;
  const bool neutral = M[0] == 1.f && M[1] == 0.f && M[2] == 0.f && M[3] == 0.f && M[4] == 1.f && M[5] == 0.f && M[6] == 0.f &&
                       M[7] == 0.f && M[8] == 1.f && K == 0.f;
  float km = 0.f;                       // K * m
  if (a.use_mean && K != 0.f) {
    double s = 0.0;
    for (int p = 0; p < AUG_PARTS; p++) s += a.scratch[(long long)n * AUG_PARTS + p];     // uniform addresses, ascending order
    km = K * (float)(s / (double)total);
  }
  const bool erase = c.ey1 > c.ey0 && c.ex1 > c.ex0;
  const long long i0 = ((long long)blockIdx.x * AUG_THREADS + threadIdx.x) * AUG_PX;
  if (i0 >= total) return;
  int x = (int)(i0 % a.size);
  long long r = i0 / a.size;
  int y = (int)(r % a.size), t = (int)(r / a.size);
  const int npx = (int)min((long long)AUG_PX, total - i0);
  aug_gptr fr = aug_frame(a, c, t);      // recomputed only where the run crosses into the next frame
  float v[AUG_PX * 3];
#pragma unroll
  for (int p = 0; p < AUG_PX; p++) {
    if (p < npx) {
      float px[3];
      if (erase && y >= c.ey0 && y < c.ey1 && x >= c.ex0 && x < c.ex1) {
        if (a.erase_mode == X3D_AUG_ERASE_PIXEL) aug_noise3(c, n, i0 + p, px);
        else px[0] = px[1] = px[2] = 0.f;
#pragma unroll
        for (int k = 0; k < 3; k++) v[p * 3 + k] = px[k];
      } else {
        aug_geom_px(a, c, fr, y, x, px);
        if (!neutral) {
          const float q0 = M[0] * px[0] + M[1] * px[1] + M[2] * px[2] + km;
          const float q1 = M[3] * px[0] + M[4] * px[1] + M[5] * px[2] + km;
          const float q2 = M[6] * px[0] + M[7] * px[1] + M[8] * px[2] + km;
          px[0] = q0; px[1] = q1; px[2] = q2;
        }
#pragma unroll
        for (int k = 0; k < 3; k++) v[p * 3 + k] = (px[k] / 255.0f - a.mean[k]) / a.std[k];
      }
      if (++x == a.size) { x = 0; if (++y == a.size) { y = 0; ++t; if (t < a.T) fr = aug_frame(a, c, t); } }
    } else {
#pragma unroll
      for (int k = 0; k < 3; k++) v[p * 3 + k] = 0.f;
    }
  }
  T* o = (T*)a.out + ((long long)n * total + i0) * 3;
  if (a.vec && npx == AUG_PX) {
#pragma unroll
    for (int e = 0; e < AUG_PX * 3; e += 8) {
      float w[8];
#pragma unroll
      for (int j = 0; j < 8; j++) w[j] = v[e + j];
      VecIO<T, 8>::store(o + e, w);
    }
  } else {
    for (int e = 0; e < npx * 3; e++) o[e] = from_f<T>(v[e]);
  }
}

extern "C" long long x3d_train_clips_aug_scratch(int N, int T, int size) {
  (void)T; (void)size;
  return N > 0 ? (long long)N * AUG_PARTS * (long long)sizeof(double) : 0;
}

extern "C" int x3d_train_clips_aug(const long long* videos, const int* geom, const float* color, const int* host_geom,
                                   const float* host_color, void* out, void* scratch, int N, int T, int rate, int size,
                                   const float* mean, const float* std, int erase_mode, int dtype, void* stream) {
  X3D_REQUIRE(N > 0 && N <= 65535, "train_clips_aug: N = %d clips (1 .. 65535)", N);
  X3D_REQUIRE(videos && geom && color && host_geom && host_color, "train_clips_aug: null table");
  X3D_REQUIRE(out && scratch && mean && std, "train_clips_aug: null pointer");
  X3D_REQUIRE(T > 0 && rate > 0 && size > 0, "train_clips_aug: bad extents T=%d rate=%d size=%d", T, rate, size);
  X3D_REQUIRE((long long)T * rate < (1ll << 30), "train_clips_aug: T * rate = %lld (below 2^30)", (long long)T * rate);
  X3D_REQUIRE(x3d_dtype_ok(dtype), "train_clips_aug: unknown dtype %d", dtype);
  X3D_REQUIRE(erase_mode == X3D_AUG_ERASE_CONST || erase_mode == X3D_AUG_ERASE_PIXEL, "train_clips_aug: unknown erase_mode %d", erase_mode);
  X3D_REQUIRE((uintptr_t)scratch % 8 == 0, "train_clips_aug: scratch not 8-byte aligned");
  const int es = dtype == X3D_F32 ? 4 : 2;
  X3D_REQUIRE((uintptr_t)out % es == 0, "train_clips_aug: out not aligned to the element size");
  bool use_mean = false;
  for (int n = 0; n < N; n++) {
    const int* g = host_geom + (long long)n * X3D_AUG_GEOM_COLS;
    const int F = g[X3D_AUG_G_F], H = g[X3D_AUG_G_H], W = g[X3D_AUG_G_W];
    X3D_REQUIRE(F > 0 && F < (1 << 30) && H > 0 && W > 0, "train_clips_aug: clip %d: bad video extents %d x %d x %d", n, F, H, W);
    X3D_REQUIRE((long long)F * H * W * 3 < (1ll << 40), "train_clips_aug: clip %d: video too large", n);
    X3D_REQUIRE(g[X3D_AUG_G_START] >= 0 && g[X3D_AUG_G_START] < F, "train_clips_aug: clip %d: start %d outside the %d frames", n,
                g[X3D_AUG_G_START], F);
    X3D_REQUIRE(g[X3D_AUG_G_FLIP] == 0 || g[X3D_AUG_G_FLIP] == 1, "train_clips_aug: clip %d: flip = %d", n, g[X3D_AUG_G_FLIP]);
    const int y0 = g[X3D_AUG_G_Y0], x0 = g[X3D_AUG_G_X0];
    if (g[X3D_AUG_G_MODE] == X3D_AUG_CROP_JITTER) {
      const int nh = g[X3D_AUG_G_NH], nw = g[X3D_AUG_G_NW];
      X3D_REQUIRE(nh >= size && nw >= size, "train_clips_aug: clip %d: resized frame %dx%d smaller than the crop %d", n, nh, nw, size);
      X3D_REQUIRE(y0 >= 0 && y0 <= nh - size && x0 >= 0 && x0 <= nw - size,
                  "train_clips_aug: clip %d: crop offset (%d, %d) outside the %dx%d frame", n, y0, x0, nh, nw);
    } else if (g[X3D_AUG_G_MODE] == X3D_AUG_CROP_RRC) {
      const int bh = g[X3D_AUG_G_BH], bw = g[X3D_AUG_G_BW];
      X3D_REQUIRE(bh > 0 && bw > 0 && y0 >= 0 && x0 >= 0 && bh <= H - y0 && bw <= W - x0,
                  "train_clips_aug: clip %d: box (%d, %d) + %d x %d outside the %d x %d frame", n, y0, x0, bh, bw, H, W);
    } else {
      X3D_REQUIRE(false, "train_clips_aug: clip %d: unknown crop mode %d", n, g[X3D_AUG_G_MODE]);
    }
    X3D_REQUIRE(0 <= g[X3D_AUG_G_EY0] && g[X3D_AUG_G_EY0] <= g[X3D_AUG_G_EY1] && g[X3D_AUG_G_EY1] <= size &&
                0 <= g[X3D_AUG_G_EX0] && g[X3D_AUG_G_EX0] <= g[X3D_AUG_G_EX1] && g[X3D_AUG_G_EX1] <= size,
                "train_clips_aug: clip %d: erase box [%d, %d) x [%d, %d) outside the %d x %d crop", n, g[X3D_AUG_G_EY0],
                g[X3D_AUG_G_EY1], g[X3D_AUG_G_EX0], g[X3D_AUG_G_EX1], size, size);
    const float* c = host_color + (long long)n * X3D_AUG_COLOR_COLS;
    for (int k = 0; k < X3D_AUG_COLOR_COLS; k++)
      X3D_REQUIRE(c[k] - c[k] == 0.f, "train_clips_aug: clip %d: colour coefficient %d is not finite", n, k);
    if (c[X3D_AUG_C_K] != 0.f) use_mean = true;
  }
  const long long total = (long long)T * size * size;
  const long long gx = ceil_div_ll(total, (long long)AUG_THREADS * AUG_PX);
  X3D_REQUIRE(gx < (1ll << 31), "train_clips_aug: too many pixels");
  AugArgs a;
  a.videos = videos; a.geom = geom; a.color = color; a.out = out; a.scratch = (double*)scratch;
  a.T = T; a.rate = rate; a.size = size; a.erase_mode = erase_mode; a.use_mean = use_mean ? 1 : 0;
  a.vec = ((uintptr_t)out % 16 == 0 && (total * 3 * es) % 16 == 0) ? 1 : 0;
  for (int k = 0; k < 3; k++) { a.mean[k] = mean[k]; a.std[k] = std[k]; }
  hipStream_t st = (hipStream_t)stream;
  if (use_mean) {
    hipLaunchKernelGGL(aug_mean_kernel, dim3(AUG_PARTS, (unsigned)N), dim3(AUG_THREADS), 0, st, a);
    X3D_LAUNCH_CHECK("train_clips_aug (mean)");
  }
  const dim3 grid((unsigned)gx, (unsigned)N);
  if (dtype == X3D_F32) hipLaunchKernelGGL((aug_apply_kernel<float>), grid, dim3(AUG_THREADS), 0, st, a);
  else if (dtype == X3D_F16) hipLaunchKernelGGL((aug_apply_kernel<f16>), grid, dim3(AUG_THREADS), 0, st, a);
  else hipLaunchKernelGGL((aug_apply_kernel<bf16>), grid, dim3(AUG_THREADS), 0, st, a);
  X3D_LAUNCH_CHECK("train_clips_aug");
  return X3D_OK;
}
