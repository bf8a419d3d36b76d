// x3d_randaug_clips: RandAugment on the decoded uint8 frames (AUG.AA_TYPE of the config, x3d_tf_amd/aug.py).  The exact
// rules -- every op's arithmetic, the tables, the refusals -- are in include/x3d_hip.h.
//
// Shape.  Per layer one apply launch over the whole batch, grid (chunk, frame, clip): blockIdx.z is the clip, so the op and
// its arguments come from a workgroup-uniform row of the device tables and the op switch is a scalar branch; clips of
// different extents and ops share the launch (workgroups past the end of their own frame, and those of a clip with
// X3D_RA_NONE, return at once).  A workgroup owns RA_CHUNK_PX consecutive pixels of one frame.
//   point ops   (everything that is one 256-entry table per channel: invert, solarize, solarize-add, posterize, brightness,
//               contrast, autocontrast, equalize): the workgroup builds the 3 x 256 table of its frame in LDS, then streams:
//               a byte head up to the first 16-byte boundary of the DESTINATION, 16 bytes per lane (aligned stores; the
//               source has any alignment), a byte tail.  Rows are 3 W bytes and frame bases H W 3 bytes apart: no alignment
//               can be assumed.  COPY streams the same way without the table.
//   pixel ops   (colour, sharpness, the affine maps): a lane owns 16 consecutive pixels = 48 bytes, stored as three 16-byte
//               vectors of unknown alignment (bytes in the frame's last, partial run).  Sharpness and the affine maps read
//               other pixels than the one they write, which is why the host never lets SRC and DST overlap.
// The statistics launch (grid (RA_STAT_PARTS, frame, clip)) runs only before a layer that needs it, and only the workgroups
// of AUTOCONTRAST / EQUALIZE / CONTRAST clips do anything: a 3 x 256 histogram in LDS (ds atomics), or the sum of L, added
// to the frame's record in scratch with integer atomics.  Integer sums commute: the same bits on every run.
// Nothing here has been timed on its own beyond tools/randaug_bench.py; the byte-granular taps of sharpness and the affine
// maps lean on the caches.
#include "common.h"

#define RA_THREADS 256
#define RA_RUN_PX 16                             // pixels per lane (pixel ops): 48 bytes
#define RA_CHUNK_PX (RA_THREADS * RA_RUN_PX)     // pixels per workgroup: 12288 bytes, a multiple of 3 and of 16
#define RA_STAT_PARTS 4
#define RA_WORDS X3D_RA_STAT_WORDS
#define RA_LSUM 768                              // word index of the uint64 L sum in a frame's record

typedef const __attribute__((address_space(1))) unsigned char* ra_gptr;   // table-borne addresses are global memory (aug.hip)
typedef __attribute__((address_space(1))) unsigned char* ra_wptr;
typedef unsigned int ra_u4 __attribute__((ext_vector_type(4)));
typedef ra_u4 ra_u4_any __attribute__((aligned(1)));                       // 16 bytes at any address

struct RaArgs {
  const long long* videos;
  const int* clips;
  const int* ops;
  const long long* xform;
  unsigned char* work;
  unsigned int* stats;
  int T, rate, layers, layer;
  int fill[3];
};

// the (clip, layer) row, in scalar registers
struct RaClip {
  int op, iarg, F, H, W, start;
  float farg;
  long long m[6], src, dst;
  long long frame_bytes;
};

__device__ __forceinline__ RaClip ra_clip(const RaArgs& a, int n) {
  RaClip c;
  const int* g = a.clips + (long long)n * X3D_RA_CLIP_COLS;
  const int* o = a.ops + ((long long)n * a.layers + a.layer) * X3D_RA_OP_COLS;
  const long long* x = a.xform + ((long long)n * a.layers + a.layer) * X3D_RA_X_COLS;
  // max(., 1) as in aug.hip: no-ops for the rows the host wrapper accepted
  c.F = max(g[0], 1); c.H = max(g[1], 1); c.W = max(g[2], 1); c.start = g[3];
  c.op = o[X3D_RA_O_OP]; c.iarg = o[X3D_RA_O_IARG]; c.farg = __int_as_float(o[X3D_RA_O_FARG]);
#pragma unroll
  for (int k = 0; k < 6; k++) c.m[k] = x[X3D_RA_X_A + k];
  c.src = x[X3D_RA_X_SRC]; c.dst = x[X3D_RA_X_DST];
  c.frame_bytes = (long long)c.H * c.W * 3;
  return c;
}

// frame t of the layer's source: the work area, or (SRC < 0) frame (start + t * rate) mod F of the video
__device__ __forceinline__ ra_gptr ra_src_frame(const RaArgs& a, const RaClip& c, int n, int t) {
  if (c.src >= 0) return (ra_gptr)(uintptr_t)(a.work + c.src) + (long long)t * c.frame_bytes;
  const unsigned frame = ((unsigned)c.start + (unsigned)t * (unsigned)a.rate) % (unsigned)c.F;
  return (ra_gptr)(uintptr_t)a.videos[n] + (long long)frame * c.frame_bytes;
}

__device__ __forceinline__ bool ra_needs_stats(int op) {
  return op == X3D_RA_AUTOCONTRAST || op == X3D_RA_EQUALIZE || op == X3D_RA_CONTRAST;
}

__device__ __forceinline__ unsigned ra_luma(unsigned r, unsigned g, unsigned b) {
  return (19595u * r + 38470u * g + 7471u * b + 32768u) >> 16;
}

// PIL's Image.blend outside [0, 1]: d + f (v - d), every step rounded to fp32, clipped, truncated
__device__ __forceinline__ unsigned ra_blend(int v, int d, float f) {
#pragma clang fp contract(off)
  const float t = f * (float)(v - d);
  const float r = (float)d + t;
  return r <= 0.f ? 0u : (r >= 255.f ? 255u : (unsigned)(int)r);
}

// ------------------------------------------------------------------------------------------------
// statistics: grid (RA_STAT_PARTS, T, N)
// ------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(RA_THREADS) void ra_stats_kernel(const RaArgs a) {
  const int n = blockIdx.z, t = blockIdx.y, part = blockIdx.x;
  const int op = a.ops[((long long)n * a.layers + a.layer) * X3D_RA_OP_COLS + X3D_RA_O_OP];
  if (!ra_needs_stats(op)) return;                      // uniform
  const RaClip c = ra_clip(a, n);
  const ra_gptr src = ra_src_frame(a, c, n, t);
  unsigned int* rec = a.stats + ((long long)n * a.T + t) * RA_WORDS;
  const long long px = (long long)c.H * c.W;
  const long long per = (px + RA_STAT_PARTS - 1) / RA_STAT_PARTS;
  const long long p0 = min((long long)part * per, px), p1 = min(p0 + per, px);
  if (op == X3D_RA_CONTRAST) {
    __shared__ unsigned long long lsum;
    if (threadIdx.x == 0) lsum = 0ull;
    __syncthreads();
    unsigned long long acc = 0ull;
    for (long long p = p0 + threadIdx.x; p < p1; p += RA_THREADS)
      acc += ra_luma(src[p * 3], src[p * 3 + 1], src[p * 3 + 2]);
    atomicAdd(&lsum, acc);
    __syncthreads();
    if (threadIdx.x == 0 && lsum) atomicAdd((unsigned long long*)(rec + RA_LSUM), lsum);
    return;
  }
  __shared__ unsigned int hist[768];
  for (int i = threadIdx.x; i < 768; i += RA_THREADS) hist[i] = 0u;
  __syncthreads();
  const long long b0 = p0 * 3, b1 = p1 * 3;
  for (long long o = b0 + (long long)threadIdx.x * 16; o < b1; o += RA_THREADS * 16) {
    unsigned ch = (unsigned)(o % 3);
    if (o + 16 <= b1) {
      const ra_u4 v = *(const __attribute__((address_space(1))) ra_u4_any*)(src + o);
#pragma unroll
      for (int j = 0; j < 16; j++) {
        atomicAdd(&hist[ch * 256 + ((v[j >> 2] >> ((j & 3) * 8)) & 255u)], 1u);
        ch = ch == 2 ? 0 : ch + 1;
      }
    } else {
      for (long long q = o; q < b1; q++) {
        atomicAdd(&hist[ch * 256 + src[q]], 1u);
        ch = ch == 2 ? 0 : ch + 1;
      }
    }
  }
  __syncthreads();
  for (int i = threadIdx.x; i < 768; i += RA_THREADS)
    if (hist[i]) atomicAdd(rec + i, hist[i]);
}

// ------------------------------------------------------------------------------------------------
// apply: grid (chunks of the largest frame, T, N)
// ------------------------------------------------------------------------------------------------
// one pixel of the affine ops (include/x3d_hip.h): 64-bit fixed point with X3D_RA_FRAC_BITS fractional bits
__device__ __forceinline__ void ra_affine_px(const RaArgs& a, const RaClip& c, const ra_gptr src, int y, int x, unsigned (&o)[3]) {
  const long long one = 1ll << X3D_RA_FRAC_BITS;
  long long sx = c.m[0] * x + c.m[1] * y + c.m[2];
  long long sy = c.m[3] * x + c.m[4] * y + c.m[5];
  if (sx < 0 || sy < 0 || sx >= (long long)c.W * one || sy >= (long long)c.H * one) {
    o[0] = (unsigned)a.fill[0]; o[1] = (unsigned)a.fill[1]; o[2] = (unsigned)a.fill[2];
    return;
  }
  sx -= one >> 1; sy -= one >> 1;
  const int ix = (int)(sx >> X3D_RA_FRAC_BITS), iy = (int)(sy >> X3D_RA_FRAC_BITS);      // arithmetic shifts: floor
  const unsigned fx = (unsigned)(sx >> (X3D_RA_FRAC_BITS - 8)) & 255u, fy = (unsigned)(sy >> (X3D_RA_FRAC_BITS - 8)) & 255u;
  const int x0 = min(max(ix, 0), c.W - 1), x1 = min(max(ix + 1, 0), c.W - 1);
  const int y0 = min(max(iy, 0), c.H - 1), y1 = min(max(iy + 1, 0), c.H - 1);
  const long long o00 = ((long long)y0 * c.W + x0) * 3, o01 = ((long long)y0 * c.W + x1) * 3;
  const long long o10 = ((long long)y1 * c.W + x0) * 3, o11 = ((long long)y1 * c.W + x1) * 3;
#pragma unroll
  for (int k = 0; k < 3; k++) {
    const unsigned top = src[o00 + k] * (256u - fx) + src[o01 + k] * fx;
    const unsigned bot = src[o10 + k] * (256u - fx) + src[o11 + k] * fx;
    o[k] = (top * (256u - fy) + bot * fy + 32768u) >> 16;
  }
}

__device__ __forceinline__ void ra_sharp_px(const RaClip& c, const ra_gptr src, int y, int x, unsigned (&o)[3]) {
  const long long at = ((long long)y * c.W + x) * 3;
  if (y == 0 || x == 0 || y == c.H - 1 || x == c.W - 1) {
#pragma unroll
    for (int k = 0; k < 3; k++) o[k] = src[at + k];
    return;
  }
  const long long row = (long long)c.W * 3;
#pragma unroll
  for (int k = 0; k < 3; k++) {
    const unsigned v = src[at + k];
    unsigned s = 4u * v + 6u;                                       // centre weight 5 = 1 + 4
#pragma unroll
    for (int dy = -1; dy <= 1; dy++)
#pragma unroll
      for (int dx = -1; dx <= 1; dx++) s += src[at + dy * row + dx * 3 + k];
    o[k] = ra_blend((int)v, (int)(s / 13u), c.farg);
  }
}

__global__ __launch_bounds__(RA_THREADS) void ra_apply_kernel(const RaArgs a) {
#pragma clang fp contract(off)
  const int n = blockIdx.z, t = blockIdx.y;
  const int op = a.ops[((long long)n * a.layers + a.layer) * X3D_RA_OP_COLS + X3D_RA_O_OP];
  if (op == X3D_RA_NONE) return;                        // uniform
  const RaClip c = ra_clip(a, n);
  const long long px = (long long)c.H * c.W;
  const long long p0 = (long long)blockIdx.x * RA_CHUNK_PX;
  if (p0 >= px) return;                                 // uniform: a smaller frame than the launch's largest
  const long long p1 = min(p0 + RA_CHUNK_PX, px);
  const ra_gptr src = ra_src_frame(a, c, n, t);
  const ra_wptr dst = (ra_wptr)(uintptr_t)(a.work + c.dst) + (long long)t * c.frame_bytes;

  const bool pixel_op = op == X3D_RA_COLOR || op == X3D_RA_SHARPNESS || op == X3D_RA_ROTATE || op == X3D_RA_SHEAR_X ||
                        op == X3D_RA_SHEAR_Y || op == X3D_RA_TRANSLATE_X || op == X3D_RA_TRANSLATE_Y;
  if (pixel_op) {
    const long long q0 = p0 + (long long)threadIdx.x * RA_RUN_PX;
    if (q0 >= p1) return;
    const int npx = (int)min((long long)RA_RUN_PX, p1 - q0);
    int x = (int)(q0 % c.W), y = (int)(q0 / c.W);
    unsigned w[RA_RUN_PX * 3 / 4];                       // the run's 48 bytes, little-endian words
#pragma unroll
    for (int k = 0; k < RA_RUN_PX * 3 / 4; k++) w[k] = 0u;
    ra_u4 in[3];
    if (op == X3D_RA_COLOR && npx == RA_RUN_PX) {
#pragma unroll
      for (int k = 0; k < 3; k++) in[k] = *(const __attribute__((address_space(1))) ra_u4_any*)(src + q0 * 3 + k * 16);
    }
#pragma unroll
    for (int p = 0; p < RA_RUN_PX; p++) {
      if (p < npx) {
        unsigned o[3];
        if (op == X3D_RA_COLOR) {
          unsigned v[3];
#pragma unroll
          for (int k = 0; k < 3; k++) {
            const int b = p * 3 + k;
            v[k] = npx == RA_RUN_PX ? (in[b >> 4][(b >> 2) & 3] >> ((b & 3) * 8)) & 255u : (unsigned)src[(q0 + p) * 3 + k];
          }
          const int d = (int)ra_luma(v[0], v[1], v[2]);
#pragma unroll
          for (int k = 0; k < 3; k++) o[k] = ra_blend((int)v[k], d, c.farg);
        } else if (op == X3D_RA_SHARPNESS) {
          ra_sharp_px(c, src, y, x, o);
        } else {
          ra_affine_px(a, c, src, y, x, o);
        }
#pragma unroll
        for (int k = 0; k < 3; k++) {
          const int b = p * 3 + k;
          w[b >> 2] |= o[k] << ((b & 3) * 8);
        }
        if (++x == c.W) { x = 0; ++y; }
      }
    }
    const ra_wptr d0 = dst + q0 * 3;
    if (npx == RA_RUN_PX) {
#pragma unroll
      for (int k = 0; k < 3; k++) {
        ra_u4 v;
        v[0] = w[k * 4]; v[1] = w[k * 4 + 1]; v[2] = w[k * 4 + 2]; v[3] = w[k * 4 + 3];
        *(__attribute__((address_space(1))) ra_u4_any*)(d0 + k * 16) = v;
      }
    } else {
#pragma unroll
      for (int b = 0; b < RA_RUN_PX * 3; b++)
        if (b < npx * 3) d0[b] = (unsigned char)(w[b >> 2] >> ((b & 3) * 8));
    }
    return;
  }

  // ---- point ops: the frame's 3 x 256 table in LDS --------------------------------------------------------------
  __shared__ unsigned int h[768];          // histogram, then its exclusive prefix sums (equalize)
  __shared__ int lo[3], hi[3], bins[3];
  __shared__ unsigned char lut[768];
  const unsigned int* rec = a.stats + ((long long)n * a.T + t) * RA_WORDS;
  const int i = threadIdx.x;               // RA_THREADS == 256: thread i builds entry i of the three channels
  if (op == X3D_RA_AUTOCONTRAST || op == X3D_RA_EQUALIZE) {
    if (i < 3) { lo[i] = 255; hi[i] = 0; bins[i] = 0; }
    __syncthreads();
#pragma unroll
    for (int ch = 0; ch < 3; ch++) {
      const unsigned cnt = rec[ch * 256 + i];
      h[ch * 256 + i] = cnt;
      if (cnt) { atomicMin(&lo[ch], i); atomicMax(&hi[ch], i); atomicAdd(&bins[ch], 1); }
    }
    __syncthreads();
    if (op == X3D_RA_EQUALIZE) {
      unsigned last[3];
#pragma unroll
      for (int ch = 0; ch < 3; ch++) last[ch] = h[ch * 256 + hi[ch]];
      __syncthreads();
      if (i < 3) {                          // exclusive prefix sums of channel i, in place
        unsigned run = 0u;
        for (int k = 0; k < 256; k++) { const unsigned cnt = h[i * 256 + k]; h[i * 256 + k] = run; run += cnt; }
      }
      __syncthreads();
#pragma unroll
      for (int ch = 0; ch < 3; ch++) {
        const unsigned step = ((unsigned)px - last[ch]) / 255u;
        unsigned v = (unsigned)i;
        if (bins[ch] >= 2 && step != 0u) v = min(255u, (step / 2u + h[ch * 256 + i]) / step);
        lut[ch * 256 + i] = (unsigned char)v;
      }
    } else {
#pragma unroll
      for (int ch = 0; ch < 3; ch++) {
        unsigned v = (unsigned)i;
        if (hi[ch] > lo[ch]) {
          const double scale = 255.0 / (double)(hi[ch] - lo[ch]);
          const double a0 = (double)i * scale, b0 = (double)lo[ch] * scale;
          const double r = a0 - b0;
          v = r <= 0.0 ? 0u : (r >= 255.0 ? 255u : (unsigned)(int)r);
        }
        lut[ch * 256 + i] = (unsigned char)v;
      }
    }
  } else if (op != X3D_RA_COPY) {
    unsigned v = (unsigned)i;
    if (op == X3D_RA_INVERT) v = 255u - v;
    else if (op == X3D_RA_SOLARIZE) v = i < c.iarg ? v : 255u - v;
    else if (op == X3D_RA_SOLARIZE_ADD) v = i < 128 ? min(255u, v + (unsigned)c.iarg) : v;
    else if (op == X3D_RA_POSTERIZE) v = c.iarg >= 8 ? v : (c.iarg <= 0 ? 0u : v & ~((1u << (8 - c.iarg)) - 1u) & 255u);
    else if (op == X3D_RA_BRIGHTNESS) v = ra_blend(i, 0, c.farg);
    else if (op == X3D_RA_CONTRAST) {
      const unsigned long long s = *(const unsigned long long*)(rec + RA_LSUM);
      const int d = (int)((double)s / (double)px + 0.5);
      v = ra_blend(i, d, c.farg);
    }
    lut[i] = lut[256 + i] = lut[512 + i] = (unsigned char)v;
  }
  __syncthreads();

  const bool copy = op == X3D_RA_COPY;
  const long long b0 = p0 * 3, b1 = p1 * 3;
  const long long head = min((long long)((16 - ((uintptr_t)(dst + b0) & 15)) & 15), b1 - b0);
  const long long nvec = (b1 - b0 - head) / 16;
  const long long tail0 = b0 + head + nvec * 16;
  if (i < head) { const long long q = b0 + i; dst[q] = copy ? src[q] : lut[(q % 3) * 256 + src[q]]; }
  if (i < b1 - tail0) { const long long q = tail0 + i; dst[q] = copy ? src[q] : lut[(q % 3) * 256 + src[q]]; }
  for (long long k = i; k < nvec; k += RA_THREADS) {
    const long long q = b0 + head + k * 16;
    ra_u4 v = *(const __attribute__((address_space(1))) ra_u4_any*)(src + q);
    if (!copy) {
      unsigned ch = (unsigned)(q % 3);
#pragma unroll
      for (int wd = 0; wd < 4; wd++) {
        unsigned r = 0u;
#pragma unroll
        for (int j = 0; j < 4; j++) {
          r |= (unsigned)lut[ch * 256 + ((v[wd] >> (j * 8)) & 255u)] << (j * 8);
          ch = ch == 2 ? 0 : ch + 1;
        }
        v[wd] = r;
      }
    }
    *(__attribute__((address_space(1))) ra_u4*)(dst + q) = v;          // 16-byte aligned by the head
  }
}

extern "C" long long x3d_randaug_scratch(int N, int T) {
  return N > 0 && T > 0 ? (long long)N * T * RA_WORDS * (long long)sizeof(unsigned int) : 0;
}

extern "C" int x3d_randaug_clips(const long long* videos, const int* clips, const int* ops, const long long* xform,
                                 const int* host_clips, const int* host_ops, const long long* host_xform, void* work,
                                 long long work_bytes, void* scratch, int N, int T, int rate, int layers, int fill_r,
                                 int fill_g, int fill_b, void* stream) {
  X3D_REQUIRE(N > 0 && N <= 65535, "randaug_clips: N = %d clips (1 .. 65535)", N);
  X3D_REQUIRE(videos && clips && ops && xform && host_clips && host_ops && host_xform, "randaug_clips: null table");
  X3D_REQUIRE(work && scratch && work_bytes > 0, "randaug_clips: null pointer");
  X3D_REQUIRE(T > 0 && T <= 65535 && rate > 0 && layers > 0, "randaug_clips: bad extents T=%d rate=%d layers=%d", T, rate, layers);
  X3D_REQUIRE((long long)T * rate < (1ll << 30), "randaug_clips: T * rate = %lld (below 2^30)", (long long)T * rate);
  X3D_REQUIRE((uintptr_t)scratch % 8 == 0, "randaug_clips: scratch not 8-byte aligned");
  X3D_REQUIRE((uintptr_t)xform % 8 == 0 && (uintptr_t)videos % 8 == 0, "randaug_clips: int64 table not 8-byte aligned");
  X3D_REQUIRE(fill_r >= 0 && fill_r <= 255 && fill_g >= 0 && fill_g <= 255 && fill_b >= 0 && fill_b <= 255,
              "randaug_clips: fill colour (%d, %d, %d) outside 0..255", fill_r, fill_g, fill_b);
  for (int n = 0; n < N; n++) {
    const int* g = host_clips + (long long)n * X3D_RA_CLIP_COLS;
    const int F = g[0], H = g[1], W = g[2], start = g[3];
    X3D_REQUIRE(F > 0 && F < (1 << 30) && H > 0 && W > 0 && H <= 32768 && W <= 32768,
                "randaug_clips: clip %d: bad video extents %d x %d x %d", n, F, H, W);
    X3D_REQUIRE((long long)F * H * W * 3 < (1ll << 40), "randaug_clips: clip %d: video too large", n);
    X3D_REQUIRE(start >= 0 && start < F, "randaug_clips: clip %d: start %d outside the %d frames", n, start, F);
    const long long bytes = (long long)T * H * W * 3;
    for (int l = 0; l < layers; l++) {
      const int* o = host_ops + ((long long)n * layers + l) * X3D_RA_OP_COLS;
      const long long* x = host_xform + ((long long)n * layers + l) * X3D_RA_X_COLS;
      const int op = o[X3D_RA_O_OP];
      X3D_REQUIRE(op >= X3D_RA_NONE && op <= X3D_RA_COPY, "randaug_clips: clip %d layer %d: unknown op %d", n, l, op);
      if (op == X3D_RA_NONE) continue;
      if (op == X3D_RA_COLOR || op == X3D_RA_CONTRAST || op == X3D_RA_BRIGHTNESS || op == X3D_RA_SHARPNESS) {
        float f;
        memcpy(&f, &o[X3D_RA_O_FARG], sizeof f);
        X3D_REQUIRE(f - f == 0.f, "randaug_clips: clip %d layer %d: factor is not finite", n, l);
      }
      if (op == X3D_RA_POSTERIZE)
        X3D_REQUIRE(o[X3D_RA_O_IARG] >= 0 && o[X3D_RA_O_IARG] <= 8, "randaug_clips: clip %d layer %d: posterize bits %d outside [0, 8]",
                    n, l, o[X3D_RA_O_IARG]);
      if (op == X3D_RA_ROTATE || op == X3D_RA_SHEAR_X || op == X3D_RA_SHEAR_Y || op == X3D_RA_TRANSLATE_X || op == X3D_RA_TRANSLATE_Y)
        for (int k = 0; k < 6; k++) {
          const long long lim = (k == 2 || k == 5) ? (1ll << 60) : (1ll << 45);
          X3D_REQUIRE(x[k] > -lim && x[k] < lim, "randaug_clips: clip %d layer %d: matrix coefficient %d out of range", n, l, k);
        }
      const long long src = x[X3D_RA_X_SRC], dst = x[X3D_RA_X_DST];
      X3D_REQUIRE(dst >= 0 && dst <= work_bytes - bytes, "randaug_clips: clip %d layer %d: destination [%lld, +%lld) outside the %lld-byte work area",
                  n, l, dst, bytes, work_bytes);
      X3D_REQUIRE(src >= -1 && src <= work_bytes - bytes, "randaug_clips: clip %d layer %d: source [%lld, +%lld) outside the %lld-byte work area",
                  n, l, src, bytes, work_bytes);
      X3D_REQUIRE(src < 0 || src + bytes <= dst || dst + bytes <= src,
                  "randaug_clips: clip %d layer %d: source %lld and destination %lld overlap (%lld bytes each)", n, l, src, dst, bytes);
    }
  }
  RaArgs a;
  a.videos = videos; a.clips = clips; a.ops = ops; a.xform = xform; a.work = (unsigned char*)work;
  a.stats = (unsigned int*)scratch; a.T = T; a.rate = rate; a.layers = layers;
  a.fill[0] = fill_r; a.fill[1] = fill_g; a.fill[2] = fill_b;
  hipStream_t st = (hipStream_t)stream;
  for (int l = 0; l < layers; l++) {
    bool stats = false;
    long long max_px = 0;
    for (int n = 0; n < N; n++) {
      const int op = host_ops[((long long)n * layers + l) * X3D_RA_OP_COLS + X3D_RA_O_OP];
      if (op == X3D_RA_NONE) continue;
      const int* g = host_clips + (long long)n * X3D_RA_CLIP_COLS;
      max_px = max(max_px, (long long)g[1] * g[2]);
      if (op == X3D_RA_AUTOCONTRAST || op == X3D_RA_EQUALIZE || op == X3D_RA_CONTRAST) stats = true;
    }
    if (max_px == 0) continue;                            // every clip sits this layer out
    a.layer = l;
    if (stats) {
      if (hipMemsetAsync(scratch, 0, (size_t)x3d_randaug_scratch(N, T), st) != hipSuccess) {
        x3d_set_error("randaug_clips: clearing the statistics failed");
        return X3D_ERR_LAUNCH;
      }
      hipLaunchKernelGGL(ra_stats_kernel, dim3(RA_STAT_PARTS, (unsigned)T, (unsigned)N), dim3(RA_THREADS), 0, st, a);
      X3D_LAUNCH_CHECK("randaug_clips (statistics)");
    }
    const unsigned gx = (unsigned)ceil_div_ll(max_px, (long long)RA_CHUNK_PX);
    hipLaunchKernelGGL(ra_apply_kernel, dim3(gx, (unsigned)T, (unsigned)N), dim3(RA_THREADS), 0, st, a);
    X3D_LAUNCH_CHECK("randaug_clips");
  }
  return X3D_OK;
}
