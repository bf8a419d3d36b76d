// Mixup / CutMix on the device (MIXUP.* of the config, x3d_tf_amd/mix.py): a clip batch mixed with its own reverse and the
// soft targets that go with it.  The exact rules are in include/x3d_hip.h.
#include "common.h"

// ------------------------------------------------------------------------------------------------
// x3d_mix_clips.  Clip i is paired with clip j = N-1-i; workgroup row blockIdx.y owns the pair, and within it ONE thread
// owns the same elements of both clips: it reads both, then writes both, so out == x needs no second copy of the batch.
// A pair is walked as R element ranges of L elements each (mixup / copy: the whole clip, R = 1; CutMix: one range per box
// row, or per frame when the box spans the width, or the whole clip when it is the frame), range r at element offset
//   off0 + (r / bh) * t_stride + (r % bh) * row_stride
// of both clips.  A range is cut into vectors of 16 bytes from its own start; its last vector may be partial and is then
// handled by element.  Range starts fall on any element (a box row of W_box * C elements is neither 16-byte aligned nor a
// multiple of the vector width, and with T*H*W*C % VEC != 0 neither are the clips): the 16-byte accesses are unaligned
// there, which the compute queues allow (common.h, load8_ragged).  Every offset is 64-bit.
// ------------------------------------------------------------------------------------------------
#define MIX_THREADS 256
#define MIX_MAX_BLOCKS 2048     // 256 CUs x 8 workgroups; the rest of the work is grid-strided

enum { MIX_OP_BLEND = 0, MIX_OP_SWAP = 1, MIX_OP_COPY = 2 };

struct MixGeom {
  long long E;            // elements per clip
  long long L;            // elements per range
  long long nvr;          // vectors per range = ceil(L / VEC)
  long long R;            // ranges per clip
  long long items;        // R * nvr
  long long t_stride, row_stride, off0;
  int bh;                 // ranges per frame (1 when R == 1 or the box spans the width)
  int R1;                 // R == 1: no division
};

template <typename T> struct MixVec;
template <> struct MixVec<float> { typedef f32x4 v; static constexpr int n = 4; };
template <> struct MixVec<bf16> { typedef bf16x8 v; static constexpr int n = 8; };
template <> struct MixVec<f16> { typedef f16x8 v; static constexpr int n = 8; };

template <typename T> __device__ __forceinline__ T blend1(T a, T b, float lam, float oml) {
  return from_f<T>(fmaf(lam, to_f<T>(a), oml * to_f<T>(b)));   // fp32 on the stored values, one rounding to storage
}

// element offset of item `it` inside a clip and how many of its VEC elements exist
template <int VEC> __device__ __forceinline__ long long mix_locate(const MixGeom& g, long long it, int& nv) {
  if (g.R1) {
    const long long e = it * VEC;
    nv = (int)min((long long)VEC, g.L - e);
    return g.off0 + e;
  }
  const long long r = it / g.nvr, v = it - r * g.nvr;
  const long long t = r / g.bh, y = r - t * g.bh;
  const long long e = v * VEC;
  nv = (int)min((long long)VEC, g.L - e);
  return g.off0 + t * g.t_stride + y * g.row_stride + e;
}

template <typename T, int OP>
__device__ __forceinline__ void mix_item(const T* xa, const T* xb, T* oa, T* ob, long long off, int nv, float lam, float oml) {
  typedef typename MixVec<T>::v V;
  constexpr int VEC = MixVec<T>::n;
  if (nv == VEC) {
    if constexpr (OP == MIX_OP_COPY) {
      *(V*)(oa + off) = *(const V*)(xa + off);
    } else {
      const V a = *(const V*)(xa + off), b = *(const V*)(xb + off);
      if constexpr (OP == MIX_OP_SWAP) {
        *(V*)(oa + off) = b;
        *(V*)(ob + off) = a;
      } else {
        V ra, rb;
#pragma unroll
        for (int e = 0; e < VEC; e++) { ra[e] = blend1<T>(a[e], b[e], lam, oml); rb[e] = blend1<T>(b[e], a[e], lam, oml); }
        *(V*)(oa + off) = ra;
        *(V*)(ob + off) = rb;
      }
    }
  } else {
    for (int e = 0; e < nv; e++) {
      if constexpr (OP == MIX_OP_COPY) {
        oa[off + e] = xa[off + e];
      } else {
        const T a = xa[off + e], b = xb[off + e];
        if constexpr (OP == MIX_OP_SWAP) { oa[off + e] = b; ob[off + e] = a; }
        else { oa[off + e] = blend1<T>(a, b, lam, oml); ob[off + e] = blend1<T>(b, a, lam, oml); }
      }
    }
  }
}

template <typename T, int OP>
__global__ __launch_bounds__(MIX_THREADS) void mix_clips_kernel(const T* x, T* out, int nclips, MixGeom g, float lam, float oml) {
  typedef typename MixVec<T>::v V;
  constexpr int VEC = MixVec<T>::n;
  const int i = blockIdx.y, j = nclips - 1 - i;
  const T* xa = x + (long long)i * g.E;
  const T* xb = x + (long long)j * g.E;
  T* oa = out + (long long)i * g.E;
  T* ob = out + (long long)j * g.E;
  const long long stride = (long long)gridDim.x * MIX_THREADS;
  if (OP != MIX_OP_COPY && i == j) {
    // the middle clip of an odd batch is its own partner: bit-identical (a blend of a value with itself is not, in general)
    if (OP == MIX_OP_SWAP || oa == xa) return;       // (a swap is preceded by a copy of the batch when out != x)
    for (long long it = (long long)blockIdx.x * MIX_THREADS + threadIdx.x; it < g.items; it += stride) {
      int nv;
      const long long off = mix_locate<VEC>(g, it, nv);
      mix_item<T, MIX_OP_COPY>(xa, xb, oa, ob, off, nv, lam, oml);
    }
    return;
  }
  // two items per trip, all loads in front of the stores (out may be x: the compiler cannot move them itself)
  for (long long it = (long long)blockIdx.x * MIX_THREADS + threadIdx.x; it < g.items; it += 2 * stride) {
    int n0, n1 = 0;
    const long long o0 = mix_locate<VEC>(g, it, n0);
    const long long it1 = it + stride;
    long long o1 = 0;
    if (it1 < g.items) o1 = mix_locate<VEC>(g, it1, n1);
    if (n0 == VEC && n1 == VEC) {
      if constexpr (OP == MIX_OP_COPY) {
        const V a0 = *(const V*)(xa + o0), a1 = *(const V*)(xa + o1);
        *(V*)(oa + o0) = a0;
        *(V*)(oa + o1) = a1;
      } else {
        const V a0 = *(const V*)(xa + o0), b0 = *(const V*)(xb + o0);
        const V a1 = *(const V*)(xa + o1), b1 = *(const V*)(xb + o1);
        if constexpr (OP == MIX_OP_SWAP) {
          *(V*)(oa + o0) = b0; *(V*)(ob + o0) = a0;
          *(V*)(oa + o1) = b1; *(V*)(ob + o1) = a1;
        } else {
          V ra0, rb0, ra1, rb1;
#pragma unroll
          for (int e = 0; e < VEC; e++) {
            ra0[e] = blend1<T>(a0[e], b0[e], lam, oml); rb0[e] = blend1<T>(b0[e], a0[e], lam, oml);
            ra1[e] = blend1<T>(a1[e], b1[e], lam, oml); rb1[e] = blend1<T>(b1[e], a1[e], lam, oml);
          }
          *(V*)(oa + o0) = ra0; *(V*)(ob + o0) = rb0;
          *(V*)(oa + o1) = ra1; *(V*)(ob + o1) = rb1;
        }
      }
    } else {
      mix_item<T, OP>(xa, xb, oa, ob, o0, n0, lam, oml);
      if (n1 > 0) mix_item<T, OP>(xa, xb, oa, ob, o1, n1, lam, oml);
    }
  }
}

template <typename T, int OP>
static int mix_launch(const void* x, void* out, int nclips, int rows, MixGeom g, float lam, hipStream_t st, const char* what) {
  constexpr int VEC = MixVec<T>::n;
  g.nvr = (g.L + VEC - 1) / VEC;
  g.items = g.R * g.nvr;
  const long long per_row = ceil_div_ll(g.items, 2 * MIX_THREADS);
  long long gx = MIX_MAX_BLOCKS / rows;
  if (gx < 1) gx = 1;
  if (gx > per_row) gx = per_row;
  hipLaunchKernelGGL((mix_clips_kernel<T, OP>), dim3((unsigned)gx, (unsigned)rows), dim3(MIX_THREADS), 0, st, (const T*)x,
                     (T*)out, nclips, g, lam, 1.0f - lam);
  X3D_LAUNCH_CHECK(what);
  return X3D_OK;
}

template <int OP>
static int mix_dispatch(int dtype, const void* x, void* out, int nclips, int rows, const MixGeom& g, float lam, hipStream_t st,
                        const char* what) {
  if (dtype == X3D_F32) return mix_launch<float, OP>(x, out, nclips, rows, g, lam, st, what);
  if (dtype == X3D_BF16) return mix_launch<bf16, OP>(x, out, nclips, rows, g, lam, st, what);
  return mix_launch<f16, OP>(x, out, nclips, rows, g, lam, st, what);
}

extern "C" int x3d_mix_clips(const void* x, void* out, int mode, float lam, int y0, int y1, int x0, int x1, int N, int T,
                             int H, int W, int C, int dtype, void* stream) {
  X3D_REQUIRE(x && out, "mix_clips: null pointer");
  X3D_REQUIRE(N > 0 && T > 0 && H > 0 && W > 0 && C > 0, "mix_clips: bad extents N=%d T=%d H=%d W=%d C=%d", N, T, H, W, C);
  X3D_REQUIRE(x3d_dtype_ok(dtype), "mix_clips: unknown dtype %d", dtype);
  X3D_REQUIRE(mode == X3D_MIX_MIXUP || mode == X3D_MIX_CUTMIX, "mix_clips: unknown mode %d", mode);
  X3D_REQUIRE(lam >= 0.f && lam <= 1.f, "mix_clips: lam = %g is not in [0, 1]", (double)lam);   // (false for NaN too)
  if (mode == X3D_MIX_CUTMIX)
    X3D_REQUIRE(0 <= y0 && y0 <= y1 && y1 <= H && 0 <= x0 && x0 <= x1 && x1 <= W,
                "mix_clips: box [%d, %d) x [%d, %d) outside the %d x %d frame", y0, y1, x0, x1, H, W);
  const int pairs = (N + 1) / 2;
  X3D_REQUIRE(pairs <= 65535, "mix_clips: N = %d clips (at most 131070)", N);
  const long long E = (long long)T * H * W * C;
  const int es = dtype == X3D_F32 ? 4 : 2;
  const unsigned long long bytes = (unsigned long long)N * (unsigned long long)E * es;
  const uintptr_t xa = (uintptr_t)x, oa = (uintptr_t)out;
  X3D_REQUIRE(xa == oa || xa + bytes <= oa || oa + bytes <= xa, "mix_clips: out overlaps x without being equal to it");
  X3D_REQUIRE(xa % es == 0 && oa % es == 0, "mix_clips: pointers not aligned to the element size");
  hipStream_t st = (hipStream_t)stream;
  MixGeom g;
  memset(&g, 0, sizeof(g));
  g.E = E;
  g.R1 = 1;
  g.R = 1;
  g.bh = 1;

  bool swap = false;
  if (mode == X3D_MIX_MIXUP) {
    if (lam > 0.f && lam < 1.f) {
      g.L = E;
      return mix_dispatch<MIX_OP_BLEND>(dtype, x, out, N, pairs, g, lam, st, "mix_clips");
    }
    if (lam == 0.f) { swap = true; y0 = 0; y1 = H; x0 = 0; x1 = W; }   // the reversed batch, bit for bit
  } else {
    swap = y1 > y0 && x1 > x0;
  }
  if (xa != oa) {                 // everything outside the box (lam = 1, an empty box: everything) is copied
    MixGeom c = g;
    c.E = 0;                      // one "clip": the whole batch as one range
    c.L = (long long)N * E;
    const int rc = mix_dispatch<MIX_OP_COPY>(dtype, x, out, 1, 1, c, lam, st, "mix_clips (copy)");
    if (rc != X3D_OK) return rc;
  }
  if (!swap || N < 2) return X3D_OK;
  const long long row = (long long)W * C;
  if (x0 == 0 && x1 == W && y0 == 0 && y1 == H) {
    g.L = E;
  } else if (x0 == 0 && x1 == W) {          // the box spans the width: one range per frame
    g.R1 = 0; g.bh = 1; g.R = T;
    g.L = (long long)(y1 - y0) * row;
    g.t_stride = (long long)H * row; g.row_stride = 0; g.off0 = (long long)y0 * row;
  } else {                                  // one range per box row
    g.R1 = 0; g.bh = y1 - y0; g.R = (long long)T * g.bh;
    g.L = (long long)(x1 - x0) * C;
    g.t_stride = (long long)H * row; g.row_stride = row; g.off0 = (long long)y0 * row + (long long)x0 * C;
  }
  return mix_dispatch<MIX_OP_SWAP>(dtype, x, out, N, N / 2, g, lam, st, "mix_clips (box)");
}

// ------------------------------------------------------------------------------------------------
// x3d_mix_targets: the soft targets of a mixed batch, built where the labels are.  One workgroup per pair (i, N-1-i) writes
// both rows (so targets may be mixed in place); the arithmetic is fp64, rounded once to fp32.
// ------------------------------------------------------------------------------------------------
#define MIXT_THREADS 256
__global__ __launch_bounds__(MIXT_THREADS) void mix_targets_kernel(const int* __restrict__ labels, const float* targets,
                                                                   float* out, int* hard, float lam_f, float eps_f, int N,
                                                                   int M) {
  const int i = blockIdx.x, j = N - 1 - i, tid = threadIdx.x;
  const double lam = (double)lam_f, oml = 1.0 - lam;
  float* yi = out + (long long)i * M;
  float* yj = out + (long long)j * M;
  if (labels) {
    const int li = labels[i], lj = labels[j];
    if (hard && tid == 0) {
      hard[i] = lam_f >= 0.5f ? li : lj;
      hard[j] = lam_f >= 0.5f ? lj : li;
    }
    // a label outside [0, M) is never used as an index: both rows that contain it are NaN (the loss is visibly non-finite)
    const bool bad = li < 0 || li >= M || lj < 0 || lj >= M;
    const double eps = (double)eps_f, on = 1.0 - eps, base = eps / (double)M;
    for (int k = tid; k < M; k += MIXT_THREADS) {
      const double si = (k == li ? on : 0.0) + base, sj = (k == lj ? on : 0.0) + base;
      float vi = (float)(lam * si + oml * sj), vj = (float)(lam * sj + oml * si);
      if (i == j) vi = vj = (float)si;
      if (bad) vi = vj = __builtin_nanf("");
      yi[k] = vi;
      yj[k] = vj;
    }
  } else {
    const float* ti = targets + (long long)i * M;
    const float* tj = targets + (long long)j * M;
    for (int k = tid; k < M; k += MIXT_THREADS) {
      const float a = ti[k], b = tj[k];            // both read before either is written: in place
      float vi = (float)(lam * (double)a + oml * (double)b), vj = (float)(lam * (double)b + oml * (double)a);
      if (i == j) vi = vj = a;
      yi[k] = vi;
      yj[k] = vj;
    }
  }
}

extern "C" int x3d_mix_targets(const int* labels, const float* targets, float* out, int* hard, float lam, float eps, int N,
                               int M, void* stream) {
  X3D_REQUIRE(out && N > 0 && M > 0, "mix_targets: bad args (N=%d M=%d)", N, M);
  X3D_REQUIRE((labels != nullptr) != (targets != nullptr), "mix_targets: exactly one of labels / targets");
  X3D_REQUIRE((long long)N * M < (1LL << 31), "mix_targets: N*M = %lld >= 2^31", (long long)N * M);
  X3D_REQUIRE(lam >= 0.f && lam <= 1.f, "mix_targets: lam = %g is not in [0, 1]", (double)lam);
  if (labels) {
    X3D_REQUIRE(eps >= 0.f && eps < 1.f, "mix_targets: eps = %g is not in [0, 1)", (double)eps);
    X3D_REQUIRE((const void*)hard != (const void*)labels, "mix_targets: hard must not be the labels themselves");
  } else {
    X3D_REQUIRE(eps == 0.f, "mix_targets: label smoothing (eps = %g) is defined for class labels only", (double)eps);
    X3D_REQUIRE(!hard, "mix_targets: hard labels exist for class labels only");
    const uintptr_t ta = (uintptr_t)targets, oa = (uintptr_t)out;
    const unsigned long long bytes = (unsigned long long)N * M * sizeof(float);
    X3D_REQUIRE(ta == oa || ta + bytes <= oa || oa + bytes <= ta, "mix_targets: out overlaps targets without being equal to it");
  }
  hipLaunchKernelGGL(mix_targets_kernel, dim3((N + 1) / 2), dim3(MIXT_THREADS), 0, (hipStream_t)stream, labels, targets, out,
                     hard, lam, eps, N, M);
  X3D_LAUNCH_CHECK("mix_targets");
  return X3D_OK;
}
