// The tile pipeline the two weights-stationary FUSED backward kernels of the stage-4/5 pointwise convs share
// (pw_bwd_wst.hip: the `c` conv, pw_bwd_wsta.hip: the `a` conv).  One persistent 8-wave workgroup per CU walks a run of
// 32-point tiles:
//   * dX = W^T dY as in pw_gemm_wst.h: a dX wave holds the 32 x Kp weight block of its input channels in REGISTERS
//     (KS x 4 VGPRs); the dY tile [Co][32 points] is staged once -- BN-backward prologue in fp32 -- into LDS in two
//     layouts: [k][32] for the transposed B-operand read of dX, and [co][32 + 8] for the row-wise A-operand read of dW;
//   * the epilogue of a dX wave goes through its private slab (lane -> row lane >> 1, 16 points) and ends in bounds-checked
//     buffer stores of dx;
//   * the dW accumulators live across all tiles of the workgroup and are flushed once.
// What a kernel adds is its epilogue, the second dW operand and which wave owns which dW tiles.  The rules both keep:
//   * ONE barrier per tile (the double-buffered dY tile); g / yraw are prefetched two tiles ahead in registers, the
//     epilogue operands one;
//   * every load of the tile loop is UNCONDITIONAL (clamped address, value selected afterwards): vmcnt retires in order, so
//     a load issued behind the prefetches -- or a conditional one the compiler cannot count -- turns the wait in front of
//     the epilogue into vmcnt(0), i.e. a full memory latency per tile (r03h: 104 us).  A per-tile scalar operand (the SE
//     gate) travels with the vector prefetch for the same reason.
// Every piece below compiles to the instructions of the text it replaced in the two kernels (all eight instantiations were
// compared, <., 7, 12, 6> sits at 256 VGPRs without scratch).  Two loops stay in the kernels because of that: the slab write
// and the loops of the dW flush.  A function is unrolled on its own before it is inlined; that pairs the slab's ds_writes
// differently (TAIL = 1 of the `a` kernel then spills 12 bytes per lane) and moves the waits of the <., 7, 12, 6> tile loop.
// bws_commit_dy takes its operands by reference for the same reason.
#pragma once
#include <stdlib.h>

#include <initializer_list>

#include "pw_gemm_ws.h"

struct PwBwdWsArgs {
  const void* g; const void* yraw; const float* coef;   // dY = A*g + B*yraw + C   rows = Co
  const void* wp; int wp_rows;                          // dgrad panel (tiled image behind the row-major one)
  void* dx;                                             // [N][Ci][P]
  float* dw;                                            // [Co][Ci]
  int N, Co, Ci;
  long long P;
  int tiles_per_block;
  BnBwdFold fold;                                       // sums != NULL: the coefficient table is derived from the BatchNorm-backward sums here (x3d_hip.h coef_fold)
  float* slab;                                          // NULL | per-workgroup partial dW slabs [gridDim.x][Co][Ci] (plain stores)
  int hot;                                              // experiments build only (X3D_PW_BWD_HOT=1): every tile load re-reads the FIRST tile (cache hits): what memory latency costs
  int noflush;                                          // experiments build only (X3D_PW_BWD_NOFLUSH=1): timing without the dW flush
};

#define BWS_BN 32    // points per tile
#define BWS_NT 512   // threads per workgroup
#define BWS_RP 40    // pitch (elements) of the row-read tiles: 80 B = 5 units, odd -> b128 rows conflict-free
constexpr int bws_nsv(int Kp) { return (Kp * 4 + BWS_NT - 1) / BWS_NT; }   // dY staging vectors (8 points) per thread and tensor

// ---- this workgroup's run of tiles
struct BwsTiles { int per_n, begin, end; };
__device__ __forceinline__ BwsTiles bws_tiles(const PwBwdWsArgs& a) {
  BwsTiles t;
  t.per_n = (int)((a.P + BWS_BN - 1) / BWS_BN);
  const int total_tiles = t.per_n * a.N;
  t.begin = blockIdx.x * a.tiles_per_block;
  t.end = min(t.begin + a.tiles_per_block, total_tiles);
  return t;
}
// sample and first point of a tile
__device__ __forceinline__ void bws_tile_pos(const BwsTiles& t, int tile, int& n, long long& p0) {
  n = tile / t.per_n;
  p0 = (long long)(tile - n * t.per_n) * BWS_BN;
}
// ... of the tile a prefetch reads: past the end of the run it re-reads the last tile (the load stays unconditional)
__device__ __forceinline__ void bws_load_pos(const PwBwdWsArgs& a, const BwsTiles& t, int tile_, int& n, long long& p0) {
  const int tile = a.hot ? t.begin : min(tile_, t.end - 1);
  bws_tile_pos(t, tile, n, p0);
}

// ---- one-time set-up: zero `nvec` 16-byte vectors at `rows` (the row-read tiles: their padding rows stay zero), fill the
// BN-backward coefficient table Cs [Kp][4]
template <typename H, int Kp>
__device__ __forceinline__ void bws_setup(const PwBwdWsArgs& a, H* rows, int nvec, float* Cs, int tid) {
  typedef typename HV<H>::x8 hx8;
  hx8 z;
#pragma unroll
  for (int e = 0; e < 8; e++) z[e] = (H)0.f;
  for (int i = tid; i < nvec; i += BWS_NT) ((hx8*)rows)[i] = z;
  for (int k = tid; k < Kp; k += BWS_NT) {
    f32x4 c = {0.f, 0.f, 0.f, 0.f};
    if (k < a.Co) {
      float cA_, cB_, cC_;
      bn_bwd_coef_load(a.coef, a.fold, k, blockIdx.x == 0 && blockIdx.y == 0, cA_, cB_, cC_);
      c[0] = cA_; c[1] = cB_; c[2] = cC_;
    }
    *(f32x4*)&Cs[k * 4] = c;
  }
}

// ---- the stationary operand: W^T rows (input channels) 32 * rb .., all Kp output channels (zero for a wave that owns none)
template <typename H, int KS>
__device__ __forceinline__ void bws_load_weights(const PwBwdWsArgs& a, int rb, bool own, int lane, typename HV<H>::x8 (&A)[KS]) {
  typedef typename HV<H>::x8 hx8;
  constexpr int WP = KS * 16 + 8;
  if (own) {
    const H* wt = (const H*)a.wp + (long long)a.wp_rows * WP + ((long long)rb * KS * 64 + lane) * 8;
#pragma unroll
    for (int ks = 0; ks < KS; ks++) A[ks] = *(const hx8*)(wt + ks * 512);
  } else {
#pragma unroll
    for (int ks = 0; ks < KS; ks++)
#pragma unroll
      for (int e = 0; e < 8; e++) A[ks][e] = (H)0.f;
  }
}

// ---- dY staging: vector v = tid + NT * i -> row v >> 2, 8 points at unit v & 3 (unconditional clamped loads)
template <typename H, int Kp>
__device__ __forceinline__ void bws_issue_dy(const PwBwdWsArgs& a, int n, long long p0, int tid, typename HV<H>::x8 (&gr)[bws_nsv(Kp)],
                                             typename HV<H>::x8 (&yr)[bws_nsv(Kp)]) {
  typedef typename HV<H>::x8 hx8;
#pragma unroll
  for (int i = 0; i < bws_nsv(Kp); i++) {
    const int v = tid + i * BWS_NT;
    const int k = v >> 2;
    const long long p = p0 + (v & 3) * 8;
    const bool ok = k < a.Co && p < a.P;
    const long long o = ok ? ((long long)n * a.Co + k) * a.P + p : 0;
    gr[i] = *(const hx8*)((const H*)a.g + o);
    yr[i] = *(const hx8*)((const H*)a.yraw + o);
  }
}
// ... BN-backward prologue in fp32, then into buffer `buf` of Yt [2][Kp][32] and of Yr [2][CoP][BWS_RP]
template <typename H, int Kp, int CoP>
__device__ __forceinline__ void bws_commit_dy(const PwBwdWsArgs& a, const long long& p0, const int& buf, const int& tid, float* const& Cs, H* const& Yt, H* const& Yr,
                                              const typename HV<H>::x8 (&gr)[bws_nsv(Kp)], const typename HV<H>::x8 (&yr)[bws_nsv(Kp)]) {
  typedef typename HV<H>::x8 hx8;
  static_assert(CoP >= Kp, "the row-read copy covers every staged dY row");
#pragma unroll
  for (int i = 0; i < bws_nsv(Kp); i++) {
    const int v = tid + i * BWS_NT;
    const int k = v >> 2;
    if (k >= Kp) continue;
    const bool ok = k < a.Co && p0 + (v & 3) * 8 < a.P;
    const f32x4 cf = *(const f32x4*)&Cs[k * 4];
    hx8 hv;
#pragma unroll
    for (int e = 0; e < 8; e++) hv[e] = (H)(ok ? cf[0] * (float)gr[i][e] + cf[1] * (float)yr[i][e] + cf[2] : 0.f);   // (C must not leak into the padding)
    *(hx8*)&Yt[(buf * Kp + k) * BWS_BN + (v & 3) * 8] = hv;
    *(hx8*)&Yr[(buf * CoP + k) * BWS_RP + (v & 3) * 8] = hv;
  }
}

// ---- dX = W^T dY: B operand from the dY tile yt [Kp][32] by transposed reads at this lane's offset, A from registers
__device__ __forceinline__ int bws_tr_off(int lane) {
  const int g16 = lane >> 4, q = (lane & 15) >> 2, pp = lane & 3;
  return (8 * (g16 >> 1) + q) * BWS_BN + 16 * (g16 & 1) + 4 * pp;
}
template <typename H, int KS>
__device__ __forceinline__ f32x16 bws_dx(const typename HV<H>::x8 (&A)[KS], const H* yt, int tr_off, bool own) {
  typedef typename HV<H>::x8 hx8;
  typedef s16x4 __attribute__((address_space(3))) * lds_s16x4_ptr;
  f32x16 acc;
#pragma unroll
  for (int e = 0; e < 16; e++) acc[e] = 0.f;
  if (own) {
    const H* xb = yt + tr_off;
#pragma unroll
    for (int ks = 0; ks < KS; ks++) {
      const s16x4 b0 = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_s16x4_ptr)(xb + ks * 16 * BWS_BN));
      const s16x4 b1 = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_s16x4_ptr)(xb + (ks * 16 + 4) * BWS_BN));
      const s16x8 bs = {b0[0], b0[1], b0[2], b0[3], b1[0], b1[1], b1[2], b1[3]};
      acc = mfma16<H>(A[ks], __builtin_bit_cast(hx8, bs), acc);
    }
  }
  return acc;
}

// ---- row of element e of a 32 x 32 MFMA accumulator (column: r = lane & 31, half = lane >> 5)
__device__ __forceinline__ int bws_acc_row(int e, int half) { return (e & 3) + 8 * (e >> 2) + 4 * half; }

// ---- epilogue through the wave-private slab [32][WS_OP], written in the accumulator layout: 8 points of row `row` at `col`
__device__ __forceinline__ void bws_slab_read(const float* myOs, int row, int col, float (&val)[8]) {
  const f32x4 v0 = *(const f32x4*)&myOs[row * WS_OP + col], v1 = *(const f32x4*)&myOs[row * WS_OP + col + 4];
#pragma unroll
  for (int e = 0; e < 4; e++) { val[e] = v0[e]; val[4 + e] = v1[e]; }
}

// ---- dx stores as bounds-checked buffer stores (offset past the sample's [Ci][P] matrix = dropped): a static count per tile
template <typename H>
__device__ __forceinline__ __amdgpu_buffer_rsrc_t bws_dx_rsrc(const PwBwdWsArgs& a, int n) {
  return __builtin_amdgcn_make_buffer_rsrc((H*)a.dx + (long long)n * a.Ci * a.P, 0, (int)((long long)a.Ci * a.P * 2), 0x00020000);
}
template <typename H>
__device__ __forceinline__ void bws_store_dx(const PwBwdWsArgs& a, __amdgpu_buffer_rsrc_t dxr, const float (&val)[8], bool ok, int m,
                                             long long p) {
  typedef __attribute__((ext_vector_type(4))) unsigned int u32x4_;
  typename HV<H>::x8 ov;
#pragma unroll
  for (int e = 0; e < 8; e++) ov[e] = (H)val[e];
  __builtin_amdgcn_raw_buffer_store_b128(__builtin_bit_cast(u32x4_, ov), dxr, ok ? (unsigned)(((long long)m * a.P + p) * 2) : 0x80000000u,
                                         0, 0);
}

// ---- dW partial -> this workgroup's slab (plain stores, added up by a later launch: x3d_hip.h dw_slab), or -> dw by fp32
// atomics.  256 workgroups x 83 KB of device-scope atomics take 17-24 us of this ~100 us launch whatever the schedule
// (they execute at the memory side at ~1.3 TB/s chip-wide); the same bytes as stores ~4 us.
// bws_flush_dw: ONE element of a wave's 32 x 32 tiles [co][ci], co = 32 * cot + bws_acc_row(e, half), ci = 32 * cit + r.
__device__ __forceinline__ float* bws_dw_slab(const PwBwdWsArgs& a) {
  return a.slab ? a.slab + (long long)blockIdx.x * a.Co * a.Ci : nullptr;
}
__device__ __forceinline__ void bws_flush_dw(const PwBwdWsArgs& a, float* slab, int co, int ci, float v) {
  if (co < a.Co && ci < a.Ci) {
    if (slab) slab[(long long)co * a.Ci + ci] = v;
    else atomicAdd(&a.dw[(long long)co * a.Ci + ci], v);
  }
}

// ---- host side
// what both kernels ask of a launch: 16-bit storage, the dgrad panel, a coefficient source, whole 8-point vectors, 32-bit
// point indices, one sample's dx inside the 2 GB buffer-store window, and 16-byte alignment of every tensor in `ps`
static inline bool bws_applies(const x3d_pw_bwd_args* b, std::initializer_list<const void*> ps) {
  if (!x3d_is_half(b->dtype) || !b->w_panel || (!b->coef && !b->coef_fold) || !b->yraw) return false;
  const long long P = (long long)b->T * b->H * b->W;
  if (P % 8 || P >= (1ll << 31) || (long long)b->Cin * P * 2 >= (1ll << 31)) return false;
  for (const void* p : ps) if (!p || ((uintptr_t)p % 16)) return false;
  return true;
}

static inline void bws_fill_args(PwBwdWsArgs& a, const x3d_pw_bwd_args* b) {
  a.g = b->g; a.yraw = b->yraw; a.coef = b->coef;
  a.wp = b->w_panel; a.wp_rows = (b->Cin + 31) & ~31;
  a.dx = b->dx; a.dw = b->dw; a.slab = b->dw_slab; a.fold = bn_bwd_fold_arg(b->coef_fold);
  a.N = b->N; a.Co = b->Cout; a.Ci = b->Cin;
  a.P = (long long)b->T * b->H * b->W;
}

// the persistent grid of each of `slices` workgroup sets over blockIdx.y (also what x3d_pw_bwd_dw_parts reports: one slab per
// blockIdx.x)
static inline void bws_grid(int N, long long P, int slices, long long* tpb, long long* gx) {
  x3d_persistent_grid(ceil_div_ll(P, 32) * N, x3d_device_cus() / slices, tpb, gx);
}

// `name`: of the entry point, for messages; `fmt`...: the instantiation's name for the dry-run dispatch
template <auto KERN, typename Args, typename... D>
static int bws_launch(Args& a, size_t lds, int slices, hipStream_t st, const char* name, const char* fmt, D... d) {
  X3D_DESCRIBE(fmt, d...);
  static bool attr_set = false;
  if (!attr_set) {
    (void)hipFuncSetAttribute((const void*)KERN, hipFuncAttributeMaxDynamicSharedMemorySize, 128 * 1024);
    attr_set = true;
  }
  const long long total_tiles = ceil_div_ll(a.P, 32) * a.N;
  X3D_REQUIRE(total_tiles < (1ll << 31), "%s: too many tiles", name);
  long long tpb, gx;
  bws_grid(a.N, a.P, slices, &tpb, &gx);
  a.tiles_per_block = (int)tpb;
  a.noflush = x3d_env_int("X3D_PW_BWD_NOFLUSH", 0);
  a.hot = x3d_env_int("X3D_PW_BWD_HOT", 0);
  hipLaunchKernelGGL(KERN, dim3((unsigned)gx, (unsigned)slices), dim3(BWS_NT), lds, st, a);
  X3D_LAUNCH_CHECK(name);
  return X3D_OK;
}
