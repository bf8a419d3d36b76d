// Weights-stationary FUSED backward of the stage-4 `c` conv (216 inner channels <-> 96 block channels on 14 x 14 planes;
// reference model.py:292-299 through SURVEY appendix A): data gradient with the swish' epilogue + per-(n, c) sums AND the
// weight gradient, one pass over g / yraw / braw.
//
// The sliced fused kernel (pw_bwd_fused.hip) covers Ci = 216 with four 64-channel slices over blockIdx.y, each re-staging
// the dY tile (PMC traffic 1.4x of the algorithmic bytes), at 247 VGPRs and seven barriers per tile: 107 us per layer, the
// largest single item of the X3D-M backward pass (11 launches).  Here ONE persistent 8-wave workgroup per CU owns ALL input
// channels, on the tile pipeline of pw_bwd_ws.h (dY staging, dX = W^T dY with wave w on input channels 32w.., slab, dx
// stores, dW flush; its rules for the tile loop hold for the loads added here).  What this file adds:
//   * epilogue per wave through its private slab: u = gate * bn_b(braw), dv = dX * swish'(u) -> HBM, the per-(n, c) sums,
//     and Xh = swish(u) -> LDS rows 32w.. of the Xh tile;
//   * dW[co][ci] += dY[co][:] . Xh[ci][:]: wave w owns the CT tiles of ITS OWN input channels (cit = w), so the B operand
//     it reads is what it just wrote: no barrier between epilogue and weight-gradient MFMAs; CT x 16 accumulator VGPRs live
//     across all tiles of the workgroup, flushed once with fp32 atomics.
// braw is prefetched one tile ahead in registers, and the SE gate travels with it.
#include "pw_bwd_ws.h"

struct PwBwdWstArgs : PwBwdWsArgs {
  const void* braw; const float* b_ss; const float* egate; double* nc_sums;
};

template <typename H, int NW, int KS, int CT>
__global__ __launch_bounds__(512, 2) void pw_bwd_wst_kernel(const PwBwdWstArgs a) {
  typedef typename HV<H>::x8 hx8;
  extern __shared__ __attribute__((aligned(16))) unsigned char smem_raw[];
  typedef H T;
  constexpr int BN = BWS_BN, OP = WS_OP, Kp = KS * 16, CoP = CT * 32, YRP = BWS_RP;   // (the Xh tile has the row-read copy's pitch)
  constexpr int NSV = bws_nsv(Kp);
  H* Yt = (H*)smem_raw;                                                          // [2][Kp][32]
  H* Yr = (H*)(smem_raw + (size_t)2 * Kp * 64);                                  // [2][CoP][YRP]
  H* Xh = (H*)(smem_raw + (size_t)2 * Kp * 64 + (size_t)2 * CoP * YRP * 2);      // [NW * 32][YRP]
  float* Cs = (float*)(smem_raw + (size_t)2 * Kp * 64 + (size_t)2 * CoP * YRP * 2 + (size_t)NW * 32 * YRP * 2);   // [Kp][4]
  float* Os = Cs + Kp * 4;                                                       // [NW][32][OP]
  const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
  const int r = lane & 31, half = lane >> 5;
  const int mt = (a.Ci + 31) >> 5;
  const BwsTiles t = bws_tiles(a);
  if (t.begin >= t.end) return;                        // (never: the grid has no empty workgroup -- a slab would stay unwritten)
  float* myOs = Os + wid * 32 * OP;
  // input channels beyond NW row blocks: SLICES over blockIdx.y (stage 5: 432 = 2 x 7 row blocks), each slice a persistent
  // workgroup set of its own that re-stages the dY tile (K = Co rows) for its NW x 32 input channels
  const int rb = blockIdx.y * NW + wid;                // this wave's row block of input channels
  const bool mw = wid < NW && rb < mt;                 // ... if it owns one

  bws_setup<H, Kp>(a, Yr, 2 * CoP * YRP / 8, Cs, tid);   // zeroes the row-read copies' padding rows (Kp.. CoP)
  hx8 A[KS];
  bws_load_weights<H, KS>(a, rb, mw, lane, A);

  hx8 g0[NSV], y0[NSV], g1[NSV], y1[NSV];
  auto issue_loads = [&](int tile_, hx8 (&gr)[NSV], hx8 (&yr)[NSV]) {
    int n;
    long long p0;
    bws_load_pos(a, t, tile_, n, p0);
    bws_issue_dy<H, Kp>(a, n, p0, tid, gr, yr);
  };
  auto commit = [&](int tile, int buf, const hx8 (&gr)[NSV], const hx8 (&yr)[NSV]) {
    int n;
    long long p0;
    bws_tile_pos(t, tile, n, p0);
    bws_commit_dy<H, Kp, CoP>(a, p0, buf, tid, Cs, Yt, Yr, gr, yr);
  };

  // ---- braw prefetch (one tile ahead): lane -> row lane >> 1 of this wave's block, points 16 * (lane & 1) .. + 15
  const int row = lane >> 1, c0 = 16 * (lane & 1);
  const int m = rb * 32 + row;                         // this lane's input channel
  const bool mrow = mw && m < a.Ci;
  hx8 eb0[2], eb1[2];
  float gl0, gl1;
  const float* gsrc = a.egate ? a.egate : a.b_ss;      // (no SE: any valid address, the value is not used)
  auto issue_braw = [&](int tile_, hx8 (&eb)[2], float& gl) {
    int n;
    long long p0;
    bws_load_pos(a, t, tile_, n, p0);
    gl = gsrc[(a.egate && mrow) ? (long long)n * a.Ci + m : 0];
#pragma unroll
    for (int hv = 0; hv < 2; hv++) {
      const long long p = p0 + c0 + 8 * hv;
      const long long o = (mrow && p < a.P) ? ((long long)n * a.Ci + m) * a.P + p : 0;
      eb[hv] = *(const hx8*)((const T*)a.braw + o);
    }
  };

  float st1 = 0.f, st2 = 0.f;                          // per-(sample, channel) sums of this lane's row
  auto flush_sums = [&](int n) {
    const float s1 = st1 + dpp_get<0xB1, 0xF>(st1), s2 = st2 + dpp_get<0xB1, 0xF>(st2);   // the two lanes of a row
    if (mrow && (lane & 1) == 0) {
      double* d = a.nc_sums + ((long long)n * a.Ci + m) * 2;
      atomic_add_d(d, (double)s1);
      atomic_add_d(d + 1, (double)s2);
    }
    st1 = 0.f;
    st2 = 0.f;
  };
  const float sb = mrow ? a.b_ss[m * 2] : 0.f, tb = mrow ? a.b_ss[m * 2 + 1] : 0.f;

  f32x16 acc_dw[CT];
#pragma unroll
  for (int s = 0; s < CT; s++)
#pragma unroll
    for (int e = 0; e < 16; e++) acc_dw[s][e] = 0.f;

  const int tr_off = bws_tr_off(lane);

  int n_prev = t.begin / t.per_n;
  issue_loads(t.begin, g0, y0);
  issue_braw(t.begin, eb0, gl0);
  __syncthreads();                                     // coefficient table, zeroed padding
  commit(t.begin, 0, g0, y0);
  __syncthreads();
  issue_loads(t.begin + 1, g1, y1);
  issue_loads(t.begin + 2, g0, y0);

  auto step = [&](int tile, int cur, hx8 (&gr)[NSV], hx8 (&yr)[NSV], hx8 (&eb)[2], float gl, hx8 (&ebn)[2], float& gln) {
    int n;
    long long p0;
    bws_tile_pos(t, tile, n, p0);
    if (n != n_prev) flush_sums(n_prev);
    n_prev = n;
    issue_braw(tile + 1, ebn, gln);                    // a whole step to land
    const float gt = (mrow && a.egate) ? gl : 1.0f;
    __amdgpu_buffer_rsrc_t dxr = bws_dx_rsrc<T>(a, n);

    const f32x16 acc = bws_dx<H, KS>(A, Yt + cur * (Kp * BN), tr_off, mw);

    // ---- the next dY tile goes into the other buffer (before the epilogue: its wait covers loads only)
    if (tile + 1 < t.end) commit(tile + 1, cur ^ 1, gr, yr);

    if (mw) {
      // ---- epilogue through the wave-private slab
#pragma unroll
      for (int e = 0; e < 16; e++) myOs[bws_acc_row(e, half) * OP + r] = acc[e];
#pragma unroll
      for (int hv = 0; hv < 2; hv++) {
        const long long p = p0 + c0 + 8 * hv;
        const bool ok = mrow && p < a.P;              // P % 8 == 0: a vector of 8 points is inside or outside
        float val[8];
        bws_slab_read(myOs, row, c0 + 8 * hv, val);
        hx8 xh;
        const SwishCoef sc_ = swish_coef(sb, tb, gt);
#pragma unroll
        for (int e = 0; e < 8; e++) {
          const float b = (float)eb[hv][e];
          float xs, d_;
          swish_bwd_(sc_, b, xs, d_);
          xh[e] = ok ? (H)xs : (H)0.f;                 // conv input of the forward pass (zero outside: dY is zero there too)
          const float dv = val[e] * d_;
          val[e] = dv;
          if (ok) { st1 += dv; st2 += dv * b; }
        }
        *(hx8*)&Xh[(wid * 32 + row) * YRP + c0 + 8 * hv] = xh;
        bws_store_dx<H>(a, dxr, val, ok, m, p);
      }
      // ---- dW tiles (cot, cit = wid): A = dY rows (row-read copy), B = this wave's own Xh rows
      const H* yrow = Yr + (cur * CoP + r) * YRP + 8 * half;
      const H* xrow = Xh + (wid * 32 + r) * YRP + 8 * half;
#pragma unroll
      for (int ks = 0; ks < BN / 16; ks++) {
        const hx8 bf = *(const hx8*)(xrow + ks * 16);
#pragma unroll
        for (int s = 0; s < CT; s++) {
          const hx8 af = *(const hx8*)(yrow + s * 32 * YRP + ks * 16);
          acc_dw[s] = mfma16<H>(af, bf, acc_dw[s]);
        }
      }
    }
    __syncthreads();                                   // one barrier per tile
    issue_loads(tile + 3, gr, yr);
  };
  for (int tile = t.begin; tile < t.end; tile += 2) {
    step(tile, 0, g1, y1, eb0, gl0, eb1, gl1);
    if (tile + 1 < t.end) step(tile + 1, 1, g0, y0, eb1, gl1, eb0, gl0);
  }
  flush_sums(n_prev);

  if (mw && !a.noflush) {
    const int ci = rb * 32 + r;
    float* slab = bws_dw_slab(a);
#pragma unroll
    for (int s = 0; s < CT; s++)
#pragma unroll
      for (int e = 0; e < 16; e++) bws_flush_dw(a, slab, s * 32 + bws_acc_row(e, half), ci, acc_dw[s][e]);
  }
}

template <int NW, int KS, int CT>
static inline size_t bw_lds_bytes() {
  return (size_t)2 * KS * 16 * 64 + (size_t)2 * CT * 32 * BWS_RP * 2 + (size_t)NW * 32 * BWS_RP * 2 + (size_t)KS * 16 * 16 +
         (size_t)NW * 32 * WS_OP * 4;
}

// the layers this kernel is for: `c` convs whose input channels exceed one panel of the sliced kernel (129..224) with at
// most 96 output channels -- stage 4 of X3D-XS / S / M / L (216 <-> 96)
bool pw_bwd_wst_applies(const x3d_pw_bwd_args* b) {
  if (x3d_env_int("X3D_PW_BWD_WST", 1) == 0) return false;   // A/B switch: 0 = off
  if (b->epi != X3D_EPI_SWISH_BWD || b->tail_c) return false;
  // stage 4: 129..224 input channels, six k-steps (the panel's pitch is roundup(Co, 16) + 8); stage 5 (round 5): 225..448 input
  // channels as two slices of seven row blocks, twelve k-steps (432 <-> 192)
  const int ks = (b->Cout + 15) >> 4;
  if (!((b->Cin > 128 && b->Cin <= 224 && ks == 6) || (b->Cin > 224 && b->Cin <= 448 && ks == 12 && x3d_env_int("X3D_PW_BWD_WST5", 1) != 0))) return false;
  return bws_applies(b, {b->g, b->yraw, b->dx, b->w_panel, b->braw});
}

static inline int bw_slices(int Ci) { return ceil_div(ceil_div(Ci, 32), 7); }   // seven row blocks each, over blockIdx.y

template <typename H, int KS, int CT>
static int bw_launch(PwBwdWstArgs& a, hipStream_t st) {
  constexpr int NW = 7;
  return bws_launch<pw_bwd_wst_kernel<H, NW, KS, CT>>(a, bw_lds_bytes<NW, KS, CT>(), bw_slices(a.Ci), st, "pw_bwd_wst",
                                                      "pw_bwd_wst_kernel<%s, %d, %d, %d>", HV<H>::name, NW, KS, CT);
}

// called by x3d_pw_bwd (pw_bwd_fused.hip) when pw_bwd_wst_applies()
int pw_bwd_wst(const x3d_pw_bwd_args* b, hipStream_t st) {
  X3D_REQUIRE(b->braw && b->b_scale_shift && b->nc_sums, "pw_bwd: SWISH_BWD needs braw/b_scale_shift/nc_sums");
  PwBwdWstArgs a;
  memset(&a, 0, sizeof(a));
  bws_fill_args(a, b);
  a.braw = b->braw; a.b_ss = b->b_scale_shift; a.egate = b->gate; a.nc_sums = b->nc_sums;
  if (((b->Cout + 15) >> 4) == 12) return b->dtype == X3D_F16 ? bw_launch<f16, 12, 6>(a, st) : bw_launch<bf16, 12, 6>(a, st);
  return b->dtype == X3D_F16 ? bw_launch<f16, 6, 3>(a, st) : bw_launch<bf16, 6, 3>(a, st);
}

// number of partial dW slabs a launch writes when given dw_slab (= its grid: x3d_hip.h)
int pw_bwd_wst_dw_parts(const x3d_pw_bwd_args* b) {
  long long tpb, gx;
  bws_grid(b->N, (long long)b->T * b->H * b->W, bw_slices(b->Cin), &tpb, &gx);
  return (int)gx;
}
