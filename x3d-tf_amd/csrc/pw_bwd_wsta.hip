// Weights-stationary FUSED backward of the stage-4 `a` conv (96 block channels -> 216 inner channels on 14 x 14 planes;
// reference model.py:246-253 through SURVEY appendix A): data gradient with the residual add (and, optionally, the
// Add + ReLU backward of the block below) AND the weight gradient, one pass over g / a_raw / x.
//
// Until round 3 this layer ran as x3d_pw_dgrad + x3d_pw_wgrad (56 + 56 us, ten launches each per X3D-M step, every one
// streaming g and a_raw -- 2 x 216 rows -- to rebuild dY) followed by x3d_tail_bwd (27 us) on the result: the sliced fused
// kernel only takes dY tiles of <= 128 rows.  On the tile pipeline of pw_bwd_ws.h (dY staging, dX = W^T dY, slab, dx
// stores, dW flush; its rules for the tile loop hold for the loads added here), with the roles of pw_bwd_wst.hip swapped:
//   * dX = W^T dY: M = Ci <= 96 (NW = 3 MFMA waves, one 32-row block each), K = Co = 216 (KS = 14 k-steps; 56 VGPRs of
//     stationary weights per wave);
//   * the x tile [Ci][32 + 8] (the conv input = the output y of the block below) is the B operand of dW and the ReLU mask of
//     the folded tail;
//   * dW[co][ci] += dY[co][:] . x[ci][:]: CT = 7 row tiles of Co x 3 of Ci = 21 tiles, wave w (of 7) owns cot = w: 3 x 16
//     accumulator VGPRs across all tiles of the workgroup, one fp32 atomic flush;
//   * epilogue (waves 0..2, private slabs): dx = dX + add; with tail_c: dx *= [x > 0] and the BN_c backward sums of the
//     block below (exactly what x3d_tail_bwd computes from the stored dx).
#include "pw_bwd_ws.h"

struct PwBwdWstaArgs : PwBwdWsArgs {
  const void* add;                                      // [N][Ci][P]
  const void* x;                                        // [N][Ci][P] conv input
  const void* tail_c; double* tail_sums_c;
};

// TAIL: 0 = plain residual add, 1 = + folded tail backward (identity shortcut below)
template <typename H, int NW, int KS, int CT, int TAIL>
__global__ __launch_bounds__(512, 2) void pw_bwd_wsta_kernel(const PwBwdWstaArgs a) {
  typedef typename HV<H>::x8 hx8;
  extern __shared__ __attribute__((aligned(16))) unsigned char smem_raw[];
  typedef H T;
  constexpr int BN = BWS_BN, OP = WS_OP, Kp = KS * 16, CoP = CT * 32, CiP = NW * 32, RP = BWS_RP;
  static_assert(CT <= 8, "weight-gradient waves");
  static_assert(TAIL == 0 || TAIL == 1, "no third epilogue operand (pw_bwd_wsta_applies)");
  constexpr int NSV = bws_nsv(Kp);
  constexpr size_t YT_B = (size_t)2 * Kp * 64, YR_B = (size_t)2 * CoP * RP * 2, XR_B = (size_t)2 * CiP * RP * 2;
  H* Yt = (H*)smem_raw;                                  // [2][Kp][32]
  H* Yr = (H*)(smem_raw + YT_B);                         // [2][CoP][RP]
  H* Xr = (H*)(smem_raw + YT_B + YR_B);                  // [2][CiP][RP]
  float* Cs = (float*)(smem_raw + YT_B + YR_B + XR_B);   // [Kp][4]
  float* Os = Cs + Kp * 4;                               // [NW][32][OP]
  const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
  const int r = lane & 31, half = lane >> 5;
  const BwsTiles t = bws_tiles(a);
  if (t.begin >= t.end) return;
  float* myOs = Os + (wid < NW ? wid : 0) * 32 * OP;
  const bool xw = wid < NW && wid * 32 < a.Ci;           // dX / epilogue wave
  const bool ww = wid < CT && wid * 32 < a.Co;           // weight-gradient wave (cot = wid)

  bws_setup<H, Kp>(a, Yr, (int)((YR_B + XR_B) / 16), Cs, tid);   // zeroes both row-read tiles
  hx8 A[KS];
  bws_load_weights<H, KS>(a, wid, xw, lane, A);

  // ---- staging: dY as in pw_bwd_ws.h; x vectors v = tid -> row tid >> 2 (tid < 4 * CiP)
  hx8 g0[NSV], y0[NSV], g1[NSV], y1[NSV], x0, x1;
  auto issue_loads = [&](int tile_, hx8 (&gr)[NSV], hx8 (&yr)[NSV], hx8& xr) __attribute__((always_inline)) {
    int n;
    long long p0;
    bws_load_pos(a, t, tile_, n, p0);
    bws_issue_dy<H, Kp>(a, n, p0, tid, gr, yr);
    {
      const int mrow = tid >> 2;
      const long long p = p0 + (tid & 3) * 8;
      const long long o = (mrow < a.Ci && p < a.P) ? ((long long)n * a.Ci + mrow) * a.P + p : 0;
      xr = *(const hx8*)((const T*)a.x + o);
    }
  };
  auto commit = [&](int tile, int buf, const hx8 (&gr)[NSV], const hx8 (&yr)[NSV], const hx8& xr) __attribute__((always_inline)) {
    int n;
    long long p0;
    bws_tile_pos(t, tile, n, p0);
    bws_commit_dy<H, Kp, CoP>(a, p0, buf, tid, Cs, Yt, Yr, gr, yr);
    const int mrow = tid >> 2;
    if (mrow < CiP) {
      const bool ok = mrow < a.Ci && p0 + (tid & 3) * 8 < a.P;
      hx8 hv = xr;
      if (!ok) {
#pragma unroll
        for (int e = 0; e < 8; e++) hv[e] = (H)0.f;
      }
      *(hx8*)&Xr[(buf * CiP + mrow) * RP + (tid & 3) * 8] = hv;
    }
  };

  // ---- epilogue operands (waves 0..NW-1): lane -> row lane >> 1 of this wave's block, points 16 * (lane & 1) .. + 15
  const int row = lane >> 1, c0 = 16 * (lane & 1);
  const int m = wid * 32 + row;                          // this lane's input channel
  const bool mrow_ok = xw && m < a.Ci;
  constexpr int NEO = 1 + TAIL;                          // add, tail_c
  hx8 eo0[NEO][2], eo1[NEO][2];
  auto issue_epi = [&](int tile_, hx8 (&eo)[NEO][2]) __attribute__((always_inline)) {
    int n;
    long long p0;
    bws_load_pos(a, t, tile_, n, p0);
#pragma unroll
    for (int hv = 0; hv < 2; hv++) {
      const long long p = p0 + c0 + 8 * hv;
      const long long o = (mrow_ok && p < a.P) ? ((long long)n * a.Ci + m) * a.P + p : 0;
      eo[0][hv] = *(const hx8*)((const T*)a.add + o);
      if constexpr (TAIL) eo[1][hv] = *(const hx8*)((const T*)a.tail_c + o);
    }
  };
  float tg = 0.f, tgc = 0.f;                             // TAIL: per-channel sums of this lane's row

  f32x16 acc_dw[NW];
#pragma unroll
  for (int s = 0; s < NW; s++)
#pragma unroll
    for (int e = 0; e < 16; e++) acc_dw[s][e] = 0.f;

  const int tr_off = bws_tr_off(lane);

  issue_loads(t.begin, g0, y0, x0);
  issue_epi(t.begin, eo0);
  __syncthreads();                                       // coefficient table, zeroed padding
  commit(t.begin, 0, g0, y0, x0);
  __syncthreads();
  issue_loads(t.begin + 1, g1, y1, x1);
  issue_loads(t.begin + 2, g0, y0, x0);

  auto step = [&](int tile, int cur, hx8 (&gr)[NSV], hx8 (&yr)[NSV], hx8& xr, hx8 (&eo)[NEO][2], hx8 (&eon)[NEO][2])
      __attribute__((always_inline)) {
    int n;
    long long p0;
    bws_tile_pos(t, tile, n, p0);
    issue_epi(tile + 1, eon);                            // a whole step to land
    __amdgpu_buffer_rsrc_t dxr = bws_dx_rsrc<T>(a, n);
    const f32x16 acc = bws_dx<H, KS>(A, Yt + cur * (Kp * BN), tr_off, xw);
    // ---- dW tiles (cot = wid, cit = 0..NW-1): A = this wave's dY rows, B = the x rows (both row-read tiles of `cur`)
    if (ww) {
      const H* yrow = Yr + (cur * CoP + wid * 32 + r) * RP + 8 * half;
      const H* xrow = Xr + (cur * CiP + r) * RP + 8 * half;
#pragma unroll
      for (int ks = 0; ks < BN / 16; ks++) {
        const hx8 af = *(const hx8*)(yrow + ks * 16);
#pragma unroll
        for (int s = 0; s < NW; s++) {
          const hx8 bf = *(const hx8*)(xrow + s * 32 * RP + ks * 16);
          acc_dw[s] = mfma16<H>(af, bf, acc_dw[s]);
        }
      }
    }
    // ---- the next tile goes into the other buffers (before the epilogue: its wait covers loads only)
    if (tile + 1 < t.end) commit(tile + 1, cur ^ 1, gr, yr, xr);

    if (xw) {
      // ---- epilogue through the wave-private slab
#pragma unroll
      for (int e = 0; e < 16; e++) myOs[bws_acc_row(e, half) * OP + r] = acc[e];
#pragma unroll
      for (int hv = 0; hv < 2; hv++) {
        const long long p = p0 + c0 + 8 * hv;
        const bool ok = mrow_ok && p < a.P;              // P % 8 == 0: a vector of 8 points is inside or outside
        float val[8];
        bws_slab_read(myOs, row, c0 + 8 * hv, val);
#pragma unroll
        for (int e = 0; e < 8; e++) val[e] += (float)eo[0][hv][e];
        if constexpr (TAIL) {   // Add + ReLU backward of the block this gradient leaves (its output is x)
          const hx8 xv = *(const hx8*)&Xr[(cur * CiP + m) * RP + c0 + 8 * hv];
#pragma unroll
          for (int e = 0; e < 8; e++) {
            const float gm = (ok && (float)xv[e] > 0.f) ? round_to<T>(val[e]) : 0.f;   // the sums describe dx as stored
            val[e] = gm;
            tg += gm;
            tgc += gm * (float)eo[1][hv][e];
          }
        }
        bws_store_dx<H>(a, dxr, val, ok, m, p);
      }
    }
    __syncthreads();                                     // one barrier per tile
    issue_loads(tile + 3, gr, yr, xr);
  };
  for (int tile = t.begin; tile < t.end; tile += 2) {
    step(tile, 0, g1, y1, x1, eo0, eo1);
    if (tile + 1 < t.end) step(tile + 1, 1, g0, y0, x0, eo1, eo0);
  }

  if constexpr (TAIL) {
    const float s0 = tg + dpp_get<0xB1, 0xF>(tg), s1 = tgc + dpp_get<0xB1, 0xF>(tgc);   // the two lanes of a row
    if (mrow_ok && (lane & 1) == 0) {
      atomic_add_d(&a.tail_sums_c[m * 2], (double)s0);
      atomic_add_d(&a.tail_sums_c[m * 2 + 1], (double)s1);
    }
  }
  if (ww && !a.noflush) {
    float* slab = bws_dw_slab(a);
#pragma unroll
    for (int s = 0; s < NW; s++)
#pragma unroll
      for (int e = 0; e < 16; e++) bws_flush_dw(a, slab, wid * 32 + bws_acc_row(e, half), s * 32 + r, acc_dw[s][e]);
  }
}

template <int NW, int KS, int CT>
static inline size_t bwa_lds_bytes() {
  return (size_t)2 * KS * 16 * 64 + (size_t)2 * CT * 32 * BWS_RP * 2 + (size_t)2 * NW * 32 * BWS_RP * 2 + (size_t)KS * 16 * 16 +
         (size_t)NW * 32 * WS_OP * 4;
}

// the layers this kernel is for: `a` convs with an identity shortcut whose dY tile is too tall for the sliced kernel --
// Co in 209..224 (fourteen k-steps), Ci <= 96: stage 4 of X3D-XS / S / M / L (96 <-> 216)
bool pw_bwd_wsta_applies(const x3d_pw_bwd_args* b) {
  if (x3d_env_int("X3D_PW_BWD_WSTA", 1) == 0) return false;   // A/B switch: 0 = off
  if (b->epi != X3D_EPI_ADD) return false;
  if (b->Cin <= 64 || b->Cin > 96 || ((b->Cout + 15) >> 4) != 14) return false;
  // (a shortcut conv below -- a third epilogue operand -- spills 76 bytes per lane: that one launch per model keeps its
  // separate x3d_tail_bwd, the caller falls back to the call without tail_c)
  if (b->tail_r) return false;
  if (b->tail_c && ((uintptr_t)b->tail_c % 16)) return false;
  return bws_applies(b, {b->g, b->yraw, b->dx, b->w_panel, b->x, b->add});
}

template <typename H, int TAIL>
static int bwa_launch(PwBwdWstaArgs& a, hipStream_t st) {
  constexpr int NW = 3, KS = 14, CT = 7;
  return bws_launch<pw_bwd_wsta_kernel<H, NW, KS, CT, TAIL>>(a, bwa_lds_bytes<NW, KS, CT>(), 1, st, "pw_bwd_wsta",
                                                             "pw_bwd_wsta_kernel<%s, %d, %d, %d, %d>", HV<H>::name, NW, KS, CT, TAIL);
}

// called by x3d_pw_bwd (pw_bwd_fused.hip) when pw_bwd_wsta_applies()
int pw_bwd_wsta(const x3d_pw_bwd_args* b, hipStream_t st) {
  X3D_REQUIRE(!b->tail_c || x3d_describe.out || (b->tail_sums_c && (!b->tail_r || b->tail_sums_r)), "pw_bwd: tail_c / tail_r need their sums");
  PwBwdWstaArgs a;
  memset(&a, 0, sizeof(a));
  bws_fill_args(a, b);
  a.add = b->add; a.x = b->x; a.tail_c = b->tail_c; a.tail_sums_c = b->tail_sums_c;
  const bool tail = b->tail_c != nullptr;
  if (b->dtype == X3D_F16) return tail ? bwa_launch<f16, 1>(a, st) : bwa_launch<f16, 0>(a, st);
  return tail ? bwa_launch<bf16, 1>(a, st) : bwa_launch<bf16, 0>(a, st);
}

int pw_bwd_wsta_dw_parts(const x3d_pw_bwd_args* b) {
  long long tpb, gx;
  bws_grid(b->N, (long long)b->T * b->H * b->W, 1, &tpb, &gx);
  return (int)gx;
}
