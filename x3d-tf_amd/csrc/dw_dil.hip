// x3d_dw3d_fwd_dil / x3d_dw3d_bwd_dil: channelwise 3x3x3 convolution, strides 1, dilation (1, d, d), padding
// (1, d, d) -- the `b` convs of a dilated stride-1 res5 (include/x3d_hip.h K6).  Contract as the dense kernels (dw_common.h).
//
// One 256-thread workgroup per (n, c) walks t.  A plane of the planes this form meets (10 x 10 .. 20 x 20) is a few hundred
// elements, so there is nothing to tile: the whole zero-haloed plane (H + 2d) x (W + 2d) of the channel sits in LDS as fp32,
// a RING of three of them (t-1, t, t+1), and every HBM element is read once and written once.  A thread owns pixels
// tid + 256 k; plane t is emitted when plane t + 1 has been staged, each output reading its 27 taps from the ring (the
// taps of a dilated stencil are d apart: no register window is shared between neighbouring outputs, which is why the strip /
// window forms of the dense kernels do not carry over).  A workgroup is one chain of dependent steps, so what it waits for is
// the latency of its loads: the elements of the next THREE planes are in flight in registers (NP > 0: up to 256 NP pixels
// per plane); larger planes stage directly (NP = 0).
//
// A step of the walk is a serial chain (LDS write, barrier, LDS reads, 27 / 54 FMAs, store, barrier) at ~4 clocks per wave64
// instruction, so the plane loop carries nothing but the taps (DESIGN section 25 has the instruction counts):
//   * the walk is unrolled by three, so the ring slot of every tap is a compile-time constant, and the nine (slot, tap row)
//     LDS addresses of a pixel are computed once, before the loop (NP > 0);
//   * D = 2 (the model's dilation) is a template argument: the column taps are immediate offsets of the LDS reads.  D = 0
//     takes the dilation at run time (3, 4);
//   * a plane outside the clip is a ZERO plane in the ring instead of a branch around its nine taps: slot 2 is still zero when
//     plane 0 is emitted, and the step behind the last plane clears its slot instead of staging;
//   * the forward holds the weights in vector registers: an FMA with a scalar-register operand issues slower (dw_common.h,
//     DW_DOT note).
// Loads and stores are per element: a 14 x 14 plane of 16-bit elements starts 8 bytes off 16-byte alignment every other
// plane and a 10 x 10 one is 200 bytes, so no vector width holds for a plane; lanes are consecutive in memory, one plane is
// one or two fully used 128-byte lines per wave.
// LDS pitch: (W + 2d) | 1 floats.  The +-d ROW taps of a lane sit d pitches away; with an even pitch (a multiple of 32 in
// the worst case) the lanes that wrap into the next row meet the lanes of the row above on the same banks.
// All products are fp32 on fp32 operands (no matrix-core form).
#include <type_traits>

#include "dw_common.h"

struct DilGeom {
  int N, C, T, H, W;
  int d;       // dilation
  int P;       // LDS pitch (floats)
  int plane;   // floats per haloed plane = (H + 2d) * P
};
struct DilFwdArgs {
  DilGeom g;
  const void* x; const float* w; void* y;
  const float* ss; int act;
  double* stats; double* pool;
  x3d_bn_fold bn;
};
struct DilBwdArgs {
  DilGeom g;
  const void* dv; const void* braw; const float* coef_nc;
  const void* araw; const float* ss_a; const float* w;
  void* ga; double* a_sums; float* dw;
};

// LDS offset of pixel p of the image inside a haloed plane
__device__ __forceinline__ int dil_off(const DilGeom& g, int p) {
  const int h = p / g.W, w = p - h * g.W;
  return (h + g.d) * g.P + w + g.d;
}
// the 27 weights of channel c into vector registers (the empty statement pins each to a VGPR)
__device__ __forceinline__ void dil_weights(const float* __restrict__ w, int c, float (&wgt)[27]) {
#pragma unroll
  for (int k = 0; k < 27; k++) {
    wgt[k] = w[c * 27 + k];
    asm volatile("" : "+v"(wgt[k]));
  }
}
// Tap-row addresses of one pixel: rows[slot][kh] = the LDS index (floats) of tap (kh, kw = 0) of the pixel at offset `o` in ring
// slot `slot`; tap kw is rows[slot][kh] + kw * d.
__device__ __forceinline__ void dil_rows(int (&rows)[3][3], int o, int plane, int d, int dP) {
#pragma unroll
  for (int sl = 0; sl < 3; sl++)
#pragma unroll
    for (int kh = 0; kh < 3; kh++) rows[sl][kh] = sl * plane + o - d + (kh - 1) * dP;
}
template <int V> using dil_c = std::integral_constant<int, V>;

template <typename T, int NP, int D>
__global__ __launch_bounds__(256) void dw3d_dil_fwd_kernel(const DilFwdArgs a) {
  extern __shared__ __attribute__((aligned(16))) float lds[];
  const DilGeom& g = a.g;
  constexpr int NK = NP > 0 ? NP : 1;
  const int HW = g.H * g.W, d = D > 0 ? D : g.d, dP = d * g.P;
  float* scratch = lds + 3 * g.plane;
  const int c = __builtin_amdgcn_readfirstlane(blockIdx.x % g.C);
  const int n = __builtin_amdgcn_readfirstlane(blockIdx.x / g.C);

  for (int i = threadIdx.x; i < 3 * g.plane; i += 256) lds[i] = 0.f;   // the halo stays zero: staging writes the image only

  float wgt[27];
  dil_weights(a.w, c, wgt);
  float sc = 1.f, sh = 0.f;
  if (a.bn.stats) bn_fold_channel(a.bn, c, n == 0 && threadIdx.x == 0, sc, sh, g.C);   // BN finalize folded in
  else if (a.ss) { sc = a.ss[c * 2]; sh = a.ss[c * 2 + 1]; }
  const int act = a.act;
  auto xf = [=](float v) {
    float u = sc * v + sh;
    return act == X3D_ACT_RELU ? fmaxf(u, 0.f) : u;
  };
  const T* xin = (const T*)a.x + ((long long)n * g.C + c) * g.T * HW;
  T* yout = (T*)a.y + ((long long)n * g.C + c) * g.T * HW;

  // NP > 0: every global access of the walk is an UNCONDITIONAL bounds-checked buffer instruction (dw_common.h raw_bload /
  // raw_bstore: a lane without a pixel, a plane behind the clip and the store of step 0 carry an out-of-range offset), so the
  // compiler counts them and waits for exactly the load it stages -- behind a conditional load every wait is vmcnt(0), which
  // would drain the planes in flight and the store of the step before at every step
  constexpr int EB = (int)sizeof(T);
  const int plB = HW * EB;
  const __amdgpu_buffer_rsrc_t rsX = __builtin_amdgcn_make_buffer_rsrc((T*)xin, 0, g.T * plB, 0x00020000);
  const __amdgpu_buffer_rsrc_t rsY = __builtin_amdgcn_make_buffer_rsrc(yout, 0, g.T * plB, 0x00020000);
  int off[NK], gofs[NK], rows[NK][3][3];
  Raw pre[3][NK];   // planes s, s+1, s+2 in flight, as loaded (converted when staged: a conversion here would wait for the load):
                    // pre[s % 3] is staged at step s and reloaded with plane s + 3
  if constexpr (NP > 0) {
#pragma unroll
    for (int k = 0; k < NK; k++) {
      const int p = threadIdx.x + k * 256;
      off[k] = p < HW ? dil_off(g, p) : -1;
      gofs[k] = p < HW ? p * EB : DW_OOB;
#pragma unroll
      for (int j = 0; j < 3; j++) raw_bload<EB>(pre[j][k], rsX, gofs[k] + j * plB, 0);
      dil_rows(rows[k], off[k] < 0 ? dP + d : off[k], g.plane, d, dP);   // (no pixel: pixel 0's taps, all inside the ring)
    }
  }
  float s1 = 0.f, s2 = 0.f;
  __syncthreads();   // zero fill done

  // output pixel: plane t-1 (kt = 0) in slot S0, t (kt = 1) in S1, t+1 (kt = 2) in S2
  auto pixel = [&](const int (&r)[3][3], auto s0, auto s1_, auto s2_) {
    constexpr int S0 = decltype(s0)::value, S1 = decltype(s1_)::value, S2 = decltype(s2_)::value;
    float acc = 0.f;
#pragma unroll
    for (int kh = 0; kh < 3; kh++)
#pragma unroll
      for (int kw = 0; kw < 3; kw++) {
        acc = __builtin_fmaf(wgt[kh * 3 + kw], lds[r[S0][kh] + kw * d], acc);
        acc = __builtin_fmaf(wgt[9 + kh * 3 + kw], lds[r[S1][kh] + kw * d], acc);
        acc = __builtin_fmaf(wgt[18 + kh * 3 + kw], lds[r[S2][kh] + kw * d], acc);
      }
    return acc;
  };
  // one step of the walk: plane s into ring slot SL = s % 3 (behind the clip: zeros), then output plane t = s - 1
  auto step = [&](auto sl, int s) {
    constexpr int SL = decltype(sl)::value;
    float* dst = lds + SL * g.plane;
    const bool real = s < g.T;
    const int t = s - 1;
    if constexpr (NP > 0) {
#pragma unroll
      for (int k = 0; k < NK; k++) if (off[k] >= 0) dst[off[k]] = real ? xf(raw_get<T>(pre[SL][k], 0)) : 0.f;
      __syncthreads();
#pragma unroll
      for (int k = 0; k < NK; k++) raw_bload<EB>(pre[SL][k], rsX, gofs[k] + (s + 3) * plB, 0);   // flies while three planes are consumed
      float out[NK];
#pragma unroll
      for (int k = 0; k < NK; k++) out[k] = 0.f;
      if (s >= 1) {   // (LDS only; a lane without a pixel computes pixel 0 again and its value goes nowhere)
#pragma unroll
        for (int k = 0; k < NK; k++) out[k] = pixel(rows[k], dil_c<(SL + 1) % 3>{}, dil_c<(SL + 2) % 3>{}, dil_c<SL>{});
      }
#pragma unroll
      for (int k = 0; k < NK; k++) {
        Raw o;
        const float v1[1] = {out[k]};
        raw_pack<T, 1>(o, v1);
        raw_bstore<EB>(o, rsY, s >= 1 ? gofs[k] + t * plB : DW_OOB, 0);
        const float v = off[k] >= 0 ? out[k] : 0.f;
        s1 += v;
        s2 += v * v;
      }
    } else {
      for (int p = threadIdx.x; p < HW; p += 256) dst[dil_off(g, p)] = real ? xf(to_f<T>(xin[s * HW + p])) : 0.f;
      __syncthreads();
      if (s >= 1) {
        for (int p = threadIdx.x; p < HW; p += 256) {
          int r[3][3];
          dil_rows(r, dil_off(g, p), g.plane, d, dP);
          const float acc = pixel(r, dil_c<(SL + 1) % 3>{}, dil_c<(SL + 2) % 3>{}, dil_c<SL>{});
          yout[t * HW + p] = from_f<T>(acc);
          s1 += acc;
          s2 += acc * acc;
        }
      }
    }
    __syncthreads();   // the next plane overwrites the slot of plane t-1
  };
  for (int s = 0; s <= g.T; s += 3) {
    step(dil_c<0>{}, s);
    if (s + 1 <= g.T) step(dil_c<1>{}, s + 1);
    if (s + 2 <= g.T) step(dil_c<2>{}, s + 2);
  }

  if (a.stats || a.pool) {
    float red[2] = {s1, s2};
    block_sum<2>(red, scratch);
    if (threadIdx.x == 0) {
      if (a.stats) {
        double* sp = stats_replica(a.stats, g.C, (unsigned)n);
        atomic_add_d(&sp[c * 2], (double)red[0]);
        atomic_add_d(&sp[c * 2 + 1], (double)red[1]);
      }
      if (a.pool) atomic_add_d(&a.pool[(long long)n * g.C + c], (double)red[0]);
    }
  }
}

// ================================================================================================
// backward (data + weight fused): two rings, dB = A*dv + B*braw + C and act = relu(s_a*araw + t_a), walked together.
//   dW[kt][kh][kw] += sum dB[t][h][w] * act[t+kt-1][h+(kh-1)d][w+(kw-1)d]
//   dA[t][h][w]     = sum w[kt][kh][kw] * dB[t+1-kt][h+(1-kh)d][w+(1-kw)d]
//   ga = dA * [s_a*araw + t_a > 0];   a_sums += (sum ga, sum ga*araw)
// With plane t+1 staged, the rings hold planes t-1 .. t+1 of both: ga[t] and the 27 dW terms of dB[t] in one walk.
// The dB ring is lds[0 .. 3 plane), the act ring lds[3 plane .. 6 plane): one address table serves both.
// ================================================================================================
template <typename T, int NP, int D>
__global__ __launch_bounds__(256) void dw3d_dil_bwd_kernel(const DilBwdArgs a) {
  extern __shared__ __attribute__((aligned(16))) float lds[];
  const DilGeom& g = a.g;
  constexpr int NK = NP > 0 ? NP : 1;
  const int HW = g.H * g.W, d = D > 0 ? D : g.d, dP = d * g.P;
  const float* Al = lds + 3 * g.plane;
  float* scratch = lds + 6 * g.plane;
  const int c = __builtin_amdgcn_readfirstlane(blockIdx.x % g.C);
  const int n = __builtin_amdgcn_readfirstlane(blockIdx.x / g.C);

  for (int i = threadIdx.x; i < 6 * g.plane; i += 256) lds[i] = 0.f;

  float wgt[27];   // (scalar registers here: 27 more vector registers would cost the backward a wave of occupancy)
#pragma unroll
  for (int k = 0; k < 27; k++) wgt[k] = a.w[c * 27 + k];
  const float sc = a.ss_a[c * 2], sh = a.ss_a[c * 2 + 1];
  const float* cf = a.coef_nc + ((long long)n * g.C + c) * 4;
  const float cA = cf[0], cB = cf[1], cC = cf[2];
  auto af = [=](float v) { return fmaxf(sc * v + sh, 0.f); };
  auto bf = [=](float dvv, float bv) { return cA * dvv + cB * bv + cC; };

  const long long base = ((long long)n * g.C + c) * g.T * HW;
  const T* araw = (const T*)a.araw + base;
  const T* dvp = (const T*)a.dv + base;
  const T* brp = (const T*)a.braw + base;
  T* gap = (T*)a.ga + base;

  constexpr int EB = (int)sizeof(T);      // unconditional bounds-checked buffer accesses, as in the forward
  const int plB = HW * EB;
  const __amdgpu_buffer_rsrc_t rsA = __builtin_amdgcn_make_buffer_rsrc((T*)araw, 0, g.T * plB, 0x00020000);
  const __amdgpu_buffer_rsrc_t rsD = __builtin_amdgcn_make_buffer_rsrc((T*)dvp, 0, g.T * plB, 0x00020000);
  const __amdgpu_buffer_rsrc_t rsR = __builtin_amdgcn_make_buffer_rsrc((T*)brp, 0, g.T * plB, 0x00020000);
  const __amdgpu_buffer_rsrc_t rsG = __builtin_amdgcn_make_buffer_rsrc(gap, 0, g.T * plB, 0x00020000);
  int off[NK], gofs[NK], rows[NK][3][3];
  Raw preA[3][NK], preD[3][NK], preR[3][NK];   // planes s, s+1, s+2 in flight as loaded, as in the forward
  float held[NK];                              // this thread's araw of the plane that is emitted next
  if constexpr (NP > 0) {
#pragma unroll
    for (int k = 0; k < NK; k++) {
      const int p = threadIdx.x + k * 256;
      off[k] = p < HW ? dil_off(g, p) : -1;
      gofs[k] = p < HW ? p * EB : DW_OOB;
      held[k] = 0.f;
#pragma unroll
      for (int j = 0; j < 3; j++) {
        raw_bload<EB>(preA[j][k], rsA, gofs[k] + j * plB, 0);
        raw_bload<EB>(preD[j][k], rsD, gofs[k] + j * plB, 0);
        raw_bload<EB>(preR[j][k], rsR, gofs[k] + j * plB, 0);
      }
      dil_rows(rows[k], off[k] < 0 ? dP + d : off[k], g.plane, d, dP);   // (no pixel: pixel 0's taps, all inside the ring)
    }
  }
  float dW[27];
#pragma unroll
  for (int k = 0; k < 27; k++) dW[k] = 0.f;
  float s1 = 0.f, s2 = 0.f;
  __syncthreads();   // zero fill done

  // one pixel of plane t: its 27 dW terms and its data gradient; planes t-1, t, t+1 in slots S0, S1, S2 of both rings
  auto pixel = [&](const int (&r)[3][3], auto s0, auto s1_, auto s2_) {
    constexpr int S0 = decltype(s0)::value, S1 = decltype(s1_)::value, S2 = decltype(s2_)::value;
    const float dBo = lds[r[S1][1] + d];
    float acc = 0.f;
#pragma unroll
    for (int kh = 0; kh < 3; kh++)
#pragma unroll
      for (int kw = 0; kw < 3; kw++) {
        const int k9 = kh * 3 + kw;
        dW[k9] = __builtin_fmaf(dBo, Al[r[S0][kh] + kw * d], dW[k9]);                  // kt = 0: dB[t] * act[t-1]
        dW[9 + k9] = __builtin_fmaf(dBo, Al[r[S1][kh] + kw * d], dW[9 + k9]);          // kt = 1
        dW[18 + k9] = __builtin_fmaf(dBo, Al[r[S2][kh] + kw * d], dW[18 + k9]);        // kt = 2: dB[t] * act[t+1]
        // the transposed taps: dB[t + 1 - kt][h + (1 - kh) d][w + (1 - kw) d]
        acc = __builtin_fmaf(wgt[k9], lds[r[S2][2 - kh] + (2 - kw) * d], acc);         // kt = 0: dB[t+1]
        acc = __builtin_fmaf(wgt[9 + k9], lds[r[S1][2 - kh] + (2 - kw) * d], acc);     // kt = 1: dB[t]
        acc = __builtin_fmaf(wgt[18 + k9], lds[r[S0][2 - kh] + (2 - kw) * d], acc);    // kt = 2: dB[t-1]
      }
    return acc;
  };
  auto step = [&](auto sl, int s) {
    constexpr int SL = decltype(sl)::value;
    float* dB = lds + SL * g.plane;
    float* dA = lds + (3 + SL) * g.plane;
    const bool real = s < g.T;
    const int t = s - 1;
    if constexpr (NP > 0) {
      float cur[NK];   // araw of plane s as staged
#pragma unroll
      for (int k = 0; k < NK; k++) {
        cur[k] = raw_get<T>(preA[SL][k], 0);
        if (off[k] >= 0) {
          dB[off[k]] = real ? bf(raw_get<T>(preD[SL][k], 0), raw_get<T>(preR[SL][k], 0)) : 0.f;
          dA[off[k]] = real ? af(cur[k]) : 0.f;
        }
      }
      __syncthreads();
#pragma unroll
      for (int k = 0; k < NK; k++) {
        raw_bload<EB>(preA[SL][k], rsA, gofs[k] + (s + 3) * plB, 0);
        raw_bload<EB>(preD[SL][k], rsD, gofs[k] + (s + 3) * plB, 0);
        raw_bload<EB>(preR[SL][k], rsR, gofs[k] + (s + 3) * plB, 0);
      }
      float out[NK];
#pragma unroll
      for (int k = 0; k < NK; k++) out[k] = 0.f;
      if (s >= 1) {
        if (threadIdx.x < HW) {   // (a lane without a pixel must not add its reads to dW)
#pragma unroll
          for (int k = 0; k < NK; k++)
            if (k == 0 || off[k] >= 0) out[k] = pixel(rows[k], dil_c<(SL + 1) % 3>{}, dil_c<(SL + 2) % 3>{}, dil_c<SL>{});
        }
      }
#pragma unroll
      for (int k = 0; k < NK; k++) {
        const float av = held[k];
        const float gv = (off[k] >= 0 && sc * av + sh > 0.f) ? out[k] : 0.f;
        Raw o;
        const float v1[1] = {gv};
        raw_pack<T, 1>(o, v1);
        raw_bstore<EB>(o, rsG, s >= 1 ? gofs[k] + t * plB : DW_OOB, 0);
        s1 += gv;
        s2 += gv * av;
        held[k] = cur[k];
      }
    } else {
      for (int p = threadIdx.x; p < HW; p += 256) {
        const int o = dil_off(g, p);
        dB[o] = real ? bf(to_f<T>(dvp[s * HW + p]), to_f<T>(brp[s * HW + p])) : 0.f;
        dA[o] = real ? af(to_f<T>(araw[s * HW + p])) : 0.f;
      }
      __syncthreads();
      if (s >= 1) {
        // (planes past 512 pixels: the thread's araw is read again here, from L2, instead of being held in registers)
        for (int p = threadIdx.x; p < HW; p += 256) {
          int r[3][3];
          dil_rows(r, dil_off(g, p), g.plane, d, dP);
          const float acc = pixel(r, dil_c<(SL + 1) % 3>{}, dil_c<(SL + 2) % 3>{}, dil_c<SL>{});
          const float av = to_f<T>(araw[t * HW + p]);
          const float gv = (sc * av + sh > 0.f) ? acc : 0.f;
          gap[t * HW + p] = from_f<T>(gv);
          s1 += gv;
          s2 += gv * av;
        }
      }
    }
    __syncthreads();   // the next planes overwrite the slots of planes t-1
  };
  for (int s = 0; s <= g.T; s += 3) {
    step(dil_c<0>{}, s);
    if (s + 1 <= g.T) step(dil_c<1>{}, s + 1);
    if (s + 2 <= g.T) step(dil_c<2>{}, s + 2);
  }

  // block reduction of the 27 weight-gradient taps and the two BN sums, as dw3d_bwd_kernel: 27 float atomics and 2 double
  // atomics per workgroup
  const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
  float red[29];
#pragma unroll
  for (int k = 0; k < 29; k++) red[k] = wave_sum_lane63(k < 27 ? dW[k] : (k == 27 ? s1 : s2));
  if (lane == 63) {
#pragma unroll
    for (int k = 0; k < 29; k++) scratch[k * 4 + wid] = red[k];
  }
  __syncthreads();
  if (threadIdx.x < 29) {
    float v = 0.f;
    for (int w = 0; w < 4; w++) v += scratch[threadIdx.x * 4 + w];
    if (threadIdx.x < 27) atomicAdd(&a.dw[c * 27 + threadIdx.x], v);
    else atomic_add_d(&a.a_sums[c * 2 + (threadIdx.x - 27)], (double)v);
  }
}

// ---- host side ---------------------------------------------------------------------------------
#define DW_DIL_MAX_PLANE 4096   // (H + 2d)(W + 2d): the planes of a dilated res5 are 10 x 10 .. 20 x 20

// the checks shared by both directions; fills g
static int dil_geom(const char* who, DilGeom& g, int N, int C, int T, int H, int W, int stride, int dilation) {
  X3D_REQUIRE(stride == 1, "%s: dilation = %d needs stride 1 (stride = %d)", who, dilation, stride);
  X3D_REQUIRE(dilation <= 4, "%s: dilation = %d is not supported (dilation must be 0 .. 4)", who, dilation);
  const long long halo = (long long)(H + 2 * dilation) * (W + 2 * dilation);
  X3D_REQUIRE(halo <= DW_DIL_MAX_PLANE, "%s: dilation = %d on a %d x %d plane needs %lld haloed elements in LDS (limit %d)", who,
              dilation, H, W, halo, DW_DIL_MAX_PLANE);
  X3D_REQUIRE((long long)T * H * W < (1ll << 31), "%s: a channel of %d x %d x %d elements is too large", who, T, H, W);
  X3D_REQUIRE((long long)N * C < (1ll << 31), "%s: grid too large", who);
  g.N = N; g.C = C; g.T = T; g.H = H; g.W = W; g.d = dilation;
  g.P = (W + 2 * dilation) | 1;
  g.plane = (H + 2 * dilation) * g.P;
  return X3D_OK;
}
// pixels per thread held in registers: 1 (<= 256 pixels), 2 (<= 512), 0 = direct staging (also for a channel of 2^30 bytes and
// more, whose offsets the out-of-range marker of the buffer accesses has no room above)
static int dil_np(const DilGeom& g, int elem_bytes) {
  const int HW = g.H * g.W;
  if ((long long)g.T * HW * elem_bytes >= (1ll << 30)) return 0;
  return HW <= 256 ? 1 : (HW <= 512 ? 2 : 0);
}

template <typename T, int NP, int D>
static int dil_fwd_go(const DilFwdArgs& a, hipStream_t st) {
  X3D_DESCRIBE("dw3d_dil_fwd_kernel<%s, %d, %d>", TypeName<T>::v, NP, D);
  const size_t lds = ((size_t)3 * a.g.plane + 16) * sizeof(float);   // ring + block_sum scratch: < 64 KB at the plane limit
  hipLaunchKernelGGL((dw3d_dil_fwd_kernel<T, NP, D>), dim3((unsigned)(a.g.N * a.g.C)), dim3(256), lds, st, a);
  X3D_LAUNCH_CHECK("dw3d_fwd");
  return X3D_OK;
}
template <typename T, int NP, int D>
static int dil_bwd_go(const DilBwdArgs& a, hipStream_t st) {
  X3D_DESCRIBE("dw3d_dil_bwd_kernel<%s, %d, %d>", TypeName<T>::v, NP, D);
  const size_t lds = ((size_t)6 * a.g.plane + 29 * 4) * sizeof(float);   // two rings: up to ~120 KB at the plane limit
  auto kern = dw3d_dil_bwd_kernel<T, NP, D>;
  if (lds > 64 * 1024) (void)hipFuncSetAttribute((const void*)kern, hipFuncAttributeMaxDynamicSharedMemorySize, 128 * 1024);
  hipLaunchKernelGGL(kern, dim3((unsigned)(a.g.N * a.g.C)), dim3(256), lds, st, a);
  X3D_LAUNCH_CHECK("dw3d_bwd");
  return X3D_OK;
}
template <typename T, int D>
static int dil_fwd_np(const DilFwdArgs& a, hipStream_t st) {
  switch (dil_np(a.g, (int)sizeof(T))) {
    case 1: return dil_fwd_go<T, 1, D>(a, st);
    case 2: return dil_fwd_go<T, 2, D>(a, st);
    default: return dil_fwd_go<T, 0, D>(a, st);
  }
}
template <typename T, int D>
static int dil_bwd_np(const DilBwdArgs& a, hipStream_t st) {
  switch (dil_np(a.g, (int)sizeof(T))) {
    case 1: return dil_bwd_go<T, 1, D>(a, st);
    case 2: return dil_bwd_go<T, 2, D>(a, st);
    default: return dil_bwd_go<T, 0, D>(a, st);
  }
}
template <typename T>
static int dil_fwd_d(const DilFwdArgs& a, hipStream_t st) { return a.g.d == 2 ? dil_fwd_np<T, 2>(a, st) : dil_fwd_np<T, 0>(a, st); }
template <typename T>
static int dil_bwd_d(const DilBwdArgs& a, hipStream_t st) { return a.g.d == 2 ? dil_bwd_np<T, 2>(a, st) : dil_bwd_np<T, 0>(a, st); }

// ---- entry points: the dense structs, the dilation as an argument of its own (include/x3d_hip.h K6, dilated form)
extern "C" int x3d_dw3d_fwd_dil(const x3d_dw3d_fwd_args* f, int dilation, void* stream) {
  X3D_REQUIRE(dilation >= 0, "dw3d_fwd: dilation = %d is negative", dilation);
  if (dilation < 2) return x3d_dw3d_fwd(f, stream);   // 0 / 1: the dense conv, as it stands
  X3D_REQUIRE(f && f->x && f->w && f->y, "dw3d_fwd: null pointer");
  X3D_REQUIRE(f->N > 0 && f->C > 0 && f->T > 0 && f->H > 0 && f->W > 0, "dw3d_fwd: bad extents");
  X3D_REQUIRE(x3d_dtype_ok(f->dtype), "dw3d_fwd: bad dtype");
  X3D_REQUIRE(f->in_act == X3D_ACT_NONE || f->in_act == X3D_ACT_RELU, "dw3d_fwd: prologue act must be none/relu");
  X3D_REQUIRE(!f->in_bn || bn_fold_valid(f->in_bn), "dw3d_fwd: incomplete x3d_bn_fold");
  hipStream_t st = (hipStream_t)stream;
  DilFwdArgs a;
  if (int rc = dil_geom("dw3d_fwd", a.g, f->N, f->C, f->T, f->H, f->W, f->stride, dilation)) return rc;
  a.x = f->x; a.w = f->w; a.y = f->y; a.ss = f->in_scale_shift; a.act = f->in_act;
  a.stats = f->stats; a.pool = f->pool;
  memset(&a.bn, 0, sizeof(a.bn));
  if (f->in_bn) a.bn = *f->in_bn;
  if (f->dtype == X3D_F32) return dil_fwd_d<float>(a, st);
  if (f->dtype == X3D_F16) return dil_fwd_d<f16>(a, st);
  return dil_fwd_d<bf16>(a, st);
}
extern "C" int x3d_dw3d_bwd_dil(const x3d_dw3d_bwd_args* f, int dilation, void* stream) {
  X3D_REQUIRE(dilation >= 0, "dw3d_bwd: dilation = %d is negative", dilation);
  if (dilation < 2) return x3d_dw3d_bwd(f, stream);
  X3D_REQUIRE(f && f->dv && f->braw && f->coef_nc && f->araw && f->a_scale_shift && f->w && f->ga &&
                  f->a_sums && f->dw, "dw3d_bwd: null pointer");
  X3D_REQUIRE(f->N > 0 && f->C > 0 && f->T > 0 && f->H > 0 && f->W > 0, "dw3d_bwd: bad extents");
  X3D_REQUIRE(x3d_dtype_ok(f->dtype), "dw3d_bwd: bad dtype");
  hipStream_t st = (hipStream_t)stream;
  DilBwdArgs a;
  if (int rc = dil_geom("dw3d_bwd", a.g, f->N, f->C, f->T, f->H, f->W, f->stride, dilation)) return rc;
  a.dv = f->dv; a.braw = f->braw; a.coef_nc = f->coef_nc; a.araw = f->araw; a.ss_a = f->a_scale_shift;
  a.w = f->w; a.ga = f->ga; a.a_sums = f->a_sums; a.dw = f->dw;
  if (f->dtype == X3D_F32) return dil_bwd_d<float>(a, st);
  if (f->dtype == X3D_F16) return dil_bwd_d<f16>(a, st);
  return dil_bwd_d<bf16>(a, st);
}
extern "C" int x3d_dw3d_kernel_name_dil(const x3d_dw3d_fwd_args* fwd, const x3d_dw3d_bwd_args* bwd, int dilation, char* out, int cap) {
  X3D_REQUIRE(out && cap > 0 && ((fwd != nullptr) != (bwd != nullptr)), "dw3d_kernel_name_dil: pass exactly one of fwd / bwd");
  out[0] = 0;
  x3d_describe = {out, cap};
  const int rc = fwd ? x3d_dw3d_fwd_dil(fwd, dilation, nullptr) : x3d_dw3d_bwd_dil(bwd, dilation, nullptr);
  x3d_describe = {nullptr, 0};
  return rc;
}
