// Stochastic depth (drop-path) of the bottleneck branch, per sample (include/x3d_hip.h K9d): the keep table, drawn on the device
// from the counter-based generator of common.h (philox4x32_10).  The residual tail forward / backward that apply the table are
// the DP forms of elem.hip's tail kernels (x3d_tail_fwd_dp / x3d_tail_bwd_dp).
#include "common.h"

#define DRAW_BLOCK 256
// ONE workgroup, and only its thread 0 touches `state`: it reads seed and step, hands them to the others through LDS and
// stores step + 1 -- nothing else reads or writes the step, so there is no race to order
__global__ __launch_bounds__(DRAW_BLOCK) void drop_path_draw_kernel(float* __restrict__ keep, const float* __restrict__ rates,
                                                                    uint32_t* state, int L, int N) {
  __shared__ uint32_t st[4];
  if (threadIdx.x == 0) {
#pragma unroll
    for (int i = 0; i < 4; i++) st[i] = state[i];
    const uint64_t next = (((uint64_t)st[3] << 32) | st[2]) + 1ull;
    state[2] = (uint32_t)next;
    state[3] = (uint32_t)(next >> 32);
  }
  __syncthreads();
  const uint32_t k0 = st[0], k1 = st[1], s_lo = st[2], s_hi = st[3];
  const int total = L * N;
  for (int i = threadIdx.x; i < total; i += DRAW_BLOCK) {
    const int l = i / N, n = i - l * N;
    const float rate = rates[l];
    const float u = philox_u24(philox4x32_10(s_lo, s_hi, (uint32_t)l, (uint32_t)n, k0, k1).v[0]);
    keep[i] = u >= rate ? 1.0f / (1.0f - rate) : 0.f;
  }
}

extern "C" int x3d_drop_path_draw(float* keep, const float* rates, void* state, int L, int N, void* stream) {
  X3D_REQUIRE(keep && rates && state && L > 0 && N > 0, "drop_path_draw: bad args");
  X3D_REQUIRE((long long)L * N <= 65536, "drop_path_draw: table of %d x %d entries (one workgroup draws at most 65536)", L, N);
  hipLaunchKernelGGL(drop_path_draw_kernel, dim3(1), dim3(DRAW_BLOCK), 0, (hipStream_t)stream, keep, rates, (uint32_t*)state, L, N);
  X3D_LAUNCH_CHECK("drop_path_draw");
  return X3D_OK;
}
