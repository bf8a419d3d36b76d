// Precise BatchNorm (NETWORK.BN.USE_PRECISE_STATS): exact pooled statistics over K training batches, from the raw fp64 sums
// every training plan already keeps per BatchNorm layer -- no second pass over activations, no host round trip.
//
//   x3d_precise_bn_accum   after one forward pass: every layer's replicated (sum, sum of squares) accumulator is summed over
//                          its copies and added into the caller's pooled buffer, the layer's element count into its count slot
//   x3d_precise_bn_final   after the last batch: mean and unbiased variance of the pooled sums -> the moving statistics
//
// Both walk one int64 table [nlayers][X3D_PBN_COLS] in device memory (include/x3d_hip.h), all layers in ONE launch: block
// (l, j) takes the channels j * 256 + t, stepping by PBN_GRID_Y * 256, of layer l and leaves at once when the layer has none
// for it.  One thread per channel, plain loads and stores, no atomics, a fixed order of additions: the same inputs give the
// same bits on every run.
#include "common.h"

#define PBN_BLOCK 256
#define PBN_GRID_Y 4      // 1024 channels per step: every BatchNorm layer of the shipped configs in one (the widest is conv5's)

// the totals of channel c over the STATS_R copies: the pairwise tree of bn_fold_channel (groups of 8 as
// ((0+1)+(2+3))+((4+5)+(6+7)), then (q0+q1)+(q2+q3)) = the xor butterfly of bn_finalize_kernel, so all three give the same bits
static_assert(STATS_R == 32, "pbn_replica_sums adds four groups of eight copies");
__device__ __forceinline__ void pbn_replica_sums(const double* __restrict__ stats, int C, int c, double& sum1, double& sum2) {
  const long long rs = stats_stride(C);
  double q1[STATS_R / 8], q2[STATS_R / 8];
#pragma unroll
  for (int r0 = 0; r0 < STATS_R; r0 += 8) {
    double p1[8], p2[8];
#pragma unroll
    for (int r = 0; r < 8; r++) { p1[r] = stats[(r0 + r) * rs + c * 2]; p2[r] = stats[(r0 + r) * rs + c * 2 + 1]; }
    q1[r0 / 8] = ((p1[0] + p1[1]) + (p1[2] + p1[3])) + ((p1[4] + p1[5]) + (p1[6] + p1[7]));
    q2[r0 / 8] = ((p2[0] + p2[1]) + (p2[2] + p2[3])) + ((p2[4] + p2[5]) + (p2[6] + p2[7]));
  }
  sum1 = (q1[0] + q1[1]) + (q1[2] + q1[3]);
  sum2 = (q2[0] + q2[1]) + (q2[2] + q2[3]);
}

// what bn_coefs hands to the moving update, from pooled totals over n elements: (float)mean and the (float) unbiased
// variance -- the same expressions in the same order, so that one batch gives what x3d_bn_finalize(momentum = 0) writes
__device__ __forceinline__ void pbn_moments(double sum1, double sum2, double n, float& mean_out, float& unb_out) {
  const double mean = sum1 / n;
  double var = sum2 / n - mean * mean;
  if (var < 0.0) var = 0.0;
  const double unb = n > 1.0 ? var * (n / (n - 1.0)) : var;
  mean_out = (float)mean;
  unb_out = (float)unb;
}

__global__ __launch_bounds__(PBN_BLOCK) void precise_bn_accum_kernel(const long long* __restrict__ table, double* __restrict__ pooled) {
  const long long* row = table + (long long)blockIdx.x * X3D_PBN_COLS;
  const int C = (int)row[X3D_PBN_C];
  const double* stats = reinterpret_cast<const double*>(row[X3D_PBN_STATS]);
  double* out = pooled + row[X3D_PBN_POOLED];
  for (int c = blockIdx.y * PBN_BLOCK + threadIdx.x; c < C; c += PBN_GRID_Y * PBN_BLOCK) {
    double sum1, sum2;
    pbn_replica_sums(stats, C, c, sum1, sum2);
    out[c * 2] += sum1;
    out[c * 2 + 1] += sum2;
  }
  // the layer's count slot: one thread per layer and launch
  if (blockIdx.y == 0 && threadIdx.x == 0) pooled[blockIdx.x] += (double)row[X3D_PBN_COUNT];
}

__global__ __launch_bounds__(PBN_BLOCK) void precise_bn_final_kernel(const long long* __restrict__ table, const double* __restrict__ pooled,
                                                                     float* __restrict__ params) {
  const long long* row = table + (long long)blockIdx.x * X3D_PBN_COLS;
  const int C = (int)row[X3D_PBN_C];
  const double* in = pooled + row[X3D_PBN_POOLED];
  const double n = pooled[blockIdx.x];
  for (int c = blockIdx.y * PBN_BLOCK + threadIdx.x; c < C; c += PBN_GRID_Y * PBN_BLOCK) {
    float mean, unb;
    pbn_moments(in[c * 2], in[c * 2 + 1], n, mean, unb);
    params[row[X3D_PBN_MEAN] + c] = mean;
    params[row[X3D_PBN_VAR] + c] = unb;
  }
}

extern "C" int x3d_precise_bn_accum(const long long* table, int nlayers, double* pooled, void* stream) {
  X3D_REQUIRE(table && pooled, "precise_bn_accum: null pointer");
  X3D_REQUIRE(nlayers >= 1, "precise_bn_accum: nlayers must be >= 1");
  X3D_REQUIRE(((uintptr_t)table % 8) == 0 && ((uintptr_t)pooled % 8) == 0, "precise_bn_accum: table / pooled not 8-byte aligned");
  hipLaunchKernelGGL(precise_bn_accum_kernel, dim3(nlayers, PBN_GRID_Y), dim3(PBN_BLOCK), 0, (hipStream_t)stream, table, pooled);
  X3D_LAUNCH_CHECK("precise_bn_accum");
  return X3D_OK;
}

extern "C" int x3d_precise_bn_final(const long long* table, int nlayers, const double* pooled, float* params,
                                    void* stream) {
  X3D_REQUIRE(table && pooled && params, "precise_bn_final: null pointer");
  X3D_REQUIRE(nlayers >= 1, "precise_bn_final: nlayers must be >= 1");
  X3D_REQUIRE(((uintptr_t)table % 8) == 0 && ((uintptr_t)pooled % 8) == 0 && ((uintptr_t)params % 4) == 0,
              "precise_bn_final: table / pooled / params misaligned");
  hipLaunchKernelGGL(precise_bn_final_kernel, dim3(nlayers, PBN_GRID_Y), dim3(PBN_BLOCK), 0, (hipStream_t)stream, table, pooled,
                     params);
  X3D_LAUNCH_CHECK("precise_bn_final");
  return X3D_OK;
}
