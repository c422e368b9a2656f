// dice_coeff counts with argmax / one-hot, per class, of one prediction or a batch of samples
// (PMU/dice_loss.py:5-12, trainer/unet_trainer.py:39-58).
#include "pmu_common.h"

namespace {

// Per-class Dice counts of one prediction: integer counters per thread (32-bit pixel decode),
// reduced by shuffles within each wave, through LDS over the block's 16 waves, and by one fp64
// atomicAdd per counter per block (integer-valued: order-independent).  The 64-bit pixel division
// and fp64 adds per pixel, and the per-counter LDS tree with 9 barriers each, made the previous
// version ~140 us per call for a 32 x 256^2 batch.
constexpr int DICE_T = 256, DICE_MAXB = 512;
// blockIdx.y: the prediction (sample) of a batched call — y + y * N K H W, its counters out + y * 3 K
__global__ __launch_bounds__(DICE_T) void dice_counts_kernel(const float* __restrict__ y, const float* __restrict__ mask,
                                                             int N, int K, int H, int W, double* __restrict__ out) {
  __shared__ unsigned red[DICE_T / 64][3 * HEAD_KMAX];
  y += (size_t)blockIdx.y * N * K * H * W;
  out += (size_t)blockIdx.y * 3 * K;
  const unsigned HW = (unsigned)H * (unsigned)W;
  const unsigned P = (unsigned)N * HW;  // < 2^31, host-checked
  const int KK = K == 1 ? 1 : K;
  unsigned loc[3 * HEAD_KMAX];
#pragma unroll
  for (int i = 0; i < 3 * HEAD_KMAX; ++i) loc[i] = 0u;
  double b0 = 0.0, b1 = 0.0, b2 = 0.0;  // K == 1
  // DB pixels per thread per round, all their loads issued before any is used (the per-pixel loop
  // was HBM-latency bound); fewer blocks, so the per-block counter atomics do not pile up on the
  // K*3 addresses (2048 blocks x 9 same-address fp64 atomics cost ~40 us per call)
  constexpr int DB = 8;
  const unsigned stride = gridDim.x * DICE_T;
  for (unsigned p0 = blockIdx.x * DICE_T + threadIdx.x; p0 < P; p0 += DB * stride) {
    float tv[DB], yv[DB][HEAD_KMAX];
#pragma unroll
    for (int b = 0; b < DB; ++b) {
      const unsigned p = p0 + b * stride;
      const bool ok = p < P;
      const unsigned pc = ok ? p : P - 1;
      const unsigned n = pc / HW, pix = pc - n * HW;
      tv[b] = ok ? mask[pc] : -1.f;
      const float* yp = y + (size_t)n * K * HW + pix;
#pragma unroll
      for (int k = 0; k < HEAD_KMAX; ++k) yv[b][k] = (k < KK) ? yp[(size_t)k * HW] : 0.f;
    }
#pragma unroll
    for (int b = 0; b < DB; ++b) {
      if (p0 + b * stride >= P) continue;
      const float t = tv[b];
      if (K == 1) {  // the mask is summed as the float it is (dice_coeff on (pred > 0.5) vs mask)
        const float pr = yv[b][0] > 0.5f ? 1.f : 0.f;
        b0 += (double)(pr * t); b1 += (double)pr; b2 += (double)t;
        continue;
      }
      float m = -INFINITY;
#pragma unroll
      for (int k = 0; k < HEAD_KMAX; ++k)
        if (k < K) m = fmaxf(m, yv[b][k]);
      float e[HEAD_KMAX];
      float sm = 0.f;
#pragma unroll
      for (int k = 0; k < HEAD_KMAX; ++k) {
        e[k] = 0.f;
        if (k < K) { e[k] = expf(yv[b][k] - m); sm += e[k]; }
      }
      int am = 0;
      float best = e[0] / sm;
#pragma unroll
      for (int k = 1; k < HEAD_KMAX; ++k) {
        if (k < K) { const float pk = e[k] / sm; if (pk > best) { best = pk; am = k; } }
      }
#pragma unroll
      for (int k = 0; k < HEAD_KMAX; ++k) {
        if (k < K) {
          const unsigned pr = (am == k) ? 1u : 0u, tk = (t == (float)k) ? 1u : 0u;
          loc[3 * k + 0] += pr & tk; loc[3 * k + 1] += pr; loc[3 * k + 2] += tk;
        }
      }
    }
  }
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  if (K == 1) {
    __shared__ double redd[DICE_T / 64][3];
    double v[3] = {b0, b1, b2};
#pragma unroll
    for (int i = 0; i < 3; ++i) {
      for (int o = 32; o > 0; o >>= 1) v[i] += __shfl_xor(v[i], o, 64);
      if (lane == 0) redd[wave][i] = v[i];
    }
    __syncthreads();
    if (threadIdx.x < 3) {
      double tsum = 0.0;
      for (int wv = 0; wv < DICE_T / 64; ++wv) tsum += redd[wv][threadIdx.x];
      atomicAdd(out + threadIdx.x, tsum);
    }
    return;
  }
#pragma unroll
  for (int i = 0; i < 3 * HEAD_KMAX; ++i) {
    if (i < 3 * KK) {
      unsigned v = loc[i];
      for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
      if (lane == 0) red[wave][i] = v;
    }
  }
  __syncthreads();
  if (threadIdx.x < 3 * KK) {
    unsigned long long tsum = 0;
    for (int wv = 0; wv < DICE_T / 64; ++wv) tsum += red[wv][threadIdx.x];
    atomicAdd(out + threadIdx.x, (double)tsum);
  }
}

}  // namespace

// S predictions of N x K x H x W against one mask: counts[S][3 K], zeroed here
static int dice_counts_launch(const float* y, const float* mask, int S, int N, int K, int H, int W, double* counts,
                              hipStream_t stream) {
  PMU_REQUIRE(y && mask && counts && S > 0 && N > 0 && K >= 1 && K <= HEAD_KMAX && H > 0 && W > 0);
  if (hipMemsetAsync(counts, 0, sizeof(double) * 3 * K * S, stream) != hipSuccess) return PMU_ERR_ARG;
  const long long P = (long long)N * H * W;
  PMU_REQUIRE(P < (1LL << 31));
  unsigned g = (unsigned)pmu_cdiv(P, DICE_T * 8);
  if (g > DICE_MAXB) g = DICE_MAXB;
  hipLaunchKernelGGL(dice_counts_kernel, dim3(g, (unsigned)S), dim3(DICE_T), 0, stream, y, mask, N, K, H, W, counts);
  PMU_CHECK_LAUNCH();
  return PMU_OK;
}

extern "C" int pmu_dice_counts(const float* y, const float* mask, int N, int K, int H, int W, double* counts,
                               void* stream) {
  return dice_counts_launch(y, mask, 1, N, K, H, W, counts, (hipStream_t)stream);
}

extern "C" int pmu_dice_counts_many(const float* y, const float* mask, int S, int N, int K, int H, int W,
                                    double* counts, void* stream) {
  PMU_REQUIRE(S <= 65535);
  return dice_counts_launch(y, mask, S, N, K, H, W, counts, (hipStream_t)stream);
}
