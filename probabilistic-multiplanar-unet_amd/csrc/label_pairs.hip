// Pairwise label-overlap counts for the generalised energy distance (pmu_label_pair_counts).
//
// maps [R][N][HW] u8: R label maps of the same N images (in use: S sample maps, then M ground truths).
//   inter[n][i][j][c] = #{p : maps[i][n][p] == c and maps[j][n][p] == c}     (symmetric; diagonal = cnt)
//   cnt[n][i][c]      = #{p : maps[i][n][p] == c}
// as float64 holding exact integers (the convention of pmu_dice_counts).  Labels >= K count nowhere; no
// one-hot is built.
//
// grid (G, N): a block walks 256-pixel steps of one image.  Per step each of its four waves reduces its
// 64 pixels to R x K ballot masks (bit p of mask[i][c] = [maps[i][p] == c]) in LDS; then the block's
// threads share the R(R+1)/2 x K (pair, class) items, item t + 256 m owned by thread t, each adding
// popcount(mask[i][c] & mask[j][c]) of the four waves to its own 32-bit LDS counter — no atomics inside the
// block, and a background-dominated map costs what any other does.  At the end each non-zero counter is
// one fp64 atomicAdd per output element (integer values: exact and order-independent, so every run gives
// the same integers); the outputs are zeroed by the entry.
#include "pmu_common.h"

namespace {

constexpr int LT = 256;              // threads per block (4 waves x 64 pixels per step)
constexpr int LP_MAXR = 64;
constexpr int LP_MAXK = 32;
constexpr int LP_MAXITEMS = PMU_LABEL_PAIRS_MAX_COUNTERS;  // 32-bit counters of a block: 32 KiB of LDS
constexpr int LP_BLOCKS = 2048;      // blocks of one launch, about

__global__ __launch_bounds__(LT) void label_pairs_kernel(const unsigned char* __restrict__ maps, int R, int N,
                                                         long long HW, int K, int items, int steps_per_block,
                                                         double* __restrict__ inter, double* __restrict__ cnt) {
  extern __shared__ __attribute__((aligned(16))) unsigned char lds[];
  // [masks u64 4 x R x K | counters u32 items | pair table u8 2 x R(R+1)/2]
  unsigned long long* masks = reinterpret_cast<unsigned long long*>(lds);
  unsigned* counters = reinterpret_cast<unsigned*>(masks + 4 * R * K);
  unsigned char* pij = reinterpret_cast<unsigned char*>(counters + items);
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int n = blockIdx.y;
  for (int e = tid; e < items; e += LT) counters[e] = 0u;
  for (int i = tid; i < R; i += LT) {  // pairs (i, j >= i) in row-major order
    int q = i * R - i * (i - 1) / 2;
    for (int j = i; j < R; ++j, ++q) {
      pij[2 * q] = (unsigned char)i;
      pij[2 * q + 1] = (unsigned char)j;
    }
  }
  const unsigned char* mn = maps + (long long)n * HW;
  const long long rstride = (long long)N * HW;
  const long long step0 = (long long)blockIdx.x * steps_per_block;
  for (int st = 0; st < steps_per_block; ++st) {
    const long long p0 = (step0 + st) * LT;
    if (p0 >= HW) break;  // block-uniform
    __syncthreads();      // the previous step's masks are read (first step: counters and table are set)
    const long long px = p0 + tid;
    unsigned long long* mw = masks + wave * R * K;
    for (int i = 0; i < R; ++i) {
      const int lab = px < HW ? (int)mn[i * rstride + px] : 255;  // 255 >= K: counted nowhere
      for (int c = 0; c < K; ++c) {
        const unsigned long long m = __ballot(lab == c);
        if (lane == 0) mw[i * K + c] = m;
      }
    }
    __syncthreads();
    for (int e = tid; e < items; e += LT) {
      const int q = e / K, c = e - q * K;
      const int a = pij[2 * q] * K + c, b = pij[2 * q + 1] * K + c;
      unsigned s = 0;
#pragma unroll
      for (int w = 0; w < 4; ++w) s += (unsigned)__popcll(masks[w * R * K + a] & masks[w * R * K + b]);
      counters[e] += s;
    }
  }
  // (each counter is touched by its own thread only: no barrier needed before the flush)
  for (int e = tid; e < items; e += LT) {
    const unsigned v = counters[e];
    if (!v) continue;
    const int q = e / K, c = e - q * K;
    const int i = pij[2 * q], j = pij[2 * q + 1];
    PMU_DCHECK(i <= j && j < R, PMU_DBG_INDEX);
    atomicAdd(inter + (((long long)n * R + i) * R + j) * K + c, (double)v);
    if (i != j)
      atomicAdd(inter + (((long long)n * R + j) * R + i) * K + c, (double)v);
    else
      atomicAdd(cnt + ((long long)n * R + i) * K + c, (double)v);
  }
}

}  // namespace

extern "C" int pmu_label_pair_counts(const unsigned char* maps, int R, int N, long long HW, int K, double* inter,
                                     double* cnt, void* stream) {
  PMU_REQUIRE(maps && inter && cnt && R >= 1 && R <= LP_MAXR && K >= 1 && K <= LP_MAXK && N >= 1 && N <= 65535);
  PMU_REQUIRE(HW >= 1 && HW < (1LL << 31));   // a block's 32-bit counters hold at most HW
  const int items = R * (R + 1) / 2 * K;
  PMU_REQUIRE(items <= LP_MAXITEMS);
  const long long steps = (HW + LT - 1) / LT;
  long long gx = LP_BLOCKS / N;
  if (gx < 1) gx = 1;
  if (gx > steps) gx = steps;
  const int spb = (int)((steps + gx - 1) / gx);
  gx = (steps + spb - 1) / spb;
  const size_t lds = (size_t)4 * R * K * 8 + (size_t)items * 4 + (size_t)R * (R + 1);
  PMU_REQUIRE(lds <= 64 * 1024);   // (implied by the bounds above: at most 22.5 + 32 + 4.1 KiB)
  hipStream_t st = (hipStream_t)stream;
  if (hipMemsetAsync(inter, 0, sizeof(double) * (size_t)N * R * R * K, st) != hipSuccess) return PMU_ERR_ARG;
  if (hipMemsetAsync(cnt, 0, sizeof(double) * (size_t)N * R * K, st) != hipSuccess) return PMU_ERR_ARG;
  hipLaunchKernelGGL(label_pairs_kernel, dim3((unsigned)gx, (unsigned)N), dim3(LT), lds, st, maps, R, N, HW, K, items,
                     spb, inter, cnt);
  PMU_CHECK_LAUNCH();
  return PMU_OK;
}
