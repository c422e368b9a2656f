// Learned multi-planar fusion on gfx950 (extends PMU/eval.py:157-203; the fusion model of Perslev et al.'s
// multi-planar U-Net): per-view, per-class weights W[v][c] and a per-class bias b[c],
//   z_c(x) = b_c + sum_v W[v][c] p_{v,c}(x),   fused = softmax(z),   label = first maximum of z,
// applied to the per-view stacks and, in the same pass, the cross-entropy of the fused softmax against the
// truth with its gradient in W and b — one streaming pass over the stacks per function evaluation of the
// host-side fit (pmu_hip/fusion.py fit_fusion).  DESIGN.md, "Learned fusion".
//
// Two kernels share the per-voxel arithmetic (fusion_voxel): fusion3_kernel reads the three standard-axis
// stacks as fuse3view_kernel does (data.hip: plane i, 32 rows j, every 32-wide k tile, view 2 transposed in
// LDS; the same fp32 softmax when logits != 0, pmu_fuse.h); fusion_oblique_kernel walks fuse_oblique_kernel's
// bricks (oblique.hip) and resamples every view through pmu_oblique_fuse.h, so a view's probability at a voxel
// is the same bits here as there.  The per-view Dice counts are today's: ballots per wave into LDS, one exact
// fp64 atomic of an integer per counter per block.
//
// Per voxel, all in fp64 and in this order, FP contraction off for the whole file:
//   z_c = b_c;  z_c = z_c + W[v][c] (double)p_{v,c} for v in view order (covering views only);
//   m = max_c z_c;  s = sum_c exp(z_c - m) in class order;  q_c = exp(z_c - m) / s;  label = first max of z;
//   t = (int)truth: outside [0, C) the voxel has fit weight 0, else w = cw[t];
//   l = w ((log s + m) - z_t);  dz_c = w (q_c - [c == t]).
// The sums [sum w, sum l, sum dz_c (C), sum dz_c p_{v,c} (V C)] are reproducible bit for bit: fp64 per thread,
// a fixed-order wave butterfly and block tree, one row per block in the caller's workspace, and a single
// block that totals the rows in a fixed order (fusion_sums_final_kernel).  No floating-point atomics.
#include "pmu_common.h"
#include "pmu_fuse.h"
#include "pmu_oblique_fuse.h"

#pragma clang fp contract(off)

namespace {

constexpr int FT = 32;                  // fusion3_kernel: tile edge (fuse3view_kernel's)
constexpr int BI = 4, BJ = 8, BK = 8;   // fusion_oblique_kernel: brick (fuse_oblique_kernel's)

// the parameters travel in the kernel arguments (read from the host arrays before the entry returns)
struct FusionParams {
  double W[FUSE_VMAX][FUSE_CMAX];
  double b[FUSE_CMAX];
  double cw[FUSE_CMAX];
};

// per-thread sums: [0] sum w, [1] sum l, [2 + c] sum dz_c, [2 + CB + v CB + c] sum dz_c p_{v,c}
template <int CB, int VB>
constexpr int acc_len() { return 2 + CB + VB * CB; }
// counters of a block: (intersection, |pred|) of VB + 1 volumes, then |truth|
template <int CB, int VB>
constexpr int cnt_len() { return (VB + 1) * CB * 2 + CB; }

// One voxel.  p[v][c]: the views' probabilities; cov: bit v set iff view v covers the voxel (and v < V);
// fit: the voxel enters the sums.  Fills q (the fused softmax) and returns the label.
template <int CB, int VB, int NA>
__device__ __forceinline__ int fusion_voxel(const FusionParams& par, int C, const float (&p)[VB][CB], unsigned cov,
                                            int t, bool fit, double (&q)[CB], double (&acc)[NA]) {
  static_assert(NA == acc_len<CB, VB>(), "accumulator layout");
  double z[CB];
#pragma unroll
  for (int c = 0; c < CB; ++c) {
    z[c] = 0.0;
    if (c >= C) continue;
    z[c] = par.b[c];
#pragma unroll
    for (int v = 0; v < VB; ++v)
      if (cov & (1u << v)) z[c] = z[c] + par.W[v][c] * (double)p[v][c];
  }
  double m = z[0];
  int label = 0;
#pragma unroll
  for (int c = 1; c < CB; ++c)
    if (c < C) {
      if (z[c] > m) label = c;
      m = fmax(m, z[c]);
    }
  double s = 0.0;
#pragma unroll
  for (int c = 0; c < CB; ++c) {
    q[c] = 0.0;
    if (c < C) { q[c] = exp(z[c] - m); s = s + q[c]; }
  }
#pragma unroll
  for (int c = 0; c < CB; ++c)
    if (c < C) q[c] = q[c] / s;
  if (fit) {
    // (selects, not indexed reads: an index that differs per lane would move the arrays out of registers)
    double zt = 0.0, w = 0.0;
#pragma unroll
    for (int c = 0; c < CB; ++c)
      if (c == t) { zt = z[c]; w = par.cw[c]; }
    const double l = w * ((log(s) + m) - zt);
    acc[0] += w;
    acc[1] += l;
#pragma unroll
    for (int c = 0; c < CB; ++c) {
      if (c >= C) break;
      const double dz = w * (q[c] - (c == t ? 1.0 : 0.0));
      acc[2 + c] += dz;
#pragma unroll
      for (int v = 0; v < VB; ++v)
        if (cov & (1u << v)) acc[2 + CB + v * CB + c] += dz * (double)p[v][c];
    }
  }
  return label;
}

// the counters of one scored volume w (its label lab) in the wave's LDS row; every lane of the wave calls it
template <int CB>
__device__ __forceinline__ void count_volume(int* row, int w, int C, bool valid, int lab, int t, int lane) {
  for (int c = 0; c < C; ++c) {
    const int np = wave_count(valid && lab == c), ni = wave_count(valid && lab == c && t == c);
    if (lane == 0) {
      row[(w * CB + c) * 2 + 0] += ni;
      row[(w * CB + c) * 2 + 1] += np;
    }
  }
}
template <int CB, int VB>
__device__ __forceinline__ void count_truth(int* row, int C, bool valid, int t, int lane) {
  for (int c = 0; c < C; ++c) {
    const int nt = wave_count(valid && t == c);
    if (lane == 0) row[(VB + 1) * CB * 2 + c] += nt;
  }
}

// counts[(V+1)][C][3] += the block's counters: one atomic per non-zero counter (integers in fp64: exact)
template <int CB, int VB, int NC>
__device__ __forceinline__ void flush_counts(const int (*red)[NC], int V, int C, double* counts) {
  static_assert(NC == cnt_len<CB, VB>(), "counter layout");
  const int tid = threadIdx.x;
  if (tid < (V + 1) * C * 3) {
    const int w = tid / (3 * C), rem = tid - w * 3 * C, c = rem / 3, q = rem - c * 3;
    const int slot = (q == 2) ? (VB + 1) * CB * 2 + c : (w * CB + c) * 2 + q;
    const int x = red[0][slot] + red[1][slot] + red[2][slot] + red[3][slot];
    if (x) atomicAdd(counts + (w * C + c) * 3 + q, (double)x);
  }
}

// The block's row of the K = 2 + C + V C sums: every accumulator through the xor butterfly of its wave (the
// same operands meet in the same order in every run), the four wave totals added in wave order.
template <int CB, int VB, int NA>
__device__ __forceinline__ void flush_sums(double (&acc)[NA], double (*sred)[NA], int V, int C,
                                           double* __restrict__ row) {
  static_assert(NA == acc_len<CB, VB>(), "accumulator layout");
  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
#pragma unroll
  for (int n = 0; n < NA; ++n) {
    const int c = n < 2 ? 0 : (n - 2) % CB, v = n < 2 + CB ? 0 : (n - 2 - CB) / CB;
    if (c >= C || v >= V) continue;   // wave-uniform
    double x = acc[n];
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) x += __shfl_xor(x, o, 64);
    if (lane == 0) sred[wv][n] = x;
  }
  __syncthreads();
  const int K = 2 + C + V * C;
  if (tid < K) {
    int n = tid;
    if (tid >= 2 + C) {
      const int kk = tid - 2 - C, v = kk / C;
      n = 2 + CB + v * CB + (kk - v * C);
    }
    row[tid] = ((sred[0][n] + sred[1][n]) + sred[2][n]) + sred[3][n];
  }
}

// sums[k] = (accumulate ? sums[k] : 0) + sum over the rows of ws[r][k], rows in a fixed order: thread t takes
// rows t, t + 256, ..., then the butterfly and the four waves in order.  One block.
__global__ __launch_bounds__(256) void fusion_sums_final_kernel(const double* __restrict__ ws, int rows, int K,
                                                                double* __restrict__ sums, int accumulate) {
  __shared__ double red[4];
  const int tid = threadIdx.x;
  for (int k = 0; k < K; ++k) {
    double x = 0.0;
    for (int r = tid; r < rows; r += 256) x += ws[(long long)r * K + k];
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) x += __shfl_xor(x, o, 64);
    if ((tid & 63) == 0) red[tid >> 6] = x;
    __syncthreads();
    if (tid == 0) {
      const double tot = ((red[0] + red[1]) + red[2]) + red[3];
      sums[k] = accumulate ? sums[k] + tot : tot;
    }
    __syncthreads();
  }
}

// ---------------- the three standard views ----------------
// v0 [D0][C][D1][D2], v1 [D1][C][D0][D2], v2 [D2][C][D0][D1], truth [D0][D1][D2] (pmu_fuse3view's operands)
struct Fusion3Args {
  const float *v0, *v1, *v2, *truth;
  int D0, D1, D2, C, logits;
  float* prob;
  int* label;
  double* counts;
  double* ws;     // [blocks][K] rows of sums, or null
  FusionParams par;
};

template <int CB>
__global__ __launch_bounds__(256) void fusion3_kernel(Fusion3Args a) {
  constexpr int VB = 3, NA = acc_len<CB, VB>(), NC = cnt_len<CB, VB>();
  __shared__ float t2[CB][FT][FT + 1];
  __shared__ int red[4][NC];
  __shared__ double sred[4][NA];
  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
  const int i = blockIdx.z, j0 = blockIdx.y * FT;
  const int tx = tid & 31, ty = tid >> 5;
  const int C = a.C;
  const long long P01 = (long long)a.D0 * a.D1, P02 = (long long)a.D0 * a.D2, P12 = (long long)a.D1 * a.D2;
  for (int e = tid; e < 4 * NC; e += 256) (&red[0][0])[e] = 0;
  double acc[NA];
#pragma unroll
  for (int n = 0; n < NA; ++n) acc[n] = 0.0;
  for (int k0 = 0; k0 < a.D2; k0 += FT) {
    __syncthreads();  // previous tile's t2 reads done (and red zeroed)
    for (int r = ty; r < FT; r += 8) {
      const int k = k0 + r, j = j0 + tx;
      const bool in = k < a.D2 && j < a.D1;
      PMU_DCHECK(!in || ((long long)k * C + C - 1) * P01 + (long long)i * a.D1 + j < (long long)a.D2 * C * P01,
                 PMU_DBG_OPERAND);
#pragma unroll
      for (int c = 0; c < CB; ++c)
        if (c < C) t2[c][r][tx] = in ? a.v2[((long long)k * C + c) * P01 + (long long)i * a.D1 + j] : 0.f;
    }
    __syncthreads();
    for (int r = ty; r < FT; r += 8) {   // four rounds for every thread: all lanes reach the ballots
      const int j = j0 + r, k = k0 + tx;
      const bool valid = j < a.D1 && k < a.D2;
      const long long vox = ((long long)i * a.D1 + j) * a.D2 + k;
      PMU_DCHECK(!valid || (vox >= 0 && vox < (long long)a.D0 * P12), PMU_DBG_OUTPUT);
      float p[VB][CB];
#pragma unroll
      for (int c = 0; c < CB; ++c) {
        p[0][c] = p[1][c] = p[2][c] = 0.f;
        if (c < C && valid) {
          p[0][c] = a.v0[((long long)i * C + c) * P12 + (long long)j * a.D2 + k];
          p[1][c] = a.v1[((long long)j * C + c) * P02 + (long long)i * a.D2 + k];
          p[2][c] = t2[c][tx][r];
        }
      }
      if (a.logits) {
        softmax_inplace(p[0], C);
        softmax_inplace(p[1], C);
        softmax_inplace(p[2], C);
      }
      const int t = valid ? (int)a.truth[vox] : -1;
      double q[CB];
      int lab = 0;
      if (valid) lab = fusion_voxel<CB, VB, NA>(a.par, C, p, 7u, t, a.ws != nullptr && t >= 0 && t < C, q, acc);
      if (a.counts) {
        count_volume<CB>(red[wv], 0, C, valid, argmax_first(p[0], C), t, lane);
        count_volume<CB>(red[wv], 1, C, valid, argmax_first(p[1], C), t, lane);
        count_volume<CB>(red[wv], 2, C, valid, argmax_first(p[2], C), t, lane);
        count_volume<CB>(red[wv], 3, C, valid, lab, t, lane);
        count_truth<CB, VB>(red[wv], C, valid, t, lane);
      }
      if (valid) {
        if (a.prob) {
#pragma unroll
          for (int c = 0; c < CB; ++c)
            if (c < C) a.prob[((long long)i * C + c) * P12 + (long long)j * a.D2 + k] = (float)q[c];
        }
        if (a.label) a.label[vox] = lab;
      }
    }
  }
  __syncthreads();
  if (a.counts) flush_counts<CB, VB, NC>(red, 3, C, a.counts);
  if (a.ws) {
    const int blk = blockIdx.z * gridDim.y + blockIdx.y;
    PMU_DCHECK(blk >= 0 && blk < (int)(gridDim.y * gridDim.z), PMU_DBG_WORKSPACE);
    flush_sums<CB, VB, NA>(acc, sred, 3, C, a.ws + (long long)blk * (2 + C + 3 * C));
  }
}

// ---------------- oblique views ----------------
// stacks [V][P][C][P][P], frames [V][9], truth [p0][p1][p2] (pmu_fuse_oblique's operands)
struct FusionObliqueArgs {
  const float* stacks;
  const double* frames;
  const float* truth;
  int V, C, P, p0, p1, p2;
  double h;
  float* prob;
  int* label;
  int* cover;
  double* counts;
  double* ws;
  FusionParams par;
};

template <int CB, int VB>
__global__ __launch_bounds__(256) void fusion_oblique_kernel(FusionObliqueArgs a) {
  constexpr int NA = acc_len<CB, VB>(), NC = cnt_len<CB, VB>();
  __shared__ int red[4][NC];
  __shared__ double sred[4][NA];
  __shared__ double fr[VB][9];
  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
  const int V = a.V, C = a.C, P = a.P;
  for (int e = tid; e < 4 * NC; e += 256) (&red[0][0])[e] = 0;
  for (int e = tid; e < 9 * V; e += 256) (&fr[0][0])[e] = a.frames[e];
  __syncthreads();
  const int i = blockIdx.y * BI + (tid >> 6);
  const int j = blockIdx.x * BJ + ((tid >> 3) & 7);
  const double d0 = (double)i - (double)(a.p0 - 1) / 2.0, d1 = (double)j - (double)(a.p1 - 1) / 2.0;
  const long long P2 = (long long)P * P, plane = (long long)a.p1 * a.p2;
  double acc[NA];
#pragma unroll
  for (int n = 0; n < NA; ++n) acc[n] = 0.0;
  for (int k0 = 0; k0 < a.p2; k0 += BK) {
    const int k = k0 + (tid & 7);
    const bool valid = i < a.p0 && j < a.p1 && k < a.p2;
    const double d2 = (double)k - (double)(a.p2 - 1) / 2.0;
    const long long vox = ((long long)i * a.p1 + j) * a.p2 + k;
    PMU_DCHECK(!valid || (vox >= 0 && vox < (long long)a.p0 * plane), PMU_DBG_OUTPUT);
    const int t = valid ? (int)a.truth[vox] : -1;
    float p[VB][CB];
    unsigned cov = 0;
    int cnt = 0;
#pragma unroll
    for (int v = 0; v < VB; ++v) {
#pragma unroll
      for (int c = 0; c < CB; ++c) p[v][c] = 0.f;
      if (v >= V) continue;   // wave-uniform
      ObliqueCell cell;
      int mv = 0;   // the view's label: 0 where it does not cover the voxel
      if (oblique_cell(fr[v], d0, d1, d2, a.h, P, valid, cell)) {
        const float* st = a.stacks + (long long)v * P * C * P2;
        cov |= 1u << v;
        ++cnt;
        float best = 0.f;
#pragma unroll
        for (int c = 0; c < CB; ++c) {
          if (c >= C) break;
          p[v][c] = oblique_prob(st, cell, C, c, P2);
          if (c == 0 || p[v][c] > best) { best = p[v][c]; mv = c; }
        }
      }
      if (a.counts) count_volume<CB>(red[wv], v, C, valid, mv, t, lane);
    }
    // a voxel no view covers: probability 0, label 0, outside the sums
    double q[CB];
#pragma unroll
    for (int c = 0; c < CB; ++c) q[c] = 0.0;
    int lab = 0;
    if (cov) lab = fusion_voxel<CB, VB, NA>(a.par, C, p, cov, t, a.ws != nullptr && t >= 0 && t < C, q, acc);
    if (a.counts) {
      count_volume<CB>(red[wv], V, C, valid, lab, t, lane);
      count_truth<CB, VB>(red[wv], C, valid, t, lane);
    }
    if (valid) {
      if (a.prob) {
#pragma unroll
        for (int c = 0; c < CB; ++c)
          if (c < C) a.prob[((long long)i * C + c) * plane + (long long)j * a.p2 + k] = (float)q[c];
      }
      if (a.label) a.label[vox] = lab;
      if (a.cover) a.cover[vox] = cnt;
    }
  }
  __syncthreads();
  if (a.counts) flush_counts<CB, VB, NC>(red, V, C, a.counts);
  if (a.ws) {
    const int blk = blockIdx.y * gridDim.x + blockIdx.x;
    PMU_DCHECK(blk >= 0 && blk < (int)(gridDim.x * gridDim.y), PMU_DBG_WORKSPACE);
    flush_sums<CB, VB, NA>(acc, sred, V, C, a.ws + (long long)blk * (2 + C + V * C));
  }
}

// W[v][c] then b[c] from the host array, cw (null: ones); false if a value is not finite
bool load_params(FusionParams& par, const double* params, const double* cw, int V, int C) {
  memset(&par, 0, sizeof(par));
  for (int v = 0; v < V; ++v)
    for (int c = 0; c < C; ++c) par.W[v][c] = params[v * C + c];
  for (int c = 0; c < C; ++c) {
    par.b[c] = params[V * C + c];
    par.cw[c] = cw ? cw[c] : 1.0;
  }
  for (int n = 0; n < V * C + C; ++n)
    if (!(params[n] - params[n] == 0.0)) return false;
  for (int c = 0; c < C; ++c)
    if (!(par.cw[c] >= 0.0 && par.cw[c] - par.cw[c] == 0.0)) return false;
  return true;
}

int launch_final(const double* ws, long long rows, int K, double* sums, int accumulate, hipStream_t st) {
  hipLaunchKernelGGL(fusion_sums_final_kernel, dim3(1), dim3(256), 0, st, ws, (int)rows, K, sums, accumulate);
  PMU_CHECK_LAUNCH();
  return PMU_OK;
}

long long fusion3_rows(int D0, int D1) { return (long long)D0 * pmu_cdiv(D1, FT); }
long long oblique_rows(int p0, int p1) { return (long long)pmu_cdiv(p0, BI) * pmu_cdiv(p1, BJ); }

}  // namespace

extern "C" size_t pmu_fusion3_ws(int D0, int D1, int D2, int C) {
  if (D0 <= 0 || D1 <= 0 || D2 <= 0 || C < 2 || C > FUSE_CMAX) return 0;
  return sizeof(double) * (size_t)fusion3_rows(D0, D1) * (size_t)(2 + C + 3 * C);
}

extern "C" int pmu_fusion3_eval(const float* v0, const float* v1, const float* v2, const float* truth, int D0, int D1,
                                int D2, int C, int logits, const double* params, const double* cw, float* prob,
                                int* label, double* counts, double* sums, int accumulate, void* ws, size_t ws_bytes,
                                void* stream) {
  PMU_REQUIRE(v0 && v1 && v2 && truth && params && D0 > 0 && D1 > 0 && D2 > 0 && C >= 2 && C <= FUSE_CMAX &&
              D0 <= 65535 && pmu_cdiv(D1, FT) <= 65535);
  PMU_REQUIRE(fusion3_rows(D0, D1) < (1LL << 31));
  PMU_REQUIRE(!sums || (ws && ((uintptr_t)ws & 7) == 0 && ws_bytes >= pmu_fusion3_ws(D0, D1, D2, C)));
  Fusion3Args a{v0, v1, v2, truth, D0, D1, D2, C, logits, prob, label, counts, sums ? (double*)ws : nullptr, {}};
  PMU_REQUIRE(load_params(a.par, params, cw, 3, C));
  hipStream_t st = (hipStream_t)stream;
  if (counts) {
    const hipError_t e = hipMemsetAsync(counts, 0, sizeof(double) * 4 * C * 3, st);
    if (e != hipSuccess) return (int)e;
  }
  const dim3 grid(1u, (unsigned)pmu_cdiv(D1, FT), (unsigned)D0);
  if (C <= 4)
    hipLaunchKernelGGL(fusion3_kernel<4>, grid, dim3(256), 0, st, a);
  else
    hipLaunchKernelGGL(fusion3_kernel<8>, grid, dim3(256), 0, st, a);
  PMU_CHECK_LAUNCH();
  if (sums) return launch_final(a.ws, fusion3_rows(D0, D1), 2 + C + 3 * C, sums, accumulate, st);
  return PMU_OK;
}

extern "C" size_t pmu_fusion_oblique_ws(int V, int C, int p0, int p1, int p2) {
  if (p0 <= 0 || p1 <= 0 || p2 <= 0 || C < 2 || C > FUSE_CMAX || V < 1 || V > FUSE_VMAX) return 0;
  return sizeof(double) * (size_t)oblique_rows(p0, p1) * (size_t)(2 + C + V * C);
}

extern "C" int pmu_fusion_oblique_eval(const float* stacks, const double* frames, int V, int C, int P, double h,
                                       const float* truth, int p0, int p1, int p2, const double* params,
                                       const double* cw, float* prob, int* label, int* cover, double* counts,
                                       double* sums, int accumulate, void* ws, size_t ws_bytes, void* stream) {
  PMU_REQUIRE(stacks && frames && truth && params && V >= 1 && V <= FUSE_VMAX && C >= 2 && C <= FUSE_CMAX && P >= 2 &&
              P <= 32768 && h > 0.0 && p0 > 0 && p1 > 0 && p2 > 0);
  PMU_REQUIRE(pmu_cdiv(p0, BI) <= 65535 && oblique_rows(p0, p1) < (1LL << 31));
  PMU_REQUIRE(!sums || (ws && ((uintptr_t)ws & 7) == 0 && ws_bytes >= pmu_fusion_oblique_ws(V, C, p0, p1, p2)));
  FusionObliqueArgs a{stacks, frames, truth, V, C, P, p0, p1, p2, h, prob, label, cover, counts,
                      sums ? (double*)ws : nullptr, {}};
  PMU_REQUIRE(load_params(a.par, params, cw, V, C));
  hipStream_t st = (hipStream_t)stream;
  if (counts) {
    const hipError_t e = hipMemsetAsync(counts, 0, sizeof(double) * (V + 1) * C * 3, st);
    if (e != hipSuccess) return (int)e;
  }
  const dim3 grid((unsigned)pmu_cdiv(p1, BJ), (unsigned)pmu_cdiv(p0, BI));
  if (C <= 4 && V <= 3)
    hipLaunchKernelGGL((fusion_oblique_kernel<4, 3>), grid, dim3(256), 0, st, a);
  else if (C <= 4)
    hipLaunchKernelGGL((fusion_oblique_kernel<4, 8>), grid, dim3(256), 0, st, a);
  else if (V <= 3)
    hipLaunchKernelGGL((fusion_oblique_kernel<8, 3>), grid, dim3(256), 0, st, a);
  else
    hipLaunchKernelGGL((fusion_oblique_kernel<8, 8>), grid, dim3(256), 0, st, a);
  PMU_CHECK_LAUNCH();
  if (sums) return launch_final(a.ws, oblique_rows(p0, p1), 2 + C + V * C, sums, accumulate, st);
  return PMU_OK;
}
