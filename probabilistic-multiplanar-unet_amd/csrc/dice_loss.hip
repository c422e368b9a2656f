// Soft Dice training loss (row a6): the differentiable form of dice_coeff (PMU/dice_loss.py:5-12, the
// same 1e-6 smoothing).  The reference only ever reports Dice; training on it is this build's addition
// (the "wavefront-reduced dice_loss.py" and the KL+Dice configuration of BASELINE.json).
//
//   K >= 2: p = softmax_K(x[n][:][i]), targets int64;  K == 1: p = x (act 0) or sigmoid(x) (act 1),
//   the target a float mask used by value.  Over the valid pixels (t != ignore_index; a target outside
//   [0, K) is excluded too and makes the loss NaN), per class and per pooling group r (the whole batch,
//   or one image with per_image):
//     I = sum p [t = k]   P = sum p   T = sum [t = k]        (K == 1: I = sum p t, T = sum t)
//     S = P + T + eps     D = (2 I + eps) / S                 loss = 1 - mean D over r, k >= first_class
//   backward, M the number of averaged terms, a = 2 / (M S), b = (2 I + eps) / (M S^2) (0 for an
//   excluded class), c_k(i) = b_k - a_k [t_i = k]:
//     K >= 2: dx_j = g p_j (c_j - sum_k p_k c_k)    act 1: dx = g c p (1 - p)    act 0: dx = g c
//
// Forward: grid (G, N) — a block never straddles images, so one kernel serves both poolings — each
// thread walking its grid-stride pixels (four consecutive ones per 16-byte load where the planes are
// aligned) with P and I in fp64 registers and T as an integer count; a 64-lane DPP / shuffle butterfly
// per wave, the four waves through LDS in fixed order, one partial row per block; then one block sums
// the rows in a fixed order in fp64 and forms D, the loss and (a, b).  No atomics: bit-identical runs.
// Backward: one elementwise pass, (a, b) read wave-uniformly.  HBM-bound: (4K + 8) N HW bytes forward,
// (8K + 8) N HW backward.
#include "pmu_common.h"

namespace {

constexpr int DT = 256;         // threads per block
constexpr int DMAXK = 8;        // classes kept in registers
constexpr int DFWD_BLOCKS = 1024;  // forward blocks of one launch: 4 per CU on 256 CUs
constexpr int DBWD_BLOCKS = 2048;
constexpr int DFWD_PX = 2048;   // pixels per forward block below the cap (two 4-pixel rounds per thread)
constexpr int DBWD_PX = 1024;
constexpr int DFT = 1024;       // threads of the finalize block
constexpr double DEPS = 1e-6;   // pmu_hip.metrics.SMOOTH

typedef long long ll2 __attribute__((ext_vector_type(2)));

int grid_x(int N, long long HW, int px, int max_blocks) {
  long long g = (HW + px - 1) / px, cap = max_blocks / N;
  if (cap < 1) cap = 1;
  if (g > cap) g = cap;
  return (int)g;
}

// workspace: [coef float R_max x K x 2 | sums double R_max x W | partials double N x G x W], R_max = N,
// W = 3K + 1 (per class I, P, T; then the count of out-of-range targets)
struct DiceWs {
  float* coef;
  double* sums;
  double* part;
  size_t bytes;
};
DiceWs dice_ws(void* ws, int N, int K, long long HW) {
  const int W = 3 * K + 1;
  const size_t coef_b = (size_t)N * K * 2 * sizeof(float);   // a multiple of 8
  const size_t sums_b = (size_t)N * W * sizeof(double);
  const size_t part_b = (size_t)N * grid_x(N, HW, DFWD_PX, DFWD_BLOCKS) * W * sizeof(double);
  char* b = (char*)ws;
  return DiceWs{(float*)b, (double*)(b + coef_b), (double*)(b + coef_b + sums_b), coef_b + sums_b + part_b};
}

template <int CTRL>
__device__ __forceinline__ double dpp_f64(double v) {
  const int lo = __builtin_amdgcn_update_dpp(0, __double2loint(v), CTRL, 0xF, 0xF, true);
  const int hi = __builtin_amdgcn_update_dpp(0, __double2hiint(v), CTRL, 0xF, 0xF, true);
  return __hiloint2double(hi, lo);
}
// pmu_group_sum in fp64: the sum over each group of CQ consecutive lanes, in every lane of the group,
// in the xor butterfly's order.  Every lane of the wave must be active.
__device__ __forceinline__ double group_sum_f64(double v, int CQ) {
  if (CQ >= 2) v += dpp_f64<0xB1>(v);    // quad_perm [1,0,3,2]
  if (CQ >= 4) v += dpp_f64<0x4E>(v);    // quad_perm [2,3,0,1]
  if (CQ >= 8) v += dpp_f64<0x141>(v);   // row_half_mirror
  if (CQ >= 16) v += dpp_f64<0x140>(v);  // row_mirror
  if (CQ >= 32) v += __shfl_xor(v, 16, 64);
  if (CQ >= 64) v += __shfl_xor(v, 32, 64);
  return v;
}

// the block's sums of vals[0..W) into part[0..W): wave butterflies, then the four waves in order
template <int W>
__device__ __forceinline__ void block_sums(const double (&vals)[W], double* __restrict__ part) {
  __shared__ double red[DT / 64][W];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
  for (int j = 0; j < W; ++j) {
    const double s = group_sum_f64(vals[j], 64);
    if (lane == 0) red[wave][j] = s;
  }
  __syncthreads();
  if ((int)threadIdx.x < W) {
    const int j = threadIdx.x;
    part[j] = ((red[0][j] + red[1][j]) + red[2][j]) + red[3][j];
  }
}

template <int K>
struct McAcc {
  double P[K], I[K];
  unsigned T[K];
  unsigned bad;
};

template <int K>
__device__ __forceinline__ void mc_fwd_px(const float (&xv)[K], long long tv, long long ignore, McAcc<K>& a) {
  if (tv == ignore) return;
  // a target outside [0, K) that is not ignore_index (see ce_fwd_kernel): left out of the sums, counted,
  // and the finalize kernel turns a non-zero count into a NaN loss; the debug build records the index
  const bool tok = tv >= 0 && tv < K;
  PMU_DCHECK(tok, PMU_DBG_INDEX);
  a.bad += tok ? 0u : 1u;
  float m = -INFINITY;
#pragma unroll
  for (int k = 0; k < K; ++k) m = fmaxf(m, xv[k]);
  float e[K], se = 0.f;
#pragma unroll
  for (int k = 0; k < K; ++k) {
    e[k] = expf(xv[k] - m);
    se += e[k];
  }
  const float inv = 1.f / se;
#pragma unroll
  for (int k = 0; k < K; ++k) {
    const double p = tok ? (double)(e[k] * inv) : 0.0;
    const bool hit = tok && (int)tv == k;
    a.P[k] += p;
    a.I[k] += hit ? p : 0.0;
    a.T[k] += hit ? 1u : 0u;
  }
}

// x[N][K][HW] logits, tgt[N][HW]; part[n][blockIdx.x][3K + 1]
template <int K>
__global__ __launch_bounds__(DT) void softdice_fwd_kernel(const float* __restrict__ x, const long long* __restrict__ tgt,
                                                          long long HW, long long ignore, int vec,
                                                          double* __restrict__ part) {
  const int n = blockIdx.y;
  const float* xn = x + (long long)n * K * HW;
  const long long* tn = tgt + (long long)n * HW;
  McAcc<K> a;
#pragma unroll
  for (int k = 0; k < K; ++k) {
    a.P[k] = 0.0;
    a.I[k] = 0.0;
    a.T[k] = 0u;
  }
  a.bad = 0u;
  const long long t0 = (long long)blockIdx.x * DT + threadIdx.x, step = (long long)gridDim.x * DT;
  float xv[K];
  if (vec) {  // HW % 4 == 0 and both bases 16-byte aligned, so every class plane of every image is
    const long long Q = HW >> 2;
    for (long long q = t0; q < Q; q += step) {
      float4 v[K];
#pragma unroll
      for (int k = 0; k < K; ++k) v[k] = pmu_ld4(xn + k * HW + 4 * q);
      const ll2 ta = *reinterpret_cast<const ll2*>(tn + 4 * q), tb = *reinterpret_cast<const ll2*>(tn + 4 * q + 2);
#pragma unroll
      for (int k = 0; k < K; ++k) xv[k] = v[k].x;
      mc_fwd_px<K>(xv, ta.x, ignore, a);
#pragma unroll
      for (int k = 0; k < K; ++k) xv[k] = v[k].y;
      mc_fwd_px<K>(xv, ta.y, ignore, a);
#pragma unroll
      for (int k = 0; k < K; ++k) xv[k] = v[k].z;
      mc_fwd_px<K>(xv, tb.x, ignore, a);
#pragma unroll
      for (int k = 0; k < K; ++k) xv[k] = v[k].w;
      mc_fwd_px<K>(xv, tb.y, ignore, a);
    }
  } else {
    for (long long p = t0; p < HW; p += step) {
#pragma unroll
      for (int k = 0; k < K; ++k) xv[k] = xn[k * HW + p];
      mc_fwd_px<K>(xv, tn[p], ignore, a);
    }
  }
  double vals[3 * K + 1];
#pragma unroll
  for (int k = 0; k < K; ++k) {
    vals[3 * k] = a.I[k];
    vals[3 * k + 1] = a.P[k];
    vals[3 * k + 2] = (double)a.T[k];
  }
  vals[3 * K] = (double)a.bad;
  block_sums<3 * K + 1>(vals, part + ((long long)n * gridDim.x + blockIdx.x) * (3 * K + 1));
}

__device__ __forceinline__ float bin_prob(float xv, int act) { return act ? 1.f / (1.f + expf(-xv)) : xv; }

// K == 1: x[N][HW] a probability (act 0) or a logit (act 1), t[N][HW] a float mask; part[n][blockIdx.x][4]
__global__ __launch_bounds__(DT) void softdice_fwd_bin_kernel(const float* __restrict__ x, const float* __restrict__ t,
                                                              long long HW, int act, int vec,
                                                              double* __restrict__ part) {
  const int n = blockIdx.y;
  const float* xn = x + (long long)n * HW;
  const float* tn = t + (long long)n * HW;
  double I = 0.0, P = 0.0, T = 0.0;
  const long long t0 = (long long)blockIdx.x * DT + threadIdx.x, step = (long long)gridDim.x * DT;
  if (vec) {
    const long long Q = HW >> 2;
    for (long long q = t0; q < Q; q += step) {
      const float4 xv = pmu_ld4(xn + 4 * q), tv = pmu_ld4(tn + 4 * q);
      const double p0 = (double)bin_prob(xv.x, act), p1 = (double)bin_prob(xv.y, act);
      const double p2 = (double)bin_prob(xv.z, act), p3 = (double)bin_prob(xv.w, act);
      I += p0 * (double)tv.x; P += p0; T += (double)tv.x;
      I += p1 * (double)tv.y; P += p1; T += (double)tv.y;
      I += p2 * (double)tv.z; P += p2; T += (double)tv.z;
      I += p3 * (double)tv.w; P += p3; T += (double)tv.w;
    }
  } else {
    for (long long p = t0; p < HW; p += step) {
      const double pv = (double)bin_prob(xn[p], act), tv = (double)tn[p];
      I += pv * tv;
      P += pv;
      T += tv;
    }
  }
  const double vals[4] = {I, P, T, 0.0};
  block_sums<4>(vals, part + ((long long)n * gridDim.x + blockIdx.x) * 4);
}

// One block.  sums[r][W] = the partial rows [r cnt, (r + 1) cnt) of part[.][W] added up, L lanes per sum
// (lane l rows l, l + L, ... in order, then the butterfly: an order fixed by the shapes); then per (r, k)
// D, a, b in fp64 -> coef[r][k][2] (fp32), and loss[0] = 1 - mean D over the classes >= first (NaN when an
// out-of-range target was counted).
__global__ __launch_bounds__(DFT) void softdice_final_kernel(const double* __restrict__ part, int R, int cnt, int K,
                                                             int first, int L, double* __restrict__ sums,
                                                             float* __restrict__ coef, float* __restrict__ loss) {
  __shared__ double ra[DFT], rb[DFT];
  const int tid = threadIdx.x, W = 3 * K + 1, items = R * W;
  const int sub = tid & (L - 1), grp = tid / L, ngrp = DFT / L;
  for (int it0 = 0; it0 < items; it0 += ngrp) {  // (a block-uniform trip count: the butterfly needs every lane)
    const int it = it0 + grp;
    double s = 0.0;
    if (it < items) {
      const int r = it / W, j = it - r * W;
      const double* p = part + (long long)r * cnt * W + j;
#pragma unroll 4
      for (int g = sub; g < cnt; g += L) s += p[(long long)g * W];
    }
    s = group_sum_f64(s, L);
    if (it < items && sub == 0) sums[it] = s;
  }
  __syncthreads();   // (sums written and read by this block only)
  const double M = (double)R * (double)(K - first);
  double acc = 0.0, bad = 0.0;
  for (int i = tid; i < R * K; i += DFT) {
    const int r = i / K, k = i - r * K;
    const double* s = sums + (long long)r * W + 3 * k;
    const double S = s[1] + s[2] + DEPS, num = 2.0 * s[0] + DEPS;
    const bool inc = k >= first;
    coef[2 * i] = inc ? (float)(2.0 / (M * S)) : 0.f;
    coef[2 * i + 1] = inc ? (float)(num / (M * S * S)) : 0.f;
    if (inc) acc += num / S;
    if (k == 0) bad += sums[(long long)r * W + 3 * K];
  }
  ra[tid] = acc;
  rb[tid] = bad;
  __syncthreads();
  for (int o = DFT / 2; o > 0; o >>= 1) {
    if (tid < o) {
      ra[tid] += ra[tid + o];
      rb[tid] += rb[tid + o];
    }
    __syncthreads();
  }
  if (tid == 0) loss[0] = rb[0] > 0.0 ? __builtin_nanf("") : (float)(1.0 - ra[0] / M);
}

template <int K>
__device__ __forceinline__ void mc_bwd_px(const float (&xv)[K], long long tv, long long ignore, const float (&ca)[K],
                                          const float (&cb)[K], float g, float (&out)[K]) {
  if (tv == ignore) {
#pragma unroll
    for (int k = 0; k < K; ++k) out[k] = 0.f;
    return;
  }
  if (tv < 0 || tv >= K) {  // out-of-range target (see mc_fwd_px): NaN gradient at this pixel
#pragma unroll
    for (int k = 0; k < K; ++k) out[k] = __builtin_nanf("");
    return;
  }
  float m = -INFINITY;
#pragma unroll
  for (int k = 0; k < K; ++k) m = fmaxf(m, xv[k]);
  float e[K], se = 0.f;
#pragma unroll
  for (int k = 0; k < K; ++k) {
    e[k] = expf(xv[k] - m);
    se += e[k];
  }
  const float inv = 1.f / se;
  float c[K], dot = 0.f;
#pragma unroll
  for (int k = 0; k < K; ++k) {
    e[k] *= inv;
    c[k] = cb[k] - ((int)tv == k ? ca[k] : 0.f);
    dot = fmaf(e[k], c[k], dot);
  }
#pragma unroll
  for (int k = 0; k < K; ++k) out[k] = g * e[k] * (c[k] - dot);
}

template <int K>
__global__ __launch_bounds__(DT) void softdice_bwd_kernel(const float* __restrict__ x, const long long* __restrict__ tgt,
                                                          long long HW, long long ignore, int per_image,
                                                          const float* __restrict__ coef, const float* __restrict__ gout,
                                                          int vec, float* __restrict__ dx) {
  const int n = blockIdx.y;
  const float* xn = x + (long long)n * K * HW;
  float* dn = dx + (long long)n * K * HW;
  const long long* tn = tgt + (long long)n * HW;
  const float* cf = coef + (per_image ? (long long)n * K * 2 : 0);   // block-uniform: scalar loads
  float ca[K], cb[K];
#pragma unroll
  for (int k = 0; k < K; ++k) {
    ca[k] = cf[2 * k];
    cb[k] = cf[2 * k + 1];
  }
  const float g = gout[0];
  const long long t0 = (long long)blockIdx.x * DT + threadIdx.x, step = (long long)gridDim.x * DT;
  float xv[K], o[K];
  if (vec) {
    const long long Q = HW >> 2;
    for (long long q = t0; q < Q; q += step) {
      float4 v[K], r[K];
#pragma unroll
      for (int k = 0; k < K; ++k) v[k] = pmu_ld4(xn + k * HW + 4 * q);
      const ll2 ta = *reinterpret_cast<const ll2*>(tn + 4 * q), tb = *reinterpret_cast<const ll2*>(tn + 4 * q + 2);
#pragma unroll
      for (int k = 0; k < K; ++k) xv[k] = v[k].x;
      mc_bwd_px<K>(xv, ta.x, ignore, ca, cb, g, o);
#pragma unroll
      for (int k = 0; k < K; ++k) {
        r[k].x = o[k];
        xv[k] = v[k].y;
      }
      mc_bwd_px<K>(xv, ta.y, ignore, ca, cb, g, o);
#pragma unroll
      for (int k = 0; k < K; ++k) {
        r[k].y = o[k];
        xv[k] = v[k].z;
      }
      mc_bwd_px<K>(xv, tb.x, ignore, ca, cb, g, o);
#pragma unroll
      for (int k = 0; k < K; ++k) {
        r[k].z = o[k];
        xv[k] = v[k].w;
      }
      mc_bwd_px<K>(xv, tb.y, ignore, ca, cb, g, o);
#pragma unroll
      for (int k = 0; k < K; ++k) {
        r[k].w = o[k];
        *reinterpret_cast<float4*>(dn + k * HW + 4 * q) = r[k];
      }
    }
  } else {
    for (long long p = t0; p < HW; p += step) {
#pragma unroll
      for (int k = 0; k < K; ++k) xv[k] = xn[k * HW + p];
      mc_bwd_px<K>(xv, tn[p], ignore, ca, cb, g, o);
#pragma unroll
      for (int k = 0; k < K; ++k) dn[k * HW + p] = o[k];
    }
  }
}

// dx = g c (act 0) or g c p (1 - p) (act 1), c = b - a t
__device__ __forceinline__ float bin_bwd_px(float xv, float tv, int act, float a, float b, float g) {
  const float c = g * fmaf(-a, tv, b);
  if (!act) return c;
  const float p = bin_prob(xv, 1);
  return c * p * (1.f - p);
}

__global__ __launch_bounds__(DT) void softdice_bwd_bin_kernel(const float* __restrict__ x, const float* __restrict__ t,
                                                              long long HW, int act, int per_image,
                                                              const float* __restrict__ coef, const float* __restrict__ gout,
                                                              int vec, float* __restrict__ dx) {
  const int n = blockIdx.y;
  const float* xn = x + (long long)n * HW;
  const float* tn = t + (long long)n * HW;
  float* dn = dx + (long long)n * HW;
  const float* cf = coef + (per_image ? (long long)n * 2 : 0);
  const float a = cf[0], b = cf[1], g = gout[0];
  const long long t0 = (long long)blockIdx.x * DT + threadIdx.x, step = (long long)gridDim.x * DT;
  if (vec) {
    const long long Q = HW >> 2;
    for (long long q = t0; q < Q; q += step) {
      const float4 xv = pmu_ld4(xn + 4 * q), tv = pmu_ld4(tn + 4 * q);
      float4 r;
      r.x = bin_bwd_px(xv.x, tv.x, act, a, b, g);
      r.y = bin_bwd_px(xv.y, tv.y, act, a, b, g);
      r.z = bin_bwd_px(xv.z, tv.z, act, a, b, g);
      r.w = bin_bwd_px(xv.w, tv.w, act, a, b, g);
      *reinterpret_cast<float4*>(dn + 4 * q) = r;
    }
  } else {
    for (long long p = t0; p < HW; p += step) dn[p] = bin_bwd_px(xn[p], tn[p], act, a, b, g);
  }
}

bool aligned16(const void* p) { return ((uintptr_t)p & 15) == 0; }

bool dice_shape_ok(int N, int K, long long HW) {
  // N is a grid dimension; a thread's pixel count is kept in 32 bits
  return N > 0 && N <= 65535 && K >= 1 && K <= DMAXK && HW > 0 && HW < (1LL << 40);
}

}  // namespace

#define DICE_FOR_K(K, CALL) \
  switch (K) {              \
    case 2: CALL(2); break; \
    case 3: CALL(3); break; \
    case 4: CALL(4); break; \
    case 5: CALL(5); break; \
    case 6: CALL(6); break; \
    case 7: CALL(7); break; \
    default: CALL(8); break; \
  }

extern "C" size_t pmu_softdice_ws(int N, int K, long long HW) {
  if (!dice_shape_ok(N, K, HW)) return 0;
  return dice_ws(nullptr, N, K, HW).bytes;
}

extern "C" int pmu_softdice_fwd(const float* x, const void* tgt, int N, int K, long long HW, int act, int per_image,
                                int first_class, long long ignore_index, float* loss, void* ws, void* stream) {
  PMU_REQUIRE(x && tgt && loss && ws && dice_shape_ok(N, K, HW));
  PMU_REQUIRE((act == 0 || act == 1) && (per_image == 0 || per_image == 1) && (first_class == 0 || first_class == 1));
  PMU_REQUIRE(((uintptr_t)ws & 7) == 0);
  const DiceWs w = dice_ws(ws, N, K, HW);
  const int G = grid_x(N, HW, DFWD_PX, DFWD_BLOCKS);
  const int vec = HW % 4 == 0 && aligned16(x) && aligned16(tgt);
  hipStream_t st = (hipStream_t)stream;
  if (K == 1) {
    hipLaunchKernelGGL(softdice_fwd_bin_kernel, dim3(G, N), dim3(DT), 0, st, x, (const float*)tgt, HW, act, vec, w.part);
  } else {
#define DICE_FWD(KK)                                                                                                \
  hipLaunchKernelGGL(softdice_fwd_kernel<KK>, dim3(G, N), dim3(DT), 0, st, x, (const long long*)tgt, HW, ignore_index, \
                     vec, w.part)
    DICE_FOR_K(K, DICE_FWD)
#undef DICE_FWD
  }
  PMU_CHECK_LAUNCH();
  const int R = per_image ? N : 1, cnt = per_image ? G : N * G, items = R * (3 * K + 1);
  int L = 1;   // lanes per sum: the block's 1024 threads over the sums, at most a wave or the rows each
  while (L < 64 && (long long)items * L * 2 <= DFT && L < cnt) L *= 2;
  hipLaunchKernelGGL(softdice_final_kernel, dim3(1), dim3(DFT), 0, st, (const double*)w.part, R, cnt, K,
                     K == 1 ? 0 : first_class, L, w.sums, w.coef, loss);
  PMU_CHECK_LAUNCH();
  return PMU_OK;
}

extern "C" int pmu_softdice_bwd(const float* x, const void* tgt, int N, int K, long long HW, int act, int per_image,
                                long long ignore_index, const float* coef, const float* gout, float* dx, void* stream) {
  PMU_REQUIRE(x && tgt && coef && gout && dx && dice_shape_ok(N, K, HW));
  PMU_REQUIRE((act == 0 || act == 1) && (per_image == 0 || per_image == 1));
  const int G = grid_x(N, HW, DBWD_PX, DBWD_BLOCKS);
  const int vec = HW % 4 == 0 && aligned16(x) && aligned16(tgt) && aligned16(dx);
  hipStream_t st = (hipStream_t)stream;
  if (K == 1) {
    hipLaunchKernelGGL(softdice_bwd_bin_kernel, dim3(G, N), dim3(DT), 0, st, x, (const float*)tgt, HW, act, per_image,
                       coef, gout, vec, dx);
  } else {
#define DICE_BWD(KK)                                                                                                \
  hipLaunchKernelGGL(softdice_bwd_kernel<KK>, dim3(G, N), dim3(DT), 0, st, x, (const long long*)tgt, HW, ignore_index, \
                     per_image, coef, gout, vec, dx)
    DICE_FOR_K(K, DICE_BWD)
#undef DICE_BWD
  }
  PMU_CHECK_LAUNCH();
  return PMU_OK;
}
