// BatchNorm2d batch statistics / running stats / backward coefficients
//     (nn.BatchNorm2d in train and eval mode, PMU/model/unet/unet_parts.py:16,19,
//      PMU/model/probabilistic_unet/probabilistic_unet.py:39,44)
// and the BatchNorm+ReLU backward partial sums, alone or formed in the pass that completes the layer's
// gradient (AvgPool2d(2, ceil_mode=True) backward and the spatial mean's, probabilistic_unet.py:36,39).
// All reductions write per-block partial slabs that are summed in a fixed order (fp64).
#include "pmu_common.h"

// ---------------- column sums: part[R][Wd] (f32) -> out[G][Wd] (f64) ----------------
namespace {
__global__ __launch_bounds__(256) void colsum_f64_kernel(const float* __restrict__ part, int R, int Wd,
                                                         double* __restrict__ out, int G) {
  __shared__ double red[4][64];
  const int col = blockIdx.x * 64 + (threadIdx.x & 63);
  const int rl = threadIdx.x >> 6;
  const int g = blockIdx.y;
  const int r0 = (int)(((long long)R * g) / G), r1 = (int)(((long long)R * (g + 1)) / G);
  double s = 0.0;
  if (col < Wd)
    for (int r = r0 + rl; r < r1; r += 4) s += (double)part[(long long)r * Wd + col];
  red[rl][threadIdx.x & 63] = s;
  __syncthreads();
  if (rl == 0 && col < Wd)
    out[(long long)g * Wd + col] = red[0][threadIdx.x] + red[1][threadIdx.x] + red[2][threadIdx.x] + red[3][threadIdx.x];
}
}  // namespace

extern "C" int pmu_colsum_groups(int R) {
  int g = R / 64;
  if (g < 1) g = 1;
  if (g > 128) g = 128;
  return g;
}

extern "C" int pmu_colsum_f64(const float* part, int R, int Wd, double* out, int G, void* stream) {
  PMU_REQUIRE(part && out && R > 0 && Wd > 0 && G > 0 && G <= R);
  hipLaunchKernelGGL(colsum_f64_kernel, dim3((unsigned)pmu_cdiv(Wd, 64), (unsigned)G), dim3(256), 0,
                     (hipStream_t)stream, part, R, Wd, out, G);
  PMU_CHECK_LAUNCH();
  return PMU_OK;
}

// ---------------- forward: batch statistics -> coefficients ----------------
namespace {
// sums of acc[g][0..1][c] over the G groups: 4 threads per channel each take every 4th group
// (their loads in flight together instead of one dependent walk of G), combined in fixed order.
// Block = 256 threads = 4 x 64 channels; returns the sums in the q == 0 threads.
__device__ __forceinline__ bool group_sums(const double* __restrict__ acc, int G, int C, double& s1, double& s2) {
  __shared__ double red[2][4][64];
  const int q = threadIdx.x >> 6, cl = threadIdx.x & 63;
  const int c = blockIdx.x * 64 + cl;
  s1 = 0.0;
  s2 = 0.0;
  if (c < C)
    for (int g = q; g < G; g += 4) {
      s1 += acc[((long long)g * 2 + 0) * C + c];
      s2 += acc[((long long)g * 2 + 1) * C + c];
    }
  red[0][q][cl] = s1;
  red[1][q][cl] = s2;
  __syncthreads();
  if (q != 0 || c >= C) return false;
  s1 = ((red[0][0][cl] + red[0][1][cl]) + red[0][2][cl]) + red[0][3][cl];
  s2 = ((red[1][0][cl] + red[1][1][cl]) + red[1][2][cl]) + red[1][3][cl];
  return true;
}

__global__ __launch_bounds__(256) void bn_fwd_finalize_kernel(const double* __restrict__ acc, int G, int C,
                                                              double count, const float* __restrict__ gamma,
                                                              const float* __restrict__ beta, float eps,
                                                              float momentum, float* running_mean,
                                                              float* running_var, long long* nbt, float* mean_out,
                                                              float* invstd_out, float* coef) {
  if (nbt && blockIdx.x == 0 && threadIdx.x == 0) nbt[0] = nbt[0] + 1;  // (one lane, a vector store)
  double s1, s2;
  if (!group_sums(acc, G, C, s1, s2)) return;
  const int c = blockIdx.x * 64 + (threadIdx.x & 63);
  const double mean = s1 / count;
  double var = s2 / count - mean * mean;
  if (var < 0.0) var = 0.0;
  const double invstd = 1.0 / sqrt(var + (double)eps);
  const double gm = gamma ? (double)gamma[c] : 1.0;
  const double bt = beta ? (double)beta[c] : 0.0;
  const float scale = (float)(gm * invstd);
  coef[c] = scale;
  coef[C + c] = (float)(bt - mean * gm * invstd);
  mean_out[c] = (float)mean;
  invstd_out[c] = (float)invstd;
  if (running_mean) {
    const double unb = count > 1.0 ? var * count / (count - 1.0) : var;
    running_mean[c] = (float)((1.0 - momentum) * (double)running_mean[c] + momentum * mean);
    running_var[c] = (float)((1.0 - momentum) * (double)running_var[c] + momentum * unb);
  }
}
}  // namespace

extern "C" int pmu_bn_fwd_finalize(const double* acc, int G, int C, double count, const float* gamma,
                                   const float* beta, float eps, float momentum, float* running_mean,
                                   float* running_var, long long* num_batches_tracked, float* mean,
                                   float* invstd, float* coef, void* stream) {
  PMU_REQUIRE(acc && G > 0 && C > 0 && count > 0 && mean && invstd && coef);
  PMU_REQUIRE((running_mean == nullptr) == (running_var == nullptr));
  hipLaunchKernelGGL(bn_fwd_finalize_kernel, dim3((unsigned)pmu_cdiv(C, 64)), dim3(256), 0, (hipStream_t)stream,
                     acc, G, C, count, gamma, beta, eps, momentum, running_mean, running_var,
                     num_batches_tracked, mean, invstd, coef);
  PMU_CHECK_LAUNCH();
  return PMU_OK;
}

namespace {
__global__ void bn_eval_coef_kernel(const float* rm, const float* rv, const float* gamma, const float* beta,
                                    float eps, int C, float* coef) {
  const int c = blockIdx.x * blockDim.x + threadIdx.x;
  if (c >= C) return;
  const float inv = 1.f / sqrtf(rv[c] + eps);
  const float g = gamma ? gamma[c] : 1.f;
  const float b = beta ? beta[c] : 0.f;
  coef[c] = g * inv;
  coef[C + c] = b - rm[c] * g * inv;
}
}  // namespace

extern "C" int pmu_bn_eval_coef(const float* running_mean, const float* running_var, const float* gamma,
                                const float* beta, float eps, int C, float* coef, void* stream) {
  PMU_REQUIRE(running_mean && running_var && C > 0 && coef);
  hipLaunchKernelGGL(bn_eval_coef_kernel, dim3((unsigned)pmu_cdiv(C, 256)), dim3(256), 0, (hipStream_t)stream,
                     running_mean, running_var, gamma, beta, eps, C, coef);
  PMU_CHECK_LAUNCH();
  return PMU_OK;
}

#ifdef PMU_EXPERIMENTS
// bf16-stored z (experiments build only: it breaks the c5 Dice contract)
// Centring of a bf16-stored z (pmu_conv3x3_fwd_dma_zb stores z - off): the coefficients every
// consumer applies to the stored value — scale, shift + off*scale (BN+ReLU: (zs + off)*scale + shift),
// mean - off (xhat = (zs + off - mean)*invstd).  In place allowed.  (The kernel has external linkage, as
// it always had: the experiments library's symbols stay as they are.)
__global__ __launch_bounds__(256) void bn_center_kernel(const float* __restrict__ coef, const float* mean,
                                                        const float* __restrict__ off, int C, float* coef_out,
                                                        float* mean_out) {
  const int c = blockIdx.x * blockDim.x + threadIdx.x;
  if (c >= C) return;
  const float sc = coef[c], sh = coef[C + c], o = off[c];
  coef_out[c] = sc;
  coef_out[C + c] = fmaf(o, sc, sh);
  if (mean && mean_out) mean_out[c] = mean[c] - o;
}

extern "C" int pmu_bn_center(const float* coef, const float* mean, const float* off, int C, float* coef_out,
                             float* mean_out, void* stream) {
  PMU_REQUIRE(coef && off && coef_out && C > 0 && (!mean || mean_out));
  hipLaunchKernelGGL(bn_center_kernel, dim3((unsigned)pmu_cdiv(C, 256)), dim3(256), 0, (hipStream_t)stream, coef, mean,
                     off, C, coef_out, mean_out);
  PMU_CHECK_LAUNCH();
  return PMU_OK;
}
#endif  // PMU_EXPERIMENTS

// ---------------- BN + ReLU backward reduction ----------------
// part[tile][2][C] = (sum g, sum g*xhat), g = da * (z*scale+shift > 0), xhat = (z-mean)*invstd
namespace {
constexpr int BNR_BYTES = 65536;  // bytes of one tensor per block
template <class ZT, class DT = float>  // z / da stored as float or bf16 (unsigned short)
__global__ __launch_bounds__(256) void bn_bwd_reduce_kernel(const DT* __restrict__ da, const ZT* __restrict__ z,
                                                            const float* __restrict__ coef, const float* __restrict__ mean,
                                                            const float* __restrict__ invstd, long long P, int C,
                                                            int ppb, float* __restrict__ part) {
  __shared__ float red[256 * 8];
  const int tid = threadIdx.x;
  const int CQ = C >> 2;
  const int npg = CQ >= 256 ? 1 : 256 / CQ;
  const int qstride = CQ >= 256 ? 256 : CQ;
  const int pg = tid / qstride;
  const int q0 = tid % qstride;
  const long long p0 = (long long)blockIdx.x * ppb;
  // each thread owns channel quads q0, q0+qstride, ... (only >1 when CQ > 256); every thread runs the
  // same number of rounds (the barriers below are block-wide), a quad past C only joins the barriers
  for (int qb = 0; qb < CQ; qb += qstride) {
    const int q = qb + q0;
    const int c = 4 * (q < CQ ? q : 0);
    const float4 sc = *reinterpret_cast<const float4*>(coef + c);
    const float4 sh = *reinterpret_cast<const float4*>(coef + C + c);
    const float4 mu = *reinterpret_cast<const float4*>(mean + c);
    const float4 is = *reinterpret_cast<const float4*>(invstd + c);
    float sg[4] = {0, 0, 0, 0}, sgx[4] = {0, 0, 0, 0};
    if (pg < npg && q < CQ) {
      // the block's pixels of this thread, in order; unrolled so 8 loads are in flight per thread
      const long long pend = min(P, p0 + ppb);
      const int nit = pend > p0 + pg ? (int)((pend - p0 - pg + npg - 1) / npg) : 0;
      const DT* dp = da + (p0 + pg) * C + c;
      const ZT* zp = z + (p0 + pg) * C + c;
      const long long step = (long long)npg * C;
#pragma unroll 4
      for (int it = 0; it < nit; ++it) {
        const float4 d = pmu_ld4(dp + it * step);
        const float4 zz = pmu_ld4(zp + it * step);
        const float dv[4] = {d.x, d.y, d.z, d.w}, zv[4] = {zz.x, zz.y, zz.z, zz.w};
        const float scv[4] = {sc.x, sc.y, sc.z, sc.w}, shv[4] = {sh.x, sh.y, sh.z, sh.w};
        const float muv[4] = {mu.x, mu.y, mu.z, mu.w}, isv[4] = {is.x, is.y, is.z, is.w};
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          const float g = fmaf(zv[e], scv[e], shv[e]) > 0.f ? dv[e] : 0.f;
          sg[e] += g;
          sgx[e] = fmaf(g, (zv[e] - muv[e]) * isv[e], sgx[e]);
        }
      }
    }
#pragma unroll
    for (int e = 0; e < 4; ++e) { red[tid * 8 + e] = sg[e]; red[tid * 8 + 4 + e] = sgx[e]; }
    __syncthreads();
    if (pg == 0 && q < CQ) {
      float t1[4] = {0, 0, 0, 0}, t2[4] = {0, 0, 0, 0};
      for (int l = 0; l < npg; ++l) {
        const int src = l * qstride + q0;
#pragma unroll
        for (int e = 0; e < 4; ++e) { t1[e] += red[src * 8 + e]; t2[e] += red[src * 8 + 4 + e]; }
      }
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        part[((long long)blockIdx.x * 2 + 0) * C + c + e] = t1[e];
        part[((long long)blockIdx.x * 2 + 1) * C + c + e] = t2[e];
      }
    }
    __syncthreads();
  }
}

// Scalar variant for channel counts that are not a multiple of 4 (any num_filters is legal in the
// reference): thread t owns channels t, t+256, ... and walks the block's pixels in order.
__global__ __launch_bounds__(256) void bn_bwd_reduce1_kernel(const float* __restrict__ da, const float* __restrict__ z,
                                                             const float* __restrict__ coef, const float* __restrict__ mean,
                                                             const float* __restrict__ invstd, long long P, int C,
                                                             int ppb, float* __restrict__ part) {
  const long long p0 = (long long)blockIdx.x * ppb;
  const long long p1 = min(P, p0 + ppb);
  for (int c = threadIdx.x; c < C; c += blockDim.x) {
    const float sc = coef[c], sh = coef[C + c], mu = mean[c], is = invstd[c];
    float sg = 0.f, sgx = 0.f;
    for (long long p = p0; p < p1; ++p) {
      const float zz = z[p * C + c];
      const float g = fmaf(zz, sc, sh) > 0.f ? da[p * C + c] : 0.f;
      sg += g;
      sgx = fmaf(g, (zz - mu) * is, sgx);
    }
    part[((long long)blockIdx.x * 2 + 0) * C + c] = sg;
    part[((long long)blockIdx.x * 2 + 1) * C + c] = sgx;
  }
}
}  // namespace

static int bn_bwd_ppb(int C) {
  int ppb = BNR_BYTES / (C * 4);
  return ppb < 1 ? 1 : ppb;
}

extern "C" int pmu_bn_bwd_tiles(int P, int C) { return pmu_cdiv(P, bn_bwd_ppb(C)); }

// the channel-quad kernel on z / da of either storage (C % 4 == 0)
template <class ZT, class DT>
static int bn_bwd_reduce_launch(const DT* da, const ZT* z, const float* coef, const float* mean, const float* invstd,
                                int P, int C, float* part, void* stream) {
  PMU_REQUIRE(da && z && coef && mean && invstd && part && P > 0 && C > 0 && C % 4 == 0);
  const int ppb = bn_bwd_ppb(C);
  hipLaunchKernelGGL((bn_bwd_reduce_kernel<ZT, DT>), dim3((unsigned)pmu_cdiv(P, ppb)), dim3(256), 0,
                     (hipStream_t)stream, da, z, coef, mean, invstd, (long long)P, C, ppb, part);
  PMU_CHECK_LAUNCH();
  return PMU_OK;
}

extern "C" int pmu_bn_bwd_reduce(const float* da, const float* z, const float* coef, const float* mean,
                                 const float* invstd, int P, int C, float* part, void* stream) {
  if (C % 4 == 0) return bn_bwd_reduce_launch<float, float>(da, z, coef, mean, invstd, P, C, part, stream);
  PMU_REQUIRE(da && z && coef && mean && invstd && part && P > 0 && C > 0);
  const int ppb = bn_bwd_ppb(C);
  hipLaunchKernelGGL(bn_bwd_reduce1_kernel, dim3((unsigned)pmu_cdiv(P, ppb)), dim3(256), 0, (hipStream_t)stream, da,
                     z, coef, mean, invstd, (long long)P, C, ppb, part);
  PMU_CHECK_LAUNCH();
  return PMU_OK;
}

// da stored as bf16 (the *_dxb input gradients' dx)
extern "C" int pmu_bn_bwd_reduce_dxb(const unsigned short* da, const float* z, const float* coef, const float* mean,
                                     const float* invstd, int P, int C, float* part, void* stream) {
  return bn_bwd_reduce_launch<float, unsigned short>(da, z, coef, mean, invstd, P, C, part, stream);
}

#ifdef PMU_EXPERIMENTS
// bf16-stored z (experiments build only: it breaks the c5 Dice contract)
extern "C" int pmu_bn_bwd_reduce_zb(const float* da, const unsigned short* z, const float* coef, const float* mean,
                                    const float* invstd, int P, int C, float* part, void* stream) {
  return bn_bwd_reduce_launch<unsigned short, float>(da, z, coef, mean, invstd, P, C, part, stream);
}
#endif  // PMU_EXPERIMENTS

// The two encoder passes that complete a layer's da (probabilistic_unet.py:26-44, the prior /
// posterior nets): AvgPool2d(2, ceil_mode) backward (SRC 1: da[n][h][w] = dpool[n][h/2][w/2] / count of
// the window's valid pixels, avgpool2_bwd's arithmetic) and the spatial mean's backward (SRC 2:
// da[n][p] = dmean[n] / (H*W), :39 torch.mean over dims 2,3), each writing da and forming the layer's
// BatchNorm+ReLU backward partial sums in the same pass — the part[tile][2][C] slab of
// bn_bwd_reduce_kernel (same blocks, same per-thread pixel order), so the layer's bn_backward takes
// them instead of a second pass over da and z.
namespace {
template <int SRC>
__global__ __launch_bounds__(256) void bn_bwd_reduce_src_kernel(const float* __restrict__ g,
                                                                const float* __restrict__ z,
                                                                const float* __restrict__ coef,
                                                                const float* __restrict__ mean,
                                                                const float* __restrict__ invstd, int N, int H, int W,
                                                                int C, int ppb, float* __restrict__ da,
                                                                float* __restrict__ part) {
  __shared__ float red[256 * 8];
  const int tid = threadIdx.x;
  const int CQ = C >> 2;
  const int npg = CQ >= 256 ? 1 : 256 / CQ;
  const int qstride = CQ >= 256 ? 256 : CQ;
  const int pg = tid / qstride;
  const int q0 = tid % qstride;
  const long long P = (long long)N * H * W;
  const long long p0 = (long long)blockIdx.x * ppb;
  const int Hp = (H + 1) / 2, Wp = (W + 1) / 2;
  const float hw = (float)(H * W);
  for (int qb = 0; qb < CQ; qb += qstride) {  // uniform trip count: the barriers below are block-wide
    const int q = qb + q0;
    const int c = 4 * (q < CQ ? q : 0);
    const float4 sc = *reinterpret_cast<const float4*>(coef + c);
    const float4 sh = *reinterpret_cast<const float4*>(coef + C + c);
    const float4 mu = *reinterpret_cast<const float4*>(mean + c);
    const float4 is = *reinterpret_cast<const float4*>(invstd + c);
    const float scv[4] = {sc.x, sc.y, sc.z, sc.w}, shv[4] = {sh.x, sh.y, sh.z, sh.w};
    const float muv[4] = {mu.x, mu.y, mu.z, mu.w}, isv[4] = {is.x, is.y, is.z, is.w};
    float sg[4] = {0, 0, 0, 0}, sgx[4] = {0, 0, 0, 0};
    if (pg < npg && q < CQ) {
      const int pend = (int)min(P, p0 + ppb);   // P < 2^31 (host-checked)
#pragma unroll 4
      for (int p = (int)p0 + pg; p < pend; p += npg) {
        const int w = p % W;
        const int t = p / W;
        const int h = t % H;
        const int n = t / H;
        float4 d;
        if (SRC == 1) {
          const int hp = h >> 1, wp = w >> 1;
          const float cnt = (float)((min(2 * hp + 2, H) - 2 * hp) * (min(2 * wp + 2, W) - 2 * wp));
          const float4 gg = *reinterpret_cast<const float4*>(g + (((long long)n * Hp + hp) * Wp + wp) * C + c);
          d = make_float4(gg.x / cnt, gg.y / cnt, gg.z / cnt, gg.w / cnt);
        } else {
          const float4 gg = *reinterpret_cast<const float4*>(g + (long long)n * C + c);
          d = make_float4(gg.x / hw, gg.y / hw, gg.z / hw, gg.w / hw);
        }
        PMU_DCHECK(p < P, PMU_DBG_OUTPUT);
        const float4 zz = *reinterpret_cast<const float4*>(z + (long long)p * C + c);
        *reinterpret_cast<float4*>(da + (long long)p * C + c) = d;
        const float dv[4] = {d.x, d.y, d.z, d.w}, zv[4] = {zz.x, zz.y, zz.z, zz.w};
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          const float gv = fmaf(zv[e], scv[e], shv[e]) > 0.f ? dv[e] : 0.f;
          sg[e] += gv;
          sgx[e] = fmaf(gv, (zv[e] - muv[e]) * isv[e], sgx[e]);
        }
      }
    }
#pragma unroll
    for (int e = 0; e < 4; ++e) { red[tid * 8 + e] = sg[e]; red[tid * 8 + 4 + e] = sgx[e]; }
    __syncthreads();
    if (pg == 0 && q < CQ) {
      float t1[4] = {0, 0, 0, 0}, t2[4] = {0, 0, 0, 0};
      for (int l = 0; l < npg; ++l) {
        const int src = l * qstride + q0;
#pragma unroll
        for (int e = 0; e < 4; ++e) { t1[e] += red[src * 8 + e]; t2[e] += red[src * 8 + 4 + e]; }
      }
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        part[((long long)blockIdx.x * 2 + 0) * C + c + e] = t1[e];
        part[((long long)blockIdx.x * 2 + 1) * C + c + e] = t2[e];
      }
    }
    __syncthreads();
  }
}
}  // namespace

template <int SRC>
static int bn_bwd_reduce_src_launch(const float* g, const float* z, const float* coef, const float* mean,
                                    const float* invstd, int N, int H, int W, int C, float* da, float* part,
                                    void* stream) {
  PMU_REQUIRE(g && z && coef && mean && invstd && da && part && N > 0 && H > 0 && W > 0 && C > 0 && C % 4 == 0);
  const long long P = (long long)N * H * W;
  PMU_REQUIRE(P < (1LL << 31));
  const int ppb = bn_bwd_ppb(C);
  hipLaunchKernelGGL(bn_bwd_reduce_src_kernel<SRC>, dim3((unsigned)pmu_cdiv(P, ppb)), dim3(256), 0, (hipStream_t)stream,
                     g, z, coef, mean, invstd, N, H, W, C, ppb, da, part);
  PMU_CHECK_LAUNCH();
  return PMU_OK;
}

// AvgPool2d(2, ceil_mode) backward into da (N x H x W x C, the pooled layer's resolution) fused with
// that layer's BN+ReLU backward partial sums (part rows = pmu_bn_bwd_tiles(N*H*W, C)); da bit-equal to
// pmu_avgpool2_bwd, part to pmu_bn_bwd_reduce on it.  C % 4 == 0.
extern "C" int pmu_avgpool2_bwd_bnr(const float* dpool, const float* z, const float* coef, const float* mean,
                                    const float* invstd, int N, int H, int W, int C, float* da, float* part,
                                    void* stream) {
  return bn_bwd_reduce_src_launch<1>(dpool, z, coef, mean, invstd, N, H, W, C, da, part, stream);
}

// The spatial mean's backward (da[n][h][w][c] = dmean[n][c] / (H*W), pmu_spatial_mean_bwd's arithmetic)
// fused with the BN+ReLU backward partial sums of the layer it averaged (part as above).  C % 4 == 0.
extern "C" int pmu_spatial_mean_bwd_bnr(const float* dmean, const float* z, const float* coef, const float* mean,
                                        const float* invstd, int N, int H, int W, int C, float* da, float* part,
                                        void* stream) {
  return bn_bwd_reduce_src_launch<2>(dmean, z, coef, mean, invstd, N, H, W, C, da, part, stream);
}

// ---------------- backward coefficients ----------------
namespace {
__global__ __launch_bounds__(256) void bn_bwd_finalize_kernel(const double* __restrict__ acc, int G, int C,
                                                              double count, const float* __restrict__ gamma,
                                                              const float* __restrict__ coef,
                                                              const float* __restrict__ mean,
                                                              const float* __restrict__ invstd, float* dgamma,
                                                              float* dbeta, float* dbias, float* bcoef) {
  double sg, sgx;
  if (!group_sums(acc, G, C, sg, sgx)) return;
  const int c = blockIdx.x * 64 + (threadIdx.x & 63);
  const double is = invstd[c];
  const double gm = gamma ? (double)gamma[c] : 1.0;
  const double scale = gm * is;
  const double c2 = sg / count, c3 = sgx / count;
  const double kx = -scale * is * c3;
  const double kc = -scale * c2;
  if (dgamma) dgamma[c] = (float)sgx;
  if (dbeta) dbeta[c] = (float)sg;
  // sum_p dz = scale*sum g + kx*(sum z - n*mean) + n*kc ; sum z == n*mean by construction
  if (dbias) dbias[c] = (float)(scale * sg + count * kc);
  bcoef[c] = coef[c];
  bcoef[C + c] = coef[C + c];
  bcoef[2 * C + c] = mean[c];
  bcoef[3 * C + c] = (float)kx;
  bcoef[4 * C + c] = (float)kc;
}
}  // namespace

extern "C" int pmu_bn_bwd_finalize(const double* acc, int G, int C, double count, const float* gamma,
                                   const float* coef, const float* mean, const float* invstd, float* dgamma,
                                   float* dbeta, float* dbias, float* bcoef, void* stream) {
  PMU_REQUIRE(acc && G > 0 && C > 0 && count > 0 && coef && mean && invstd && bcoef);
  hipLaunchKernelGGL(bn_bwd_finalize_kernel, dim3((unsigned)pmu_cdiv(C, 64)), dim3(256), 0, (hipStream_t)stream,
                     acc, G, C, count, gamma, coef, mean, invstd, dgamma, dbeta, dbias, bcoef);
  PMU_CHECK_LAUNCH();
  return PMU_OK;
}

// ---------------- BN + ReLU applied: out = relu(z*scale + shift) ----------------
namespace {
__global__ __launch_bounds__(256) void bnrelu_apply_kernel(const float* __restrict__ z, const float* __restrict__ coef,
                                                           long long total4, int C, float* __restrict__ out) {
  const int CQ = C >> 2;
  for (long long e = (long long)blockIdx.x * blockDim.x + threadIdx.x; e < total4;
       e += (long long)gridDim.x * blockDim.x) {
    const int c = (int)(e % CQ) * 4;
    const float4 v = *reinterpret_cast<const float4*>(z + 4 * e);
    const float4 sc = *reinterpret_cast<const float4*>(coef + c);
    const float4 sh = *reinterpret_cast<const float4*>(coef + C + c);
    *reinterpret_cast<float4*>(out + 4 * e) =
        make_float4(fmaxf(0.f, fmaf(v.x, sc.x, sh.x)), fmaxf(0.f, fmaf(v.y, sc.y, sh.y)),
                    fmaxf(0.f, fmaf(v.z, sc.z, sh.z)), fmaxf(0.f, fmaf(v.w, sc.w, sh.w)));
  }
}

__global__ __launch_bounds__(256) void bnrelu_apply1_kernel(const float* __restrict__ z, const float* __restrict__ coef,
                                                            long long total, int C, float* __restrict__ out) {
  for (long long e = (long long)blockIdx.x * blockDim.x + threadIdx.x; e < total;
       e += (long long)gridDim.x * blockDim.x) {
    const int c = (int)(e % C);
    out[e] = fmaxf(0.f, fmaf(z[e], coef[c], coef[C + c]));
  }
}
}  // namespace

extern "C" int pmu_bnrelu_apply(const float* z, const float* coef, long long P, int C, float* out, void* stream) {
  PMU_REQUIRE(z && coef && out && P > 0 && C > 0);
  if (C % 4 != 0) {  // any channel count (scalar path)
    hipLaunchKernelGGL(bnrelu_apply1_kernel, dim3(grid_for(P * C)), dim3(256), 0, (hipStream_t)stream, z, coef, P * C,
                       C, out);
    PMU_CHECK_LAUNCH();
    return PMU_OK;
  }
  const long long total4 = P * (C / 4);
  hipLaunchKernelGGL(bnrelu_apply_kernel, dim3(grid_for(total4)), dim3(256), 0, (hipStream_t)stream, z, coef, total4,
                     C, out);
  PMU_CHECK_LAUNCH();
  return PMU_OK;
}
