// MaxPool2d(2) and AvgPool2d(2, ceil_mode=True) backward (PMU/model/unet/unet_parts.py:33,
// PMU/model/probabilistic_unet/probabilistic_unet.py:36), the max-pool's also fused with the pooled
// layer's BatchNorm+ReLU backward: its partial sums (part[block][2][C], summed in a fixed order by
// pmu_colsum_f64) and its dz.
#include <algorithm>

#include "pmu_stage.h"

// ---------------- MaxPool2d(2) backward ----------------
namespace {
// RAW: the pooled tensor is z itself (a standalone Down block on an arbitrary input), not relu(z*sc+sh)
template <bool RAW>
__global__ __launch_bounds__(256) void maxpool2_bwd1_kernel(const float* __restrict__ dpool, const float* __restrict__ z,
                                                            const float* __restrict__ coef, int N, int H, int W, int C,
                                                            float* __restrict__ dx, int accumulate) {
  const int Hp = H / 2, Wp = W / 2;
  const long long total = (long long)N * H * W * C;
  for (long long e = (long long)blockIdx.x * blockDim.x + threadIdx.x; e < total;
       e += (long long)gridDim.x * blockDim.x) {
    const int c = (int)(e % C);
    const long long p = e / C;
    const int w = (int)(p % W), h = (int)((p / W) % H);
    const long long n = p / ((long long)W * H);
    float o = accumulate ? dx[e] : 0.f;
    const int hp = h >> 1, wp = w >> 1;
    if (hp < Hp && wp < Wp) {
      const int me = ((h & 1) << 1) | (w & 1);
      const float sc = RAW ? 1.f : coef[c], sh = RAW ? 0.f : coef[C + c];
      const long long b = ((n * H + 2 * hp) * W + 2 * wp) * C + c;
      const long long off[4] = {0, C, (long long)W * C, (long long)W * C + C};
      float best = RAW ? z[b] : fmaxf(0.f, fmaf(z[b], sc, sh));
      int arg = 0;
#pragma unroll
      for (int k = 1; k < 4; ++k) {
        const float v = RAW ? z[b + off[k]] : fmaxf(0.f, fmaf(z[b + off[k]], sc, sh));
        if (v > best) { best = v; arg = k; }
      }
      if (arg == me) o += dpool[((n * Hp + hp) * Wp + wp) * C + c];
    }
    dx[e] = o;
  }
}

// grid-stride over dx elements in channel quads
template <bool RAW, class ZT>  // z stored as float or bf16 (unsigned short)
__global__ __launch_bounds__(256) void maxpool2_bwd_kernel(const float* __restrict__ dpool, const ZT* __restrict__ z,
                                                           const float* __restrict__ coef, int N, int H, int W, int C,
                                                           float* __restrict__ dx, int accumulate) {
  const int CQ = C >> 2;
  const int Hp = H / 2, Wp = W / 2;
  const long long total = (long long)N * H * W * CQ;
  for (long long e = (long long)blockIdx.x * blockDim.x + threadIdx.x; e < total;
       e += (long long)gridDim.x * blockDim.x) {
    const int q = (int)(e % CQ);
    long long p = e / CQ;
    const int w = (int)(p % W);
    const int h = (int)((p / W) % H);
    const int n = (int)(p / ((long long)W * H));
    const int c = 4 * q;
    float4 o = accumulate ? *reinterpret_cast<const float4*>(dx + p * C + c) : make_float4(0.f, 0.f, 0.f, 0.f);
    const int hp = h >> 1, wp = w >> 1;
    if (hp < Hp && wp < Wp) {
      const int me = ((h & 1) << 1) | (w & 1);
      const float4 sc = RAW ? make_float4(1.f, 1.f, 1.f, 1.f) : *reinterpret_cast<const float4*>(coef + c);
      const float4 sh = RAW ? make_float4(0.f, 0.f, 0.f, 0.f) : *reinterpret_cast<const float4*>(coef + C + c);
      const long long b = (((long long)n * H + 2 * hp) * W + 2 * wp) * C + c;
      const long long off[4] = {0, C, (long long)W * C, (long long)W * C + C};
      float best[4];
      int arg[4] = {0, 0, 0, 0};
      {
        const float4 v = pmu_ld4(z + b);
        if (RAW) {
          best[0] = v.x; best[1] = v.y; best[2] = v.z; best[3] = v.w;
        } else {
          best[0] = fmaxf(0.f, fmaf(v.x, sc.x, sh.x)); best[1] = fmaxf(0.f, fmaf(v.y, sc.y, sh.y));
          best[2] = fmaxf(0.f, fmaf(v.z, sc.z, sh.z)); best[3] = fmaxf(0.f, fmaf(v.w, sc.w, sh.w));
        }
      }
#pragma unroll
      for (int k = 1; k < 4; ++k) {
        const float4 v = pmu_ld4(z + b + off[k]);
        const float a0 = RAW ? v.x : fmaxf(0.f, fmaf(v.x, sc.x, sh.x)), a1 = RAW ? v.y : fmaxf(0.f, fmaf(v.y, sc.y, sh.y));
        const float a2 = RAW ? v.z : fmaxf(0.f, fmaf(v.z, sc.z, sh.z)), a3 = RAW ? v.w : fmaxf(0.f, fmaf(v.w, sc.w, sh.w));
        if (a0 > best[0]) { best[0] = a0; arg[0] = k; }
        if (a1 > best[1]) { best[1] = a1; arg[1] = k; }
        if (a2 > best[2]) { best[2] = a2; arg[2] = k; }
        if (a3 > best[3]) { best[3] = a3; arg[3] = k; }
      }
      const float4 g = *reinterpret_cast<const float4*>(dpool + (((long long)n * Hp + hp) * Wp + wp) * C + c);
      if (arg[0] == me) o.x += g.x;
      if (arg[1] == me) o.y += g.y;
      if (arg[2] == me) o.z += g.z;
      if (arg[3] == me) o.w += g.w;
    }
    *reinterpret_cast<float4*>(dx + p * C + c) = o;
  }
}
}  // namespace

extern "C" int pmu_maxpool2_bwd(const float* dpool, const float* z, const float* coef, int N, int H, int W,
                                int C, float* dx, int accumulate, void* stream) {
  PMU_REQUIRE(dpool && z && dx && N > 0 && H > 1 && W > 1 && C > 0);
  const bool vec = C % 4 == 0;  // channel quads; else the scalar kernel.  coef null: RAW
  const auto kernel = vec ? (coef ? maxpool2_bwd_kernel<false, float> : maxpool2_bwd_kernel<true, float>)
                          : (coef ? maxpool2_bwd1_kernel<false> : maxpool2_bwd1_kernel<true>);
  hipLaunchKernelGGL(kernel, dim3(grid_for((long long)N * H * W * (vec ? C / 4 : C))), dim3(256), 0,
                     (hipStream_t)stream, dpool, z, coef, N, H, W, C, dx, accumulate);
  PMU_CHECK_LAUNCH();
  return PMU_OK;
}

#ifdef PMU_EXPERIMENTS
// bf16-stored z (experiments build only: it breaks the c5 Dice contract)
extern "C" int pmu_maxpool2_bwd_zb(const float* dpool, const unsigned short* z, const float* coef, int N, int H, int W,
                                   int C, float* dx, int accumulate, void* stream) {
  PMU_REQUIRE(dpool && z && coef && dx && N > 0 && H > 1 && W > 1 && C > 0 && C % 4 == 0);
  hipLaunchKernelGGL((maxpool2_bwd_kernel<false, unsigned short>), dim3(grid_for((long long)N * H * W * (C / 4))),
                     dim3(256), 0, (hipStream_t)stream, dpool, z, coef, N, H, W, C, dx, accumulate);
  PMU_CHECK_LAUNCH();
  return PMU_OK;
}
#endif  // PMU_EXPERIMENTS

// ---------------- MaxPool2d(2) backward + BN+ReLU backward partial sums ----------------
// MaxPool2d(2) backward into the skip gradient fused with the BatchNorm+ReLU backward partial sums
// of the pooled layer (its da is complete once the pooled gradient has been routed): a thread owns one
// channel quad of one 2x2 window (ceil-sized, so the odd last row / column of an odd map is covered
// for the sums), reads its four z quads once (maxpool2_bwd_kernel re-reads the window per output
// element), adds dpool to the first max, writes da and accumulates (sum g, sum g*xhat),
// g = da * (z*scale+shift > 0), xhat = (z-mean)*invstd — the part[block][2][C] slab bn_bwd_reduce
// would compute from a second pass over da and z.  Block = 256 threads over wpb windows.
// Streaming form (as frame_stream_kernel): a thread's windows run in ping-pong pairs, the next
// window's nine float4 loads in flight while this one is routed and stored; every load is
// unconditional (addresses clamped into the map, the values of outside pixels / partial windows
// masked afterwards) and only the stores are predicated — loads under per-window branches, consumed
// right after, left one global round trip exposed per window (4.9 TB/s at c5's 512^2 level).
namespace {
struct MpWin {
  float4 z[4], d[4], g;
};

// DT: storage of dpool and of the accumulated skip gradient (float, or bf16 as unsigned short: the
// *_dxb input gradients' dx; the sum is formed and written in fp32, torch.autocast's gradient
// accumulation of the skip activation)
template <bool ACC, class DT = float>
__device__ __forceinline__ void mp_load(const DT* __restrict__ dpool, const float* __restrict__ z,
                                        const DT* __restrict__ dx, long long wi, int H, int W, int C, int c,
                                        MpWin& m) {
  const int Hp = H / 2, Wp = W / 2, Hc = (H + 1) / 2, Wc = (W + 1) / 2;
  const int wc = (int)(wi % Wc);
  const long long r = wi / Wc;
  const int hc = (int)(r % Hc);
  const int n = (int)(r / Hc);
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    const int h = min(2 * hc + (k >> 1), H - 1), w = min(2 * wc + (k & 1), W - 1);
    const long long off = (((long long)n * H + h) * W + w) * C + c;
    m.z[k] = *reinterpret_cast<const float4*>(z + off);
    if (ACC) m.d[k] = pmu_ld4(dx + off);
  }
  const long long po = (((long long)n * Hp + min(hc, Hp - 1)) * Wp + min(wc, Wp - 1)) * C + c;
  m.g = pmu_ld4(dpool + po);
}

template <bool ACC, bool ST = true>
__device__ __forceinline__ void mp_route(const MpWin& m, long long wi, bool valid, int H, int W, int C, int c,
                                         const float (&scv)[4], const float (&shv)[4], const float (&muv)[4],
                                         const float (&isv)[4], float* __restrict__ dx, float (&sg)[4], float (&sgx)[4]) {
  const int Hp = H / 2, Wp = W / 2, Hc = (H + 1) / 2, Wc = (W + 1) / 2;
  const int wc = (int)(wi % Wc);
  const long long r = wi / Wc;
  const int hc = (int)(r % Hc);
  const int n = (int)(r / Hc);
  const bool full = hc < Hp && wc < Wp;
  float zv[4][4], dv[4][4];
  bool ok[4];
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    ok[k] = valid && 2 * hc + (k >> 1) < H && 2 * wc + (k & 1) < W;
    zv[k][0] = m.z[k].x; zv[k][1] = m.z[k].y; zv[k][2] = m.z[k].z; zv[k][3] = m.z[k].w;
    if (ACC) { dv[k][0] = m.d[k].x; dv[k][1] = m.d[k].y; dv[k][2] = m.d[k].z; dv[k][3] = m.d[k].w; }
    else { dv[k][0] = 0.f; dv[k][1] = 0.f; dv[k][2] = 0.f; dv[k][3] = 0.f; }
  }
  const float gv[4] = {full ? m.g.x : 0.f, full ? m.g.y : 0.f, full ? m.g.z : 0.f, full ? m.g.w : 0.f};
#pragma unroll
  for (int e = 0; e < 4; ++e) {  // route dpool to the first max of relu(z*sc+sh) (a full window only: gv = 0 else)
    float best = fmaxf(0.f, fmaf(zv[0][e], scv[e], shv[e]));
    int arg = 0;
#pragma unroll
    for (int k = 1; k < 4; ++k) {
      const float a = fmaxf(0.f, fmaf(zv[k][e], scv[e], shv[e]));
      if (a > best) { best = a; arg = k; }
    }
#pragma unroll
    for (int k = 0; k < 4; ++k) dv[k][e] += arg == k ? gv[e] : 0.f;
  }
#pragma unroll
  for (int k = 0; k < 4; ++k) {
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      const float gg = (ok[k] && fmaf(zv[k][e], scv[e], shv[e]) > 0.f) ? dv[k][e] : 0.f;
      sg[e] += gg;
      sgx[e] = fmaf(gg, (zv[k][e] - muv[e]) * isv[e], sgx[e]);
    }
  }
  if constexpr (!ST) return;
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    if (!ok[k]) continue;
    const int h = 2 * hc + (k >> 1), w = 2 * wc + (k & 1);
    const long long off = (((long long)n * H + h) * W + w) * C + c;
    PMU_DCHECK(off + 4 <= (long long)n * H * W * C + (long long)H * W * C, PMU_DBG_OUTPUT);
    *reinterpret_cast<float4*>(dx + off) = make_float4(dv[k][0], dv[k][1], dv[k][2], dv[k][3]);
  }
}

// base: the skip gradient accumulated into (ACC; dx itself for fp32, a bf16 tensor for DT = bf16).
// dx and base may alias (pmu_maxpool2_bwd_bnr accumulates in place), so neither is __restrict__: each
// element's store follows its own load in the same thread, and no other thread touches that element.
// ST = false: the partial sums only (da not stored: maxpool2_bwd_bnbwd_kernel re-forms it)
template <bool ACC, class DT = float, bool ST = true>
__global__ __launch_bounds__(256) void maxpool2_bwd_bnr_kernel(const DT* __restrict__ dpool,
                                                               const float* __restrict__ z,
                                                               const float* __restrict__ coef,
                                                               const float* __restrict__ mean,
                                                               const float* __restrict__ invstd, int N, int H, int W,
                                                               int C, int wpb, float* dx,
                                                               float* __restrict__ part, const DT* base) {
  __shared__ float red[256 * 8];
  const int tid = threadIdx.x;
  const int CQ = C >> 2;
  const int npg = CQ >= 256 ? 1 : 256 / CQ;
  const int qstride = CQ >= 256 ? 256 : CQ;
  const int pg = tid / qstride, q0 = tid % qstride;
  const int Hc = (H + 1) / 2, Wc = (W + 1) / 2;
  const long long nwin = (long long)N * Hc * Wc;
  const long long w0 = (long long)blockIdx.x * wpb;
  const long long wend = min(nwin, w0 + wpb);
  // every thread runs the same number of channel-quad rounds (the barriers below are block-wide);
  // a thread whose quad lies past C in the last round only joins the barriers
  for (int qb = 0; qb < CQ; qb += qstride) {
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
      const long long last = wend - 1;
      MpWin A, B;
      long long wi = w0 + pg;
      mp_load<ACC>(dpool, z, base, min(wi, last), H, W, C, c, A);
      for (; wi < wend; wi += 2 * npg) {
        const long long wb = wi + npg, wa = wi + 2 * npg;
        mp_load<ACC>(dpool, z, base, min(wb, last), H, W, C, c, B);
        __builtin_amdgcn_sched_barrier(0);
        mp_route<ACC, ST>(A, wi, true, H, W, C, c, scv, shv, muv, isv, dx, sg, sgx);
        __builtin_amdgcn_sched_barrier(0);
        mp_load<ACC>(dpool, z, base, min(wa, last), H, W, C, c, A);
        __builtin_amdgcn_sched_barrier(0);
        mp_route<ACC, ST>(B, min(wb, last), wb < wend, H, W, C, c, scv, shv, muv, isv, dx, sg, sgx);
        __builtin_amdgcn_sched_barrier(0);
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

// windows per block of the fused max-pool backward: about 128 KB of z per block
static int mpb_wpb(int C) {
  const int w = 8192 / C;
  return w < 1 ? 1 : w;
}

extern "C" int pmu_maxpool2_bwd_bnr_tiles(int N, int H, int W, int C) {
  return (int)pmu_cdiv((long long)N * ((H + 1) / 2) * ((W + 1) / 2), mpb_wpb(C));
}

// dx: where da is stored (ST; null for the stats-only forms); base: the skip gradient added (ACC; else null)
template <bool ACC, class DT, bool ST>
static int maxpool2_bwd_bnr_launch(const DT* dpool, const DT* base, const float* z, const float* coef,
                                   const float* mean, const float* invstd, int N, int H, int W, int C, float* dx,
                                   float* part, void* stream) {
  PMU_REQUIRE(dpool && z && coef && mean && invstd && part && N > 0 && H > 1 && W > 1 && C > 0 && C % 4 == 0);
  const int R = pmu_maxpool2_bwd_bnr_tiles(N, H, W, C);
  hipLaunchKernelGGL((maxpool2_bwd_bnr_kernel<ACC, DT, ST>), dim3((unsigned)R), dim3(256), 0, (hipStream_t)stream,
                     dpool, z, coef, mean, invstd, N, H, W, C, mpb_wpb(C), dx, part, base);
  PMU_CHECK_LAUNCH();
  return PMU_OK;
}

extern "C" int pmu_maxpool2_bwd_bnr(const float* dpool, const float* z, const float* coef, const float* mean,
                                    const float* invstd, int N, int H, int W, int C, float* dx, int accumulate,
                                    float* part, void* stream) {
  PMU_REQUIRE(dx);
  if (accumulate)
    return maxpool2_bwd_bnr_launch<true, float, true>(dpool, dx, z, coef, mean, invstd, N, H, W, C, dx, part, stream);
  return maxpool2_bwd_bnr_launch<false, float, true>(dpool, nullptr, z, coef, mean, invstd, N, H, W, C, dx, part,
                                                     stream);
}

// As pmu_maxpool2_bwd_bnr with the pooled gradient and the skip gradient stored as bf16 (the *_dxb
// input gradients' dx): da = skip + routed dpool formed in fp32 and written to dx (a separate fp32
// tensor); skip null: da = the routed dpool alone.
extern "C" int pmu_maxpool2_bwd_bnr_dxb(const unsigned short* dpool, const unsigned short* skip, const float* z,
                                        const float* coef, const float* mean, const float* invstd, int N, int H,
                                        int W, int C, float* dx, float* part, void* stream) {
  PMU_REQUIRE(dx);
  if (skip)
    return maxpool2_bwd_bnr_launch<true, unsigned short, true>(dpool, skip, z, coef, mean, invstd, N, H, W, C, dx,
                                                               part, stream);
  return maxpool2_bwd_bnr_launch<false, unsigned short, true>(dpool, nullptr, z, coef, mean, invstd, N, H, W, C, dx,
                                                              part, stream);
}

// The stats-only forms (da not stored; maxpool2_bwd_bnbwd_kernel below turns the same da into the pooled
// layer's dz): bf16 dpool and skip, and fp32 (config c2's skip levels; part bit-equal to
// pmu_maxpool2_bwd_bnr accumulating into skip).
extern "C" int pmu_maxpool2_bwd_bnr_stats_dxb(const unsigned short* dpool, const unsigned short* skip, const float* z,
                                              const float* coef, const float* mean, const float* invstd, int N,
                                              int H, int W, int C, float* part, void* stream) {
  PMU_REQUIRE(skip);
  return maxpool2_bwd_bnr_launch<true, unsigned short, false>(dpool, skip, z, coef, mean, invstd, N, H, W, C, nullptr,
                                                              part, stream);
}

extern "C" int pmu_maxpool2_bwd_bnr_stats(const float* dpool, const float* skip, const float* z, const float* coef,
                                          const float* mean, const float* invstd, int N, int H, int W, int C,
                                          float* part, void* stream) {
  PMU_REQUIRE(skip);
  return maxpool2_bwd_bnr_launch<true, float, false>(dpool, skip, z, coef, mean, invstd, N, H, W, C, nullptr, part,
                                                     stream);
}

// ---------------- MaxPool2d(2) backward + BN+ReLU backward applied ----------------
// The pooled layer's BN+ReLU backward applied to da = skip + routed dpool, written as the operand dz of
// its input / weight gradients: the fp32 da maxpool2_bwd_bnr_kernel<.., ST> would store, and
// pmu_frame_to_bf16 / pmu_frame_to_f32 of Src(da, BNBWD) re-read, is formed in registers instead (same
// values: the routing of mp_route, the formula of the frame streams, RNE), after the stats-only pass made
// the coefficients.  A thread owns one channel quad of 2x2 windows, two windows in flight per step.
namespace {
__device__ __forceinline__ float mp_bnbwd1(float x, float z, float sc, float sh, float mu, float kx, float kc) {
  return fmaf(sc, fmaf(z, sc, sh) > 0.f ? x : 0.f, fmaf(kx, z - mu, kc));
}
struct MpBwdCoef {
  float sc[4], sh[4];                           // forward BN scale / shift (the max-pool's argmax)
  float bsc[4], bsh[4], mu[4], kx[4], kc[4];    // backward coefficients (bcoef, 5 C)
};
template <bool BF>
__device__ __forceinline__ void mp_apply(const MpWin& m, long long wi, bool valid, int H, int W, int c, int ldo,
                                         long long lim, const MpBwdCoef& k, void* __restrict__ out) {
  const int Hp = H / 2, Wp = W / 2, Hc = (H + 1) / 2, Wc = (W + 1) / 2;
  const int wc = (int)(wi % Wc);
  const long long r = wi / Wc;
  const int hc = (int)(r % Hc);
  const int n = (int)(r / Hc);
  const bool full = hc < Hp && wc < Wp;
  float zv[4][4], dv[4][4];
#pragma unroll
  for (int q = 0; q < 4; ++q) {
    zv[q][0] = m.z[q].x; zv[q][1] = m.z[q].y; zv[q][2] = m.z[q].z; zv[q][3] = m.z[q].w;
    dv[q][0] = m.d[q].x; dv[q][1] = m.d[q].y; dv[q][2] = m.d[q].z; dv[q][3] = m.d[q].w;
  }
  const float gv[4] = {full ? m.g.x : 0.f, full ? m.g.y : 0.f, full ? m.g.z : 0.f, full ? m.g.w : 0.f};
#pragma unroll
  for (int e = 0; e < 4; ++e) {
    float best = fmaxf(0.f, fmaf(zv[0][e], k.sc[e], k.sh[e]));
    int arg = 0;
#pragma unroll
    for (int q = 1; q < 4; ++q) {
      const float a = fmaxf(0.f, fmaf(zv[q][e], k.sc[e], k.sh[e]));
      if (a > best) { best = a; arg = q; }
    }
#pragma unroll
    for (int q = 0; q < 4; ++q) dv[q][e] += arg == q ? gv[e] : 0.f;
  }
#pragma unroll
  for (int q = 0; q < 4; ++q) {
    const int h = 2 * hc + (q >> 1), w = 2 * wc + (q & 1);
    if (!valid || h >= H || w >= W) continue;
    float o[4];
#pragma unroll
    for (int e = 0; e < 4; ++e) o[e] = mp_bnbwd1(dv[q][e], zv[q][e], k.bsc[e], k.bsh[e], k.mu[e], k.kx[e], k.kc[e]);
    const long long off = (((long long)n * H + h) * W + w) * ldo + c;
    PMU_DCHECK(off + 4 <= lim, PMU_DBG_OUTPUT);
    (void)lim;
    if (BF)
      *reinterpret_cast<uint2*>(static_cast<unsigned short*>(out) + off) =
          make_uint2(pmu_pk_bf16(o[0], o[1]), pmu_pk_bf16(o[2], o[3]));
    else
      *reinterpret_cast<float4*>(static_cast<float*>(out) + off) = make_float4(o[0], o[1], o[2], o[3]);
  }
}

// DT: storage of dpool and skip (bf16 bits: the *_dxb gradients; float: the fp32 path); BF: dz as bf16
// bits (the bf16 convs' operand) or fp32 (the Winograd input gradient's)
template <class DT, bool BF>
__global__ __launch_bounds__(256) void maxpool2_bwd_bnbwd_kernel(const DT* __restrict__ dpool,
                                                                 const DT* __restrict__ skip,
                                                                 const float* __restrict__ z,
                                                                 const float* __restrict__ coef,
                                                                 const float* __restrict__ bcoef, int N, int H, int W,
                                                                 int C, int ldo, void* __restrict__ out) {
  const int CQ = C >> 2, qs = CQ < 256 ? CQ : 256, wpt = 256 / qs;  // windows per block step
  const int q0 = threadIdx.x % qs, wl = threadIdx.x / qs;
  const long long nwin = (long long)N * ((H + 1) / 2) * ((W + 1) / 2), last = nwin - 1;
  const long long lim = (long long)N * H * W * ldo;
  const long long step = (long long)gridDim.x * wpt;
  for (int qb = 0; qb < CQ; qb += qs) {  // (qs divides CQ: C % 4 == 0 and CQ < 256 or CQ % 256 == 0)
    const int c = 4 * (qb + q0);
    MpBwdCoef k;
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      k.sc[e] = coef[c + e];
      k.sh[e] = coef[C + c + e];
      k.bsc[e] = bcoef[c + e];
      k.bsh[e] = bcoef[C + c + e];
      k.mu[e] = bcoef[2 * C + c + e];
      k.kx[e] = bcoef[3 * C + c + e];
      k.kc[e] = bcoef[4 * C + c + e];
    }
    for (long long wi = (long long)blockIdx.x * wpt + wl; wi < nwin; wi += 2 * step) {
      const long long wj = wi + step;
      MpWin A, B;
      mp_load<true, DT>(dpool, z, skip, wi, H, W, C, c, A);
      mp_load<true, DT>(dpool, z, skip, min(wj, last), H, W, C, c, B);
      mp_apply<BF>(A, wi, true, H, W, c, ldo, lim, k, out);
      mp_apply<BF>(B, min(wj, last), wj < nwin, H, W, c, ldo, lim, k, out);
    }
  }
}
}  // namespace

template <class DT, bool BF>
static int maxpool2_bwd_bnbwd_launch(const DT* dpool, const DT* skip, const float* z, const float* coef,
                                     const float* bcoef, int N, int H, int W, int C, int ldo, void* dz, void* stream) {
  PMU_REQUIRE(dpool && skip && z && coef && bcoef && dz && N > 0 && H > 1 && W > 1 && C > 0 && C % 4 == 0 && ldo == C);
  const int CQ = C / 4;
  PMU_REQUIRE(CQ < 256 ? 256 % CQ == 0 : CQ % 256 == 0);
  const int wpt = 256 / (CQ < 256 ? CQ : 256);
  const long long nwin = (long long)N * ((H + 1) / 2) * ((W + 1) / 2);
  const long long blocks = std::min<long long>(pmu_cdiv(nwin, 2LL * wpt), 1LL << 20);
  hipLaunchKernelGGL((maxpool2_bwd_bnbwd_kernel<DT, BF>), dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream,
                     dpool, skip, z, coef, bcoef, N, H, W, C, ldo, dz);
  PMU_CHECK_LAUNCH();
  return PMU_OK;
}

extern "C" int pmu_maxpool2_bwd_bnbwd_dxb(const unsigned short* dpool, const unsigned short* skip, const float* z,
                                          const float* coef, const float* bcoef, int N, int H, int W, int C, int ldo,
                                          unsigned short* dz, void* stream) {
  return maxpool2_bwd_bnbwd_launch<unsigned short, true>(dpool, skip, z, coef, bcoef, N, H, W, C, ldo, dz, stream);
}

// The fp32 form (config c2's skip levels): dpool and skip fp32, dz fp32 — bit-equal to pmu_frame_to_f32 of
// Src(pmu_maxpool2_bwd_bnr's da accumulated into skip, BNBWD, bcoef, z).
extern "C" int pmu_maxpool2_bwd_bnbwd(const float* dpool, const float* skip, const float* z, const float* coef,
                                      const float* bcoef, int N, int H, int W, int C, int ldo, float* dz,
                                      void* stream) {
  return maxpool2_bwd_bnbwd_launch<float, false>(dpool, skip, z, coef, bcoef, N, H, W, C, ldo, dz, stream);
}

// ---------------- AvgPool2d(2, ceil_mode=True) backward ----------------
namespace {
__global__ __launch_bounds__(256) void avgpool2_bwd_kernel(const float* __restrict__ dpool, int N, int H, int W, int C,
                                                           float* __restrict__ dx) {
  const int Hp = (H + 1) / 2, Wp = (W + 1) / 2;
  const long long total = (long long)N * H * W * C;
  for (long long e = (long long)blockIdx.x * blockDim.x + threadIdx.x; e < total;
       e += (long long)gridDim.x * blockDim.x) {
    const int c = (int)(e % C);
    long long p = e / C;
    const int w = (int)(p % W);
    const int h = (int)((p / W) % H);
    const int n = (int)(p / ((long long)W * H));
    const int hp = h >> 1, wp = w >> 1;
    const int cnt = (min(2 * hp + 2, H) - 2 * hp) * (min(2 * wp + 2, W) - 2 * wp);
    dx[e] = dpool[(((long long)n * Hp + hp) * Wp + wp) * C + c] / (float)cnt;
  }
}

// Vector path (C % 4 == 0, < 2^31 float4 units): one float4 per thread, 32-bit decode.  The scalar
// kernel above paid four 64-bit divisions per element.
__global__ __launch_bounds__(256) void avgpool2_bwd_vec_kernel(const float* __restrict__ dpool, int N, int H, int W,
                                                               int C, unsigned units, float* __restrict__ dx) {
  const int Hp = (H + 1) / 2, Wp = (W + 1) / 2;
  const unsigned CQ = (unsigned)C >> 2, Wu = (unsigned)W, Hu = (unsigned)H;
  for (unsigned u = blockIdx.x * blockDim.x + threadIdx.x; u < units; u += gridDim.x * blockDim.x) {
    const unsigned p = u / CQ, cq = u - p * CQ;
    const unsigned t = p / Wu, w = p - t * Wu;
    const unsigned n = t / Hu, h = t - n * Hu;
    const int hp = (int)h >> 1, wp = (int)w >> 1;
    const float cnt = (float)((min(2 * hp + 2, H) - 2 * hp) * (min(2 * wp + 2, W) - 2 * wp));
    const float4 g = *reinterpret_cast<const float4*>(dpool + ((size_t)(n * Hp + hp) * Wp + wp) * C + 4 * cq);
    *reinterpret_cast<float4*>(dx + (size_t)u * 4) = make_float4(g.x / cnt, g.y / cnt, g.z / cnt, g.w / cnt);
  }
}
}  // namespace

extern "C" int pmu_avgpool2_bwd(const float* dpool, int N, int H, int W, int C, float* dx, void* stream) {
  PMU_REQUIRE(dpool && dx && N > 0 && H > 0 && W > 0 && C > 0);
  const long long units = (long long)N * H * W * (C / 4);
  if (C % 4 == 0 && units < (1LL << 31)) {
    long long g = (units + 255) / 256;
    if (g > 16384) g = 16384;
    hipLaunchKernelGGL(avgpool2_bwd_vec_kernel, dim3((unsigned)g), dim3(256), 0, (hipStream_t)stream, dpool, N, H, W,
                       C, (unsigned)units, dx);
    PMU_CHECK_LAUNCH();
    return PMU_OK;
  }
  hipLaunchKernelGGL(avgpool2_bwd_kernel, dim3(grid_for((long long)N * H * W * C)), dim3(256), 0,
                     (hipStream_t)stream, dpool, N, H, W, C, dx);
  PMU_CHECK_LAUNCH();
  return PMU_OK;
}
